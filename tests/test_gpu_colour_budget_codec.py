"""`codec.ColourBudgetCodec` against its synchronous sibling `container.encode_colour_images_to_budget`,
and `codec._PlaneBudgetCodec`, the two switches inside `BudgetCodec` it rests on, alone.

The configurations of tests/colour_budget_cases.py; launch by launch and replayed as graphs, `one_stream_steps` on and off, with
whatever hardware queues the process has. Over 2 * depth + 1 consecutive steps whose pictures alternate between two batches and whose
budgets differ in every step and for every picture -- built from the bounds of a first sibling call: exactly the sum of a triple's
bounds, one byte under it, a budget at which chroma's unused bytes move Y a point finer, under the header, and a scalar --:
  * `image_containers()` equals the sibling's blobs byte for byte;
  * 'rate_point', 'upper_bound_bytes', the plane budgets ('budget_bytes') and 'promised' equal the sibling's `info` element for
    element, and so do the picture-level keys;
  * 'sse_rgb' equals `colour.sse_rgb_numpy` of the decoded blobs and `reconstruction_rgb` equals `decode_colour_images`.
A pinned-host input with `fetch_reconstruction=True` and a ladder with a price are among the modes. One sequence runs between guard
bands with the inner slots' scratch, the colour rings and the colour step's own budget buffers poisoned between steps, under two
poisons. `_PlaneBudgetCodec` at 50 x 83 equals `BudgetCodec` at 64 x 96 on the numpy-edge-padded batch but for 'sse' and byte 23 of
the blobs, and a device tensor of budgets gives what the same values give as a host array. The refusals come last, the public
`BudgetCodec(pad=True)` among them."""
import numpy
import pytest
import torch

import budget_slot_buffers
import colour_budget_cases as cases
import guarded
import slot_buffers
from test_gpu_frame_container import CODED, edge_padded, images_of, models  # noqa: F401 (`models` is a fixture)

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F)
SHARE = 0.9                          # at these sizes the headers dominate every plane: the chroma planes need about a third each to be promised
NO_BUDGET = 1 << 62
PLANE_KEYS = ('rate_point', 'upper_bound_bytes', 'blob_bytes', 'promised', 'fits', 'nb_bits', 'coder_bits', 'exception_bits', 'sse', 'nb_deads',
              'container_bytes', 'budget_bytes')
# name: (configuration, ColourBudgetCodec arguments, feed pinned host batches, chroma share)
MODES = {
    'launches': ('fixed_L10_exception_K3_50x83_N3', {}, False, SHARE),
    'launches_one_stream': ('learned_L3_K2_64x96_N2', {'one_stream_steps': True}, False, SHARE),
    'graphs_two_streams': ('fixed_L10_exception_K3_50x83_N3', {'use_graphs': True, 'nb_transform_streams': 2}, False, SHARE),
    'graphs_one_stream': ('learned_L10_exception_K2_50x83_N2_chroma_doubled', {'use_graphs': True, 'nb_transform_streams': 2, 'one_stream_steps': True},
                          False, SHARE),
    'graphs_default_share': ('learned_L3_K2_64x96_N2', {'use_graphs': True}, False, 0.25),
    'pinned_fetch': ('learned_L10_exception_K2_50x83_N2_chroma_doubled', {'fetch_reconstruction': True}, True, SHARE),
    'priced_graphs': ('fixed_L3_K3_64x96_N3_priced', {'use_graphs': True}, False, SHARE),
}


def _feed(array, host):
    tensor = torch.from_numpy(array)
    return tensor.pin_memory() if host else tensor.cuda()


def _capacity(config):
    (_, _, _, _, count, _, _) = cases.CONFIGS[config]
    return 8*count*CODED[0]*CODED[1]


def _sibling(models, config, seed, budgets, share):
    """`encode_colour_images_to_budget` of batch `seed` at these budgets, and what its blobs decode to; once per call."""
    from autoencoder_based_image_compression_amd import colour, container
    budgets = numpy.asarray(budgets, dtype=numpy.int64)
    key = ('colour_budget_sibling', config, seed, tuple(budgets.reshape(-1).tolist()), share)
    if key not in models:
        (learned, _, _, _, count, _, _) = cases.CONFIGS[config]
        (ladder, chroma_ladder) = cases.ladders_of(models, config)
        rgb = cases.pictures(config, seed)
        (blobs, info) = container.encode_colour_images_to_budget(rgb, models[learned]['encoder'], ladder, budgets, chroma_ladder=chroma_ladder,
                                                                 chroma_share=share)
        decoded = numpy.concatenate([container.decode_colour_images(blob, models[learned]['decoder']) for blob in blobs])
        info['budget_bytes'] = numpy.broadcast_to(budgets, (count,))
        models[key] = {'rgb': rgb, 'blobs': blobs, 'info': info, 'decoded': decoded, 'sse_rgb': colour.sse_rgb_numpy(rgb, decoded)}
    return models[key]


def _step_budgets(models, config, seed, share, nb_steps):
    """The budgets of every step, built from the bounds of a first sibling call on batch `seed`."""
    first = _sibling(models, config, seed, NO_BUDGET, share)['info']
    (upper, valid) = (first['upper_bound_bytes'], first['valid_points'])
    (n, _, k) = upper.shape
    exact = []
    for shift in range(k):
        built = cases.exact_budgets(upper, valid, share, shift)
        if built is not None:
            exact += [built[0], built[0] - 1]
    spill = cases.spill_budgets(upper, valid, share)
    # always there: under and around the header, every picture between two sums of bounds, and a scalar that fits everything
    always = [numpy.array([0, 47, 48, 49, 50][:n], dtype=numpy.int64), cases.HEADER + upper[:, :, -1].sum(axis=1) + numpy.arange(n)*97 + 13,
              numpy.int64(cases.HEADER + upper[:, :, 0].sum(axis=1).max())]
    variants = exact[:2] + always[:1] + ([spill] if spill is not None else []) + always[1:] + exact[2:]
    return [variants[(step + 2*seed) % len(variants)] for step in range(nb_steps)]


def _colour_codec(models, config, more, share, **extra):
    from autoencoder_based_image_compression_amd import codec
    (learned, _, _, size, count, _, _) = cases.CONFIGS[config]
    (ladder, chroma_ladder) = cases.ladders_of(models, config)
    return codec.ColourBudgetCodec(models[learned]['variables'], learned, ladder, count, size[0], size[1], chroma_ladder=chroma_ladder,
                                   chroma_share=share, nb_in_flight=2, container_capacity_bytes=_capacity(config), **dict(more, **extra))


def _check_step(c, ticket, expected, step):
    info = expected['info']
    r = ticket.result()
    n = ticket.nb_images
    for key in PLANE_KEYS:
        assert r[key].shape[:2] == (n, 3), (step, key)
    for (key, theirs) in (('rate_point', 'rate_point'), ('upper_bound_bytes', 'upper_bound_bytes'), ('budget_bytes', 'plane_budget_bytes'),
                          ('promised', 'plane_promised'), ('blob_bytes', 'plane_blob_bytes'), ('picture_budget_bytes', 'budget_bytes'),
                          ('picture_blob_bytes', 'blob_bytes'), ('picture_promised', 'promised'), ('picture_fits', 'fits')):
        print('step', step, key, numpy.asarray(r[key]).tolist(), 'sibling', numpy.asarray(info[theirs]).tolist())
        assert r[key].dtype == info[theirs].dtype and numpy.array_equal(r[key], info[theirs]), (step, key)
    assert numpy.array_equal(r['fits'], r['blob_bytes'] <= r['budget_bytes'])
    assert not (r['picture_promised'] & ~r['picture_fits']).any()
    blobs = ticket.image_containers()
    assert [bytes(blob) for blob in blobs] == expected['blobs'], step
    assert [len(blob) for blob in blobs] == r['picture_blob_bytes'].tolist()
    with pytest.raises(RuntimeError, match='image_containers'):
        ticket.container()
    assert r['sse_rgb'].dtype == numpy.int64 and numpy.array_equal(r['sse_rgb'], expected['sse_rgb']), step
    merged = ticket.reconstruction_rgb.cpu().numpy()
    assert numpy.array_equal(merged, expected['decoded']), step
    if c.fetch_reconstruction:
        assert isinstance(ticket.reconstruction_host, numpy.ndarray) and numpy.array_equal(ticket.reconstruction_host, merged), step
    else:
        assert ticket.reconstruction_host is None
    return r


@pytest.mark.parametrize('mode', sorted(MODES))
def test_colour_budget_steps_equal_the_sibling(models, mode):
    (config, more, host, share) = MODES[mode]
    (_, _, nb_points, size, count, _, _) = cases.CONFIGS[config]
    with _colour_codec(models, config, more, share) as c:
        assert c.depth == min(c.luma.nb_slots, c.chroma.nb_slots//2) >= 1 and len(c._steps) == c.depth
        assert c.luma.budgets_on_device and not c.chroma.budgets_on_device and c.luma.pad and c.chroma.pad
        assert (c.luma.h_image, c.luma.w_image) == size and (c.chroma.h_image, c.chroma.w_image) == ((size[0] + 1)//2, (size[1] + 1)//2)
        nb_steps = 2*c.depth + 1
        budgets = [_step_budgets(models, config, seed, share, nb_steps) for seed in (0, 1)]
        (seen_points, seen_promises) = (set(), set())
        pending = []
        for step in range(nb_steps):
            seed = step % 2
            expected = _sibling(models, config, seed, budgets[seed][step], share)
            given = budgets[seed][step]
            ticket = c.submit(_feed(expected['rgb'], host), given if step % 3 else numpy.asarray(given).tolist())
            if host:
                assert ticket.fed_event is not None
            pending.append((ticket, expected, step))
            if len(pending) == c.depth:                      # looked at while `depth` - 1 steps behind it are pending
                r = _check_step(c, *pending.pop(0))
                seen_points |= set(r['rate_point'][:, 0].tolist())
                seen_promises |= set(r['picture_promised'].tolist())
        for entry in pending:
            _check_step(c, *entry)
        assert len(seen_points) > 1 and False in seen_promises and (True in seen_promises or share != SHARE)
    c.close()                                                # idempotent


def test_a_default_budget_and_results_collected_late(models):
    """No ticket is touched until every step is submitted; the budgets come from the constructor in every other step."""
    config = 'fixed_L10_exception_K3_50x83_N3'
    default = _step_budgets(models, config, 0, SHARE, 1)[0]
    with _colour_codec(models, config, {}, SHARE, budget_bytes=default) as c:
        nb_steps = 2*c.depth + 1
        budgets = _step_budgets(models, config, 1, SHARE, nb_steps)
        entries = []
        for step in range(nb_steps):
            if step % 2:
                expected = _sibling(models, config, 1, budgets[step], SHARE)
                entries.append((c.submit(_feed(expected['rgb'], False), budgets[step]), expected, step))
            else:
                expected = _sibling(models, config, 0, default, SHARE)
                entries.append((c.submit(_feed(expected['rgb'], False)), expected, step))
        for (ticket, expected, step) in entries[-c.depth:]:
            _check_step(c, ticket, expected, step)
        for (ticket, expected, step) in entries[:-c.depth]:      # the pictures have come round; everything `result()` returns is the ticket's own
            r = ticket.result()
            assert numpy.array_equal(r['rate_point'], expected['info']['rate_point']) and numpy.array_equal(r['sse_rgb'], expected['sse_rgb'])
            assert [bytes(blob) for blob in ticket.image_containers()] == expected['blobs']
    with _colour_codec(models, config, {}, SHARE) as c:
        with pytest.raises(ValueError, match='budget_bytes'):
            c.submit(_feed(cases.pictures(config), False))


def _poison_rings(c, guard, poison):
    c.drain()
    guard.check(keep=True)
    for inner in (c.luma, c.chroma):
        assert slot_buffers.poison_scratch(inner, poison) > 0 and budget_slot_buffers.poison_scratch(inner, poison) > 0
        for reference in (getattr(inner, '_frame_references', None) or ()):
            slot_buffers.fill_bytes(reference, poison)
    for ring in c._steps:
        for tensor in (ring.rgb_in, ring.rgb_out, ring.sse, ring.pinned_sse, ring.pinned_budgets, ring.budgets, ring.luma_budgets) + tuple(ring.planes):
            slot_buffers.fill_bytes(tensor, poison)
    torch.cuda.synchronize()


@pytest.mark.parametrize('graphs', [False, True], ids=['launches', 'graphs'])
def test_colour_budget_steps_on_poisoned_rings(models, graphs):
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    config = 'fixed_L10_exception_K3_50x83_N3'
    seen = {}
    for poison in POISONS:
        with guarded.guarded((device, pipeline, codec), poison) as guard:
            with _colour_codec(models, config, {'use_graphs': True} if graphs else {}, SHARE) as c:
                torch.cuda.synchronize()
                _poison_rings(c, guard, poison)
                nb_steps = 2*c.depth + 1
                budgets = [_step_budgets(models, config, seed, SHARE, nb_steps) for seed in (0, 1)]
                values = []
                for step in range(nb_steps):
                    seed = (step//c.depth) % 2
                    expected = _sibling(models, config, seed, budgets[seed][step], SHARE)
                    ticket = c.submit(_feed(expected['rgb'], step % 2 == 1), budgets[seed][step])      # device and pinned batches in turn
                    r = _check_step(c, ticket, expected, step)
                    values.append([r[key].tobytes() for key in sorted(r)])
                    _poison_rings(c, guard, poison)
        seen[poison] = values
    assert seen[POISONS[0]] == seen[POISONS[1]]


# ---- `_PlaneBudgetCodec` alone ---------------------------------------------------------------------------------------------------------

PLANE_SIZE = (50, 83)
PLANE_N = 3


def _plane_ladder(models, learned):
    from autoencoder_based_image_compression_amd import ratecontrol
    m = models[learned]
    return ratecontrol.RateLadder((m['bin_widths'][None]*numpy.array([[1.], [2.], [4.]], dtype=numpy.float32)).astype(numpy.float32),
                                  numpy.stack([models['probabilities']]*3), m['map_mean'], 67)


def _plane_codec(models, learned, cls, size, **more):
    return cls(models[learned]['variables'], learned, _plane_ladder(models, learned), PLANE_N, size[0], size[1], nb_in_flight=2, keep_reconstruction=True,
               container_capacity_bytes=8*PLANE_N*CODED[0]*CODED[1], **more)


@pytest.mark.parametrize('graphs', [False, True], ids=['launches', 'graphs'])
@pytest.mark.parametrize('learned', [False, True], ids=['fixed', 'learned'])
def test_a_padded_plane_codec_equals_the_budget_codec_of_the_padded_batch(models, learned, graphs):
    from autoencoder_based_image_compression_amd import codec, container
    (h, w) = PLANE_SIZE
    more = {'use_graphs': True, 'nb_transform_streams': 2} if graphs else {}
    ladder = _plane_ladder(models, learned)
    with _plane_codec(models, learned, codec._PlaneBudgetCodec, PLANE_SIZE, pad=True, **more) as padded, \
            _plane_codec(models, learned, codec._PlaneBudgetCodec, PLANE_SIZE, pad=True, budgets_on_device=True, **more) as on_device, \
            _plane_codec(models, learned, codec.BudgetCodec, CODED, **more) as reference:
        assert (padded.h_in, padded.w_in, padded.h_image, padded.w_image) == CODED + PLANE_SIZE
        upper = None
        seen = set()
        for step in range(2*padded.nb_slots + 1):
            images = images_of(PLANE_SIZE, step % 2, PLANE_N)
            if upper is None:
                budgets = numpy.full(PLANE_N, NO_BUDGET, dtype=numpy.int64)
            else:                                            # from the first step's bounds: at a point's bound, and one byte under it
                budgets = numpy.array([upper[i, (step + i) % 3] - (step//3) % 2 for i in range(PLANE_N)], dtype=numpy.int64)
            expected_ticket = reference.submit(torch.from_numpy(edge_padded(images)).cuda(), budgets)
            tickets = (padded.submit(torch.from_numpy(images).cuda(), budgets),
                       # a device tensor, written on the caller's stream just before; a host array and a list in turn
                       on_device.submit(torch.from_numpy(images).cuda(), (torch.from_numpy(budgets).cuda() + 0) if step % 3 != 2 else
                                        (budgets if step % 2 else budgets.tolist())))
            expected = expected_ticket.result()
            whole = expected_ticket.reconstruction_uint8.cpu().numpy()
            difference = images.astype(numpy.int64) - whole[:, :h, :w].astype(numpy.int64)
            for ticket in tickets:
                r = ticket.result()
                assert sorted(r) == sorted(expected)
                for key in r:
                    if key != 'sse':
                        assert r[key].dtype == expected[key].dtype and numpy.array_equal(r[key], expected[key]), (step, key)
                assert numpy.array_equal(r['sse'], (difference*difference).sum(axis=(1, 2))) and r['sse'].dtype == expected['sse'].dtype
                assert numpy.array_equal(r['budget_bytes'], budgets)
                assert tuple(ticket.reconstruction_uint8.shape) == (PLANE_N, h, w)
                assert numpy.array_equal(ticket.reconstruction_uint8.cpu().numpy(), whole[:, :h, :w])
                blobs = ticket.image_containers()
                for (i, (blob, other)) in enumerate(zip(blobs, expected_ticket.image_containers())):
                    assert blob[:23] == other[:23] and blob[24:] == other[24:] and blob[23] == (14 << 4 | 13) and other[23] == 0
                    k = int(r['rate_point'][i])
                    assert blob == container.encode_images(images[i:i + 1], models[learned]['encoder'], ladder.bin_widths_points[k], ladder.map_mean,
                                                           ladder.binary_probabilities_points[k], 67, pad=True)[0]
            seen |= set(expected['rate_point'].tolist())
            if upper is None:
                upper = expected['upper_bound_bytes']
        assert seen == {0, 1, 2}
        # budgets on the device are the luminance codec's alone, and are what they say
        with pytest.raises(ValueError, match='budgets_on_device'):
            padded.submit(torch.from_numpy(images).cuda(), torch.from_numpy(budgets).cuda())
        for bad in (torch.from_numpy(budgets).cuda().int(), torch.from_numpy(budgets[:2].copy()).cuda(), torch.from_numpy(budgets),
                    torch.from_numpy(numpy.stack([budgets, budgets], axis=1)).cuda()[:, 0]):
            with pytest.raises(ValueError):
                on_device.submit(torch.from_numpy(images).cuda(), bad)


def test_a_step_with_budgets_on_the_device_fetches_none(models, monkeypatch):
    """Neither captured nor eager: `device.fetch_prefix` is not called by a step of a codec with `budgets_on_device`, and is by one
    without."""
    from autoencoder_based_image_compression_amd import codec, device
    calls = []
    real = device.fetch_prefix
    monkeypatch.setattr(device, 'fetch_prefix', lambda *arguments: (calls.append(1), real(*arguments))[1])
    images = torch.from_numpy(images_of(PLANE_SIZE, 0, PLANE_N)).cuda()
    budgets = torch.full((PLANE_N,), NO_BUDGET, dtype=torch.int64, device='cuda')
    for graphs in (False, True):
        more = {'use_graphs': True} if graphs else {}
        with _plane_codec(models, False, codec._PlaneBudgetCodec, PLANE_SIZE, pad=True, budgets_on_device=True, **more) as c:
            for _ in range(3):
                assert c.submit(images, budgets).result()['budget_bytes'].tolist() == [NO_BUDGET]*PLANE_N
        assert calls == []
        with _plane_codec(models, False, codec._PlaneBudgetCodec, PLANE_SIZE, pad=True, **more) as c:
            c.submit(images, NO_BUDGET).result()
        assert calls
        del calls[:]


def test_what_is_refused(models):
    from autoencoder_based_image_compression_amd import codec, ratecontrol
    config = 'fixed_L10_exception_K3_50x83_N3'
    (learned, _, _, size, count, _, _) = cases.CONFIGS[config]
    (ladder, _) = cases.ladders_of(models, config)
    variables = models[learned]['variables']
    fewer = ratecontrol.RateLadder(ladder.bin_widths_points[:2], ladder.binary_probabilities_points[:2], ladder.map_mean, 67)
    shorter = ratecontrol.RateLadder(ladder.bin_widths_points, numpy.ascontiguousarray(ladder.binary_probabilities_points[:, :, :3]), ladder.map_mean, 67)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for (bad, error) in (({'coding_tile': (2, 3)}, ValueError), ({'chroma_options': {'coding_tile': (2, 3)}}, ValueError),
                         ({'rdo_lambda': 0.02}, ValueError), ({'chroma_options': {'rdo_lambda': 0.02}}, ValueError),
                         ({'pad': True}, ValueError), ({'keep_reconstruction': True}, ValueError), ({'chroma_options': {'pad': True}}, ValueError),
                         ({'chroma_ladder': fewer}, ValueError), ({'chroma_ladder': shorter}, ValueError), ({'chroma_ladder': 'coarse'}, TypeError),
                         ({'chroma_share': 0.}, ValueError), ({'chroma_share': 1.}, ValueError), ({'chroma_share': -0.5}, ValueError),
                         ({'budget_bytes': [1, 2]}, ValueError), ({'budgets_on_device': True}, ValueError)):
        with pytest.raises(error):
            codec.ColourBudgetCodec(variables, learned, ladder, count, size[0], size[1], **bad)
    with pytest.raises(TypeError):
        codec.ColourBudgetCodec(variables, learned, None, count, size[0], size[1])
    assert torch.cuda.memory_allocated() == before           # in front of every allocation
    for (bad, match) in (({'coding_tile': (2, 3)}, 'coding_tile'), ({'rdo_lambda': 0.02}, 'rdo_lambda'), ({'pad': True}, 'pad'),
                         ({'keep_reconstruction': True}, 'keep_reconstruction'), ({'chroma_share': 1.}, 'chroma_share')):
        with pytest.raises(ValueError, match=match):
            codec.ColourBudgetCodec(variables, learned, ladder, count, size[0], size[1], **bad)
    # a chroma codec of one slot cannot hold Cb and Cr of one colour step
    with pytest.raises(ValueError, match='cannot hold'):
        codec.ColourBudgetCodec(variables, learned, ladder, count, size[0], size[1], use_graphs=True, nb_transform_streams=2, one_stream_steps=True,
                                nb_in_flight=2, chroma_options={'nb_in_flight': -1})
    # the public rate-control codecs go on refusing `pad`, word for word
    for (cls, more) in ((codec.BudgetCodec, {'budget_bytes': 4096}), (codec.TiledBudgetCodec, {'coding_tile': (2, 3), 'budget_bytes': 4096}),
                        (codec.QualityCodec, {'target_psnr': 30.}), (codec.TiledQualityCodec, {'coding_tile': (2, 3), 'target_psnr': 30.})):
        with pytest.raises(ValueError, match='do not take `pad`'):
            cls(variables, learned, ladder, count, 50, 83, pad=True, **more)
    with pytest.raises(TypeError):
        codec.BudgetCodec(variables, learned, ladder, count, 64, 96, budgets_on_device=True)
    rgb = cases.pictures(config)
    with _colour_codec(models, config, {}, SHARE) as c:
        for bad in ([1, 2], 1.5, numpy.zeros((count, 1), dtype=numpy.int64)):
            with pytest.raises(ValueError):
                c.submit(_feed(rgb, False), bad)
        with pytest.raises(ValueError):
            c.submit(_feed(rgb[:2], False), 100000)          # another batch size
        with pytest.raises(ValueError, match='pinned'):
            c.submit(torch.from_numpy(rgb), 100000)
        # and goes on working
        expected = _sibling(models, config, 0, 100000, SHARE)
        _check_step(c, c.submit(_feed(rgb, False), 100000), expected, 'after')
