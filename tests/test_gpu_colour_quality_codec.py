"""`codec.ColourQualityCodec` against the numpy rule on the reference table of
tests/colour_quality_cases.py and against its synchronous sibling `container.encode_colour_images_to_quality`, and
`codec._PlaneQualityCodec`, the switches inside `QualityCodec` it rests on, alone.

The configurations of tests/colour_budget_cases.py (50 x 83 and 64 x 96, N = 2..3, K = 2..3, fixed and learned bin widths, with and
without an exception map, one priced ladder), three chroma shares, launch by launch and replayed as graphs. The steps of a codec run
through the threshold sets of the table -- 0, 2^62, for every k the sum of the three entries at (k, k, k) and that sum less 1, per
picture --, so consecutive steps differ in their thresholds and land on different points though no launch argument differs. On every
step:
  * 'rate_point', 'met', 'max_sse' (what the planes' searches used: the luminance's was formed on the device), 'sse', 'picture_sse',
    'picture_max_sse' and 'picture_met' equal the rule's on the table, element for element; so does the sibling's `info`;
  * 'probe_points' and 'probe_sse' equal the rule's, and `probe_sse[i, r] == sse[i]` wherever `probe_points[i, r] == rate_point[i]`: on
    50 x 83 this fails if a probe counts the coded plane;
  * `image_containers()[i]` equals the sibling's blob and the assembly of the three `encode_images(..., pad=True)` blobs at the points;
  * `decode_colour_images` of the blob reproduces `reconstruction_rgb`, and 'sse_rgb' is `colour.sse_rgb_numpy` of it.
The threshold sets are asserted, on the reference's outcome, to reach two luminance points and both values of 'picture_met'."""
import numpy
import pytest
import torch

import colour_budget_cases as cases
import colour_quality_cases as quality
from test_gpu_frame_container import CODED, images_of, models  # noqa: F401 (`models` is a fixture)

pytestmark = pytest.mark.gpu

PLANE_KEYS = ('rate_point', 'first_point', 'met', 'max_sse', 'probe_points', 'probe_sse', 'upper_bound_bytes', 'blob_bytes', 'promised', 'fits',
              'nb_bits', 'coder_bits', 'exception_bits', 'sse', 'nb_deads', 'container_bytes', 'budget_bytes')
MODES = {'launches': {}, 'graphs': {'use_graphs': True, 'nb_transform_streams': 2}}


def _sibling(models, config, share, thresholds):
    """`encode_colour_images_to_quality` of the configuration's batch at these thresholds, and what its blobs decode to; once."""
    from autoencoder_based_image_compression_amd import colour, container
    key = ('colour_quality_sibling', config, share, tuple(numpy.asarray(thresholds).reshape(-1).tolist()))
    if key not in models:
        case = quality.case_of(models, config)
        (blobs, info) = container.encode_colour_images_to_quality(case.rgb, case.encoder, case.decoder, case.ladder, max_sse=thresholds,
                                                                  chroma_ladder=case.chroma_ladder, chroma_share=share)
        decoded = numpy.concatenate([container.decode_colour_images(blob, case.decoder) for blob in blobs])
        models[key] = {'blobs': [bytes(blob) for blob in blobs], 'info': info, 'decoded': decoded, 'sse_rgb': colour.sse_rgb_numpy(case.rgb, decoded)}
    return models[key]


def _colour_codec(models, config, more, share, **extra):
    from autoencoder_based_image_compression_amd import codec
    case = quality.case_of(models, config)
    return codec.ColourQualityCodec(case.variables, case.learned, case.ladder, case.count, case.size[0], case.size[1], chroma_ladder=case.chroma_ladder,
                                    chroma_share=share, nb_in_flight=2, container_capacity_bytes=8*case.count*CODED[0]*CODED[1], **dict(more, **extra))


def _check_step(case, ticket, expected, sibling, step):
    r = ticket.result()
    n = ticket.nb_images
    for key in PLANE_KEYS:
        assert r[key].shape[:2] == (n, 3), (step, key)
    for key in ('rate_point', 'met', 'max_sse', 'sse', 'probe_points', 'probe_sse', 'picture_sse', 'picture_max_sse', 'picture_met'):
        print('step', step, key, numpy.asarray(r[key]).tolist(), 'rule', expected[key].tolist())
        assert r[key].dtype == expected[key].dtype and numpy.array_equal(r[key], expected[key]), (step, key)
    assert (r['first_point'] == 0).all()
    taken = r['probe_points'] == r['rate_point'][:, :, None]
    assert taken.any(axis=2).all()                           # every plane was probed at the point it took (met or not: the idle rounds probe it)
    assert numpy.array_equal(r['probe_sse'][taken], numpy.broadcast_to(r['sse'][:, :, None], taken.shape)[taken]), step
    info = sibling['info']
    for (key, theirs) in (('rate_point', 'rate_point'), ('met', 'plane_met'), ('max_sse', 'plane_max_sse'), ('sse', 'sse'),
                          ('probe_points', 'probe_points'), ('probe_sse', 'probe_sse'), ('blob_bytes', 'plane_blob_bytes'),
                          ('picture_max_sse', 'max_sse'), ('picture_sse', 'picture_sse'), ('picture_met', 'met'), ('picture_blob_bytes', 'blob_bytes')):
        assert r[key].dtype == info[theirs].dtype and numpy.array_equal(r[key], info[theirs]), (step, key)
    blobs = [bytes(blob) for blob in ticket.image_containers()]
    assert blobs == sibling['blobs'], step
    assert blobs == [bytes(case.picture_blob(i, expected['rate_point'][i])) for i in range(n)], step
    assert [len(blob) for blob in blobs] == r['picture_blob_bytes'].tolist()
    with pytest.raises(RuntimeError, match='image_containers'):
        ticket.container()
    merged = ticket.reconstruction_rgb.cpu().numpy()
    assert numpy.array_equal(merged, sibling['decoded']), step
    assert r['sse_rgb'].dtype == numpy.int64 and numpy.array_equal(r['sse_rgb'], sibling['sse_rgb']), step
    return r


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('share', quality.SHARES, ids=['quarter', 'third', 'nine_tenths'])
@pytest.mark.parametrize('config', sorted(cases.CONFIGS))
def test_colour_quality_steps_equal_the_rule_and_the_sibling(models, config, share, mode):
    case = quality.case_of(models, config)
    sets = case.threshold_sets()
    outcomes = quality.assert_the_set_tells(case.table, sets, share)
    rgb = torch.from_numpy(case.rgb).cuda()
    with _colour_codec(models, config, MODES[mode], share) as c:
        assert c.luma.thresholds_on_device and not c.chroma.thresholds_on_device and c.luma.pad and c.chroma.pad
        assert (c.luma.h_image, c.luma.w_image) == case.size and (c.chroma.h_image, c.chroma.w_image) == ((case.size[0] + 1)//2, (case.size[1] + 1)//2)
        pending = []
        results = []
        for (step, (thresholds, expected)) in enumerate(zip(sets, outcomes)):
            ticket = c.submit(rgb, max_sse=thresholds if step % 3 else thresholds.tolist())
            pending.append((ticket, expected, _sibling(models, config, share, thresholds), step))
            if len(pending) == c.depth:                      # looked at while `depth` - 1 steps behind it are pending
                results.append(_check_step(case, *pending.pop(0)))
        results += [_check_step(case, *entry) for entry in pending]
    # two consecutive submits, the same pictures, the same launches: thresholds 0 and 2^62 land on the two ends of the ladder
    assert results[0]['rate_point'].tolist() == [[0]*3]*case.count and results[1]['rate_point'].tolist() == [[case.nb_points - 1]*3]*case.count
    assert not results[0]['picture_met'].any() and results[1]['picture_met'].all()
    c.close()                                                # idempotent


def test_a_default_target_in_decibels_a_pinned_batch_and_late_results(models):
    from autoencoder_based_image_compression_amd import ratecontrol
    config = 'fixed_L10_exception_K3_50x83_N3'
    case = quality.case_of(models, config)
    samples = ratecontrol.colour_nb_samples(*case.size)
    from autoencoder_based_image_compression_amd.kodak.tools import tools as tls
    target = float(min(tls.psnr_from_sse(int(s), samples) for s in case.table[:, :, 1].sum(axis=1))) - 0.01
    default = ratecontrol.max_sse_for_psnr(target, samples)
    other = case.threshold_sets()[2]
    pinned = torch.from_numpy(case.rgb).pin_memory()
    with _colour_codec(models, config, {'fetch_reconstruction': True}, 1./3., target_psnr=target) as c:
        entries = []
        for step in range(2*c.depth + 1):
            thresholds = other if step % 2 else numpy.full(case.count, default, dtype=numpy.int64)
            ticket = c.submit(pinned, max_sse=other) if step % 2 else c.submit(pinned)
            assert ticket.fed_event is not None
            entries.append((ticket, quality.rule(case.table, thresholds, 1./3.), _sibling(models, config, 1./3., thresholds), step))
        for entry in entries[-c.depth:]:
            _check_step(case, *entry)
            assert numpy.array_equal(entry[0].reconstruction_host, entry[0].reconstruction_rgb.cpu().numpy())
        for (ticket, expected, sibling, step) in entries[:-c.depth]:      # the pictures have come round; what `result()` returns is the ticket's own
            r = ticket.result()
            assert numpy.array_equal(r['rate_point'], expected['rate_point']) and numpy.array_equal(r['sse_rgb'], sibling['sse_rgb'])
            assert [bytes(blob) for blob in ticket.image_containers()] == sibling['blobs']
        # a target per picture, and in decibels at submit
        r = c.submit(pinned, target_psnr=[target, 99., 1.]).result()
        thresholds = ratecontrol.max_sse_for_psnr(numpy.array([target, 99., 1.]), samples)
        assert thresholds[1] == 0 and thresholds[2] > 219*219*samples       # 99 dB: no error at all; 1 dB: more than two BT.601 planes can differ by
        assert r['picture_max_sse'].tolist() == thresholds.tolist()
        assert numpy.array_equal(r['picture_met'], quality.rule(case.table, thresholds, 1./3.)['picture_met']) and r['picture_met'][1:].tolist() == [False, True]


# ---- `_PlaneQualityCodec` alone ----------------------------------------------------------------------------------------------------------

PLANE_SIZE = (50, 83)
PLANE_N = 3


def _plane_codec(models, cls, size, ladder, **more):
    return cls(models[False]['variables'], False, ladder, PLANE_N, size[0], size[1], nb_in_flight=2, keep_reconstruction=True,
               container_capacity_bytes=8*PLANE_N*CODED[0]*CODED[1], **more)


@pytest.mark.parametrize('graphs', [False, True], ids=['launches', 'graphs'])
def test_a_padded_plane_codec_probes_the_real_pixels(models, graphs):
    """Every probe of a padded plane is `frame_sse_u8` of the padded plane's reconstruction at the probe's point: the table of
    `encode_images(pad=True)` -> `decode_images`. Thresholds on the device give what the same values give as a host array."""
    from autoencoder_based_image_compression_amd import codec, container, ratecontrol
    config = 'fixed_L10_exception_K3_50x83_N3'
    case = quality.case_of(models, config)
    table = case.table[:, 0]                                 # the luminance planes: 50 x 83, coded at 64 x 96
    planes = torch.from_numpy(case.planes[0]).cuda()
    more = {'use_graphs': True, 'nb_transform_streams': 2} if graphs else {}
    first = numpy.zeros(PLANE_N, dtype=numpy.int64)
    with _plane_codec(models, codec._PlaneQualityCodec, PLANE_SIZE, case.ladder, pad=True, **more) as padded, \
            _plane_codec(models, codec._PlaneQualityCodec, PLANE_SIZE, case.ladder, pad=True, thresholds_on_device=True, **more) as on_device:
        assert (padded.h_in, padded.w_in, padded.h_image, padded.w_image) == CODED + PLANE_SIZE
        seen = set()
        for step in range(2*padded.nb_slots + 1):
            thresholds = numpy.array([table[i, (step + i) % 3] - (step//3) % 2 for i in range(PLANE_N)], dtype=numpy.int64)
            (point, met, probe_points, probe_sse) = ratecontrol.select_by_quality(table, first, thresholds)
            tickets = (padded.submit(planes, max_sse=thresholds),
                       # a device tensor, written on the caller's stream just before; a host array and a list in turn
                       on_device.submit(planes, max_sse=(torch.from_numpy(thresholds).cuda() + 0) if step % 3 != 2 else
                                        (thresholds if step % 2 else thresholds.tolist())))
            for ticket in tickets:
                r = ticket.result()
                for (key, value) in (('rate_point', point), ('met', met), ('probe_points', probe_points), ('probe_sse', probe_sse),
                                     ('max_sse', thresholds), ('sse', table[numpy.arange(PLANE_N), point])):
                    assert r[key].dtype == value.dtype and numpy.array_equal(r[key], value), (step, key)
                for (i, blob) in enumerate(ticket.image_containers()):
                    assert bytes(blob) == bytes(case.blobs[(0, i, int(point[i]))])
            seen |= set(point.tolist())
        assert seen == {0, 1, 2}
        # thresholds on the device are the luminance codec's alone, and are what they say
        on_the_device = torch.from_numpy(thresholds).cuda()
        with pytest.raises(ValueError, match='thresholds_on_device'):
            padded.submit(planes, max_sse=on_the_device)
        with pytest.raises(ValueError, match='not both'):
            on_device.submit(planes, target_psnr=30., max_sse=on_the_device)
        for bad in (on_the_device.int(), on_the_device[:2].clone(), torch.from_numpy(thresholds),
                    torch.from_numpy(numpy.stack([thresholds, thresholds], axis=1)).cuda()[:, 0]):
            with pytest.raises(ValueError):
                on_device.submit(planes, max_sse=bad)


def test_a_step_with_thresholds_on_the_device_fetches_budgets_only(models, monkeypatch):
    """Neither captured nor eager: a step of a codec with `thresholds_on_device` calls `device.fetch_prefix` once, for its budgets;
    one without calls it twice."""
    from autoencoder_based_image_compression_amd import codec, device
    case = quality.case_of(models, 'fixed_L10_exception_K3_50x83_N3')
    calls = []
    real = device.fetch_prefix
    monkeypatch.setattr(device, 'fetch_prefix', lambda *arguments: (calls.append(1), real(*arguments))[1])
    planes = torch.from_numpy(case.planes[0]).cuda()
    thresholds = torch.full((PLANE_N,), quality.TOP, dtype=torch.int64, device='cuda')
    for graphs in (False, True):
        more = {'use_graphs': True} if graphs else {}
        counts = []
        for on_device in (True, False):
            with _plane_codec(models, codec._PlaneQualityCodec, PLANE_SIZE, case.ladder, pad=True, thresholds_on_device=on_device, **more) as c:
                for _ in range(3):
                    r = c.submit(planes, max_sse=thresholds if on_device else quality.TOP).result()
                    assert r['max_sse'].tolist() == [quality.TOP]*PLANE_N and r['rate_point'].tolist() == [2]*PLANE_N
                counts.append(len(calls))
            del calls[:]
        (with_it, without) = counts
        # every analysis side that is launched -- eager: one per step; graphs: what is captured or warmed up, none per replay -- fetches
        # the budgets once, and without the switch the thresholds as well
        assert with_it > 0 and without == 2*with_it and (graphs or with_it == 3)


def test_what_is_refused(models):
    from autoencoder_based_image_compression_amd import codec, ratecontrol
    config = 'fixed_L10_exception_K3_50x83_N3'
    case = quality.case_of(models, config)
    (ladder, variables, learned, count, size) = (case.ladder, case.variables, case.learned, case.count, case.size)
    fewer = ratecontrol.RateLadder(ladder.bin_widths_points[:2], ladder.binary_probabilities_points[:2], ladder.map_mean, 67)
    shorter = ratecontrol.RateLadder(ladder.bin_widths_points, numpy.ascontiguousarray(ladder.binary_probabilities_points[:, :, :3]), ladder.map_mean, 67)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for (bad, error, match) in (({'budget_bytes': 100000}, ValueError, 'budget_bytes'), ({'chroma_options': {'budget_bytes': 5}}, ValueError, 'budget_bytes'),
                                ({'coding_tile': (2, 3)}, ValueError, 'coding_tile'), ({'chroma_options': {'coding_tile': (2, 3)}}, ValueError, 'coding_tile'),
                                ({'rdo_lambda': 0.02}, ValueError, 'rdo_lambda'), ({'chroma_options': {'rdo_lambda': 0.02}}, ValueError, 'rdo_lambda'),
                                ({'pad': True}, ValueError, '`pad`'), ({'keep_reconstruction': True}, ValueError, 'keep_reconstruction'),
                                ({'chroma_options': {'pad': True}}, ValueError, '`pad`'), ({'thresholds_on_device': True}, ValueError, 'thresholds_on_device'),
                                ({'chroma_ladder': fewer}, ValueError, 'rate points'), ({'chroma_ladder': shorter}, ValueError, 'truncated unary'),
                                ({'chroma_ladder': 'coarse'}, TypeError, 'RateLadder'), ({'chroma_share': 0.}, ValueError, 'chroma_share'),
                                ({'chroma_share': 1.}, ValueError, 'chroma_share'), ({'chroma_share': -0.5}, ValueError, 'chroma_share'),
                                ({'target_psnr': 30., 'max_sse': 5}, ValueError, 'not both'), ({'max_sse': [1, 2]}, ValueError, 'per picture'),
                                ({'max_sse': 1.5}, ValueError, 'integer'), ({'target_psnr': [30., 31.]}, ValueError, 'per picture')):
        with pytest.raises(error, match=match):
            codec.ColourQualityCodec(variables, learned, ladder, count, size[0], size[1], **bad)
    with pytest.raises(TypeError):
        codec.ColourQualityCodec(variables, learned, None, count, size[0], size[1])
    assert torch.cuda.memory_allocated() == before           # in front of every allocation
    # the public rate-control codecs go on refusing `pad`, and none of them takes thresholds on the device
    for (cls, more) in ((codec.QualityCodec, {'target_psnr': 30.}), (codec.TiledQualityCodec, {'coding_tile': (2, 3), 'target_psnr': 30.}),
                        (codec.BudgetCodec, {'budget_bytes': 4096})):
        with pytest.raises(ValueError, match='do not take `pad`'):
            cls(variables, learned, ladder, count, 50, 83, pad=True, **more)
    with pytest.raises(TypeError):
        codec.QualityCodec(variables, learned, ladder, count, 64, 96, target_psnr=30., thresholds_on_device=True)
    rgb = torch.from_numpy(case.rgb).cuda()
    with _colour_codec(models, config, {}, 1./3.) as c:
        with pytest.raises(ValueError, match='neither'):                  # neither, and no default
            c.submit(rgb)
        with pytest.raises(ValueError, match='not both'):
            c.submit(rgb, target_psnr=30., max_sse=1000)
        for bad in ([1, 2], 1.5, numpy.zeros((count, 1), dtype=numpy.int64), -1, (1 << 62) + 1):
            with pytest.raises(ValueError):
                c.submit(rgb, max_sse=bad)
        with pytest.raises(ValueError):
            c.submit(rgb[:2], max_sse=1000)                  # another batch size
        with pytest.raises(ValueError, match='pinned'):
            c.submit(torch.from_numpy(case.rgb), max_sse=1000)
        # and goes on working
        thresholds = case.threshold_sets()[2]
        _check_step(case, c.submit(rgb, max_sse=thresholds), quality.rule(case.table, thresholds, 1./3.), _sibling(models, config, 1./3., thresholds), 'after')
