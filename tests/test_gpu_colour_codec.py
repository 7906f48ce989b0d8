"""`codec.ColourCodec`: batches of three 99 x 165 RGB pictures through two `BatchCodec(pad=True)`.

In every mode below -- launch by launch, replayed graphs on two transform streams, pinned batches in with the merged picture
fetched, and with containers as EAE1 and in coding tiles --, over 3 * depth + 1 consecutive steps with `depth` of them pending at
any time, every step is held against plain `BatchCodec(pad=True, keep_reconstruction=True)` steps on `colour.split_420_numpy`'s
planes. The steps go through four different batches in an order (`_schedule`) in which no step takes the batch of the step before
it, nor the batch that its ring entry, its luminance slot or its chroma slots held the time before: a merge that ran after its
inner slot came round, a plane buffer or batch copy that was not refreshed, or a reconstruction of the previous round would be
another picture.
  * every key of `result()` is (N, 3): the three inner results, in the order Y, Cb, Cr;
  * the merged picture is `colour.merge_420_numpy` of those codecs' kept reconstructions, 'sse_rgb' `colour.sse_rgb_numpy`;
  * `container()` / `image_containers()` are `container.encode_colour_images` of the step's pictures, byte for byte, and
    `container.decode_colour_images(container())` is the merged picture.
`test_results_collected_late_are_their_own_steps` submits such a sequence and touches no ticket until all of it is submitted:
`result()` and the containers are then still each step's own. One sequence runs on guard-banded buffers with the colour codec's own rings (batch copies, plane buffers, RGB outputs, squared
errors) and the inner codecs' scratch poisoned between the steps, under two poisons. The refusals of the constructor and of
`submit` are reached last."""
import numpy
import pytest
import torch

import guarded
import slot_buffers
from test_gpu_colour_container import pictures_of, points_of
from test_gpu_frame_container import models  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

N = 3
SIZE = (99, 165)
CHROMA = (50, 83)
RATE = 'L10_exception_67'
POISONS = (0xFF, 0x7F)
CAPACITY = 8*N*112*176
NB_BATCHES = 4
# name: (ColourCodec arguments, feed pinned host batches, chroma at doubled bin widths)
MODES = {
    'launches': ({}, False, False),
    'graphs_two_streams': ({'use_graphs': True, 'nb_transform_streams': 2}, False, True),
    'pinned_fetch': ({'fetch_reconstruction': True}, True, False),
    'container_EAE1': ({'emit_container': True, 'container_capacity_bytes': CAPACITY}, False, True),
    'container_tiles_2x3_graphs': ({'emit_container': True, 'container_capacity_bytes': CAPACITY, 'coding_tile': (2, 3), 'use_graphs': True}, True, False),
}
INNER_ONLY = ('use_graphs', 'nb_transform_streams', 'fetch_reconstruction')      # what does not change a plain codec's results


def _feed(pictures, host):
    tensor = torch.from_numpy(pictures)
    return tensor.pin_memory() if host else tensor.cuda()


def _colour_codec(models, more, doubled, **extra):
    from autoencoder_based_image_compression_amd import codec
    (_, luma, chroma) = points_of(models, False, RATE, doubled)
    return codec.ColourCodec(models[False]['variables'], False, *luma, N, SIZE[0], SIZE[1], chroma=chroma, nb_in_flight=2, **dict(more, **extra))


def _expected(models, more, doubled):
    """For the four batches: what plain codecs give for the three planes, once per set of options that changes a plain codec's results."""
    from autoencoder_based_image_compression_amd import codec, colour, container
    plain = {key: value for (key, value) in more.items() if key not in INNER_ONLY}
    cache_key = ('colour_expected', tuple(sorted(plain.items())), doubled)
    if cache_key in models:
        return models[cache_key]
    (encoder, luma, chroma) = points_of(models, False, RATE, doubled)
    variables = models[False]['variables']
    out = []
    with codec.BatchCodec(variables, False, *luma, N, SIZE[0], SIZE[1], nb_in_flight=2, keep_reconstruction=True, pad=True, **plain) as luma_codec, \
            codec.BatchCodec(variables, False, *(chroma or luma), N, CHROMA[0], CHROMA[1], nb_in_flight=2, keep_reconstruction=True, pad=True,
                             **plain) as chroma_codec:
        for seed in range(NB_BATCHES):
            rgb = pictures_of(SIZE, seed, N)
            planes = colour.split_420_numpy(rgb)
            results = []
            reconstructions = []
            for (plane, inner) in zip(planes, (luma_codec, chroma_codec, chroma_codec)):
                ticket = inner.submit(torch.from_numpy(plane).cuda())
                results.append(ticket.result())
                reconstructions.append(ticket.reconstruction_uint8.cpu().numpy())
            merged = colour.merge_420_numpy(*reconstructions)
            entry = {'rgb': rgb, 'results': results, 'merged': merged, 'sse_rgb': colour.sse_rgb_numpy(rgb, merged)}
            if plain.get('emit_container'):
                extra = {'coding_tile': plain['coding_tile']} if 'coding_tile' in plain else {}
                entry['blob'] = container.encode_colour_images(rgb, encoder, *luma, chroma=chroma, **extra)[0]
                entry['image_blobs'] = [container.encode_colour_images(rgb[i:i + 1], encoder, *luma, chroma=chroma, **extra)[0] for i in range(N)]
            out.append(entry)
    for a in range(NB_BATCHES):
        for b in range(a):
            assert not numpy.array_equal(out[a]['merged'], out[b]['merged']) and not numpy.array_equal(out[a]['sse_rgb'], out[b]['sse_rgb'])
    models[cache_key] = out
    return out


def _schedule(c, steps):
    """The batch every step takes: never that of the step before, nor the one the same ring entry, luminance slot or pair of chroma
    slots (either parity) held the time before."""
    periods = sorted({1, c.depth, c.luma.nb_slots, c.chroma.nb_slots//2, -(-c.chroma.nb_slots//2)})
    assert len(periods) < NB_BATCHES
    order = []
    for step in range(steps):
        taken = {order[step - period] for period in periods if step >= period}
        order.append(min(batch for batch in range(NB_BATCHES) if batch not in taken))
    assert all(order[step] != order[step - period] for period in periods for step in range(period, steps))
    return order


def _check_step(models, c, ticket, expected, step, pictures=True):
    from autoencoder_based_image_compression_amd import container
    r = ticket.result()
    assert sorted(r) == sorted(list(expected['results'][0]) + ['sse_rgb']), step
    for key in expected['results'][0]:
        assert r[key].shape == (N, 3), (step, key)
        for (k, inner) in enumerate(expected['results']):
            assert numpy.array_equal(r[key][:, k], inner[key]) and r[key].dtype == inner[key].dtype, (step, key, k)
    assert r['sse_rgb'].dtype == numpy.int64 and numpy.array_equal(r['sse_rgb'], expected['sse_rgb']), step
    assert ticket.merged_event.query()
    for (inner, plane_result) in zip(ticket.tickets, expected['results']):
        assert numpy.array_equal(inner.result()['nb_bits'], plane_result['nb_bits'])
    if pictures:                                         # valid until the colour slot comes round
        assert ticket.reconstruction_rgb.is_cuda
        merged = ticket.reconstruction_rgb.cpu().numpy()
        assert merged.shape == (N,) + SIZE + (3,) and numpy.array_equal(merged, expected['merged']), step
        if c.fetch_reconstruction:
            assert isinstance(ticket.reconstruction_host, numpy.ndarray) and numpy.array_equal(ticket.reconstruction_host, merged), step
        else:
            assert ticket.reconstruction_host is None
    if c.emit_container:
        blob = ticket.container()
        assert blob == expected['blob'], step
        assert ticket.image_containers() == expected['image_blobs'], step
        assert numpy.array_equal(container.decode_colour_images(blob, models[False]['decoder']), expected['merged']), step


@pytest.mark.parametrize('mode', sorted(MODES))
def test_colour_steps_equal_three_plain_steps_and_their_merge(models, mode):
    (more, host, doubled) = MODES[mode]
    expected = _expected(models, more, doubled)
    with _colour_codec(models, more, doubled) as c:
        assert c.depth == min(c.luma.nb_slots, c.chroma.nb_slots//2) >= 1 and len(c._steps) == c.depth
        assert (c.luma.h_image, c.luma.w_image, c.chroma.h_image, c.chroma.w_image) == SIZE + CHROMA
        assert (c.luma.batch_size, c.chroma.batch_size) == (N, N) and c.luma.pad and c.chroma.pad
        steps = 3*c.depth + 1
        order = _schedule(c, steps)
        tickets = []
        for step in range(steps):
            entry = expected[order[step]]
            tickets.append((c.submit(_feed(entry['rgb'], host)), entry))
            if host:
                assert tickets[-1][0].fed_event is not None
            # the oldest step whose ring entry the next submit takes: looked at while it and the `depth` - 1 steps behind it are pending
            oldest = step - c.depth + 1
            if oldest >= 0:
                _check_step(models, c, tickets[oldest][0], tickets[oldest][1], oldest)
        for oldest in range(steps - c.depth + 1, steps):
            _check_step(models, c, tickets[oldest][0], tickets[oldest][1], oldest)
    c.close()                                            # idempotent


@pytest.mark.parametrize('mode', ['launches', 'container_tiles_2x3_graphs'])
def test_results_collected_late_are_their_own_steps(models, mode):
    """No ticket is touched until every step is submitted: each ring entry has been reused, with other pictures, up to three times by
    then. What `result()` and the containers give is the ticket's own (the pictures are the slots' and have come round)."""
    (more, host, doubled) = MODES[mode]
    expected = _expected(models, more, doubled)
    with _colour_codec(models, more, doubled) as c:
        steps = 3*c.depth + 1
        order = _schedule(c, steps)
        tickets = [c.submit(_feed(expected[batch]['rgb'], host)) for batch in order]
        for (step, (ticket, batch)) in enumerate(zip(tickets, order)):
            _check_step(models, c, ticket, expected[batch], step, pictures=step >= steps - c.depth)


def _poison_rings(c, guard, poison):
    c.drain()
    guard.check(keep=True)
    for inner in (c.luma, c.chroma):
        assert slot_buffers.poison_scratch(inner, poison) > 0
    for ring in c._steps:
        for tensor in (ring.rgb_in, ring.rgb_out, ring.sse, ring.pinned_sse) + tuple(ring.planes) + ((ring.pinned_rgb,) if ring.pinned_rgb is not None else ()):
            slot_buffers.fill_bytes(tensor, poison)
    torch.cuda.synchronize()


@pytest.mark.parametrize('graphs', [False, True], ids=['launches', 'graphs'])
def test_colour_steps_on_poisoned_rings(models, graphs):
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    more = {'emit_container': True, 'container_capacity_bytes': CAPACITY}
    expected = _expected(models, more, False)
    seen = {}
    for poison in POISONS:
        with guarded.guarded((device, pipeline, codec), poison) as guard:
            with _colour_codec(models, more, False, use_graphs=graphs) as c:
                torch.cuda.synchronize()
                _poison_rings(c, guard, poison)
                values = []
                for step in range(2*c.depth + 1):
                    entry = expected[(step//c.depth) % NB_BATCHES]
                    ticket = c.submit(_feed(entry['rgb'], step % 2 == 1))              # device and pinned batches in turn
                    _check_step(models, c, ticket, entry, step)
                    r = ticket.result()
                    values.append([r[key].tobytes() for key in sorted(r)])
                    _poison_rings(c, guard, poison)
        seen[poison] = values
    assert seen[POISONS[0]] == seen[POISONS[1]]


def test_what_is_refused(models):
    from autoencoder_based_image_compression_amd import codec
    (_, luma, _) = points_of(models, False, RATE, False)
    variables = models[False]['variables']
    # a chroma codec of one slot cannot hold Cb and Cr of one colour step
    with pytest.raises(ValueError, match='cannot hold'):
        codec.ColourCodec(variables, False, *luma, N, SIZE[0], SIZE[1], use_graphs=True, nb_transform_streams=2, one_stream_steps=True, nb_in_flight=2,
                          chroma_options={'nb_in_flight': -1})
    for bad in ({'pad': True}, {'keep_reconstruction': True}, {'chroma_options': {'emit_container': True}},
                {'chroma_options': {'fetch_reconstruction': True}}, {'chroma': luma[:3]}):
        with pytest.raises(ValueError):
            codec.ColourCodec(variables, False, *luma, N, SIZE[0], SIZE[1], **bad)
    with pytest.raises(ValueError):
        codec.ColourCodec(variables, False, *luma, N, 0, SIZE[1])
    rgb = pictures_of(SIZE, 0, N)
    with _colour_codec(models, {}, False, chroma_options={'nb_in_flight': 3}) as c:
        assert c.chroma.nb_in_flight <= 3
        with pytest.raises(ValueError):
            c.submit(torch.from_numpy(rgb[:, :, :, :2].copy()).cuda())                 # not three channels
        with pytest.raises(ValueError):
            c.submit(torch.from_numpy(rgb[:2]).cuda())                                 # another batch size
        with pytest.raises(ValueError):
            c.submit(torch.from_numpy(rgb[:, :98].copy()).cuda())                      # another height
        with pytest.raises(TypeError):
            c.submit(torch.from_numpy(rgb).cuda().int())
        with pytest.raises(ValueError, match='pinned'):
            c.submit(torch.from_numpy(rgb))                                            # a host batch that is not pinned
        # and goes on working; without `emit_container` the containers say so
        ticket = c.submit(torch.from_numpy(rgb).cuda())
        assert ticket.result()['sse_rgb'].shape == (N,)
        with pytest.raises(RuntimeError, match='emit_container'):
            ticket.container()


def test_a_submit_that_fails_half_way_leaves_a_working_codec(models):
    """The Cr submit raises after the luminance and Cb steps were queued: `submit` re-raises behind a drain, and the steps that
    follow -- on a chroma ring now one step out of pairs -- are right."""
    expected = _expected(models, {}, False)
    with _colour_codec(models, {}, False) as c:
        _check_step(models, c, c.submit(_feed(expected[0]['rgb'], False)), expected[0], 0)
        (real, calls) = (c.chroma.submit, [])

        def failing(plane):
            calls.append(plane)
            if len(calls) == 2:
                raise RuntimeError('injected')
            return real(plane)

        c.chroma.submit = failing
        try:
            with pytest.raises(RuntimeError, match='injected'):
                c.submit(_feed(expected[1]['rgb'], False))
        finally:
            del c.chroma.submit
        assert all(slot.free.is_set() for inner in (c.luma, c.chroma) for slot in inner._slots)        # drained
        steps = 3*c.depth + 1
        order = _schedule(c, steps)
        tickets = [c.submit(_feed(expected[batch]['rgb'], False)) for batch in order[:c.depth]]
        for (step, (ticket, batch)) in enumerate(zip(tickets, order)):
            _check_step(models, c, ticket, expected[batch], step)
        for (step, batch) in enumerate(order[c.depth:]):
            _check_step(models, c, c.submit(_feed(expected[batch]['rgb'], False)), expected[batch], c.depth + step)
