"""`codec.ColourDecoder`: `EAC1` blobs of three 99 x 165 RGB pictures through two `BatchDecoder(pad=True,
keep_reconstruction=True)` and one `device.colour_merge_420_words` launch per step, against `container.decode_colour_images` of the
same blobs, byte for byte.

In every mode below -- launch by launch with the decoder's own defaults, replayed graphs, the result left on the device, coding tiles
of (2, 3) with graphs, chroma at doubled bin widths --, over 3 * depth + 1 consecutive steps with `depth` of them pending at any time,
the steps go through four different batches in the order of tests/test_gpu_colour_codec.py's `_schedule`: no step takes the batch of
the step before it, nor the batch that its ring entry, its luminance slot or its pair of chroma slots held the time before, so a merge
that ran after an inner slot came round, or a colour slot that was not rewritten, would be another picture. The same sequence runs
with no ticket touched until all of it is submitted. Then: a step of three single-picture blobs at two rate points, a partial step,
a corrupted Cb stream, a `submit` that fails half way, a sequence on guard-banded buffers with the colour ring and the inner
decoders' scratch (tests/slot_buffers.py) poisoned between the steps under two poisons, the refusals, and
`BatchDecoder(keep_reconstruction=True)` on its own."""
import numpy
import pytest
import torch

import guarded
import slot_buffers
from test_gpu_colour_codec import _schedule
from test_gpu_colour_container import pictures_of, points_of
from test_gpu_frame_container import arguments_of, images_of, models  # noqa: F401 (`models` is a fixture)

pytestmark = pytest.mark.gpu

N = 3
SIZE = (99, 165)
CHROMA = (50, 83)
RATE = 'L10_exception_67'
LENGTH = 10
POISONS = (0xFF, 0x7F)
NB_BATCHES = 4
# name: (ColourDecoder arguments, what the blobs are coded with, chroma at doubled bin widths)
MODES = {
    'launches_defaults': ({}, {}, False),
    'graphs': ({'use_graphs': True, 'nb_in_flight': 2}, {}, False),
    'device_result': ({'fetch_reconstruction': False, 'nb_in_flight': 2}, {}, False),
    'tiles_2x3_graphs': ({'coding_tile': (2, 3), 'use_graphs': True, 'nb_in_flight': 2}, {'coding_tile': (2, 3)}, False),
    'chroma_doubled': ({'nb_in_flight': 2}, {}, True),
}


def _decoder(models, **more):
    from autoencoder_based_image_compression_amd import codec
    return codec.ColourDecoder(models[False]['variables'], False, N, SIZE[0], SIZE[1], LENGTH, **more)


def _encode(models, rgb, doubled=False, coarse=False, **coded):
    """(EAC1 blob, `decode_colour_images` of it); coarse: luminance and chroma at doubled bin widths, another rate point."""
    from autoencoder_based_image_compression_amd import container
    (encoder, luma, chroma) = points_of(models, False, RATE, doubled)
    if coarse:
        luma = (luma[0]*numpy.float32(2.),) + luma[1:]
    blob = container.encode_colour_images(rgb, encoder, *luma, chroma=chroma, **coded)[0]
    return (blob, container.decode_colour_images(blob, models[False]['decoder']))


def _batches(models, coded, doubled):
    """For the four batches: (blob, expected pictures), once per way of coding them."""
    key = ('colour_decoder_batches', tuple(sorted(coded.items())), doubled)
    if key not in models:
        out = [_encode(models, pictures_of(SIZE, seed, N), doubled, **coded) for seed in range(NB_BATCHES)]
        for a in range(NB_BATCHES):
            assert out[a][1].shape == (N,) + SIZE + (3,) and out[a][1].dtype == numpy.uint8
            assert all(not numpy.array_equal(out[a][1], out[b][1]) for b in range(a))
        models[key] = out
    return models[key]


def _array(value):
    return value.cpu().numpy() if isinstance(value, torch.Tensor) else value


def _check_step(d, ticket, expected, step, pictures=True):
    value = ticket.result()
    assert ticket.errors == [None]*ticket.nb_images and ticket.merged_event.query(), step
    assert len(ticket.tickets) == 3 and all(inner.errors == [None]*ticket.nb_images for inner in ticket.tickets)
    assert (isinstance(value, numpy.ndarray) and value.dtype == numpy.uint8) if d.fetch_reconstruction else (value.is_cuda and value.dtype == torch.uint8)
    assert tuple(value.shape) == expected.shape, step
    if pictures:                                         # valid until the colour slot comes round
        assert numpy.array_equal(_array(value), expected), step


@pytest.mark.parametrize('mode', sorted(MODES))
def test_colour_steps_equal_decode_colour_images(models, mode):
    (more, coded, doubled) = MODES[mode]
    batches = _batches(models, coded, doubled)
    with _decoder(models, **more) as d:
        assert d.depth == min(d.luma.nb_slots, d.chroma.nb_slots//2) >= 1 and len(d._steps) == d.depth
        assert d.chroma.nb_in_flight == 2*d.luma.nb_in_flight and d.luma.nb_streams == d.chroma.nb_streams
        assert (d.luma.image_size, d.chroma.image_size) == (SIZE, CHROMA) and d.luma.pad and d.chroma.pad
        assert not d.luma.fetch_reconstruction and not d.chroma.fetch_reconstruction and d.luma.keep_reconstruction
        assert all((step.pinned if d.fetch_reconstruction else step.device).numel() == -(-N*SIZE[0]*SIZE[1]*3//16)*16 for step in d._steps)
        steps = 3*d.depth + 1
        order = _schedule(d, steps)
        tickets = []
        for step in range(steps):
            tickets.append(d.submit(batches[order[step]][0]))
            assert tickets[-1].nb_images == N
            # the oldest step whose ring entry the next submit takes: looked at while it and the `depth` - 1 steps behind it are pending
            oldest = step - d.depth + 1
            if oldest >= 0:
                _check_step(d, tickets[oldest], batches[order[oldest]][1], oldest)
        for oldest in range(steps - d.depth + 1, steps):
            _check_step(d, tickets[oldest], batches[order[oldest]][1], oldest)
    d.close()                                            # idempotent


@pytest.mark.parametrize('mode', ['launches_defaults', 'tiles_2x3_graphs'])
def test_results_collected_late(models, mode):
    """No ticket is touched until every step is submitted: `submit` itself waited for the merges whose slots it took. The pictures of
    the last `depth` steps are still in their slots; the errors of every step are its own."""
    (more, coded, doubled) = MODES[mode]
    batches = _batches(models, coded, doubled)
    with _decoder(models, **more) as d:
        steps = 3*d.depth + 1
        order = _schedule(d, steps)
        tickets = [d.submit(batches[batch][0]) for batch in order]
        for (step, (ticket, batch)) in enumerate(zip(tickets, order)):
            _check_step(d, ticket, batches[batch][1], step, pictures=step >= steps - d.depth)


def test_single_picture_blobs_at_two_rate_points_and_a_partial_step(models):
    rgb = pictures_of(SIZE, 11, N)
    singles = [_encode(models, rgb[i:i + 1], coarse=(i == 1)) for i in range(N)]
    fine = _encode(models, rgb[1:2])
    assert not numpy.array_equal(singles[1][1], fine[1])                      # another rate point, other pictures
    batches = _batches(models, {}, False)
    pair = _encode(models, rgb[:2])
    with _decoder(models, nb_in_flight=2) as d:
        ticket = d.submit([blob for (blob, _) in singles])
        assert ticket.nb_images == N
        _check_step(d, ticket, numpy.concatenate([pictures for (_, pictures) in singles]), 0)
        # one blob of two pictures, then one of two and one of one, then two pictures alone again
        partial = d.submit(pair[0])
        assert partial.nb_images == 2 and partial.result().shape == (2,) + SIZE + (3,)
        _check_step(d, partial, pair[1], 1)
        _check_step(d, d.submit([pair[0], singles[2][0]]), numpy.concatenate([pair[1], singles[2][1]]), 2)
        _check_step(d, d.submit(batches[0][0]), batches[0][1], 3)             # the next full step is clean
        _check_step(d, d.submit([singles[1][0], singles[0][0]]), numpy.concatenate([singles[1][1], singles[0][1]]), 4)
        _check_step(d, d.submit(batches[1][0]), batches[1][1], 5)


def _outcome(call):
    try:
        return ('bytes', call())
    except Exception as exc:
        return ('error', type(exc), str(exc))


@pytest.mark.parametrize('graphs', [False, True], ids=['launches', 'graphs'])
def test_a_corrupted_cb_stream_stays_with_its_picture(models, graphs):
    """A byte flipped in the middle of the longest arithmetic-coded stream of picture 1's Cb plane, chosen as
    tests/test_gpu_batch_decoder.py chooses it: that picture's outcome is `decode_colour_images`' on its own corrupted blob -- the same
    exception type, or the same bytes --, pictures 0 and 2 and the next step are clean."""
    from autoencoder_based_image_compression_amd import container
    rgb = pictures_of(SIZE, 21, N)
    singles = [_encode(models, rgb[i:i + 1]) for i in range(N)]
    (_, y_blob, cb_blob, cr_blob) = container.split_colour_blob(singles[1][0])
    header = container.read_header(cb_blob)
    sizes = (header['bits'].astype(numpy.int64) + 7)//8
    longest = int(numpy.argmax(sizes[:, 0]))
    assert sizes[longest, 0] >= 8
    position = header['payload_offset'] + int(sizes.reshape(-1)[:2*longest].sum()) + int(sizes[longest, 0])//2
    corrupted = bytearray(cb_blob)
    corrupted[position] ^= 0xFF
    assert container.read_header(bytes(corrupted))['payload_offset'] == header['payload_offset']
    corrupted = container.assemble_colour_blob(SIZE, y_blob, bytes(corrupted), cr_blob)
    expected = _outcome(lambda: container.decode_colour_images(corrupted, models[False]['decoder']))
    with _decoder(models, use_graphs=graphs, nb_in_flight=2) as d:
        for _ in range(2):
            ticket = d.submit([singles[0][0], corrupted, singles[2][0]])
            result = ticket.result(raise_errors=False)
            assert ticket.errors[0] is None and ticket.errors[2] is None
            assert numpy.array_equal(result[0], singles[0][1][0]) and numpy.array_equal(result[2], singles[2][1][0])
            if expected[0] == 'error':
                assert type(ticket.errors[1]) is expected[1]
                assert ticket.errors[1] is ticket.tickets[1].errors[1] and ticket.tickets[0].errors[1] is None
                with pytest.raises(expected[1]):
                    ticket.result()
            else:
                assert ticket.errors[1] is None and numpy.array_equal(result[1], expected[1][0])
                assert not numpy.array_equal(result[1], singles[1][1][0])
            clean = d.submit([blob for (blob, _) in singles])
            _check_step(d, clean, numpy.concatenate([pictures for (_, pictures) in singles]), 1)


def test_a_submit_that_fails_half_way_leaves_a_working_decoder(models):
    """The Cr submit raises after the luminance and Cb steps were queued: `submit` re-raises behind a drain, and the steps that
    follow -- on a chroma ring now one step out of pairs -- are right."""
    batches = _batches(models, {}, False)
    with _decoder(models, nb_in_flight=2) as d:
        _check_step(d, d.submit(batches[0][0]), batches[0][1], 0)
        (real, calls) = (d.chroma.submit, [])

        def failing(blobs):
            calls.append(blobs)
            if len(calls) == 2:
                raise RuntimeError('injected')
            return real(blobs)

        d.chroma.submit = failing
        try:
            with pytest.raises(RuntimeError, match='injected'):
                d.submit(batches[1][0])
        finally:
            del d.chroma.submit
        assert all(slot.free.is_set() for inner in (d.luma, d.chroma) for slot in inner._slots)        # drained
        steps = 3*d.depth + 1
        order = _schedule(d, steps)
        tickets = [d.submit(batches[batch][0]) for batch in order[:d.depth]]
        for (step, (ticket, batch)) in enumerate(zip(tickets, order)):
            _check_step(d, ticket, batches[batch][1], step)
        for (step, batch) in enumerate(order[d.depth:]):
            _check_step(d, d.submit(batches[batch][0]), batches[batch][1], d.depth + step)


def _poison_rings(d, guard, poison):
    d.drain()
    guard.check(keep=True)
    for inner in (d.luma, d.chroma):
        assert slot_buffers.poison_scratch(inner, poison) > 0
    for ring in d._steps:
        slot_buffers.fill_bytes(ring.pinned if ring.pinned is not None else ring.device, poison)
    torch.cuda.synchronize()


@pytest.mark.parametrize('mode', ['launches_fetched', 'graphs_on_device'])
def test_colour_steps_on_poisoned_rings(models, mode):
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    batches = _batches(models, {}, False)
    more = {'launches_fetched': {}, 'graphs_on_device': {'use_graphs': True, 'fetch_reconstruction': False}}[mode]
    pair = _encode(models, pictures_of(SIZE, 5, N)[:2])
    seen = {}
    for poison in POISONS:
        with guarded.guarded((device, pipeline, codec), poison) as guard:
            with _decoder(models, nb_in_flight=2, **more) as d:
                torch.cuda.synchronize()
                _poison_rings(d, guard, poison)
                values = []
                for step in range(2*d.depth + 2):
                    (blob, expected) = batches[(step//d.depth) % NB_BATCHES] if step != d.depth else pair      # one partial step
                    ticket = d.submit(blob)
                    _check_step(d, ticket, expected, step)
                    values.append(_array(ticket.result()).tobytes())
                    if step == d.depth:
                        # behind the last word of two pictures the slot still holds the poison
                        whole = _array(d._steps[step % d.depth].pinned if d.fetch_reconstruction else d._steps[step % d.depth].device)
                        written = -(-expected.size//16)*16
                        assert not whole[expected.size:written].any() and (whole[written:] == poison).all()
                    _poison_rings(d, guard, poison)
        seen[poison] = values
    assert seen[POISONS[0]] == seen[POISONS[1]]


def test_what_is_refused(models):
    from autoencoder_based_image_compression_amd import codec, container
    variables = models[False]['variables']
    batches = _batches(models, {}, False)
    tiled = _batches(models, {'coding_tile': (2, 3)}, False)
    # a chroma decoder of one slot cannot hold Cb and Cr of one colour step
    with pytest.raises(ValueError, match='cannot hold'):
        _decoder(models, chroma_options={'nb_in_flight': 1})
    for bad in ({'use_graphs': True}, {'fetch_reconstruction': False}, {'coding_tile': (2, 3)}, {'pad': True}, {'device': 'cuda'}):
        with pytest.raises(ValueError, match='chroma_options'):
            _decoder(models, chroma_options=bad)
    with pytest.raises(ValueError):
        codec.ColourDecoder(variables, False, N, 0, SIZE[1], LENGTH)
    with pytest.raises(ValueError):
        codec.ColourDecoder(variables, False, 0, SIZE[0], SIZE[1], LENGTH)
    other = _encode(models, pictures_of((100, 166), 0, N))[0]
    with _decoder(models, nb_in_flight=2, chroma_options={'nb_in_flight': 3, 'nb_streams': 1, 'payload_capacity_bytes': 1 << 20,
                                                         'truncated_unary_length': LENGTH}) as d:
        assert d.chroma.nb_in_flight == 3 and d.depth == 1 and d.chroma.payload_capacity_bytes == 1 << 20
        for bad in (container.split_colour_blob(batches[0][0])[1],          # an EAE1 plane blob, not an EAC1
                    batches[0][0][:-1], b'', other,                         # truncated, empty, another size
                    [batches[0][0], batches[1][0]],                         # six pictures
                    [], tiled[0][0]):                                       # none; planes coded in tiles
            with pytest.raises(ValueError):
                d.submit(bad)
        _check_step(d, d.submit(batches[2][0]), batches[2][1], 0)           # and goes on working
    with _decoder(models, nb_in_flight=2, coding_tile=(2, 3)) as d:
        with pytest.raises(ValueError, match='coding_tile'):
            d.submit(batches[0][0])                                         # EAE1 planes given to a decoder of tiles
        assert all(slot.free.is_set() for inner in (d.luma, d.chroma) for slot in inner._slots)
        _check_step(d, d.submit(tiled[1][0]), tiled[1][1], 0)
    with pytest.raises(RuntimeError, match='closed'):
        d.submit(tiled[1][0])
    with pytest.raises(TypeError):
        codec.RegionDecoder(variables, False, 1, 112, 176, LENGTH, (2, 3), (32, 32), keep_reconstruction=True)


def test_batch_decoder_keeps_its_reconstruction(models):
    """`BatchDecoder(keep_reconstruction=True)`: `reconstruction_uint8`, read behind `decoded_event` on another stream, is `result()`,
    with `pad` (the top-left view of the coded planes) and without, launch by launch and replayed; without the keyword neither
    attribute exists."""
    from autoencoder_based_image_compression_amd import codec, container
    variables = models[False]['variables']
    (encoder, bin_widths, map_mean, probabilities, idx_map_exception) = arguments_of(models, False, RATE)
    cases = []
    for (size, pad) in ((SIZE, True), ((112, 176), False)):
        blobs = [container.encode_images(images_of(size, seed, N), encoder, bin_widths, map_mean, probabilities, idx_map_exception, pad=pad)[0]
                 for seed in (0, 1)]
        cases.append((size, pad, blobs, [container.decode_images(blob, models[False]['decoder']) for blob in blobs]))
    side = torch.cuda.Stream()
    for (size, pad, blobs, expected) in cases:
        two = container.encode_images(images_of(size, 2, 2), encoder, bin_widths, map_mean, probabilities, idx_map_exception, pad=pad)[0]
        two_expected = container.decode_images(two, models[False]['decoder'])
        for graphs in (False, True):
            with codec.BatchDecoder(variables, False, N, size[0], size[1], LENGTH, pad=pad, use_graphs=graphs, nb_in_flight=2,
                                    keep_reconstruction=True) as d:
                for step in range(5):
                    ticket = d.submit(blobs[step % 2])
                    with torch.cuda.stream(side):
                        side.wait_event(ticket.decoded_event)
                        kept = ticket.reconstruction_uint8.clone()
                    side.synchronize()
                    assert ticket.reconstruction_uint8.is_cuda and tuple(ticket.reconstruction_uint8.shape) == (N,) + size
                    assert ticket.reconstruction_uint8.is_contiguous() == (not pad)
                    assert numpy.array_equal(kept.cpu().numpy(), expected[step % 2]), (size, graphs, step)
                    assert numpy.array_equal(ticket.result(), expected[step % 2])
                partial = d.submit(two)
                assert tuple(partial.reconstruction_uint8.shape) == (2,) + size
                assert numpy.array_equal(partial.result(), two_expected) and numpy.array_equal(partial.reconstruction_uint8.cpu().numpy(), two_expected)
        with codec.BatchDecoder(variables, False, N, size[0], size[1], LENGTH, pad=pad, nb_in_flight=2) as d:
            ticket = d.submit(blobs[0])
            assert not hasattr(ticket, 'decoded_event') and not hasattr(ticket, 'reconstruction_uint8') and not d.keep_reconstruction
            assert numpy.array_equal(ticket.result(), expected[0])
