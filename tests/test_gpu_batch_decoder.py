"""`codec.BatchDecoder`: `EAE1` blobs in, reconstructions out, byte for byte what `container.decode_images` gives for the same blobs
-- launch by launch and replayed as hipGraphs, fetched to pinned memory and left on the device; steps whose images come from
different blobs, partial steps, slots that come round again, blobs straight out of `codec.BatchCodec(emit_container=True)`, and
a corrupted stream that must stay with its image."""
import os

import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coder_golden.npz')
BATCH = 3
SHAPES = [(64, 96), (48, 80)]          # map sizes 24 and 15: with 15 no stream piece is a multiple of 16 bytes


@pytest.fixture(scope='module')
def model():
    from autoencoder_based_image_compression_amd import pipeline
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    v = var.random_variables(1., False, seed=4, bias_std=0.01)
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    with numpy.load(GOLD) as g:
        probabilities = g['real_probabilities_1']
    return {'variables': v, 'encoder': pipeline.DeviceEncoder(v, False), 'decoder': pipeline.DeviceDecoder(v, False),
            'probabilities': probabilities, 'length': probabilities.shape[1], 'cache': {}}


def _images(shape, seed, count=BATCH):
    """Noise, a noisy ramp and a flat image: three different entropies."""
    rng = numpy.random.RandomState(seed)
    (h, w) = shape
    noise = rng.randint(16, 236, size=(h, w))
    ramp = numpy.clip(numpy.broadcast_to(16 + 219*numpy.arange(w)/(w - 1), (h, w)) + rng.randint(-4, 5, size=(h, w)), 16, 235)
    flat = numpy.full((h, w), 90 + seed % 50)
    return numpy.stack([(noise, ramp, flat)[i % 3] for i in range(count)]).astype(numpy.uint8)


def _encoded(model, shape, scale, idx_map_exception, seed=0, count=BATCH):
    """Once per case, shared by every test that needs it: (blob, `decode_images` of it)."""
    from autoencoder_based_image_compression_amd import container
    key = (shape, scale, idx_map_exception, seed, count)
    if key not in model['cache']:
        bin_widths = numpy.full(128, scale, dtype=numpy.float32)
        map_mean = numpy.random.RandomState(shape[1] + seed).normal(scale=0.1, size=128).astype(numpy.float32)
        (blob, _) = container.encode_images(_images(shape, seed, count), model['encoder'], bin_widths, map_mean, model['probabilities'],
                                            idx_map_exception)
        model['cache'][key] = (blob, container.decode_images(blob, model['decoder']))
    return model['cache'][key]


def _decoder(model, shape, **arguments):
    from autoencoder_based_image_compression_amd import codec
    # (these random weights code the small bin width at more than the default capacity's 8 bits per pixel)
    arguments.setdefault('payload_capacity_bytes', 4*BATCH*shape[0]*shape[1])
    arguments.setdefault('nb_in_flight', 2)
    arguments.setdefault('nb_streams', 1)
    return codec.BatchDecoder(model['variables'], False, BATCH, shape[0], shape[1], model['length'], **arguments)


def _array(result):
    return result.cpu().numpy() if isinstance(result, torch.Tensor) else numpy.array(result)


@pytest.mark.parametrize('fetch', [True, False])
@pytest.mark.parametrize('graphs', [False, True])
@pytest.mark.parametrize('scale,idx_map_exception', [(1.0, 67), (1.0, -1), (0.05, 67), (0.05, -1)])
@pytest.mark.parametrize('shape', SHAPES)
def test_a_blob_decodes_to_what_decode_images_gives(model, shape, scale, idx_map_exception, graphs, fetch):
    (blob, expected) = _encoded(model, shape, scale, idx_map_exception)
    with _decoder(model, shape, use_graphs=graphs, fetch_reconstruction=fetch) as decoder:
        for _ in range(3):                     # the launch-by-launch step, then (with graphs) replays of two slots
            ticket = decoder.submit(blob)
            result = ticket.result()
            assert isinstance(result, numpy.ndarray if fetch else torch.Tensor)
            assert result.shape == expected.shape and result.dtype == (numpy.uint8 if fetch else torch.uint8)
            assert numpy.array_equal(_array(result), expected)
            assert ticket.errors == [None]*BATCH and ticket.nb_images == BATCH


@pytest.mark.parametrize('graphs', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_mixed_and_partial_steps(model, shape, graphs):
    """Three single-image blobs at three bin widths, with two exception indices and without one, in one step; then two of three
    images (one blob of two, and two blobs of one); then one: every image equals `decode_images` of its own blob."""
    singles = [_encoded(model, shape, scale, idx, seed=seed, count=1) for (seed, (scale, idx)) in enumerate([(1.0, 67), (0.05, 5), (0.3, -1)])]
    (pair_blob, pair_expected) = _encoded(model, shape, 0.05, 67, seed=7, count=2)
    with _decoder(model, shape, use_graphs=graphs) as decoder:
        for order in ((0, 1, 2), (2, 0, 1)):
            result = decoder.submit([singles[k][0] for k in order]).result()
            assert result.shape == (3,) + shape
            for (position, k) in enumerate(order):
                assert numpy.array_equal(result[position], singles[k][1][0]), (order, position)
        ticket = decoder.submit(pair_blob)
        assert ticket.nb_images == 2 and numpy.array_equal(ticket.result(), pair_expected) and ticket.errors == [None, None]
        result = decoder.submit((singles[1][0], singles[0][0])).result()
        assert result.shape == (2,) + shape
        assert numpy.array_equal(result[0], singles[1][1][0]) and numpy.array_equal(result[1], singles[0][1][0])
        assert numpy.array_equal(decoder.submit(singles[2][0]).result(), singles[2][1])
        # the full step again, behind the partial ones
        result = decoder.submit([singles[k][0] for k in (0, 1, 2)]).result()
        assert all(numpy.array_equal(result[k], singles[k][1][0]) for k in range(3))


def test_slots_come_round_again_with_other_blobs(model):
    """3 x nb_slots steps alternating between two blob sets of different payload sizes, graphs on, two streams, the pipeline kept
    full: every ticket holds its own step's images (a pinned buffer or a head reused too early would show the other set's)."""
    shape = SHAPES[1]
    sets = [_encoded(model, shape, 0.05, 67), _encoded(model, shape, 1.0, -1, seed=3)]
    assert len(sets[0][0]) != len(sets[1][0]) and not numpy.array_equal(sets[0][1], sets[1][1])
    with _decoder(model, shape, use_graphs=True, nb_streams=2, nb_in_flight=3) as decoder:
        assert decoder.nb_slots == 3
        tickets = []
        checked = 0
        for step in range(3*decoder.nb_slots):
            tickets.append(decoder.submit(sets[step % 2][0]))
            while checked <= step - (decoder.nb_slots - 1):      # a result is valid until its slot is submitted again
                assert numpy.array_equal(tickets[checked].result(), sets[checked % 2][1]), checked
                checked += 1
        decoder.drain()
        for k in range(checked, len(tickets)):
            assert numpy.array_equal(tickets[k].result(), sets[k % 2][1]), k


@pytest.mark.parametrize('idx_map_exception', [67, -1])
def test_round_trip_through_the_pipelined_codec(model, idx_map_exception):
    """BatchCodec(emit_container=True) -> the step's blob and its per-image blobs -> BatchDecoder -> the codec's own reconstruction."""
    from autoencoder_based_image_compression_amd import codec
    shape = SHAPES[0]
    bin_widths = numpy.full(128, 0.5, dtype=numpy.float32)
    map_mean = numpy.random.RandomState(11).normal(scale=0.1, size=128).astype(numpy.float32)
    images = torch.from_numpy(_images(shape, 5)).cuda()
    with codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], idx_map_exception, BATCH, *shape,
                          keep_reconstruction=True, emit_container=True) as encoder:
        ticket = encoder.submit(images)
        ticket.result()
        (blob, image_blobs) = (ticket.container(), ticket.image_containers())
        reconstruction = ticket.reconstruction_uint8.cpu().numpy()
    with _decoder(model, shape, use_graphs=True) as decoder:
        assert numpy.array_equal(decoder.submit(blob).result(), reconstruction)
        assert numpy.array_equal(decoder.submit(image_blobs).result(), reconstruction)
        assert numpy.array_equal(decoder.submit(image_blobs[::-1]).result(), reconstruction[::-1])


def _outcome(call):
    try:
        return ('bytes', call())
    except Exception as exc:
        return ('error', type(exc), str(exc))


@pytest.mark.parametrize('graphs', [False, True])
def test_a_corrupted_stream_stays_with_its_image(model, graphs):
    """One image's payload altered as tests/test_container.py does (a byte flipped well inside an arithmetic-coded stream, the
    header still valid): that image's outcome is `decode_images`' on its own blob -- the same exception, or the same bytes --, its
    neighbours are their clean decode, and so is the next step."""
    from autoencoder_based_image_compression_amd import container
    shape = SHAPES[0]
    singles = [_encoded(model, shape, 0.05, 67, seed=20 + k, count=1) for k in range(3)]
    header = container.read_header(singles[1][0])
    sizes = (header['bits'].astype(numpy.int64) + 7)//8
    longest = int(numpy.argmax(sizes[:, 0]))
    assert sizes[longest, 0] >= 8
    position = header['payload_offset'] + int(sizes.reshape(-1)[:2*longest].sum()) + int(sizes[longest, 0])//2
    corrupted = bytearray(singles[1][0])
    corrupted[position] ^= 0xFF
    corrupted = bytes(corrupted)
    assert container.read_header(corrupted)['payload_offset'] == header['payload_offset']
    expected = _outcome(lambda: container.decode_images(corrupted, model['decoder']))
    with _decoder(model, shape, use_graphs=graphs) as decoder:
        for _ in range(2):
            ticket = decoder.submit([singles[0][0], corrupted, singles[2][0]])
            result = ticket.result(raise_errors=False)
            assert ticket.errors[0] is None and ticket.errors[2] is None
            assert numpy.array_equal(result[0], singles[0][1][0]) and numpy.array_equal(result[2], singles[2][1][0])
            if expected[0] == 'error':
                assert (type(ticket.errors[1]), str(ticket.errors[1])) == expected[1:]
                with pytest.raises(expected[1]):
                    ticket.result()
            else:
                assert ticket.errors[1] is None and numpy.array_equal(result[1], expected[1][0])
                assert not numpy.array_equal(result[1], singles[1][1][0])
            # the next step of this decoder is clean
            clean = decoder.submit([s[0] for s in singles])
            assert numpy.array_equal(clean.result(), numpy.concatenate([s[1] for s in singles])) and clean.errors == [None]*3


def test_refused_steps_and_lifetime(model):
    from autoencoder_based_image_compression_amd import codec, container
    shape = SHAPES[1]
    (blob, expected) = _encoded(model, shape, 1.0, 67)
    (other, _) = _encoded(model, SHAPES[0], 1.0, 67)
    tiled = container.encode_images(_images(shape, 0), model['encoder'], numpy.ones(128, dtype=numpy.float32), numpy.zeros(128, dtype=numpy.float32),
                                    model['probabilities'], 67, coding_tile=(2, 2))[0]
    decoder = _decoder(model, shape, payload_capacity_bytes=len(blob))
    assert decoder.payload_capacity_bytes == -(-len(blob)//16)*16
    for (bad, match) in ((other, 'images'), (tiled, 'decode_region'), ([blob, blob], 'images'), (blob[:-1], None)):
        with pytest.raises(ValueError, match=match):
            decoder.submit(bad)
    small = _decoder(model, shape, payload_capacity_bytes=64)
    with pytest.raises(ValueError, match='payload'):
        small.submit(blob)
    small.close()
    assert numpy.array_equal(decoder.submit(blob).result(), expected)          # a refused step leaves the decoder usable
    decoder.close()
    decoder.close()
    with pytest.raises(RuntimeError):
        decoder.submit(blob)
    with codec.BatchDecoder(model['variables'], False, 2, 32, 48, model['length'], nb_in_flight=1) as default:
        assert default.payload_capacity_bytes == 2*32*48 and default.nb_slots == 1
    for capacity in (0, -16):
        with pytest.raises(ValueError, match='payload_capacity_bytes'):
            codec.BatchDecoder(model['variables'], False, 2, 32, 48, model['length'], payload_capacity_bytes=capacity)
    # nothing asked for: the default streams are capped to the process's hardware queues without a warning, two more slots than streams
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        with codec.BatchDecoder(model['variables'], False, 1, 32, 48, model['length']) as default:
            assert 1 <= default.nb_streams <= codec.DECODER_STREAMS and default.nb_slots == default.nb_streams + 2
            assert default.nb_streams == codec.stream_budget(codec.DECODER_STREAMS, 1)[0]


def test_kodak_sized_steps_pipelined_on_two_streams(model):
    """The operating point itself: 24 images of 512x768 per step (the conv launches are cut, the coder runs its large-batch kernels,
    a step lasts milliseconds), four steps in flight on two streams, graphs on, with a one-image decoder on the same streams between
    the blocks. Steps that overlap on the device must not see each other: every step of every block reports no error, and the steps
    whose planes are still valid behind the drain hold the right bytes."""
    from autoencoder_based_image_compression_amd import codec, container
    (batch, shape) = (24, (512, 768))
    bin_widths = numpy.ones(128, dtype=numpy.float32)
    map_mean = numpy.random.RandomState(5).normal(scale=0.1, size=128).astype(numpy.float32)
    images = numpy.concatenate([_images(shape, seed, 3) for seed in range(batch//3)])
    (blob, _) = container.encode_images(images, model['encoder'], bin_widths, map_mean, model['probabilities'], 67)
    expected = container.decode_images(blob, model['decoder'])
    header = container.read_header(blob)
    singles = container.assemble_image_blobs(False, batch, shape[0], shape[1], 67, header['bin_widths'], header['map_mean'],
                                             header['binary_probabilities'], header['exception_probabilities'], header['bits'],
                                             blob[header['payload_offset']:])
    arguments = {'use_graphs': True, 'nb_streams': 2, 'nb_in_flight': 4}
    with codec.BatchDecoder(model['variables'], False, batch, shape[0], shape[1], model['length'], payload_capacity_bytes=len(blob), **arguments) as full, \
            codec.BatchDecoder(model['variables'], False, 1, shape[0], shape[1], model['length'], payload_capacity_bytes=len(blob), **arguments) as single:
        for block in range(3):
            tickets = [full.submit(blob) for _ in range(20)]
            full.drain()
            for (step, ticket) in enumerate(tickets):
                ticket.result(raise_errors=False)
                assert ticket.errors == [None]*batch, (block, step, [repr(e) for e in ticket.errors if e is not None][:3])
            for ticket in tickets[-full.nb_slots:]:
                assert numpy.array_equal(ticket.result(), expected), block
            tickets = [single.submit(singles[k % batch]) for k in range(24)]
            single.drain()
            for (k, ticket) in enumerate(tickets):
                ticket.result(raise_errors=False)
                assert ticket.errors == [None], (block, k, repr(ticket.errors[0]))
            for (k, ticket) in list(enumerate(tickets))[-single.nb_slots:]:
                assert numpy.array_equal(ticket.result(), expected[k % batch:k % batch + 1]), (block, k)
