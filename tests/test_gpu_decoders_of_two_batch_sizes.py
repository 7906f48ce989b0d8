"""Two resident decoders of different batch sizes in one process, their steps captured into hipGraphs, with `container.decode_images`
between their replays ("Fills inside a captured step"). Every step of every decoder must report no error and
decode to `decode_images`' bytes, whichever decoder captured or ran last. With `hipMemsetAsync` for the fills at the start of
`eae_hip_decode` and of a pure `eae_hip_coder_decode_batch`, the replays of the 24-image decoder came back, once the one-image decoder
had captured its steps, with every status of a slot nonzero and a failure word that is no count (10 of 12 steps of the untiled
decoder, 12 of 12 behind a `decode_images` call), while the same steps issued launch by launch were right. Untiled and in tiles of
16: the tiled decoder runs the same two entry points."""
import os

import numpy
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coder_golden.npz')
(BATCH, SHAPE, STEPS) = (24, (512, 768), 12)


def _images(seed, count):
    rng = numpy.random.RandomState(seed)
    (h, w) = SHAPE
    noise = rng.randint(16, 236, size=(h, w))
    ramp = numpy.clip(numpy.broadcast_to(16 + 219*numpy.arange(w)/(w - 1), (h, w)) + rng.randint(-4, 5, size=(h, w)), 16, 235)
    flat = numpy.full((h, w), 90 + seed % 50)
    return numpy.stack([(noise, ramp, flat)[i % 3] for i in range(count)]).astype(numpy.uint8)


def _run(decoder, blobs, expected, name):
    """STEPS steps in flight, a drain: no step may report an error; the steps whose planes are still valid hold the right bytes."""
    tickets = [decoder.submit(blobs[k % len(blobs)]) for k in range(STEPS)]
    decoder.drain()
    for (k, ticket) in enumerate(tickets):
        ticket.result(raise_errors=False)
        assert ticket._error is None, (name, k, repr(ticket._error))
        assert all(error is None for error in ticket.errors), (name, k, [repr(e) for e in ticket.errors if e is not None][:2])
    for k in range(STEPS - decoder.nb_slots, STEPS):
        assert numpy.array_equal(tickets[k].result(), expected(k)), (name, k)


@pytest.mark.parametrize('tile', [None, (16, 16)])
def test_replays_of_one_decoder_behind_captures_and_calls_of_another_size(tile):
    from autoencoder_based_image_compression_amd import codec, container, pipeline
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    v = var.random_variables(1., False, seed=4, bias_std=0.01)
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    with numpy.load(GOLD) as g:
        probabilities = g['real_probabilities_1']
    (encoder, model) = (pipeline.DeviceEncoder(v, False), pipeline.DeviceDecoder(v, False))
    bin_widths = numpy.ones(128, dtype=numpy.float32)
    map_mean = numpy.random.RandomState(5).normal(scale=0.1, size=128).astype(numpy.float32)
    images = numpy.concatenate([_images(seed, 3) for seed in range(BATCH//3)])
    (blob, _) = container.encode_images(images, encoder, bin_widths, map_mean, probabilities, 67, coding_tile=tile)
    singles = [container.encode_images(images[k:k + 1], encoder, bin_widths, map_mean, probabilities, 67, coding_tile=tile)[0] for k in range(4)]
    expected = container.decode_images(blob, model)

    def whole(k):
        return expected

    def one(k):
        return expected[k % len(singles):k % len(singles) + 1]

    def build(n):
        return codec.BatchDecoder(v, False, n, SHAPE[0], SHAPE[1], probabilities.shape[1], payload_capacity_bytes=len(blob), use_graphs=True,
                                  nb_streams=2, nb_in_flight=4, coding_tile=tile)

    with build(BATCH) as full:
        _run(full, [blob], whole, 'the 24-image decoder, alone')
        with build(1) as single:
            _run(single, singles, one, 'the one-image decoder')
            _run(full, [blob], whole, 'the 24-image decoder behind the one-image decoder\'s captures')
            _run(single, singles, one, 'the one-image decoder again')
            assert numpy.array_equal(container.decode_images(blob, model), expected)
            _run(single, singles, one, 'the one-image decoder behind decode_images of 24')
            _run(full, [blob], whole, 'the 24-image decoder behind decode_images of 24')
            assert numpy.array_equal(container.decode_images(singles[1], model), expected[1:2])
            _run(single, singles, one, 'the one-image decoder behind decode_images of one')
            _run(full, [blob], whole, 'the 24-image decoder behind decode_images of one')
