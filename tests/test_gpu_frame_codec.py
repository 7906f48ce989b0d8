"""`codec.BatchCodec(pad=True)` and `codec.BatchDecoder(pad=True)`: images of 50 x 83, coded as 64 x 96.

The codec: in every mode below, over three consecutive steps of different images (a stale padded input would show), every key of
`result()` equals the same codec built at 64 x 96 on the numpy-edge-padded batch, except 'sse', which is numpy's on the crop of
that codec's kept reconstruction against the real input; the containers are byte for byte `container.encode_images(..., pad=True)`;
the reconstruction is (3, 50, 83), the crop. The decoder: `result()` equals `container.decode_images` on those blobs, whole, in
single-image blobs, in a partial step and in coding tiles; a blob of another crop and a decoder without `pad` refuse in `submit`; a
corrupted stream fails its own image only. The combinations that are out of scope raise ValueError. Last, a step sequence of each
on poisoned, guard-banded slots as tests/test_gpu_codec_slots.py runs them, with the buffers the feature adds poisoned here."""
import numpy
import pytest
import torch

import guarded
import slot_buffers
from test_gpu_frame_container import CODED, N, arguments_of, edge_padded, images_of, models  # noqa: F401 (`models` is a fixture)

pytestmark = pytest.mark.gpu

SIZE = (50, 83)
RATE = 'L10_exception_67'
POISONS = (0xFF, 0x7F)
KEYS = ('nb_bits', 'coder_bits', 'exception_bits', 'nb_deads')
# name: (BatchCodec arguments, feed pinned host batches)
CODEC_MODES = {
    'launches': ({}, False),
    'graphs_two_streams': ({'use_graphs': True, 'nb_transform_streams': 2}, False),
    'one_stream_graphs': ({'use_graphs': True, 'nb_transform_streams': 2, 'one_stream_steps': True}, False),
    'container': ({'emit_container': True}, False),
    'container_tiles_2x3': ({'emit_container': True, 'coding_tile': (2, 3)}, False),
    'container_graphs_pinned': ({'emit_container': True, 'use_graphs': True}, True),
    'fetch_pinned': ({'fetch_reconstruction': True}, True),
    'rdo': ({'emit_container': True, 'rdo_lambda': 0.02}, False),
}


def _codec(models, learned, size, pad, **arguments):
    from autoencoder_based_image_compression_amd import codec
    (_, bin_widths, map_mean, probabilities, idx_map_exception) = arguments_of(models, learned, RATE)
    if arguments.get('emit_container'):
        arguments = dict(arguments, container_capacity_bytes=8*N*CODED[0]*CODED[1])
    if pad:
        arguments = dict(arguments, pad=True)
    return codec.BatchCodec(models[learned]['variables'], learned, bin_widths, map_mean, probabilities, idx_map_exception, N, size[0], size[1],
                            nb_in_flight=2, keep_reconstruction=True, **arguments)


def _feed(images, host):
    tensor = torch.from_numpy(images)
    return tensor.pin_memory() if host else tensor.cuda()


def _real_sse(images, reconstruction):
    (h, w) = images.shape[1:]
    difference = images.astype(numpy.int64) - reconstruction[:, :h, :w].astype(numpy.int64)
    return (difference*difference).sum(axis=(1, 2))


def _check_step(models, learned, padded_codec, reference_codec, images, host, more):
    """One step of both codecs; returns the padded codec's blobs (or None)."""
    from autoencoder_based_image_compression_amd import container
    (h, w) = SIZE
    fed = _feed(images, host)
    ticket = padded_codec.submit(fed)
    reference_ticket = reference_codec.submit(_feed(edge_padded(images), False))
    (r, reference) = (ticket.result(), reference_ticket.result())
    assert sorted(r) == sorted(reference)
    whole = reference_ticket.reconstruction_uint8.cpu().numpy()
    for key in r:
        if key != 'sse':
            assert numpy.array_equal(r[key], reference[key]), key
    assert numpy.array_equal(reference['sse'], _real_sse(edge_padded(images), whole))          # the reference codec's, over 64 x 96
    assert numpy.array_equal(r['sse'], _real_sse(images, whole)) and r['sse'].dtype == reference['sse'].dtype
    assert (r['sse'] < reference['sse']).any()                                                  # the padding's error is not in it
    reconstruction = ticket.reconstruction_uint8
    assert tuple(reconstruction.shape) == (N, h, w) and numpy.array_equal(reconstruction.cpu().numpy(), whole[:, :h, :w])
    if padded_codec.fetch_reconstruction:
        assert ticket.reconstruction_host.shape == (N, h, w) and numpy.array_equal(ticket.reconstruction_host, whole[:, :h, :w])
    if not padded_codec.emit_container:
        return None
    arguments = arguments_of(models, learned, RATE)
    extra = {key: more[key] for key in ('coding_tile', 'rdo_lambda') if key in more}
    assert ticket.container() == container.encode_images(images, *arguments, pad=True, **extra)[0]
    blobs = ticket.image_containers()
    assert blobs == [container.encode_images(images[i:i + 1], *arguments, pad=True, **extra)[0] for i in range(N)]
    # the same bytes as the unpadded codec's but for the crop
    for (blob, other) in zip(blobs, reference_ticket.image_containers()):
        assert blob[:23] == other[:23] and blob[24:] == other[24:] and blob[23] == (14 << 4 | 13) and other[23] == 0
    return blobs


# every mode with fixed bin widths; with learned ones the three that differ in how the latent stage is launched
CODEC_CASES = [(False, mode) for mode in sorted(CODEC_MODES)] + [(True, mode) for mode in ('launches', 'graphs_two_streams', 'container')]


@pytest.mark.parametrize('learned,mode', CODEC_CASES, ids=['{0}-{1}'.format('learned' if learned else 'fixed', mode) for (learned, mode) in CODEC_CASES])
def test_padded_codec_equals_the_codec_of_the_padded_batch(models, learned, mode):
    (more, host) = CODEC_MODES[mode]
    with _codec(models, learned, SIZE, True, **more) as padded_codec, _codec(models, learned, CODED, False, **more) as reference_codec:
        assert (padded_codec.h_in, padded_codec.w_in, padded_codec.h_image, padded_codec.w_image) == CODED + SIZE
        for seed in (0, 1, 0):
            _check_step(models, learned, padded_codec, reference_codec, images_of(SIZE, seed), host, more)


def test_a_padded_codec_at_a_multiple_of_16_is_the_codec(models):
    from autoencoder_based_image_compression_amd import codec
    images = images_of(CODED, 2)
    with _codec(models, False, CODED, True, emit_container=True) as padded_codec, _codec(models, False, CODED, False, emit_container=True) as plain:
        (a, b) = (padded_codec.submit(_feed(images, False)), plain.submit(_feed(images, False)))
        (ra, rb) = (a.result(), b.result())
        assert sorted(ra) == sorted(rb) and all(numpy.array_equal(ra[key], rb[key]) for key in ra)
        assert a.container() == b.container() and a.image_containers() == b.image_containers()
        assert numpy.array_equal(a.reconstruction_uint8.cpu().numpy(), b.reconstruction_uint8.cpu().numpy())
        with pytest.raises(ValueError):
            padded_codec.submit(_feed(images_of(SIZE), False))
    # real sizes in, the coded size's answer out
    assert codec.default_nb_in_flight(*SIZE) == codec.default_nb_in_flight(*CODED)
    assert codec.default_nb_in_flight(500, 750) == codec.default_nb_in_flight(512, 752)
    assert codec.product_mode(500, 750) == codec.product_mode(512, 752)


# ---- BatchDecoder(pad=True) --------------------------------------------------------------------------------------------------------

def _array(result):
    return result.cpu().numpy() if isinstance(result, torch.Tensor) else numpy.array(result)


def _blobs(models, size, seed, coding_tile=None, count=N):
    from autoencoder_based_image_compression_amd import container
    more = {} if coding_tile is None else {'coding_tile': coding_tile}
    key = ('frame_blobs', size, seed, coding_tile, count)
    if key not in models:
        arguments = arguments_of(models, False, RATE)
        images = images_of(size, seed, count)
        blob = container.encode_images(images, *arguments, pad=size != CODED, **more)[0]
        singles = [container.encode_images(images[i:i + 1], *arguments, pad=size != CODED, **more)[0] for i in range(count)]
        models[key] = (blob, singles, container.decode_images(blob, models[False]['decoder']))
    return models[key]


def _decoder(models, size, pad=True, **arguments):
    from autoencoder_based_image_compression_amd import codec
    return codec.BatchDecoder(models[False]['variables'], False, N, size[0], size[1], 10, nb_in_flight=2, payload_capacity_bytes=8*N*CODED[0]*CODED[1],
                              pad=pad, **arguments)


@pytest.mark.parametrize('fetch', [True, False], ids=['fetched', 'on_device'])
@pytest.mark.parametrize('graphs', [False, True], ids=['launches', 'graphs'])
@pytest.mark.parametrize('coding_tile', [None, (2, 3)], ids=['EAE1', 'tiles_2x3'])
def test_padded_decoder_equals_decode_images(models, coding_tile, graphs, fetch):
    (blob, singles, expected) = _blobs(models, SIZE, 0, coding_tile)
    (other_blob, other_singles, other) = _blobs(models, SIZE, 1, coding_tile)
    assert expected.shape == (N,) + SIZE and not numpy.array_equal(expected, other)
    with _decoder(models, SIZE, use_graphs=graphs, fetch_reconstruction=fetch, coding_tile=coding_tile) as decoder:
        assert (decoder.h_in, decoder.w_in, decoder.image_size) == CODED + (SIZE,)
        for (step, (blobs, images)) in enumerate(((blob, expected), (other_singles, other), (singles[::-1], expected[::-1]),
                                                  (other_singles[:2], other[:2]), (blob, expected))):      # a partial step among them
            ticket = decoder.submit(blobs)
            result = ticket.result()
            assert isinstance(result, numpy.ndarray if fetch else torch.Tensor), step
            assert tuple(result.shape) == images.shape and numpy.array_equal(_array(result), images), step
            assert ticket.errors == [None]*images.shape[0]


def test_the_decoders_refuse_another_crop(models):
    from autoencoder_based_image_compression_amd import codec
    (blob, singles, expected) = _blobs(models, SIZE, 0)
    (narrower, _, _) = _blobs(models, (49, 96), 0)
    (plain, _, plain_expected) = _blobs(models, CODED, 0)
    (tiled, _, _) = _blobs(models, SIZE, 0, (2, 3))
    with _decoder(models, SIZE) as decoder:
        for refused in (narrower, plain, [singles[0], narrower], tiled):
            with pytest.raises(ValueError):
                decoder.submit(refused)
        assert numpy.array_equal(decoder.submit(blob).result(), expected)          # and goes on working
    with _decoder(models, CODED, pad=False) as decoder:
        with pytest.raises(ValueError, match='crop'):
            decoder.submit(blob)
        assert numpy.array_equal(decoder.submit(plain).result(), plain_expected)
    with _decoder(models, CODED, pad=True) as decoder:                             # a padded decoder at a multiple of 16 takes crop 0 only
        with pytest.raises(ValueError, match='crop'):
            decoder.submit(blob)
        assert numpy.array_equal(decoder.submit(plain).result(), plain_expected)
    with pytest.raises(ValueError, match='crop'):
        codec.RegionSource(tiled)
    codec.RegionSource(_blobs(models, CODED, 0, (2, 3))[0])


def test_a_corrupted_stream_fails_its_own_image_only(models):
    from autoencoder_based_image_compression_amd import container
    (_, singles, expected) = _blobs(models, SIZE, 0)
    header = container.read_header(singles[1])
    sizes = (header['bits'].astype(numpy.int64) + 7)//8
    outcome = None
    for longest in numpy.argsort(-sizes[:, 0], kind='stable')[:8]:
        position = header['payload_offset'] + int(sizes.reshape(-1)[:2*int(longest)].sum()) + int(sizes[longest, 0])//2
        corrupted = bytearray(singles[1])
        corrupted[position] ^= 0xFF
        corrupted = bytes(corrupted)
        try:
            outcome = ('bytes', container.decode_images(corrupted, models[False]['decoder']))
        except Exception as exc:
            outcome = ('error', type(exc), str(exc))
        if outcome[0] == 'error' or not numpy.array_equal(outcome[1], expected[1:2]):
            break
    else:
        raise AssertionError('no flipped byte changed what decode_images gives')
    with _decoder(models, SIZE) as decoder:
        ticket = decoder.submit([singles[0], corrupted, singles[2]])
        result = ticket.result(raise_errors=False)
        assert result.shape == (N,) + SIZE and ticket.errors[0] is None and ticket.errors[2] is None
        assert numpy.array_equal(result[0], expected[0]) and numpy.array_equal(result[2], expected[2])
        if outcome[0] == 'error':
            assert (type(ticket.errors[1]), str(ticket.errors[1])) == outcome[1:]
        else:
            assert ticket.errors[1] is None and numpy.array_equal(result[1], outcome[1][0])
        assert numpy.array_equal(decoder.submit(singles).result(), expected)       # the next step is clean


# ---- what is out of scope says so --------------------------------------------------------------------------------------------------

def test_the_rate_control_codecs_refuse_pad(models):
    from autoencoder_based_image_compression_amd import codec, ratecontrol
    m = models[False]
    ladder = ratecontrol.RateLadder(m['bin_widths'][None]*numpy.array([[1.], [2.]], dtype=numpy.float32),
                                    numpy.stack([models['probabilities']]*2), m['map_mean'], 67)
    for (cls, more) in ((codec.BudgetCodec, {'budget_bytes': 4096}), (codec.TiledBudgetCodec, {'coding_tile': (2, 3), 'budget_bytes': 4096}),
                        (codec.QualityCodec, {'target_psnr': 30.}), (codec.TiledQualityCodec, {'coding_tile': (2, 3), 'target_psnr': 30.})):
        with pytest.raises(ValueError, match='do not take `pad`'):
            cls(m['variables'], False, ladder, N, SIZE[0], SIZE[1], pad=True, **more)
    with pytest.raises(ValueError):
        _codec(models, False, SIZE, False)
    with pytest.raises(ValueError):
        _decoder(models, SIZE, pad=False)
    with pytest.raises(ValueError):
        _codec(models, False, (0, 83), True)


# ---- poisoned slots and buffers ----------------------------------------------------------------------------------------------------

def _poison(c, guard, poison):
    """Between two steps (tests/test_gpu_codec_slots.py): the bands, then every SCRATCH buffer of every slot, and what the feature
    adds beside the slots -- the codec's real-size references of the replayed steps -- filled with the poison byte. (The padded
    batch is the static input `graphs[1]` on the graph path, which the slot table poisons, and an allocator temporary between
    bands on the launch path.)"""
    c.drain()
    guard.check(keep=True)
    assert slot_buffers.poison_scratch(c, poison) > 0
    for reference in (getattr(c, '_frame_references', None) or ()):
        slot_buffers.fill_bytes(reference, poison)
    torch.cuda.synchronize()


@pytest.mark.parametrize('mode', ['launches', 'graphs'])
def test_padded_codec_steps_on_poisoned_slots(models, mode):
    from autoencoder_based_image_compression_amd import codec, container, device, pipeline
    arguments = arguments_of(models, False, RATE)
    sets = []
    for seed in (0, 1):
        images = images_of(SIZE, seed)
        blob = container.encode_images(images, *arguments, pad=True)[0]
        decoded = container.decode_images(blob, models[False]['decoder'])
        sets.append((images, blob, decoded, _real_sse(images, decoded)))
    more = {'emit_container': True, 'fetch_reconstruction': True}
    if mode == 'graphs':
        more['use_graphs'] = True
    seen = {}
    for poison in POISONS:
        with guarded.guarded((device, pipeline, codec), poison) as guard:
            with _codec(models, False, SIZE, True, **more) as c:
                torch.cuda.synchronize()
                _poison(c, guard, poison)
                values = []
                for step in range(2*c.nb_slots + 1):
                    (images, blob, decoded, sse) = sets[(step//c.nb_slots) % 2]
                    ticket = c.submit(_feed(images, step % 2 == 1))              # device and pinned batches in turn
                    r = ticket.result()
                    assert numpy.array_equal(r['sse'], sse), step
                    assert ticket.container() == blob, step
                    assert numpy.array_equal(ticket.reconstruction_uint8.cpu().numpy(), decoded), step
                    assert numpy.array_equal(ticket.reconstruction_host, decoded), step
                    values.append([r[key].tobytes() for key in KEYS + ('sse', 'container_bytes')])
                    if mode == 'graphs':
                        assert len(c._frame_references) == c.nb_slots
                        assert all(tuple(slot.graphs[1].shape) == (N,) + CODED for slot in c._slots)
                    _poison(c, guard, poison)
        seen[poison] = values
    assert seen[POISONS[0]] == seen[POISONS[1]]


@pytest.mark.parametrize('mode', ['launches', 'graphs'])
def test_padded_decoder_steps_on_poisoned_slots(models, mode):
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    sets = [_blobs(models, SIZE, 0), _blobs(models, SIZE, 1)]
    seen = {}
    for poison in POISONS:
        with guarded.guarded((device, pipeline, codec), poison) as guard:
            with _decoder(models, SIZE, use_graphs=mode == 'graphs', nb_streams=1) as decoder:
                torch.cuda.synchronize()
                _poison(decoder, guard, poison)
                values = []
                for step in range(2*decoder.nb_slots + 1):
                    (blob, singles, expected) = sets[(step//decoder.nb_slots) % 2]
                    count = 2 if step == 3 else N                                  # one partial step
                    result = numpy.array(decoder.submit(blob if step % 2 == 0 else singles[:count]).result())
                    assert result.shape == (count,) + SIZE and numpy.array_equal(result, expected[:count]), step
                    values.append(result.tobytes())
                    _poison(decoder, guard, poison)
        seen[poison] = values
    assert seen[POISONS[0]] == seen[POISONS[1]]
