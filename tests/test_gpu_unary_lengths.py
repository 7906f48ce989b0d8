"""The containers and the resident codecs at truncated unary lengths other than 10 ("Buffer discipline").

L is the number of columns of the probability table. `csrc/hip/coder_simd.hip` codes 1 <= L <= 32 with the 64-maps-per-wavefront
kernels and every longer table with the general kernel; decision capacity, stream stride and LDS are sized from L; and everything a
slot or a step head keeps behind a `[..][L]` table sits at an offset that moves with L. The other GPU modules of the codecs and
containers take their table from the golden file (128 x 10). Here every public path runs at L = 1, 2, 3, 31, 32, 33 and 255
(tests/unary_length_cases.py says why those), with and without an exception map:

* `container.encode_images` -> `decode_images` as EAE1, as EAT1 in tiles of (4, 4) on an 11 x 13 plane, and `decode_region`;
* `codec.BatchCodec(emit_container=True)`, whole maps and in tiles, launch by launch and replayed as hipGraphs;
* `codec.BatchDecoder`, whole maps and in tiles, launches and graphs, with a partial step;
* `codec.RegionDecoder`, launches and graphs, fetched to pinned memory;
* a decoder built for L = 32 refuses a blob of L = 33 and the other way round, before any launch.

The reference depends on no kernel under test (tests/unary_length_cases.py): the numpy quantiser on `DeviceEncoder`'s latents, the
host coder per (image, tile, map), numpy probability rows for the exception map, `DeviceDecoder` on the numpy-dequantised symbols,
integer squared errors. Every comparison is exact: header fields, bit counts, payload bytes, dead maps, pixels.

Every test runs inside `guarded.guarded((device, pipeline, codec), 0xFF)`, the bands checked after every step; at L = 1, 33 and 255
the SCRATCH buffers of tests/slot_buffers.py are poisoned between the steps of `BatchCodec` and `BatchDecoder`. (`CASES` says what
was left out to keep the module's wall time near that of tests/test_gpu_codec_slots.py.)"""
import time

import numpy
import pytest
import torch

import guarded
import slot_buffers
import unary_length_cases as cases
from test_gpu_codec_slots import _image_sets

pytestmark = pytest.mark.gpu

BATCH = cases.BATCH
REGION = (32, 48)
PLACES = [(0, 0), (5, 7), (64, 96), (144, 160), (100, 150)]          # the `four_classes` requests of tests/test_gpu_region_decoder.py
# (length, poison). Every length runs under 0xFF. The repeats under 0x7F at L = 1 and 33 (one length on each side of the choice of
# kernels) passed on the commit that added this module and were then left out, as was the region decoder's device-resident fetch
# mode: with them the module took 7.3 s against the 3.2 s of tests/test_gpu_codec_slots.py in the same run, without them 4.4 s
# against 2.6 s. What is left is one codec per (length, exception map, whole maps / tiles, launches / graphs): no length and no codec
# is left out.
SECOND_POISON_LENGTHS = ()
CASES = [(length, 0xFF) for length in cases.LENGTHS] + [(length, 0x7F) for length in SECOND_POISON_LENGTHS]
REGION_CASES = [(length, poison) for (length, poison) in CASES if length not in (2, 31)]
SCRATCH_LENGTHS = (1, 33, 255)
MODES = {'launches': {}, 'graphs': {'use_graphs': True}}
KEYS = ('nb_bits', 'coder_bits', 'exception_bits', 'sse', 'nb_deads')
_STARTED = [None]


def _ids(pairs):
    return ['L{0}-0x{1:02X}'.format(length, poison) for (length, poison) in pairs]


@pytest.fixture(autouse=True)
def guard(request):
    """Every test runs on poisoned buffers between guard bands, the resident codecs' slots included (tests/guarded.py): the poison
    is the test's `poison` parameter, 0xFF for a test without one."""
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    callspec = getattr(request.node, 'callspec', None)
    poison = callspec.params.get('poison', 0xFF) if callspec is not None else 0xFF
    with guarded.guarded((device, pipeline, codec), poison) as g:
        yield g


@pytest.fixture(scope='module')
def model():
    from autoencoder_based_image_compression_amd import pipeline
    _STARTED[0] = time.time()
    v = cases.variables()
    yield {'variables': v, 'encoder': pipeline.DeviceEncoder(v, False), 'decoder': pipeline.DeviceDecoder(v, False), 'cache': {}}
    print('\ntests/test_gpu_unary_lengths.py: {0:.1f} s from the first fixture to the last test'.format(time.time() - _STARTED[0]))


# ---- the inputs and the reference, once per module ----------------------------------------------------------------------------------

def _cached(model, key, make):
    if key not in model['cache']:
        model['cache'][key] = make()
    return model['cache'][key]


def _latents(model, shape):
    """[(images, latents float32 [N, h, w, 128] as numpy)] of the two image sets."""
    def make():
        return [(images, model['encoder'](torch.from_numpy(images).cuda()).cpu().numpy()) for images in _image_sets(shape)]
    return _cached(model, ('latents', shape), make)


def _inputs(model, shape, length):
    """The inputs of a (shape, length): bin widths, map mean, the numpy symbols of both sets, the table fitted to them, and the
    reference reconstruction (`DeviceDecoder` on the numpy-dequantised symbols) with its integer squared error."""
    def make():
        (widths, mean) = (cases.bin_widths(length), cases.map_mean())
        sets = []
        for (images, latents) in _latents(model, shape):
            symbols = cases.quantise(latents, widths, mean)
            (_, decoded, _) = model['decoder'](torch.from_numpy(cases.dequantise(symbols, widths, mean)).cuda())
            decoded = decoded.cpu().numpy()
            decoded.setflags(write=False)
            sets.append({'images': images, 'symbols': symbols, 'decoded': decoded, 'sse': cases.squared_errors(images, decoded),
                         'nb_deads': cases.dead_maps(symbols)})
        return {'widths': widths, 'mean': mean, 'sets': sets, 'table': cases.fitted_table([s['symbols'] for s in sets], length)}
    return _cached(model, ('inputs', shape, length), make)


def _references(model, shape, length, idx_map_exception, tile):
    """Per image set, the longer payload first: the inputs and the host coder's blob parts, and what a ticket must report."""
    def make():
        inputs = _inputs(model, shape, length)
        out = []
        for which in inputs['sets']:
            host = cases.host_reference(which['symbols'], inputs['table'], idx_map_exception, tile)
            bits = cases.coder_bits(host['bits'], idx_map_exception)
            charged = cases.exception_bits(which['symbols'], idx_map_exception)
            out.append(dict(which, host=host, payload_bytes=len(host['payload']), coder_bits=bits, exception_bits=charged, nb_bits=bits + charged,
                            container_bytes=numpy.array([len(p) for p in host['image_payloads']], dtype=numpy.int64)))
        out.sort(key=lambda reference: -reference['payload_bytes'])
        print('payload bytes of the two sets:', [reference['payload_bytes'] for reference in out])
        assert out[0]['payload_bytes'] >= out[1]['payload_bytes'] > 0
        return out
    return _cached(model, ('references', shape, length, idx_map_exception, tile), make)


def _check_blob(model, blob, reference, shape, length, idx_map_exception, tile, images=None):
    inputs = _inputs(model, shape, length)
    if images is not None:          # the single-image blob of image `images`
        (i, host) = (images, reference['host'])
        rows = host['exception_rows'][i:i + 1] if idx_map_exception >= 0 else host['exception_rows']
        reference = {'host': {'bits': host['bits'][i:i + 1], 'payload': host['image_payloads'][i], 'exception_rows': rows},
                     'images': reference['images'][i:i + 1]}
    return cases.check_blob(blob, reference['host'], reference['images'], length, inputs['widths'], inputs['mean'], inputs['table'],
                            idx_map_exception, tile)


def _encode(model, images, shape, length, idx_map_exception, tile):
    from autoencoder_based_image_compression_amd import container
    inputs = _inputs(model, shape, length)
    more = {} if tile is None else {'coding_tile': tile}
    return container.encode_images(images, model['encoder'], inputs['widths'], inputs['mean'], inputs['table'], idx_map_exception, **more)


def _encoded(model, shape, length, idx_map_exception, tile):
    """The blobs of `container.encode_images` for the two sets, in the references' order, each held against the host reference."""
    def make():
        out = []
        for reference in _references(model, shape, length, idx_map_exception, tile):
            (blob, _) = _encode(model, reference['images'], shape, length, idx_map_exception, tile)
            _check_blob(model, blob, reference, shape, length, idx_map_exception, tile)
            out.append(blob)
        return out
    return _cached(model, ('encoded', shape, length, idx_map_exception, tile), make)


def _encoded_image(model, shape, length, idx_map_exception, tile, which, image):
    """The single-image blob of image `image` of set `which`, held against the host reference's share of that image."""
    def make():
        reference = _references(model, shape, length, idx_map_exception, tile)[which]
        (blob, _) = _encode(model, reference['images'][image:image + 1], shape, length, idx_map_exception, tile)
        _check_blob(model, blob, reference, shape, length, idx_map_exception, tile, images=image)
        return blob
    return _cached(model, ('image', shape, length, idx_map_exception, tile, which, image), make)


def _shape(tile):
    return cases.WHOLE_SHAPE if tile is None else cases.TILED_SHAPE


# ---- the inputs themselves ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('length', cases.LENGTHS)
def test_both_sides_of_the_prefix_are_populated(model, length):
    """Conditions on the module's own inputs, not measurements: at every length enough symbols reach the Exp-Golomb suffix, and
    (for L > 1) enough stop inside the prefix; every table entry is a probability (`fitted_table`)."""
    for shape in (cases.WHOLE_SHAPE, cases.TILED_SHAPE):
        (escaped, inside) = cases.populations([s['symbols'] for s in _inputs(model, shape, length)['sets']], length)
        print('L', length, 'bin width', cases.BIN_WIDTH[length], 'shape', shape, '|s| >= L:', round(escaped, 3), '0 < |s| < L:', round(inside, 3))
        assert escaped >= cases.MIN_SHARE_ESCAPED, (shape, escaped)
        assert length == 1 or inside >= cases.MIN_SHARE_INSIDE, (shape, inside)


# ---- container.encode_images / decode_images / decode_region --------------------------------------------------------------------------

@pytest.mark.parametrize('idx_map_exception', cases.EXCEPTION_MAPS)
@pytest.mark.parametrize('length,poison', CASES, ids=_ids(CASES))
def test_eae1_containers(model, length, poison, idx_map_exception):
    from autoencoder_based_image_compression_amd import container
    shape = cases.WHOLE_SHAPE
    for reference in _references(model, shape, length, idx_map_exception, None):
        (blob, info) = _encode(model, reference['images'], shape, length, idx_map_exception, None)
        _check_blob(model, blob, reference, shape, length, idx_map_exception, None)
        assert numpy.array_equal(info['nb_bits'], reference['host']['bits'].astype(numpy.int64).sum(axis=(1, 3)))
        assert info['payload_bytes'] == reference['payload_bytes'] and len(blob) == info['header_bytes'] + info['payload_bytes']
        assert numpy.array_equal(container.decode_images(blob, model['decoder']), reference['decoded'])


@pytest.mark.parametrize('idx_map_exception', cases.EXCEPTION_MAPS)
@pytest.mark.parametrize('length,poison', CASES, ids=_ids(CASES))
def test_eat1_containers_and_regions(model, length, poison, idx_map_exception):
    """Tiles of (4, 4) on the 11 x 13 plane; a corner, an odd place and the whole image as regions."""
    from autoencoder_based_image_compression_amd import container
    (shape, tile) = (cases.TILED_SHAPE, cases.CODING_TILE)
    for reference in _references(model, shape, length, idx_map_exception, tile):
        (blob, info) = _encode(model, reference['images'], shape, length, idx_map_exception, tile)
        _check_blob(model, blob, reference, shape, length, idx_map_exception, tile)
        assert numpy.array_equal(info['tile_bits'], reference['host']['bits']) and info['payload_bytes'] == reference['payload_bytes']
        assert numpy.array_equal(container.decode_images(blob, model['decoder']), reference['decoded'])
        for (y0, x0, rh, rw) in ((0, 0, 24, 40), (31, 45, 35, 50), (0, 0) + shape):
            crop = container.decode_region(blob, model['decoder'], (y0, x0, rh, rw))
            assert numpy.array_equal(crop, reference['decoded'][:, y0:y0 + rh, x0:x0 + rw]), (y0, x0, rh, rw)


# ---- the resident codecs ----------------------------------------------------------------------------------------------------------------

def _between_steps(c, guard, length, poison):
    """After every step: the bands; at the lengths of SCRATCH_LENGTHS also poison in every buffer a step must not depend on."""
    c.drain()
    guard.check(keep=True)
    if length in SCRATCH_LENGTHS:
        assert slot_buffers.poison_scratch(c, poison) > 0


def _check_tilings(c):
    return [name for (owner, table) in slot_buffers.owners(c) for name in slot_buffers.check_tiling(owner, table)]


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('tile', [None, cases.CODING_TILE], ids=['whole_maps', 'tiles_4x4'])
@pytest.mark.parametrize('idx_map_exception', cases.EXCEPTION_MAPS)
@pytest.mark.parametrize('length,poison', CASES, ids=_ids(CASES))
def test_batch_codec(model, guard, length, poison, idx_map_exception, tile, mode):
    """2 x nb_slots + 1 steps, the longer payload first in every slot: every ticket equals the host reference, its blob
    `container.encode_images`' byte for byte, its reconstruction the reference's."""
    from autoencoder_based_image_compression_amd import codec
    shape = _shape(tile)
    inputs = _inputs(model, shape, length)
    references = _references(model, shape, length, idx_map_exception, tile)
    blobs = _encoded(model, shape, length, idx_map_exception, tile)
    arguments = dict(MODES[mode], emit_container=True, nb_in_flight=1, keep_reconstruction=True,
                     container_capacity_bytes=2*references[0]['payload_bytes'])          # capacity is not what is under test
    if idx_map_exception >= 0:
        arguments['hist_radius'] = max(length, cases.HIST_RADIUS)
    if tile is not None:
        arguments['coding_tile'] = tile
    with codec.BatchCodec(model['variables'], False, inputs['widths'], inputs['mean'], inputs['table'], idx_map_exception, BATCH, shape[0],
                          shape[1], **arguments) as c:
        assert c.truncated_unary_length == length and 'table' in _check_tilings(c)
        torch.cuda.synchronize()
        _between_steps(c, guard, length, poison)
        for step in range(2*c.nb_slots + 1):
            which = (step//c.nb_slots) % 2
            reference = references[which]
            ticket = c.submit(torch.from_numpy(reference['images']).cuda())
            r = ticket.result()
            for key in KEYS:
                assert numpy.array_equal(r[key], reference[key]), (step, key, r[key].tolist(), reference[key].tolist())
            assert numpy.array_equal(r['container_bytes'], reference['container_bytes']), step
            blob = ticket.container()
            _check_blob(model, blob, reference, shape, length, idx_map_exception, tile)
            assert blob == blobs[which], step
            assert numpy.array_equal(ticket.reconstruction_uint8.cpu().numpy(), reference['decoded']), step
            if mode == 'graphs':
                assert all(slot.graphs is not None for slot in c._slots)
            _between_steps(c, guard, length, poison)


def _decoder_steps(model, shape, length, tile):
    """[(blobs, expected images)]: a full step of the longer payload (with an exception map), one of the shorter (without), a
    partial step of two single-image blobs, one with and one without an exception map, and the full steps again."""
    with_map = _references(model, shape, length, 67, tile)
    without = _references(model, shape, length, -1, tile)
    long_ = (_encoded(model, shape, length, 67, tile)[0], with_map[0]['decoded'])
    short = (_encoded(model, shape, length, -1, tile)[1], without[1]['decoded'])
    partial = ([_encoded_image(model, shape, length, 67, tile, 0, 0), _encoded_image(model, shape, length, -1, tile, 0, 1)],
               numpy.stack([with_map[0]['decoded'][0], without[0]['decoded'][1]]))
    assert len(long_[0]) > len(short[0])
    capacity = 2*max(with_map[0]['payload_bytes'], without[0]['payload_bytes'])
    return [long_, short, partial, long_, short], capacity


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('tile', [None, cases.CODING_TILE], ids=['whole_maps', 'tiles_4x4'])
@pytest.mark.parametrize('length,poison', CASES, ids=_ids(CASES))
def test_batch_decoder(model, guard, length, poison, tile, mode):
    """Blobs with and without an exception map through one decoder of two slots; the partial step leaves a third of the head's
    `prob_row` at -1. Whole maps are fetched to pinned memory, tiles left on the device."""
    from autoencoder_based_image_compression_amd import codec
    shape = _shape(tile)
    (steps, capacity) = _decoder_steps(model, shape, length, tile)
    fetch = tile is None
    with codec.BatchDecoder(model['variables'], False, BATCH, shape[0], shape[1], length, nb_in_flight=2, nb_streams=1, payload_capacity_bytes=capacity,
                            fetch_reconstruction=fetch, coding_tile=tile, **MODES[mode]) as decoder:
        assert decoder.nb_slots == 2 and 'head' in _check_tilings(decoder)
        torch.cuda.synchronize()
        _between_steps(decoder, guard, length, poison)
        for (step, (blobs, expected)) in enumerate(steps):
            ticket = decoder.submit(blobs)
            result = ticket.result()
            assert isinstance(result, numpy.ndarray if fetch else torch.Tensor), step
            result = numpy.array(result) if fetch else result.cpu().numpy()
            assert ticket.nb_images == expected.shape[0] and ticket.errors == [None]*expected.shape[0], step
            assert numpy.array_equal(result, expected), step
            if mode == 'graphs':
                assert all(slot.graph is not None for slot in decoder._slots)
            _between_steps(decoder, guard, length, poison)


@pytest.mark.parametrize('fetch', [True], ids=['fetched'])
@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('length,poison', REGION_CASES, ids=_ids(REGION_CASES))
def test_region_decoder(model, guard, length, poison, mode, fetch):
    """The five requests over a source with an exception map and one without: a full step, a partial one, a step that mixes the two
    sources and sends the first slot round again, and one crop alone. Every crop is the reference reconstruction's. (The crops left
    on the device, `fetch_reconstruction=False`, run at L = 10 in tests/test_gpu_region_decoder.py; see `CASES`.)"""
    from autoencoder_based_image_compression_amd import codec
    (shape, tile) = (cases.TILED_SHAPE, cases.CODING_TILE)
    references = [_references(model, shape, length, 67, tile)[0], _references(model, shape, length, -1, tile)[1]]
    sources = [codec.RegionSource(_encoded(model, shape, length, 67, tile)[0]), codec.RegionSource(_encoded(model, shape, length, -1, tile)[1])]
    steps = [[(0, k) + PLACES[k] for k in range(3)], [(1, 0) + PLACES[3], (1, 1) + PLACES[4]],
             [(0, 2) + PLACES[4], (1, 0) + PLACES[0], (0, 1) + PLACES[2]], [(1, 2) + PLACES[1]]]
    capacity = 2*BATCH*int(max(reference['container_bytes'].max() for reference in references))
    with codec.RegionDecoder(model['variables'], False, BATCH, shape[0], shape[1], length, coding_tile=tile, region=REGION, nb_in_flight=2,
                             nb_streams=1, payload_capacity_bytes=capacity, fetch_reconstruction=fetch, **MODES[mode]) as decoder:
        assert decoder.nb_slots == 2
        for (step, requests) in enumerate(steps):
            ticket = decoder.submit([(sources[s], image, y0, x0) for (s, image, y0, x0) in requests])
            result = ticket.result()
            assert isinstance(result, numpy.ndarray if fetch else torch.Tensor), step
            result = numpy.array(result) if fetch else result.cpu().numpy()
            assert result.shape == (len(requests),) + REGION and ticket.errors == [None]*len(requests), step
            for (k, (s, image, y0, x0)) in enumerate(requests):
                assert numpy.array_equal(result[k], references[s]['decoded'][image, y0:y0 + REGION[0], x0:x0 + REGION[1]]), (step, k)
            if mode == 'graphs':
                assert all(slot.graph is not None for slot in decoder._slots)
            decoder.drain()
            guard.check(keep=True)


# ---- the boundary between the two routes of the coder ------------------------------------------------------------------------------------

def test_a_decoder_refuses_the_length_across_the_boundary(model):
    """A decoder built for L = 32 refuses a blob of L = 33 and the other way round, on the host: no pinned byte is written and no
    step is counted. And the two lengths do not code alike: a codec that ignored L could not give both payloads."""
    from autoencoder_based_image_compression_amd import codec
    (whole, tiled, tile) = (cases.WHOLE_SHAPE, cases.TILED_SHAPE, cases.CODING_TILE)
    payloads = {length: _references(model, whole, length, 67, None)[0]['host']['payload'] for length in (32, 33)}
    assert payloads[32] != payloads[33]
    assert not numpy.array_equal(_references(model, whole, 32, 67, None)[0]['host']['bits'], _references(model, whole, 33, 67, None)[0]['host']['bits'])
    for (built, other) in ((32, 33), (33, 32)):
        decoders = [(codec.BatchDecoder(model['variables'], False, BATCH, whole[0], whole[1], built, nb_in_flight=2, nb_streams=1,
                                        payload_capacity_bytes=2*_references(model, whole, built, 67, None)[0]['payload_bytes']),
                     _encoded(model, whole, other, 67, None)[0], _encoded(model, whole, built, 67, None)[0],
                     _references(model, whole, built, 67, None)[0]['decoded']),
                    (codec.BatchDecoder(model['variables'], False, BATCH, tiled[0], tiled[1], built, nb_in_flight=2, nb_streams=1, coding_tile=tile,
                                        payload_capacity_bytes=2*_references(model, tiled, built, 67, tile)[0]['payload_bytes']),
                     _encoded(model, tiled, other, 67, tile)[0], _encoded(model, tiled, built, 67, tile)[0],
                     _references(model, tiled, built, 67, tile)[0]['decoded'])]
        region = codec.RegionDecoder(model['variables'], False, BATCH, tiled[0], tiled[1], built, coding_tile=tile, region=REGION, nb_in_flight=2, nb_streams=1)
        for (decoder, refused, accepted, expected) in decoders:
            with decoder:
                before = [(slot.head_host.copy(), slot.payload_host.copy(), slot.count) for slot in decoder._slots]
                with pytest.raises(ValueError, match='truncated unary length of {0}, the decoder was built for {1}'.format(other, built)):
                    decoder.submit(refused)
                for (slot, (head, payload, count)) in zip(decoder._slots, before):
                    assert numpy.array_equal(slot.head_host, head) and numpy.array_equal(slot.payload_host, payload) and slot.count == count == 0
                assert numpy.array_equal(decoder.submit(accepted).result(), expected)          # and the decoder is still usable
        with region:
            before = [(slot.head_host.copy(), slot.payload_host.copy(), slot.count) for slot in region._slots]
            with pytest.raises(ValueError, match='truncated unary length'):
                region.submit([(codec.RegionSource(_encoded(model, tiled, other, 67, tile)[0]), 0, 0, 0)])
            for (slot, (head, payload, count)) in zip(region._slots, before):
                assert numpy.array_equal(slot.head_host, head) and numpy.array_equal(slot.payload_host, payload) and slot.count == count == 0
