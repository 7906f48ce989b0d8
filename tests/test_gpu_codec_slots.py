"""`codec.BatchCodec` and `codec.BatchDecoder` step after step on POISONED slots between guard bands.

The codecs make their per-slot buffers once and reuse them for every step (`codec._Slot`, `_DecodeLane`, `_DecodeSlot`). The other
modules that send a slot round again alternate two valid data sets: they find a buffer reused too early, not one that is read before
it is written -- the previous step left plausible bytes there. Here every case

* builds its codec inside `guarded.guarded((device, pipeline, codec), poison)`, so every DEVICE allocation of a slot lies between two guard
  bands (pinned requests -- pinned_out, pinned_sse, pinned_payload, pinned_emit, pinned_head, pinned_status, pinned_rec and the
  like -- and allocations made during a graph capture pass through the guard: tests/guarded.py; the pinned ones are poisoned like
  the rest but have no bands), and the bands are verified after EVERY step
  (`Guard.check(keep=True)`: an overrun is reported with the step that made it);
* between two steps drains the codec and fills every buffer tests/slot_buffers.py classifies as SCRATCH -- device and pinned, the
  static tensors of the captured graphs too -- with the poison byte, through the leaf views only, so the accumulators, counters and
  constants in the same storage stay;
* runs 2 x nb_slots + 1 steps (the decoder: its nine-step sequence) of alternating entropy, so that a long payload precedes a short
  one in every slot, launch by launch and replayed as hipGraphs, under the poisons 0xFF and 0x7F;
* requires every ticket to equal, exactly, the references the other modules use -- bit counts, dead maps and exception-map cost of
  the image-by-image path, `container.encode_images` byte for byte, `container.decode_images` for reconstruction and squared error
  --, computed once per module outside the guard, and the values under the two poisons to be identical.

One more case shows that the harness has teeth: with the CARRIED accumulators `flags` and `sse` poisoned as well, inside replayed
graphs, the tickets' dead-map counts and squared errors are wrong for one round of the slots and right again afterwards. (The
decoder's tables hold no CARRIED word that is neither a counter nor polled, so it has no such case.)

Before the first poisoned run every word a kernel uses as an address, a length or a row index was traced to the launch of the same
step that writes it ("Buffer discipline"). On the commit that added this module every case passed as it stood: no
stale read was found."""
import os
import time

import numpy
import pytest
import torch

import guarded
import slot_buffers

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coder_golden.npz')
BATCH = 3
POISONS = (0xFF, 0x7F)
MODES = {'launches': {}, 'graphs': {'use_graphs': True}}
KEYS = ('nb_bits', 'coder_bits', 'exception_bits', 'sse', 'nb_deads')
_STARTED = [None]


def _images(shape, seed, count=BATCH):
    """Noise, a noisy ramp and a flat image: three different entropies (tests/test_gpu_batch_decoder.py)."""
    rng = numpy.random.RandomState(seed)
    (h, w) = shape
    noise = rng.randint(16, 236, size=(h, w))
    ramp = numpy.clip(numpy.broadcast_to(16 + 219*numpy.arange(w)/(w - 1), (h, w)) + rng.randint(-4, 5, size=(h, w)), 16, 235)
    flat = numpy.full((h, w), 90 + seed % 50)
    return numpy.stack([(noise, ramp, flat)[i % 3] for i in range(count)]).astype(numpy.uint8)


def _image_sets(shape):
    """Two batches of different entropy: noise / ramp / flat, and flat / ramp / flat."""
    return [_images(shape, 0), numpy.ascontiguousarray(_images(shape, 3)[[2, 1, 2]])]


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    from autoencoder_based_image_compression_amd import pipeline
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    _STARTED[0] = time.time()
    with numpy.load(GOLD) as g:
        probabilities = g['real_probabilities_1']
    path = str(tmp_path_factory.mktemp('slots')/'binary_probabilities.npy')
    numpy.save(path, probabilities)
    out = {'probabilities': probabilities, 'path': path, 'length': probabilities.shape[1], 'cache': {}}
    for (learned, seed) in ((False, 4), (True, 5)):
        v = var.random_variables(1., learned, seed=seed, bias_std=0.01)
        v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
        out[learned] = {'variables': v, 'encoder': pipeline.DeviceEncoder(v, learned), 'decoder': pipeline.DeviceDecoder(v, learned)}
    yield out
    print('\ntests/test_gpu_codec_slots.py: {0:.1f} s from the first fixture to the last test'.format(time.time() - _STARTED[0]))


# ---- BatchCodec ------------------------------------------------------------------------------------------------------------------

def _widths(learned, shape, scale):
    if not learned:
        return (numpy.full(128, scale, dtype=numpy.float32), numpy.random.RandomState(shape[1]).normal(scale=0.1, size=128).astype(numpy.float32))
    rng = numpy.random.RandomState(17)
    return (rng.uniform(0.6, 1.4, size=128).astype(numpy.float32), rng.normal(scale=0.05, size=128).astype(numpy.float32))


def _image_by_image(m, learned, images, bin_widths, map_mean, path, idx_map_exception):
    """Bits of the lossless code and dead maps as the reference-shaped functions of `kodak/` give them image by image
    (tests/test_gpu_codec.py: `reference_shaped_path`)."""
    from autoencoder_based_image_compression_amd.kodak.lossless import compression
    from autoencoder_based_image_compression_amd.kodak.tools import tools as tls
    y = m['encoder'](torch.from_numpy(images).cuda()).cpu().numpy()
    centered = y - numpy.tile(map_mean, y.shape[:3] + (1,))
    cq = tls.quantize_per_map(centered, bin_widths)
    nb_bits = numpy.array([compression.rescale_compress_lossless_maps(cq[j], bin_widths, path, idx_map_exception)
                           for j in range(images.shape[0])], dtype=numpy.int64)
    return nb_bits, numpy.asarray(tls.count_nb_deads(cq)).astype(numpy.int64)


def _codec_references(model, learned, shape, scale, idx_map_exception, tile):
    """Once per (model kind, shape, bin width, exception map, coding tile), shared by the launch modes and the poisons: for each of
    the two image sets the blob of `container.encode_images`, its bit counts, `decode_images` of it and the squared error against
    it, and the image-by-image path's bits and dead maps."""
    from autoencoder_based_image_compression_amd import container
    key = ('codec', learned, shape, scale, idx_map_exception, tile)
    if key in model['cache']:
        return model['cache'][key]
    m = model[learned]
    (bin_widths, map_mean) = _widths(learned, shape, scale)
    arguments = (m['encoder'], bin_widths, map_mean, model['probabilities'], idx_map_exception)
    out = []
    for images in _image_sets(shape):
        (whole_blob, whole) = container.encode_images(images, *arguments)
        (blob, info) = (whole_blob, whole) if tile is None else container.encode_images(images, *arguments, coding_tile=tile)

        def coder_bits(per_map):
            per_map = per_map.astype(numpy.int64).copy()
            if idx_map_exception >= 0:
                per_map[:, idx_map_exception] = 0           # charged by its entropy (compression.py:68-81)
            return per_map.sum(axis=1)
        (path_bits, nb_deads) = _image_by_image(m, learned, images, bin_widths, map_mean, model['path'], idx_map_exception)
        exception_bits = path_bits - coder_bits(whole['nb_bits'])
        assert (exception_bits >= 0).all() and (idx_map_exception >= 0 or not exception_bits.any())
        decoded = container.decode_images(blob, m['decoder'])
        assert numpy.array_equal(decoded, container.decode_images(whole_blob, m['decoder']))
        difference = images.astype(numpy.int64) - decoded.astype(numpy.int64)
        out.append({'images': images, 'blob': blob, 'payload_bytes': info['payload_bytes'], 'decoded': decoded,
                    'sse': (difference*difference).sum(axis=(1, 2)), 'nb_deads': nb_deads, 'exception_bits': exception_bits,
                    'coder_bits': coder_bits(info['nb_bits']), 'nb_bits': coder_bits(info['nb_bits']) + exception_bits})
    # the longer payload first: it then precedes the shorter one in every slot. (At bin width 1.0 these random weights leave most maps
    # dead whatever the image and the two differ by a few bytes only; at 0.05 by a third.)
    out.sort(key=lambda reference: -reference['payload_bytes'])
    print('payload bytes of the two sets:', [reference['payload_bytes'] for reference in out])
    assert out[0]['payload_bytes'] >= out[1]['payload_bytes'] > 0
    model['cache'][key] = (bin_widths, map_mean, out)
    return model['cache'][key]


FIXED_1 = (False, (64, 96), 1.0, 67)
FIXED_2 = (False, (48, 80), 0.05, 67)
FIXED_3 = (False, (64, 96), 0.05, -1)
DEAD = (False, (64, 96), 100.0, 67)          # a bin width at which every map is dead (at 1.0 these random weights leave none)
# name: ((model kind, shape, bin width, exception map), coding tile, BatchCodec arguments, feed pinned host batches, launch modes)
CODEC_CASES = {
    'device_coder_fetch': (FIXED_1, None, {'fetch_reconstruction': True}, True, ('launches', 'graphs')),
    'container_exception_67': (FIXED_2, None, {'emit_container': True}, False, ('launches', 'graphs')),
    'container_no_exception': (FIXED_3, None, {'emit_container': True}, False, ('launches', 'graphs')),
    'tiles_2x2_on_3x5': (FIXED_2, (2, 2), {'emit_container': True}, False, ('launches', 'graphs')),
    'tiles_2x4_on_3x5': (FIXED_2, (2, 4), {'emit_container': True}, False, ('launches', 'graphs')),
    'tiles_2x2_on_4x6': (FIXED_3, (2, 2), {'emit_container': True}, False, ('launches', 'graphs')),
    'tiles_2x4_on_4x6': (FIXED_3, (2, 4), {'emit_container': True}, False, ('launches', 'graphs')),
    'fused_latent_two_streams': (FIXED_1, None, {'fuse_latent': True, 'nb_transform_streams': 2}, False, ('launches', 'graphs')),
    'learned_bin_widths': ((True, (48, 80), 1.0, 67), None, {}, False, ('launches', 'graphs')),
    'host_coder': (FIXED_1, None, {'coder': 'host'}, True, ('launches',)),
    'one_stream_steps': (FIXED_1, None, {'one_stream_steps': True}, False, ('launches', 'graphs')),
}


def _build_codec(model, case, mode, **more):
    """case: a key of CODEC_CASES, or such a row itself."""
    from autoencoder_based_image_compression_amd import codec
    ((learned, shape, scale, idx_map_exception), tile, arguments, _, _) = CODEC_CASES[case] if isinstance(case, str) else case
    (bin_widths, map_mean, _) = _codec_references(model, learned, shape, scale, idx_map_exception, tile)
    arguments = dict(arguments, **MODES[mode], **more)
    if tile is not None:
        arguments['coding_tile'] = tile
    if arguments.get('emit_container'):
        # (these random weights code the small bin width at more than the default capacity's 8 bits per pixel; tiles pay more)
        arguments['container_capacity_bytes'] = 8*BATCH*shape[0]*shape[1]
    return codec.BatchCodec(model[learned]['variables'], learned, bin_widths, map_mean, model['probabilities'], idx_map_exception, BATCH,
                            shape[0], shape[1], nb_in_flight=2, keep_reconstruction=True, **arguments)


def _submit(c, reference, host):
    images = torch.from_numpy(reference['images'])
    images = images.pin_memory() if host else images.cuda()
    ticket = c.submit(images)
    ticket.fed_from = images          # a pinned batch stays the caller's until its copy is through
    return ticket


def _codec_step_values(c, ticket, reference, step):
    """Asserts the ticket against the references; returns what the two poisons must agree on, copied out of the slot."""
    r = ticket.result()
    for key in KEYS:
        print('step', step, key, r[key].tolist(), 'reference', reference[key].tolist())
        assert numpy.array_equal(r[key], reference[key]), (step, key)
    values = [r[key].tobytes() for key in KEYS]
    if c.emit_container:
        assert int(r['container_bytes'].sum()) == reference['payload_bytes'], step
        blob = ticket.container()
        assert blob == reference['blob'], step
        values += [r['container_bytes'].tobytes(), blob]
    reconstruction = ticket.reconstruction_uint8.cpu().numpy()
    assert numpy.array_equal(reconstruction, reference['decoded']), step
    values.append(reconstruction.tobytes())
    if c.fetch_reconstruction:
        assert numpy.array_equal(ticket.reconstruction_host, reference['decoded']), step
        values.append(ticket.reconstruction_host.tobytes())
    return values


def _check_tilings(c):
    checked = [name for (owner, table) in slot_buffers.owners(c) for name in slot_buffers.check_tiling(owner, table)]
    assert 'block' in checked or 'head' in checked
    return checked


def _poison_between_steps(c, guard, poison):
    """The per-case procedure between two steps: the bands, then drain -> poison every SCRATCH buffer of every slot."""
    c.drain()
    guard.check(keep=True)
    assert slot_buffers.poison_scratch(c, poison) > 0


@pytest.mark.parametrize('case,mode', [(case, mode) for case in CODEC_CASES for mode in CODEC_CASES[case][4]])
def test_batch_codec_steps_on_poisoned_slots(model, case, mode):
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    ((learned, shape, scale, idx_map_exception), tile, _, host, _) = CODEC_CASES[case]
    (_, _, references) = _codec_references(model, learned, shape, scale, idx_map_exception, tile)
    assert references[0]['payload_bytes'] > references[1]['payload_bytes']          # a long payload precedes a short one in every slot
    seen = {}
    for poison in POISONS:
        with guarded.guarded((device, pipeline, codec), poison) as guard:
            with _build_codec(model, case, mode) as c:
                checked = _check_tilings(c)
                assert ('table' in checked) == c.emit_container
                torch.cuda.synchronize()
                _poison_between_steps(c, guard, poison)          # what construction left is no better than what a step leaves
                values = []
                for step in range(2*c.nb_slots + 1):
                    reference = references[(step//c.nb_slots) % 2]          # slot k: the long payload, the short one, (slot 0) the long one
                    ticket = _submit(c, reference, host)
                    values.append(_codec_step_values(c, ticket, reference, step))
                    if mode == 'graphs':
                        assert all(slot.graphs is not None and len(slot_buffers.tensors_of(slot, slot_buffers.SLOT, 'graphs[2]')) == 1 for slot in c._slots)
                    _poison_between_steps(c, guard, poison)
        seen[poison] = values
    assert seen[POISONS[0]] == seen[POISONS[1]]


def test_a_poisoned_accumulator_shows_in_the_tickets(model):
    """The harness has teeth: `flags` and the squared errors of `sse` are CARRIED (the kernels only set / add, publish_step zeroes them
    for the slot's next step), carry no address and no counter, and are filled like the SCRATCH buffers here -- inside replayed
    graphs. Every slot's next ticket then reports no dead map and a squared error off by the poison; the step after it, on the same
    slot, is right again: publish_step has restored the accumulators."""
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    case = (DEAD, None, {}, False, ('graphs',))          # the plain device coder, device batches
    ((learned, shape, scale, idx_map_exception), tile, _, host, _) = case
    (_, _, references) = _codec_references(model, learned, shape, scale, idx_map_exception, tile)
    reference = max(references, key=lambda reference: int(reference['nb_deads'].sum()))
    dead = reference['nb_deads'] > 0
    assert dead.any()                                             # there are dead maps to lose
    for poison in POISONS:
        with guarded.guarded((device, pipeline, codec), poison) as guard:
            with _build_codec(model, case, 'graphs') as c:
                _codec_step_values(c, _submit(c, reference, host), reference, 'warm')          # the capture is behind us
                _poison_between_steps(c, guard, poison)
                for slot in c._slots:
                    assert slot_buffers.SLOT['flags'].cls == slot_buffers.SLOT['sse'].cls == slot_buffers.CARRIED
                    slot_buffers.fill_bytes(slot.flags, poison)
                    slot_buffers.fill_bytes(slot.sse[:BATCH], poison)      # (not the word behind them: the conv workspace's error count)
                torch.cuda.synchronize()
                for step in range(c.nb_slots):
                    r = _submit(c, reference, host).result()
                    print('step', step, 'nb_deads', r['nb_deads'].tolist(), 'sse', r['sse'].tolist(), 'reference', reference['nb_deads'].tolist(),
                          reference['sse'].tolist())
                    assert not r['nb_deads'].any() and (r['nb_deads'] != reference['nb_deads'])[dead].all(), step
                    assert (r['sse'] != reference['sse']).all(), step
                    for key in ('coder_bits', 'exception_bits'):          # what does not go through those words is untouched
                        assert numpy.array_equal(r[key], reference[key]), (step, key)
                    _poison_between_steps(c, guard, poison)
                for step in range(c.nb_slots):
                    _codec_step_values(c, _submit(c, reference, host), reference, ('restored', step))
                    _poison_between_steps(c, guard, poison)


# ---- BatchDecoder ----------------------------------------------------------------------------------------------------------------

def _outcome(call):
    try:
        return ('bytes', call())
    except Exception as exc:
        return ('error', type(exc), str(exc))


def _encoded(model, shape, tile, scale, idx_map_exception, seed=0, count=BATCH):
    """Once per case: (blob, `decode_images` of it)."""
    from autoencoder_based_image_compression_amd import container
    key = ('blob', shape, tile, scale, idx_map_exception, seed, count)
    if key not in model['cache']:
        m = model[False]
        bin_widths = numpy.full(128, scale, dtype=numpy.float32)
        map_mean = numpy.random.RandomState(shape[1] + seed).normal(scale=0.1, size=128).astype(numpy.float32)
        more = {} if tile is None else {'coding_tile': tile}
        (blob, _) = container.encode_images(_images(shape, seed, count), m['encoder'], bin_widths, map_mean, model['probabilities'],
                                            idx_map_exception, **more)
        model['cache'][key] = (blob, container.decode_images(blob, m['decoder']))
    return model['cache'][key]


def _decoder_steps(model, shape, tile):
    """The nine steps of a decoder case on two slots, [(blobs, expected images, index of the corrupted image or None)]: full steps of
    a long and of a short payload, two images (one blob of two), one image, the full steps again, a step with one corrupted stream
    (a byte flipped well inside an arithmetic-coded stream, as tests/test_gpu_batch_decoder.py does) and, two steps later and so in
    the same slot, the same step clean."""
    from autoencoder_based_image_compression_amd import container
    key = ('steps', shape, tile)
    if key in model['cache']:
        return model['cache'][key]
    long_ = _encoded(model, shape, tile, 0.05, 67)
    short = _encoded(model, shape, tile, 1.0, -1, seed=3)
    pair = _encoded(model, shape, tile, 0.05, 67, seed=7, count=2)
    singles = [_encoded(model, shape, tile, 0.05, 67, seed=20 + k, count=1) for k in range(3)]
    assert len(long_[0]) > len(short[0])
    header = container.read_header(singles[1][0])
    sizes = (header['bits'].astype(numpy.int64).reshape(-1, 2) + 7)//8          # payload order: (tile ->) map -> piece
    clean = numpy.concatenate([s[1] for s in singles])
    for longest in numpy.argsort(-sizes[:, 0], kind='stable')[:8]:           # the longest arithmetic-coded pieces first (a tile's are short)
        position = header['payload_offset'] + int(sizes.reshape(-1)[:2*int(longest)].sum()) + int(sizes[longest, 0])//2
        corrupted = bytearray(singles[1][0])
        corrupted[position] ^= 0xFF
        corrupted = bytes(corrupted)
        assert sizes[longest, 0] >= 1 and container.read_header(corrupted)['payload_offset'] == header['payload_offset']
        outcome = _outcome(lambda: container.decode_images(corrupted, model[False]['decoder']))
        if outcome[0] == 'error' or not numpy.array_equal(outcome[1], singles[1][1]):
            break                                                            # the flipped byte shows: an error, or other pixels
    else:
        raise AssertionError('no flipped byte changed what decode_images gives')
    print('corrupted stream', int(longest), 'of', sizes[longest, 0], 'bytes ->', outcome[0] if outcome[0] == 'bytes' else outcome[1:])
    steps = [(long_[0], long_[1], None), (short[0], short[1], None), (pair[0], pair[1], None), (singles[2][0], singles[2][1], None),
             (long_[0], long_[1], None), (short[0], short[1], None),
             ([singles[0][0], corrupted, singles[2][0]], clean, (1, outcome)), (pair[0], pair[1], None),
             ([s[0] for s in singles], clean, None)]
    model['cache'][key] = steps
    return steps


# name: (shape, coding tile, fetch the reconstruction, streams: with two the two slots' lanes run on a stream each)
DECODER_CASES = {
    'whole_maps_3x5_fetched': ((48, 80), None, True, 1),
    'whole_maps_4x6_on_device': ((64, 96), None, False, 2),
    'tiles_2x2_on_3x5_on_device': ((48, 80), (2, 2), False, 1),
    'tiles_2x4_on_4x6_fetched': ((64, 96), (2, 4), True, 2),
    'tiles_2x4_on_3x5_fetched': ((48, 80), (2, 4), True, 1),
    'tiles_2x2_on_4x6_on_device': ((64, 96), (2, 2), False, 1),
}


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('case', sorted(DECODER_CASES))
def test_batch_decoder_steps_on_poisoned_slots(model, case, mode):
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    (shape, tile, fetch, nb_streams) = DECODER_CASES[case]
    steps = _decoder_steps(model, shape, tile)
    seen = {}
    for poison in POISONS:
        with guarded.guarded((device, pipeline, codec), poison) as guard:
            # (these random weights code the small bin width at more than the default capacity's 8 bits per pixel; tiles pay more)
            with codec.BatchDecoder(model[False]['variables'], False, BATCH, shape[0], shape[1], model['length'], nb_in_flight=2, nb_streams=nb_streams,
                                    payload_capacity_bytes=8*BATCH*shape[0]*shape[1], fetch_reconstruction=fetch, coding_tile=tile,
                                    **MODES[mode]) as decoder:
                assert decoder.nb_slots == 2 and 'status' in _check_tilings(decoder)
                # (as many streams as the process's hardware queues allow: two on the runtime's default of four)
                assert len({slot.lane.stream for slot in decoder._slots}) == decoder.nb_streams == codec.stream_budget(nb_streams, 1)[0]
                torch.cuda.synchronize()
                _poison_between_steps(decoder, guard, poison)
                values = []
                for (step, (blobs, expected, corrupted)) in enumerate(steps):
                    ticket = decoder.submit(blobs)
                    result = ticket.result(raise_errors=False)
                    assert isinstance(result, numpy.ndarray if fetch else torch.Tensor), step
                    result = numpy.array(result) if fetch else result.cpu().numpy()
                    assert result.shape == expected.shape and ticket.nb_images == expected.shape[0], step
                    for image in range(expected.shape[0]):
                        if corrupted is not None and image == corrupted[0]:
                            outcome = corrupted[1]
                            if outcome[0] == 'error':
                                assert (type(ticket.errors[image]), str(ticket.errors[image])) == outcome[1:], step
                                values.append(repr(outcome[1:]))
                                continue                      # (nothing is promised about the pixels of an image that failed)
                            assert ticket.errors[image] is None and numpy.array_equal(result[image], outcome[1][0]), step
                            assert not numpy.array_equal(result[image], expected[image]), step
                        else:
                            assert ticket.errors[image] is None, (step, image, repr(ticket.errors[image]))
                            assert numpy.array_equal(result[image], expected[image]), (step, image)
                        values.append(result[image].tobytes())
                    if mode == 'graphs':
                        assert all(slot.graph is not None for slot in decoder._slots)
                    _poison_between_steps(decoder, guard, poison)
        seen[poison] = values
    assert seen[POISONS[0]] == seen[POISONS[1]]
