"""`codec.RegionDecoder`: requests (source, image, y0, x0) in, crops out, byte for byte what `container.decode_region` gives for the
same request and what `container.decode_images` holds at that place. First the two kernels it adds, each
alone between guard bands: `device.tile_symbols_dequantize_placed` bit for bit against `device.tile_symbols_dequantize_rows` on the
plan put together, and `device.publish_crops` against numpy slices. Then the decoder: launch by launch and replayed as hipGraphs,
fetched to pinned memory and left on the device, on planes whose tiles fall into four, two and one shape class; steps that mix
sources, partial steps, slots that come round again, a source given as a file object, a corrupted tile that must stay with its crop,
what `submit` and the constructor refuse, and steps on poisoned slots."""
import gc
import io
import os

import numpy
import pytest
import torch

import guarded
import slot_buffers

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coder_golden.npz')
BATCH = 3
REGION = (32, 48)
POISONS = (0xFF, 0x7F)
# name: (image shape, coding tile, requests (y0, x0)): latent planes 11 x 13 in tiles of (4, 4) (four shape classes) and in one tile per
# map, 4 x 6 in tiles of (2, 4) (the window is the plane); the first plane's requests end in its bottom-right corner and an odd place
CASES = {
    'four_classes': ((176, 208), (4, 4), [(0, 0), (5, 7), (64, 96), (144, 160), (100, 150)]),
    'one_tile_per_map': ((176, 208), (16, 16), [(0, 0), (5, 7), (64, 96), (144, 160), (100, 150)]),
    'window_is_the_plane': ((64, 96), (2, 4), [(0, 0), (5, 7), (32, 48), (17, 30), (32, 0)]),
}


@pytest.fixture(autouse=True, params=POISONS)
def guard(request):
    """Every test runs twice, on buffers poisoned with 0xFF (NaN, -1) and with 0x7F (3.4e38, 32639): what device.py allocates and
    what the tests allocate through the guard keeps the poison until a kernel writes it, and a byte written outside a tensor fails
    the test."""
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


def _dev():
    from autoencoder_based_image_compression_amd import device
    return device


# ---- tile_symbols_dequantize_placed ----------------------------------------------------------------------------------------------------

def _int16_poison(byte):
    return numpy.array([byte, byte], dtype=numpy.uint8).view(numpy.int16)[0]


def _kernel_inputs(h, w, coding_tile, poison):
    """Three images of symbols in tile-major runs, the entries in a shuffled order with gaps of 5 symbols (holding the poison)
    between the runs; three different rows of bin widths and of means (tests/test_gpu_batch_decoder_tiles.py)."""
    from autoencoder_based_image_compression_amd import container
    n = 3
    rng = numpy.random.RandomState(h*w)
    symbols = rng.randint(-300, 300, size=(n, 128, h, w)).astype(numpy.int16)
    (tiles, _) = container.coding_tile_grid(h, w, coding_tile)
    entries = [(i, t) for i in range(n) for t in range(len(tiles))]
    entries = [entries[k] for k in rng.permutation(len(entries))]
    (rows, pos) = ([], 0)
    for (i, t) in entries:
        (r0, c0, nr, nc) = (int(x) for x in tiles[t, :4])
        rows.append((i, r0, c0, nr, nc, pos))
        pos += 128*nr*nc + 5
    plan = numpy.array(rows, dtype=numpy.int64).reshape(-1, 6)
    buffer = numpy.full(pos, _int16_poison(poison), dtype=numpy.int16)
    for (i, r0, c0, nr, nc, off) in plan.tolist():
        buffer[off:off + 128*nr*nc] = symbols[i, :, r0:r0 + nr, c0:c0 + nc].reshape(-1)
    bin_widths = rng.uniform(0.01, 3., size=(n, 128)).astype(numpy.float32)
    means = rng.normal(size=(n, 128)).astype(numpy.float32)
    return n, plan, buffer, bin_widths, means


def _halves(plan):
    """A plan of `tile_symbols_dequantize_rows` -> (static slots int64 [k, 3], placement int32 [k, 4])."""
    slots = numpy.ascontiguousarray(plan[:, 3:6])
    placement = numpy.zeros((plan.shape[0], 4), dtype=numpy.int32)
    placement[:, :3] = plan[:, :3]
    placement[:, 3] = 0x5A5A5A5A          # the unused word is not looked at
    return slots, placement


def _placed_outputs(h, w, coding_tile, poison):
    """-> {name: int32 bit patterns} of the placed kernel's outputs, each already held against `tile_symbols_dequantize_rows` on the
    equivalent plan. Inputs between bands poisoned with `poison`, outputs between bands filled with 0xFF."""
    dev = _dev()
    (inputs, guard) = (guarded.Guard(poison), guarded.Guard(0xFF))
    up = inputs.upload
    (n, plan, buffer, bin_widths, means) = _kernel_inputs(h, w, coding_tile, poison)
    (buffer_d, rows_d, mean_d) = (up(buffer), up(bin_widths), up(means))
    outs = {}

    def run(name, plan, shape, mean, full=True):
        (slots, placement) = _halves(plan)
        # a slot of image -1 or n is an absent one: the reference leaves its row out
        present = plan[(plan[:, 0] >= 0) & (plan[:, 0] < shape[0])]
        got = guard.empty(shape, dtype=torch.float32, device='cuda')
        assert dev.tile_symbols_dequantize_placed(buffer_d, up(slots), slots, up(placement), rows_d, mean, got) is got
        reference = guard.empty(shape, dtype=torch.float32, device='cuda')
        dev.tile_symbols_dequantize_rows(buffer_d, up(present), present, rows_d, mean, reference)
        (got, reference) = (got.view(torch.int32).cpu().numpy(), reference.view(torch.int32).cpu().numpy())
        assert numpy.array_equal(got, reference), name
        assert numpy.isnan(got.view(numpy.float32)).any() != full, name            # nothing keeps the fill / the absent slots' pixels do
        outs[name] = got

    run('mean', plan, (n, h, w, 128), mean_d)
    run('no mean', plan, (n, h, w, 128), None)
    # into a sub-plane that cuts through tiles: negative origins, tiles that reach past it, the image order reversed
    (r0, r1, c0, c1) = (h//3, max(h//3 + 1, h - 1), w//4, max(w//4 + 1, w - 2))
    sub_plan = plan.copy()
    sub_plan[:, 0] = n - 1 - sub_plan[:, 0]
    sub_plan[:, 1] -= r0
    sub_plan[:, 2] -= c0
    assert (sub_plan[:, 1:3] < 0).any() or (r0, c0) == (0, 0)
    run('sub-plane', sub_plan, (n, r1 - r0, c1 - c0, 128), mean_d)
    # slots of image -1 and of image n: skipped, the output keeps its fill there; origins far outside write nothing either
    absent = plan.copy()
    absent[0, 0] = -1
    absent[1, 0] = n
    absent[2, 1:3] = (0x7FFFFFF0, -0x7FFFFFF0)
    run('absent', absent, (n, h, w, 128), mean_d, full=False)
    torch.cuda.synchronize()
    inputs.check()
    guard.check()
    return outs


@pytest.mark.parametrize('h, w, coding_tile', [(5, 7, (2, 3)), (3, 2, (1, 1)), (9, 70, (9, 65))])
def test_the_placed_kernel_is_the_rows_kernel(h, w, coding_tile):
    first = _placed_outputs(h, w, coding_tile, POISONS[0])
    again = _placed_outputs(h, w, coding_tile, POISONS[1])
    assert sorted(first) == sorted(again) == ['absent', 'mean', 'no mean', 'sub-plane']
    for name in first:           # the defined outputs do not depend on what lies around the inputs
        assert first[name].tobytes() == again[name].tobytes(), name
    assert not numpy.array_equal(first['mean'][0], first['mean'][1])


def test_the_placed_kernel_refuses_before_any_launch():
    dev = _dev()
    (n, plan, buffer, bin_widths, means) = _kernel_inputs(5, 7, (2, 3), 0xFF)
    (slots, placement) = _halves(plan)
    (buffer_d, slots_d, placement_d) = (torch.from_numpy(buffer).cuda(), torch.from_numpy(slots).cuda(), torch.from_numpy(placement).cuda())
    (rows_d, mean_d) = (torch.from_numpy(bin_widths).cuda(), torch.from_numpy(means).cuda())
    out = torch.full((n, 5, 7, 128), 7., device='cuda')
    for (row, col, value) in ((0, 0, 0), (2, 1, 0), (1, 0, -3), (0, 2, buffer.size), (1, 2, -1), (3, 2, buffer.size - 10)):      # malformed static rows
        bad = slots.copy()
        bad[row, col] = value
        with pytest.raises(dev.HipError):
            dev.tile_symbols_dequantize_placed(buffer_d, torch.from_numpy(bad).cuda(), bad, placement_d, rows_d, mean_d, out)
    with pytest.raises(dev.HipError):                                                                                  # the two copies differ in shape
        dev.tile_symbols_dequantize_placed(buffer_d, slots_d[:-1], slots, placement_d, rows_d, mean_d, out)
    with pytest.raises(dev.HipError):                                                                                  # a placement of another length
        dev.tile_symbols_dequantize_placed(buffer_d, slots_d, slots, placement_d[:-1], rows_d, mean_d, out)
    with pytest.raises(dev.HipError):
        dev.tile_symbols_dequantize_placed(buffer_d, slots_d, slots, placement_d.long(), rows_d, mean_d, out)
    for (rows, mean) in ((rows_d[:2], mean_d), (rows_d, mean_d[:2]), (rows_d.double(), mean_d), (rows_d, mean_d.double()), (rows_d.t(), mean_d)):
        with pytest.raises(dev.HipError):
            dev.tile_symbols_dequantize_placed(buffer_d, slots_d, slots, placement_d, rows, mean, out)
    with pytest.raises(dev.HipError):
        dev.tile_symbols_dequantize_placed(buffer_d.int(), slots_d, slots, placement_d, rows_d, mean_d, out)
    with pytest.raises(dev.HipError):
        dev.tile_symbols_dequantize_placed(buffer_d, slots_d, slots, placement_d, rows_d, mean_d, out[..., :64])
    torch.cuda.synchronize()
    assert bool((out == 7.).all())                                                                                     # nothing was launched


# ---- publish_crops ---------------------------------------------------------------------------------------------------------------------

(PLANES, CROP) = ((3, 40, 52), (7, 13))          # 3 x 7 x 13 = 273 bytes: the last of 18 words holds one byte and 15 of pad
ORIGINS = {
    'inside': [(0, 0), (33, 39), (5, 7)],              # the first, the last, an odd column
    'outside': [(-2, -3), (35, 41), (34, -1)],         # a few pixels outside: the clamped crop
    'odd': [(1, 1), (2, 3), (33, 37)],
}


def _expected_crops(planes, origins):
    (ch, cw) = CROP
    out = []
    for (plane, (y, x)) in zip(planes, origins):
        (y, x) = (min(max(y, 0), PLANES[1] - ch), min(max(x, 0), PLANES[2] - cw))
        out.append(plane[y:y + ch, x:x + cw])
    return numpy.stack(out)


@pytest.mark.parametrize('pinned', [False, True])
@pytest.mark.parametrize('name', sorted(ORIGINS))
def test_publish_crops_cuts_the_clamped_crops(guard, name, pinned):
    dev = _dev()
    rng = numpy.random.RandomState(len(name))
    planes = rng.randint(0, 256, size=PLANES).astype(numpy.uint8)
    (ch, cw) = CROP
    nbytes = PLANES[0]*ch*cw
    words = -(-nbytes//16)*16
    assert (nbytes, words) == (273, 288)
    planes_d = guard.upload(planes)
    origins_d = guard.upload(numpy.array(ORIGINS[name], dtype=numpy.int32))
    whole = torch.full((words + 16,), 0x5A, dtype=torch.uint8).pin_memory() if pinned else guard.full((words + 16,), 0x5A, dtype=torch.uint8, device='cuda')
    dev.publish_crops(planes_d, origins_d, whole[:words], ch, cw)
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert numpy.array_equal(got[:nbytes].reshape(PLANES[0], ch, cw), _expected_crops(planes, ORIGINS[name]))
    assert (got[nbytes:words] == 0).all()              # the pad of the last word
    assert (got[words:] == 0x5A).all()                 # the word behind it
    guard.check()


def test_publish_crops_refuses_before_any_launch(guard):
    from autoencoder_based_image_compression_amd import _native
    dev = _dev()
    lib = _native.hip()
    planes = guard.full(PLANES, 3, dtype=torch.uint8, device='cuda')
    origins = guard.zeros((3, 2), dtype=torch.int32, device='cuda')
    dst = guard.full((304,), 0x5A, dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    (p, o, d) = (planes.data_ptr(), origins.data_ptr(), dst.data_ptr())
    for (arguments, status) in (((p, 3, 40, 52, o, 7, 13, d + 8, 288), -1),          # dst not 16-byte aligned
                                ((p, 3, 40, 52, o, 7, 13, d, 280), -1),              # a capacity that is no multiple of 16
                                ((p + 1, 3, 40, 52, o, 7, 13, d, 288), -1),          # planes not 4-byte aligned
                                ((None, 3, 40, 52, o, 7, 13, d, 288), -1), ((p, 3, 40, 52, None, 7, 13, d, 288), -1),
                                ((p, 3, 40, 52, o, 7, 13, None, 288), -1), ((p, 0, 40, 52, o, 7, 13, d, 288), -1),
                                ((p, 3, 40, 52, o, 0, 13, d, 288), -1),
                                ((p, 3, 40, 52, o, 7, 13, d, 272), -2),              # a capacity below the crops rounded up
                                ((p, 3, 40, 52, o, 41, 13, d, 304), -2),             # ch > H
                                ((p, 3, 40, 52, o, 7, 53, d, 304), -2)):             # cw > W
        assert lib.eae_hip_publish_crops(*arguments, stream) == status, arguments
    with pytest.raises(dev.HipError):
        dev.publish_crops(planes, origins, dst[:280], 7, 13)
    with pytest.raises(dev.HipError):
        dev.publish_crops(planes, origins[:2], dst[:288], 7, 13)
    with pytest.raises(dev.HipError):
        dev.publish_crops(planes, origins, torch.zeros(288, dtype=torch.uint8), 7, 13)          # host memory that is not pinned
    with pytest.raises(dev.HipError):
        dev.publish_crops(planes.int(), origins, dst[:288], 7, 13)
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all())


# ---- the decoder -------------------------------------------------------------------------------------------------------------------------

_CACHE = {}


@pytest.fixture(scope='module')
def weights():
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    v = var.random_variables(1., False, seed=4, bias_std=0.01)
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    with numpy.load(GOLD) as g:
        probabilities = g['real_probabilities_1']
    return {'variables': v, 'probabilities': probabilities, 'length': probabilities.shape[1]}


def _model(weights):
    """The encoder and decoder the references are made with, once per module (their tensors outlive the test that made them)."""
    from autoencoder_based_image_compression_amd import pipeline
    if 'model' not in _CACHE:
        _CACHE['model'] = (pipeline.DeviceEncoder(weights['variables'], False), pipeline.DeviceDecoder(weights['variables'], False))
    return _CACHE['model']


def _images(shape, seed, count=BATCH):
    """Noise, a noisy ramp and a flat image: three different entropies (tests/test_gpu_batch_decoder.py)."""
    rng = numpy.random.RandomState(seed)
    (h, w) = shape
    noise = rng.randint(16, 236, size=(h, w))
    ramp = numpy.clip(numpy.broadcast_to(16 + 219*numpy.arange(w)/(w - 1), (h, w)) + rng.randint(-4, 5, size=(h, w)), 16, 235)
    flat = numpy.full((h, w), 90 + seed % 50)
    return numpy.stack([(noise, ramp, flat)[i % 3] for i in range(count)]).astype(numpy.uint8)


def _encoded(weights, shape, tile, scale, idx_map_exception, seed=0, count=BATCH):
    """Once per case, shared by every test that needs it: (`EAT1` blob, `decode_images` of it)."""
    from autoencoder_based_image_compression_amd import container
    key = ('blob', shape, tile, scale, idx_map_exception, seed, count)
    if key not in _CACHE:
        (encoder, decoder) = _model(weights)
        bin_widths = numpy.full(128, scale, dtype=numpy.float32)
        map_mean = numpy.random.RandomState(shape[1] + seed).normal(scale=0.1, size=128).astype(numpy.float32)
        (blob, _) = container.encode_images(_images(shape, seed, count), encoder, bin_widths, map_mean, weights['probabilities'],
                                            idx_map_exception, coding_tile=tile)
        expected = container.decode_images(blob, decoder)
        expected.setflags(write=False)
        _CACHE[key] = (blob, expected)
    return _CACHE[key]


def _reference(weights, key, blob, image, y0, x0):
    """`container.decode_region` of one request, once per (blob, request)."""
    from autoencoder_based_image_compression_amd import container
    key = ('crop', key, image, y0, x0)
    if key not in _CACHE:
        _CACHE[key] = container.decode_region(blob, _model(weights)[1], (y0, x0) + REGION, images=[image])[0]
    return _CACHE[key]


def _decoder(weights, shape, tile, **arguments):
    from autoencoder_based_image_compression_amd import codec
    # (these random weights code the small bin width at more than the default capacity's 16 bits per symbol, the more so in tiles)
    arguments.setdefault('payload_capacity_bytes', 8*BATCH*shape[0]*shape[1])
    arguments.setdefault('nb_in_flight', 2)
    arguments.setdefault('nb_streams', 1)
    batch = arguments.pop('batch_size', BATCH)
    return codec.RegionDecoder(weights['variables'], False, batch, shape[0], shape[1], weights['length'], coding_tile=tile, region=REGION,
                               **arguments)


def _array(result):
    return result.cpu().numpy() if isinstance(result, torch.Tensor) else numpy.array(result)


def _check_crops(weights, ticket, requests, blobs, fetch=True):
    """blobs: {id(source): (key, blob, decode_images of it)}. Every crop against `decode_region` and against `decode_images`' slice."""
    result = ticket.result()
    assert isinstance(result, numpy.ndarray if fetch else torch.Tensor)
    assert tuple(result.shape) == (len(requests),) + REGION and result.dtype == (numpy.uint8 if fetch else torch.uint8)
    assert ticket.errors == [None]*len(requests) and ticket.nb_images == len(requests)
    result = _array(result)
    for (k, (source, image, y0, x0)) in enumerate(requests):
        (key, blob, expected) = blobs[id(source)]
        assert numpy.array_equal(result[k], expected[image, y0:y0 + REGION[0], x0:x0 + REGION[1]]), (k, image, y0, x0)
        assert numpy.array_equal(result[k], _reference(weights, key, blob, image, y0, x0)), (k, image, y0, x0)
    return result


@pytest.mark.parametrize('graphs,fetch', [(False, True), (True, True), (True, False), (False, False)])
@pytest.mark.parametrize('scale,idx_map_exception', [(1.0, 67), (0.05, -1)])
@pytest.mark.parametrize('case', sorted(CASES))
def test_crops_are_what_decode_region_gives(weights, case, scale, idx_map_exception, graphs, fetch):
    """A full step, a partial one, and a third that sends the first slot round again: the five requests over the three images."""
    from autoencoder_based_image_compression_amd import codec
    (shape, tile, places) = CASES[case]
    (blob, expected) = _encoded(weights, shape, tile, scale, idx_map_exception)
    source = codec.RegionSource(blob)
    blobs = {id(source): ((case, scale, idx_map_exception), blob, expected)}
    requests = [(source, k % BATCH, y0, x0) for (k, (y0, x0)) in enumerate(places)]
    with _decoder(weights, shape, tile, use_graphs=graphs, fetch_reconstruction=fetch) as decoder:
        assert decoder.coding_tile == (min(tile[0], shape[0]//16), min(tile[1], shape[1]//16)) and decoder.nb_slots == 2
        assert decoder.window == codec.region_window(shape[0]//16, shape[1]//16, REGION)
        for step in (requests[:3], requests[3:], [requests[4], requests[0], requests[2]], requests[1:2]):
            _check_crops(weights, decoder.submit(step), step, blobs, fetch)
        if graphs:
            assert all(slot.graph is not None for slot in decoder._slots)


@pytest.mark.parametrize('graphs', [False, True])
def test_steps_that_mix_sources_and_a_file_object(weights, graphs):
    """Two sources of different bin widths, one with an exception map and one without, and the first again as a file object, in one
    step and in both orders; the pipeline kept full over more steps than slots."""
    from autoencoder_based_image_compression_amd import codec
    (shape, tile, places) = CASES['four_classes']
    made = [_encoded(weights, shape, tile, 1.0, 67), _encoded(weights, shape, tile, 0.05, -1, seed=3)]
    sources = [codec.RegionSource(made[0][0]), codec.RegionSource(made[1][0]), codec.RegionSource(io.BytesIO(made[0][0]))]
    blobs = {id(sources[0]): (('mix', 0), ) + made[0], id(sources[1]): (('mix', 1),) + made[1], id(sources[2]): (('mix', 0),) + made[0]}
    steps = [[(sources[0], 0) + places[1], (sources[1], 1) + places[4], (sources[2], 2) + places[3]],
             [(sources[1], 0) + places[3], (sources[2], 1) + places[2]],
             [(sources[1], 2) + places[0], (sources[1], 2) + places[0], (sources[0], 1) + places[4]]]
    with _decoder(weights, shape, tile, use_graphs=graphs, nb_streams=2, nb_in_flight=3) as decoder:
        tickets = []
        checked = 0
        for step in range(3*decoder.nb_slots):
            tickets.append(decoder.submit(steps[step % 3]))
            while checked <= step - (decoder.nb_slots - 1):      # a result is valid until its slot is submitted again
                _check_crops(weights, tickets[checked], steps[checked % 3], blobs)
                checked += 1
        decoder.drain()
        for k in range(checked, len(tickets)):
            _check_crops(weights, tickets[k], steps[k % 3], blobs)


def _outcome(call):
    try:
        return ('bytes', call())
    except Exception as exc:
        return ('error', type(exc), str(exc))


def _corrupted(weights, kind, blob, header, streams, hit):
    """-> (corrupted blob, outcome of `decode_region` of the crop on it). streams: the crop's own streams, payload order.
    'flipped byte': a byte flipped in the middle of the longest arithmetic-coded stream, as tests/test_gpu_batch_decoder_tiles.py
    chooses it: the coder may fail, or decode other symbols. 'stream of ones': every byte of an arithmetic-coded stream becomes 0xFF:
    the code value stays at the top of the interval, so every decision decodes as 1, every one of the tile's 16 symbols escapes to
    its Exp-Golomb suffix and sign -- two bypass bits at least each --, and the stream chosen has fewer than 32 bypass bits: the
    bypass stream under-runs and the coder MUST fail."""
    from autoencoder_based_image_compression_amd import container
    bits = header['bits'].astype(numpy.int64).reshape(-1, 2)
    sizes = (bits + 7)//8                                                         # payload order: tile -> map -> piece
    corrupted = bytearray(blob)
    if kind == 'flipped byte':
        chosen = int(streams[numpy.argmax(sizes[streams, 0])])
        assert sizes[chosen, 0] >= 8
        corrupted[header['payload_offset'] + int(sizes.reshape(-1)[:2*chosen].sum()) + int(sizes[chosen, 0])//2] ^= 0xFF
    else:
        usable = streams[(bits[streams, 0] >= 1) & (bits[streams, 1] < 32) & (streams % 128 != header['idx_map_exception'])]
        assert usable.size
        chosen = int(usable[numpy.argmax(sizes[usable, 0])])
        start = header['payload_offset'] + int(sizes.reshape(-1)[:2*chosen].sum())
        corrupted[start:start + int(sizes[chosen, 0])] = b'\xff'*int(sizes[chosen, 0])
    corrupted = bytes(corrupted)
    assert container.read_header(corrupted)['payload_offset'] == header['payload_offset']          # the header is still valid
    return corrupted, _outcome(lambda: container.decode_region(corrupted, _model(weights)[1], hit + REGION, images=[0])[0])


@pytest.mark.parametrize('graphs', [False, True])
@pytest.mark.parametrize('kind,scale', [('flipped byte', 0.05), ('stream of ones', 1.0)])
def test_a_corrupted_tile_stays_with_its_crop(weights, kind, scale, graphs):
    """One stream among the tiles of ONE crop is corrupted (`_corrupted`; the header still valid): that crop's outcome is
    `decode_region`'s on the corrupted source -- for the 'stream of ones' an exception for certain, and `errors` holds it --; a crop
    of the same source that does not touch the tile, the crops of the clean source and the next step are clean."""
    from autoencoder_based_image_compression_amd import codec, container
    (shape, tile, places) = CASES['four_classes']
    (blob, expected) = _encoded(weights, shape, tile, scale, 67, seed=21, count=1)
    layout = codec.region_layout(BATCH, shape[0]//16, shape[1]//16, tile, *codec.region_window(shape[0]//16, shape[1]//16, REGION))
    (hit, far) = ((5, 7), (144, 160))
    # (the two windows share a tile: the stream is one of the tiles that only the first crop touches)
    touched = sorted({t for (t, _, _, _) in codec.place_region(layout, *hit)[1]} - {t for (t, _, _, _) in codec.place_region(layout, *far)[1]})
    assert touched == [0, 1, 4]
    header = container.read_header(blob)
    streams = numpy.concatenate([numpy.arange(t*128, (t + 1)*128) for t in touched])
    (corrupted, outcome) = _corrupted(weights, kind, blob, header, streams, hit)
    if kind == 'stream of ones':
        assert outcome[0] == 'error' and outcome[1] is RuntimeError, outcome
    (clean, bad) = (codec.RegionSource(blob), codec.RegionSource(corrupted))
    blobs = {id(clean): (('corrupt', scale), blob, expected), id(bad): (('corrupt', scale), blob, expected)}
    with _decoder(weights, shape, tile, use_graphs=graphs) as decoder:
        for _ in range(2):
            requests = [(clean, 0) + hit, (bad, 0) + hit, (bad, 0) + far]
            ticket = decoder.submit(requests)
            result = ticket.result(raise_errors=False)
            assert ticket.errors[0] is None and ticket.errors[2] is None
            for k in (0, 2):
                (y0, x0) = requests[k][2:]
                assert numpy.array_equal(result[k], expected[0, y0:y0 + REGION[0], x0:x0 + REGION[1]]), k
            if outcome[0] == 'error':
                assert (type(ticket.errors[1]), str(ticket.errors[1])) == outcome[1:]
                with pytest.raises(outcome[1]):
                    ticket.result()
            else:
                assert ticket.errors[1] is None and numpy.array_equal(result[1], outcome[1])
                assert not numpy.array_equal(result[1], result[0])
            # the next step of this decoder is clean
            again = [(clean, 0) + hit, (clean, 0) + far]
            _check_crops(weights, decoder.submit(again), again, blobs)


def test_refused_steps_and_lifetime(weights, guard):
    from autoencoder_based_image_compression_amd import codec, container
    (shape, tile, places) = CASES['four_classes']
    (blob, expected) = _encoded(weights, shape, tile, 1.0, 67)
    source = codec.RegionSource(blob)
    blobs = {id(source): (('four_classes', 1.0, 67), blob, expected)}
    (other_tile, _) = _encoded(weights, shape, (16, 16), 1.0, 67)
    (other_size, _) = _encoded(weights, CASES['window_is_the_plane'][0], (4, 4), 1.0, 67, count=1)
    (encoder, _) = _model(weights)
    (plain, _) = container.encode_images(_images(shape, 0, 1), encoder, numpy.ones(128, dtype=numpy.float32), numpy.zeros(128, dtype=numpy.float32),
                                         weights['probabilities'], 67)
    header = container.read_header(blob)
    fields = container._fields(True, BATCH, shape[0], shape[1], 67, header['bin_widths'], header['map_mean'], header['binary_probabilities'],
                               header['exception_probabilities'], header['coding_tile'])
    learned = container._pack_header(fields, header['bits'].reshape(-1, 2)) + blob[header['payload_offset']:]
    longer = numpy.concatenate([header['binary_probabilities'], header['binary_probabilities'][:, :1]], axis=1)
    fields = container._fields(False, BATCH, shape[0], shape[1], -1, header['bin_widths'], header['map_mean'], longer,
                               numpy.zeros((0, longer.shape[1])), header['coding_tile'])
    other_length = container._pack_header(fields, header['bits'].reshape(-1, 2)) + blob[header['payload_offset']:]
    ok = (source, 0, 0, 0)
    decoder = _decoder(weights, shape, tile)
    heads = [(slot.head_host.copy(), slot.payload_host.copy()) for slot in decoder._slots]
    for (bad, match) in (([(codec.RegionSource(other_size), 0, 0, 0)], 'images'), ([ok, (codec.RegionSource(other_tile), 0, 0, 0)], 'coding_tile'),
                         ([(codec.RegionSource(other_length), 0, 0, 0)], 'truncated unary length'),
                         ([(codec.RegionSource(learned), 0, 0, 0)], 'other kind of model'), ([(codec.RegionSource(plain), 0, 0, 0)], 'EAE1'),
                         ([(source, BATCH, 0, 0)], 'no image'), ([(source, -1, 0, 0)], 'no image'),
                         ([(source, 0, shape[0] - REGION[0] + 1, 0)], 'leaves'), ([(source, 0, 0, -1)], 'leaves'),
                         ([ok]*(BATCH + 1), 'at most'), ([], 'at least one'), ([(blob, 0, 0, 0)], 'request')):
        with pytest.raises(ValueError, match=match):
            decoder.submit(bad)
    for (slot, (head, payload)) in zip(decoder._slots, heads):          # no pinned byte was written
        assert numpy.array_equal(slot.head_host, head) and numpy.array_equal(slot.payload_host, payload)
    small = _decoder(weights, shape, tile, payload_capacity_bytes=16)
    with pytest.raises(ValueError, match='payload'):
        small.submit([(source, 0) + places[2]])
    small.close()
    _check_crops(weights, decoder.submit([ok]), [ok], blobs)          # a refused step leaves the decoder usable
    assert decoder in codec._LIVE[decoder.device.index]
    decoder.close()
    decoder.close()
    assert decoder not in codec._LIVE[decoder.device.index]
    with pytest.raises(RuntimeError):
        decoder.submit([ok])
    # the constructor refuses before it allocates anything (the closed decoders above are collected first: their slots' memory
    # must not come back while the refusals run)
    del small
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for bad in ((0, 2), (2, -1), (2,), 2, (2.0, 2), (True, 2), 'ab', (70000, 2)):
        with pytest.raises(ValueError, match='coding_tile|coding tile'):
            _decoder(weights, shape, bad)
    build = lambda **more: codec.RegionDecoder(weights['variables'], False, more.pop('batch_size', BATCH), more.pop('h_in', shape[0]),
                                                more.pop('w_in', shape[1]), more.pop('length', weights['length']),
                                                coding_tile=more.pop('coding_tile', tile), region=more.pop('region', REGION), **more)
    for (more, match) in (({'region': (0, 48)}, 'region'), ({'region': (32,)}, 'region'), ({'region': (shape[0] + 1, 48)}, 'region'),
                          ({'h_in': 100}, 'strides'), ({'length': 0}, 'unary'), ({'length': 256}, 'unary'), ({'batch_size': 0}, 'batch_size'),
                          ({'payload_capacity_bytes': 0}, 'payload_capacity_bytes'),
                          ({'h_in': 1024, 'w_in': 1024, 'coding_tile': (1, 1), 'batch_size': 2000}, '65535'),          # 2,000 crops of 42 slots
                          ({'h_in': 8208, 'w_in': 8208, 'coding_tile': (16, 16), 'region': (8200, 8200), 'batch_size': 1}, 'window')):
        with pytest.raises(ValueError, match=match):
            build(**more)
    gc.collect()
    assert torch.cuda.memory_allocated() == before


# ---- slot discipline -----------------------------------------------------------------------------------------------------------------------

def _poison_between_steps(decoder, guard, poison):
    """Every buffer a step must not depend on is filled with the poison: the SCRATCH entries of tests/slot_buffers.py for the lane and
    the slot the region decoder shares with `BatchDecoder` (NOT among them: `head_bytes` and the decoder's static tables, constants;
    `seq_dev` / `pinned_seq`, the step counter). `head` is filled field by field: the alignment gaps between its fields keep what
    they held. No kernel reads them, and `check_tiling` bounds them by `max_gap=15` bytes."""
    decoder.drain()
    guard.check(keep=True)
    assert slot_buffers.poison_scratch(decoder, poison) > 0


@pytest.mark.parametrize('fetch', [True, False])
@pytest.mark.parametrize('case', ['four_classes', 'window_is_the_plane'])
def test_steps_on_poisoned_slots(weights, case, fetch):
    """A `use_graphs` decoder inside `guarded.guarded((device, pipeline, codec), poison)`: between two steps every scratch buffer of
    every lane and slot, device and pinned, is filled with the poison, and the bands are checked. A long payload precedes a short
    one in every slot, a partial step follows a full one; the crops are the references' and the same under both poisons."""
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    (shape, tile, places) = CASES[case]
    long_ = _encoded(weights, shape, tile, 0.05, 67)
    short = _encoded(weights, shape, tile, 1.0, -1, seed=3)
    assert len(long_[0]) > len(short[0])
    seen = {}
    for poison in POISONS:
        with guarded.guarded((device, pipeline, codec), poison) as inner:
            sources = [codec.RegionSource(long_[0]), codec.RegionSource(short[0])]
            blobs = {id(sources[0]): ((case, 'long'),) + long_, id(sources[1]): ((case, 'short'),) + short}
            steps = [[(sources[0], k, y0, x0) for (k, (y0, x0)) in enumerate(places[:3])], [(sources[0], 2) + places[3], (sources[0], 1) + places[4]],
                     [(sources[1], k, y0, x0) for (k, (y0, x0)) in enumerate(places[:3])], [(sources[1], 0) + places[4]],
                     [(sources[0], 1) + places[2], (sources[1], 1) + places[2], (sources[0], 0) + places[3]]]
            with _decoder(weights, shape, tile, use_graphs=True, fetch_reconstruction=fetch) as decoder:
                torch.cuda.synchronize()
                if poison == POISONS[0]:
                    # the classified parts cover the containers of every lane and slot: what is poisoned is all there is
                    checked = [name for (owner, table) in slot_buffers.owners(decoder) for name in slot_buffers.check_tiling(owner, table)]
                    assert 'head' in checked and 'status' in checked
                _poison_between_steps(decoder, inner, poison)          # what construction left is no better than what a step leaves
                values = []
                for requests in steps:
                    values.append(_check_crops(weights, decoder.submit(requests), requests, blobs, fetch).tobytes())
                    assert all(slot.graph is not None for slot in decoder._slots)
                    _poison_between_steps(decoder, inner, poison)
        seen[poison] = values
    assert seen[POISONS[0]] == seen[POISONS[1]]
