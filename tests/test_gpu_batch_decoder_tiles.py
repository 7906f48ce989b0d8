"""`codec.BatchDecoder(coding_tile=...)`: `EAT1` blobs in, reconstructions out, byte for byte what `container.decode_images` gives
for the same blobs. First the kernel it adds, `device.tile_symbols_dequantize_rows`, bit for bit against
`device.tile_symbols_dequantize` called image by image, between guard bands and under two poisons. Then the decoder: launch by launch
and replayed as hipGraphs, fetched to pinned memory and left on the device, on planes whose tiles fall into four, two and one shape
class; steps whose images come from different blobs, partial steps, slots that come round again, blobs straight out of
`codec.BatchCodec(emit_container=True, coding_tile=...)`, a corrupted tile that must stay with its image, the steps it refuses, and
the operating point itself."""
import os

import numpy
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coder_golden.npz')
BATCH = 3
SHAPES = [(48, 80), (64, 96)]          # latent planes 3 x 5 (ragged) and 4 x 6 (even)
TILES = [(2, 2), (2, 4), (16, 16)]     # (2, 2): four shape classes on 3 x 5, one on 4 x 6; (2, 4): four and two; (16, 16): one tile per map


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------

def _dev():
    from autoencoder_based_image_compression_amd import device
    return device


def _int16_poison(byte):
    return numpy.array([byte, byte], dtype=numpy.uint8).view(numpy.int16)[0]


def _kernel_inputs(h, w, coding_tile, poison):
    """Three images of symbols in tile-major runs, the entries in a shuffled order with gaps of 5 symbols (holding the poison)
    between the runs; three different rows of bin widths and of means."""
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
    assert not numpy.array_equal(bin_widths[0], bin_widths[1]) and not numpy.array_equal(means[1], means[2])
    return n, plan, buffer, bin_widths, means


def _image_by_image(dev, guard, inputs, buffer_d, plan, rows_d, mean_d, shape):
    """`tile_symbols_dequantize` once per image of the OUTPUT, with that image's row, into an output of its own."""
    up = inputs.upload
    out = guard.empty(shape, dtype=torch.float32, device='cuda')
    for image in range(shape[0]):
        own = plan[plan[:, 0] == image].copy()
        own[:, 0] = 0
        dev.tile_symbols_dequantize(buffer_d, up(own), own, rows_d[image], None if mean_d is None else mean_d[image], out[image:image + 1])
    return out


def _kernel_outputs(h, w, coding_tile, poison):
    """-> {name: int32 bit patterns} of the rows kernel's outputs, each already held against `tile_symbols_dequantize` image by image.
    Inputs between bands poisoned with `poison`, outputs between bands filled with 0xFF (NaN: an element never written fails)."""
    dev = _dev()
    (inputs, guard) = (guarded.Guard(poison), guarded.Guard(0xFF))
    up = inputs.upload
    (n, plan, buffer, bin_widths, means) = _kernel_inputs(h, w, coding_tile, poison)
    (buffer_d, plan_d, rows_d, mean_d) = (up(buffer), up(plan), up(bin_widths), up(means))
    outs = {}

    def compare(name, got, reference):
        (got, reference) = (got.view(torch.int32).cpu().numpy(), reference.view(torch.int32).cpu().numpy())
        assert numpy.array_equal(got, reference), name
        assert not numpy.isnan(got.view(numpy.float32)).any(), name            # every latent belongs to a tile: nothing keeps the fill
        outs[name] = got

    for (name, mean) in (('mean', mean_d), ('no mean', None)):
        out = guard.empty((n, h, w, 128), dtype=torch.float32, device='cuda')
        assert dev.tile_symbols_dequantize_rows(buffer_d, plan_d, plan, rows_d, mean, out) is out
        compare(name, out, _image_by_image(dev, guard, inputs, buffer_d, plan, rows_d, mean, (n, h, w, 128)))
    # into a sub-plane that cuts through tiles: negative origins, tiles that reach past it, the image order reversed
    (r0, r1, c0, c1) = (h//3, max(h//3 + 1, h - 1), w//4, max(w//4 + 1, w - 2))
    sub_plan = plan.copy()
    sub_plan[:, 0] = n - 1 - sub_plan[:, 0]
    sub_plan[:, 1] -= r0
    sub_plan[:, 2] -= c0
    assert (sub_plan[:, 1:3] < 0).any() or (r0, c0) == (0, 0)
    sub = guard.empty((n, r1 - r0, c1 - c0, 128), dtype=torch.float32, device='cuda')
    dev.tile_symbols_dequantize_rows(buffer_d, up(sub_plan), sub_plan, rows_d, mean_d, sub)
    compare('sub-plane', sub, _image_by_image(dev, guard, inputs, buffer_d, sub_plan, rows_d, mean_d, tuple(sub.shape)))
    torch.cuda.synchronize()
    inputs.check()
    guard.check()
    return outs


@pytest.mark.parametrize('h, w, coding_tile', [(5, 7, (2, 3)), (3, 2, (1, 1)), (9, 70, (9, 65))])
def test_the_rows_kernel_is_the_kernel_image_by_image(h, w, coding_tile):
    first = _kernel_outputs(h, w, coding_tile, 0xFF)
    again = _kernel_outputs(h, w, coding_tile, 0x7F)
    assert sorted(first) == sorted(again) == ['mean', 'no mean', 'sub-plane']
    for name in first:           # the defined outputs do not depend on what lies around the inputs
        assert first[name].tobytes() == again[name].tobytes(), name
    # and the rows are what make the images differ: image 1 with image 0's row is another plane
    assert not numpy.array_equal(first['mean'][0], first['mean'][1])


def test_the_rows_kernel_refuses_before_any_launch():
    dev = _dev()
    (n, plan, buffer, bin_widths, means) = _kernel_inputs(5, 7, (2, 3), 0xFF)
    (buffer_d, plan_d) = (torch.from_numpy(buffer).cuda(), torch.from_numpy(plan).cuda())
    (rows_d, mean_d) = (torch.from_numpy(bin_widths).cuda(), torch.from_numpy(means).cuda())
    out = torch.full((n, 5, 7, 128), 7., device='cuda')
    for (row, col, value) in ((0, 0, n), (1, 0, -1), (0, 3, 0), (2, 4, 0), (0, 5, buffer.size), (1, 5, -1)):          # malformed plan rows
        bad = plan.copy()
        bad[row, col] = value
        with pytest.raises(dev.HipError):
            dev.tile_symbols_dequantize_rows(buffer_d, torch.from_numpy(bad).cuda(), bad, rows_d, mean_d, out)
    with pytest.raises(dev.HipError):                                                                                  # the two plans differ in shape
        dev.tile_symbols_dequantize_rows(buffer_d, plan_d[:-1], plan, rows_d, mean_d, out)
    for (rows, mean) in ((rows_d[:2], mean_d), (rows_d, mean_d[:2]), (rows_d[0], mean_d), (rows_d, mean_d[0]),        # the wrong size
                         (rows_d.double(), mean_d), (rows_d, mean_d.double()), (rows_d.half(), None),                  # the wrong dtype
                         (rows_d.t(), mean_d)):                                                                        # not contiguous
        with pytest.raises(dev.HipError):
            dev.tile_symbols_dequantize_rows(buffer_d, plan_d, plan, rows, mean, out)
    with pytest.raises(dev.HipError):
        dev.tile_symbols_dequantize_rows(buffer_d.int(), plan_d, plan, rows_d, mean_d, out)
    with pytest.raises(dev.HipError):
        dev.tile_symbols_dequantize_rows(buffer_d, plan_d, plan, rows_d, mean_d, out[..., :64])
    torch.cuda.synchronize()
    assert bool((out == 7.).all())                                                                                     # nothing was launched


# ---- the decoder -----------------------------------------------------------------------------------------------------------------------

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


def _encoded(model, shape, tile, scale, idx_map_exception, seed=0, count=BATCH):
    """Once per case, shared by every test that needs it: (`EAT1` blob, `decode_images` of it). tile=None: the `EAE1` blob."""
    from autoencoder_based_image_compression_amd import container
    key = (shape, tile, scale, idx_map_exception, seed, count)
    if key not in model['cache']:
        bin_widths = numpy.full(128, scale, dtype=numpy.float32)
        map_mean = numpy.random.RandomState(shape[1] + seed).normal(scale=0.1, size=128).astype(numpy.float32)
        (blob, _) = container.encode_images(_images(shape, seed, count), model['encoder'], bin_widths, map_mean, model['probabilities'],
                                            idx_map_exception, coding_tile=tile)
        assert bytes(blob[:4]) == (container.TILE_MAGIC if tile is not None else container.MAGIC)
        expected = container.decode_images(blob, model['decoder'])
        expected.setflags(write=False)
        model['cache'][key] = (blob, expected)
    return model['cache'][key]


def _decoder(model, shape, tile, **arguments):
    from autoencoder_based_image_compression_amd import codec
    # (these random weights code the small bin width at more than the default capacity's 8 bits per pixel, the more so in tiles)
    arguments.setdefault('payload_capacity_bytes', 8*BATCH*shape[0]*shape[1])
    arguments.setdefault('nb_in_flight', 2)
    arguments.setdefault('nb_streams', 1)
    arguments.setdefault('batch_size', BATCH)
    batch = arguments.pop('batch_size')
    return codec.BatchDecoder(model['variables'], False, batch, shape[0], shape[1], model['length'], coding_tile=tile, **arguments)


def _array(result):
    return result.cpu().numpy() if isinstance(result, torch.Tensor) else numpy.array(result)


@pytest.mark.parametrize('fetch', [True, False])
@pytest.mark.parametrize('graphs', [False, True])
@pytest.mark.parametrize('scale,idx_map_exception', [(1.0, 67), (1.0, -1), (0.05, 67), (0.05, -1)])
@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('shape', SHAPES)
def test_a_blob_decodes_to_what_decode_images_gives(model, shape, tile, scale, idx_map_exception, graphs, fetch):
    (blob, expected) = _encoded(model, shape, tile, scale, idx_map_exception)
    with _decoder(model, shape, tile, use_graphs=graphs, fetch_reconstruction=fetch) as decoder:
        assert decoder.coding_tile == (min(tile[0], shape[0]//16), min(tile[1], shape[1]//16))
        for _ in range(3):                     # the launch-by-launch step, then (with graphs) replays of two slots
            ticket = decoder.submit(blob)
            result = ticket.result()
            assert isinstance(result, numpy.ndarray if fetch else torch.Tensor)
            assert result.shape == expected.shape and result.dtype == (numpy.uint8 if fetch else torch.uint8)
            assert numpy.array_equal(_array(result), expected)
            assert ticket.errors == [None]*BATCH and ticket.nb_images == BATCH


@pytest.mark.parametrize('graphs', [False, True])
@pytest.mark.parametrize('shape,tile', [(SHAPES[0], (2, 2)), (SHAPES[1], (2, 4))])
def test_mixed_and_partial_steps(model, shape, tile, graphs):
    """Three single-image blobs at three bin widths, with two exception indices and without one, in one step, in two orders; then two
    of three images (one blob of two, and two blobs of one); then one; then the full step again: every image equals `decode_images`
    of its own blob."""
    singles = [_encoded(model, shape, tile, scale, idx, seed=seed, count=1) for (seed, (scale, idx)) in enumerate([(1.0, 67), (0.05, 5), (0.3, -1)])]
    (pair_blob, pair_expected) = _encoded(model, shape, tile, 0.05, 67, seed=7, count=2)
    with _decoder(model, shape, tile, use_graphs=graphs) as decoder:
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
    (shape, tile) = (SHAPES[0], (2, 2))
    sets = [_encoded(model, shape, tile, 0.05, 67), _encoded(model, shape, tile, 1.0, -1, seed=3)]
    assert len(sets[0][0]) != len(sets[1][0]) and not numpy.array_equal(sets[0][1], sets[1][1])
    with _decoder(model, shape, tile, use_graphs=True, nb_streams=2, nb_in_flight=3) as decoder:
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
    """BatchCodec(emit_container=True, coding_tile=(2, 4)) -> the step's `EAT1` blob and its per-image blobs -> BatchDecoder of the
    same tile -> the codec's own reconstruction."""
    from autoencoder_based_image_compression_amd import codec, container
    (shape, tile) = (SHAPES[1], (2, 4))
    bin_widths = numpy.full(128, 0.5, dtype=numpy.float32)
    map_mean = numpy.random.RandomState(11).normal(scale=0.1, size=128).astype(numpy.float32)
    images = torch.from_numpy(_images(shape, 5)).cuda()
    with codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], idx_map_exception, BATCH, *shape,
                          keep_reconstruction=True, emit_container=True, coding_tile=tile) as encoder:
        ticket = encoder.submit(images)
        ticket.result()
        (blob, image_blobs) = (ticket.container(), ticket.image_containers())
        reconstruction = ticket.reconstruction_uint8.cpu().numpy()
    assert bytes(blob[:4]) == container.TILE_MAGIC and len(image_blobs) == BATCH
    with _decoder(model, shape, tile, use_graphs=True) as decoder:
        assert numpy.array_equal(decoder.submit(blob).result(), reconstruction)
        assert numpy.array_equal(decoder.submit(image_blobs).result(), reconstruction)
        assert numpy.array_equal(decoder.submit(image_blobs[::-1]).result(), reconstruction[::-1])


def _outcome(call):
    try:
        return ('bytes', call())
    except Exception as exc:
        return ('error', type(exc), str(exc))


@pytest.mark.parametrize('graphs', [False, True])
def test_a_corrupted_tile_stays_with_its_image(model, graphs):
    """One image's payload altered (a byte flipped in the middle of the longest arithmetic-coded stream over all its tiles, the
    header still valid): that image's outcome is `decode_images`' on its own blob -- the same exception, or the same bytes --, its
    neighbours are their clean decode, and so is the next step."""
    from autoencoder_based_image_compression_amd import container
    (shape, tile) = ((128, 192), (4, 8))
    singles = [_encoded(model, shape, tile, 0.05, 67, seed=20 + k, count=1) for k in range(3)]
    header = container.read_header(singles[1][0])
    assert header['format'] == 'EAT1' and header['bits'].shape == (1, 4, 128, 2)
    sizes = (header['bits'].astype(numpy.int64).reshape(-1, 2) + 7)//8          # payload order: tile -> map -> piece
    longest = int(numpy.argmax(sizes[:, 0]))
    assert sizes[longest, 0] >= 8
    position = header['payload_offset'] + int(sizes.reshape(-1)[:2*longest].sum()) + int(sizes[longest, 0])//2
    corrupted = bytearray(singles[1][0])
    corrupted[position] ^= 0xFF
    corrupted = bytes(corrupted)
    assert container.read_header(corrupted)['payload_offset'] == header['payload_offset']
    expected = _outcome(lambda: container.decode_images(corrupted, model['decoder']))
    with _decoder(model, shape, tile, use_graphs=graphs) as decoder:
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
    from autoencoder_based_image_compression_amd import codec
    (shape, tile) = (SHAPES[0], (2, 2))
    (blob, expected) = _encoded(model, shape, tile, 1.0, 67)
    (plain, plain_expected) = _encoded(model, shape, None, 1.0, 67)
    (other_tile, _) = _encoded(model, shape, (2, 4), 1.0, 67)
    (other_size, _) = _encoded(model, SHAPES[1], tile, 1.0, 67)
    decoder = _decoder(model, shape, tile, payload_capacity_bytes=len(blob))
    for (bad, match) in ((plain, 'coding_tile'), (other_tile, 'coding_tile'), (other_size, 'images'), ([blob, blob], 'images'), (blob[:-1], None)):
        with pytest.raises(ValueError, match=match):
            decoder.submit(bad)
    small = _decoder(model, shape, tile, payload_capacity_bytes=64)
    with pytest.raises(ValueError, match='payload'):
        small.submit(blob)
    small.close()
    assert numpy.array_equal(decoder.submit(blob).result(), expected)          # a refused step leaves the decoder usable
    decoder.close()
    decoder.close()
    with pytest.raises(RuntimeError):
        decoder.submit(blob)
    # the constructor refuses a bad tile, and more (image, tile) pairs than a step can hold, before it allocates anything
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for bad in ((0, 2), (2, -1), (2,), (2, 2, 2), 2, (2.0, 2), (True, 2), 'ab', (70000, 2), (2, 65536)):
        with pytest.raises(ValueError, match='coding_tile|coding tile'):
            _decoder(model, shape, bad)
    with pytest.raises(ValueError, match='65535'):
        _decoder(model, (1024, 1024), (1, 1), batch_size=16)                   # 16 x 4,096 pairs
    assert torch.cuda.memory_allocated() == before
    # a decoder built without `coding_tile` still refuses EAT1, with the function that reads such blobs, and reads EAE1
    with codec.BatchDecoder(model['variables'], False, BATCH, shape[0], shape[1], model['length'], nb_in_flight=2, nb_streams=1,
                            payload_capacity_bytes=len(plain)) as untiled:
        assert untiled.coding_tile is None
        with pytest.raises(ValueError, match='decode_region'):
            untiled.submit(blob)
        assert numpy.array_equal(untiled.submit(plain).result(), plain_expected)


def test_kodak_sized_steps_in_tiles_of_16(model):
    """The operating point itself: 24 images of 512 x 768 per step in tiles of (16, 16) -- six tiles a map, 18,432 pairs of streams a
    step --, graphs on, two streams, a few steps in flight, then a drain: every step reports no error, and the steps whose planes are
    still valid hold the bytes of `decode_images`."""
    from autoencoder_based_image_compression_amd import codec, container
    (batch, shape, tile) = (24, (512, 768), (16, 16))
    bin_widths = numpy.ones(128, dtype=numpy.float32)
    map_mean = numpy.random.RandomState(5).normal(scale=0.1, size=128).astype(numpy.float32)
    images = numpy.concatenate([_images(shape, seed, 3) for seed in range(batch//3)])
    (blob, _) = container.encode_images(images, model['encoder'], bin_widths, map_mean, model['probabilities'], 67, coding_tile=tile)
    expected = container.decode_images(blob, model['decoder'])
    with codec.BatchDecoder(model['variables'], False, batch, shape[0], shape[1], model['length'], payload_capacity_bytes=len(blob),
                            use_graphs=True, nb_streams=2, nb_in_flight=4, coding_tile=tile) as full:
        assert full._n_streams == batch*6*128
        tickets = [full.submit(blob) for _ in range(8)]
        full.drain()
        for (step, ticket) in enumerate(tickets):
            ticket.result(raise_errors=False)
            assert ticket.errors == [None]*batch, (step, [repr(e) for e in ticket.errors if e is not None][:3])
        for ticket in tickets[-full.nb_slots:]:
            assert numpy.array_equal(ticket.result(), expected)
