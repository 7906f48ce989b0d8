"""The tile-indexed container EAT1 on the device (container.py, csrc/hip/tile_symbols.hip): with one tile
per map it is EAE1's payload; every tile's streams are the host coder's on that tile's symbols; full and region decodes equal the
in-memory path and its crops bit for bit; a region decode reads and depends on the listed tiles only; the two kernels
(eae_hip_tile_symbols_gather, eae_hip_tile_symbols_dequantize) equal numpy slicing and dequantize_maps; and a 16384 x 8192 image
codes with memory bounded by one group."""
import io
import os

import numpy
import pytest
import torch

from unary_length_cases import host_encode_maps

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _guarded_buffers(request):
    """Every test of this module runs on poisoned buffers between guard bands: what device.py / pipeline.py allocate holds 0xFF bytes
    (NaN, -1) until a kernel writes it, and a byte written outside a tensor fails the test (tests/guarded.py). The guard keeps its
    allocations until the test ends, and test_a_large_image_with_coding_tiles bounds the peak of allocated memory over four groups
    of tiles: there only requests of up to 1 MB are guarded (the per-group streams, symbols and workspaces are torch's own)."""
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    limits = {'passthrough_bytes': 1 << 20} if request.node.name == 'test_a_large_image_with_coding_tiles' else {}
    with guarded.guarded((device, pipeline), 0xFF, **limits):
        yield


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coder_golden.npz')


@pytest.fixture(scope='module')
def model():
    from autoencoder_based_image_compression_amd import pipeline
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    v = var.random_variables(1., False, seed=4, bias_std=0.01)
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    with numpy.load(GOLD) as g:
        probabilities = g['real_probabilities_1']
    return {'variables': v, 'encoder': pipeline.DeviceEncoder(v, False), 'decoder': pipeline.DeviceDecoder(v, False),
            'probabilities': probabilities}


def _images(seed, shape):
    rng = numpy.random.RandomState(seed)
    x = rng.randint(16, 236, size=shape).astype(numpy.float32)
    x = (x + numpy.roll(x, 1, 1) + numpy.roll(x, 1, 2))/numpy.float32(3.)
    return numpy.round(x).astype(numpy.uint8)


def in_memory_path(model, images, bin_widths, map_mean):
    from autoencoder_based_image_compression_amd import device as dev
    y = model['encoder'](torch.from_numpy(images).cuda())
    q = dev.quantize_maps(y, torch.from_numpy(bin_widths).cuda(), torch.from_numpy(map_mean).cuda(), want_shifted=True, want_symbols=True)
    (_, rec, _) = model['decoder'](q['shifted'])
    return q['symbols'].cpu().numpy(), rec.cpu().numpy()


def _encode(model, images, scale, idx_map_exception, **kwargs):
    from autoencoder_based_image_compression_amd import container
    rng = numpy.random.RandomState(images.shape[1] + images.shape[2])
    bin_widths = numpy.full(128, scale, dtype=numpy.float32)
    map_mean = rng.normal(scale=0.1, size=128).astype(numpy.float32)
    (blob, info) = container.encode_images(images, model['encoder'], bin_widths, map_mean, model['probabilities'], idx_map_exception,
                                           **kwargs)
    return blob, info, bin_widths, map_mean


@pytest.mark.parametrize('coding_tile', [(4, 6), (100, 100), (4, 7)])
def test_one_tile_per_map_is_the_eae1_payload(model, coding_tile):
    """coding_tile >= (h, w): the EAT1 payload is EAE1's byte for byte, and both decode to the same images."""
    from autoencoder_based_image_compression_amd import container
    images = _images(1, (2, 64, 96))
    (blob, info, bw, mean) = _encode(model, images, 0.5, 67)
    (tiled, tiled_info, _, _) = _encode(model, images, 0.5, 67, coding_tile=coding_tile)
    header = container.read_header(blob)
    tile_header = container.read_header(tiled)
    assert tiled[:4] == b'EAT1' and tile_header['coding_tile'] == (4, 6)
    assert tiled[tile_header['payload_offset']:] == blob[header['payload_offset']:]
    assert numpy.array_equal(tile_header['bits'].reshape(-1, 2), header['bits'])
    assert numpy.array_equal(tiled_info['nb_bits'], info['nb_bits'])
    assert len(tiled) == tiled_info['header_bytes'] + tiled_info['payload_bytes']
    rec = container.decode_images(blob, model['decoder'])
    assert numpy.array_equal(container.decode_images(tiled, model['decoder']), rec)
    assert numpy.array_equal(rec, in_memory_path(model, images, bw, mean)[1])


def test_eae1_is_one_group_of_whole_maps_without_a_copy(model, monkeypatch):
    """EAE1 through the group coder: one tile per map and all images in one group whatever `tiles_per_call` says, so one coder batch
    over 3 x 128 maps each way, and the symbols are coded where the quantiser left them: no gather launch."""
    from autoencoder_based_image_compression_amd import container
    from autoencoder_based_image_compression_amd import device as dev
    images = _images(21, (3, 32, 48))
    (expected, _, bw, mean) = _encode(model, images, 0.5, 67)
    (encode_batch, decode_batch, gather) = (dev.coder_encode_batch, dev.coder_decode_batch, dev.tile_symbols_gather)
    calls = {'encode': [], 'decode': [], 'gather': 0}

    def counting_encode(symbols_planar, *args, **kwargs):
        calls['encode'].append(symbols_planar.numel()//symbols_planar.shape[-1])
        return encode_batch(symbols_planar, *args, **kwargs)

    def counting_decode(streams, *args, **kwargs):
        calls['decode'].append(streams.n_maps)
        return decode_batch(streams, *args, **kwargs)

    def counting_gather(*args, **kwargs):
        calls['gather'] += 1
        return gather(*args, **kwargs)

    monkeypatch.setattr(dev, 'coder_encode_batch', counting_encode)
    monkeypatch.setattr(dev, 'coder_decode_batch', counting_decode)
    monkeypatch.setattr(dev, 'tile_symbols_gather', counting_gather)
    (blob, _, _, _) = _encode(model, images, 0.5, 67, tiles_per_call=1)
    assert calls == {'encode': [384], 'decode': [], 'gather': 0}
    reconstruction = container.decode_images(blob, model['decoder'], tiles_per_call=1)
    assert calls == {'encode': [384], 'decode': [384], 'gather': 0}
    assert blob[:4] == b'EAE1' and blob == expected
    assert numpy.array_equal(reconstruction, in_memory_path(model, images, bw, mean)[1])


@pytest.mark.parametrize('idx_map_exception', [67, -1])
@pytest.mark.parametrize('shape, coding_tile, scale', [((3, 80, 112), (2, 3), 0.05), ((1, 48, 64), (1, 1), 0.5),
                                                       ((2, 96, 80), (4, 2), 0.05)])
def test_every_tile_is_the_host_coder_on_its_symbols(model, shape, coding_tile, scale, idx_map_exception):
    """Each (image, tile)'s streams, bytes and both bit counts, equal eae_coder_encode_maps run on that tile's symbols, sliced by
    numpy from quantize_maps' output. The small bin width produces Exp-Golomb escapes."""
    from autoencoder_based_image_compression_amd import container
    images = _images(shape[1], shape)
    (blob, info, bw, mean) = _encode(model, images, scale, idx_map_exception, coding_tile=coding_tile, tiles_per_call=5)
    (symbols, _) = in_memory_path(model, images, bw, mean)
    header = container.read_header(blob)
    (h, w) = (shape[1]//16, shape[2]//16)
    symbols = symbols.reshape(shape[0], 128, h, w)
    if scale < 0.1:
        assert numpy.abs(symbols).max() > 10
    (tiles, _) = container.coding_tile_grid(h, w, coding_tile)
    table = numpy.concatenate([model['probabilities'], header['exception_probabilities']])
    plan = container.region_plan(header, (0, 0, shape[1], shape[2]))
    ranges = dict(zip(plan['entries'], plan['ranges']))
    assert numpy.array_equal(info['tile_bits'], header['bits'])
    for i in range(shape[0]):
        prob_row = numpy.arange(128, dtype=numpy.int32)
        if idx_map_exception >= 0:
            prob_row[idx_map_exception] = 128 + i
        for (t, (r0, c0, rows, cols, _)) in enumerate(tiles.tolist()):
            planar = symbols[i, :, r0:r0 + rows, c0:c0 + cols].reshape(128, rows*cols)
            (streams, stride, bac, byp) = host_encode_maps(planar, table, prob_row)
            assert numpy.array_equal(header['bits'][i, t, :, 0], bac) and numpy.array_equal(header['bits'][i, t, :, 1], byp), (i, t)
            expected = b''.join(streams[m, :(int(bac[m]) + 7)//8].tobytes() + streams[m, stride//2:stride//2 + (int(byp[m]) + 7)//8].tobytes()
                                for m in range(128))
            (a, b) = ranges[(i, t)]
            assert blob[a:b] == expected, (i, t)


@pytest.mark.parametrize('tile', [None, (2, 3)])
def test_full_decode_equals_the_in_memory_path(model, tile):
    from autoencoder_based_image_compression_amd import container
    shape = (3, 80, 112)
    images = _images(7, shape)
    (blob, _, bw, mean) = _encode(model, images, 0.05, 67, coding_tile=(2, 3), tiles_per_call=4)
    (symbols, rec) = in_memory_path(model, images, bw, mean)
    symbols = symbols.reshape(3, 128, 5, 7)
    (header, decoded) = container.decode_tile_symbols(blob, tiles_per_call=7)
    (tiles, _) = container.coding_tile_grid(5, 7, (2, 3))
    for i in range(3):
        for (t, (r0, c0, rows, cols, _)) in enumerate(tiles.tolist()):
            assert numpy.array_equal(decoded[i][t].cpu().numpy(), symbols[i, :, r0:r0 + rows, c0:c0 + cols]), (i, t)
    assert numpy.array_equal(container.decode_images(blob, model['decoder'], tile=tile), rec)
    assert numpy.array_equal(container.decode_images(blob, model['decoder'], tile=tile, tiles_per_call=1), rec)
    with pytest.raises(ValueError):
        container.decode_symbols(blob)
    # the transform windows combine with the coding tiles on the encoder side too
    (blob_windows, _, _, _) = _encode(model, images, 0.05, 67, coding_tile=(2, 3), tile=(2, 2))
    assert blob_windows == blob


def _regions(height, width):
    return [(0, 0, 24, 40), (0, width - 40, 24, 40), (height - 24, 0, 24, 40), (height - 24, width - 40, 24, 40), (0, 0, 1, 1),
            (height - 1, width - 1, 1, 1), (37, 53, 1, 1), (13, 0, 29, width), (0, 29, height, 3), (31, 45, 35, 50), (17, 47, 2, 2),
            (0, 0, height, width), (5, 9, height - 11, width - 23)]


@pytest.mark.parametrize('kind', ['EAT1', 'EAE1'])
def test_region_decode_equals_the_crop(model, kind):
    from autoencoder_based_image_compression_amd import container
    shape = (3, 96, 128)
    images = _images(9, shape)
    kwargs = {'coding_tile': (2, 3)} if kind == 'EAT1' else {}
    (blob, _, _, _) = _encode(model, images, 0.5, 67, **kwargs)
    full = container.decode_images(blob, model['decoder'])
    for region in _regions(96, 128):
        (y0, x0, rh, rw) = region
        crop = full[:, y0:y0 + rh, x0:x0 + rw]
        assert numpy.array_equal(container.decode_region(blob, model['decoder'], region), crop), region
    for (region, subset) in (((31, 45, 35, 50), [2, 0]), ((0, 0, 96, 128), [1]), ((95, 0, 1, 128), [0, 2])):
        (y0, x0, rh, rw) = region
        out = container.decode_region(io.BytesIO(blob), model['decoder'], region, images=subset, tile=(2, 2), tiles_per_call=3)
        assert numpy.array_equal(out, full[subset, y0:y0 + rh, x0:x0 + rw]), (region, subset)


class CountingFile(io.BytesIO):
    def __init__(self, data):
        super().__init__(data)
        self.nbytes = 0

    def read(self, size=-1):
        data = super().read(size)
        self.nbytes += len(data)
        return data


def test_region_decode_is_local(model):
    """Bytes of tiles the plan does not list do not matter; a flipped byte of a listed tile changes the result or raises the
    coder's error, and the device stays in working order. Through a file, exactly the header and the listed ranges are read."""
    from autoencoder_based_image_compression_amd import container
    images = _images(13, (2, 128, 160))
    (blob, _, _, _) = _encode(model, images, 0.5, 67, coding_tile=(2, 2))
    region = (50, 70, 20, 20)
    header = container.read_header(blob)
    plan = container.region_plan(header, region, images=[1])
    expected = container.decode_region(blob, model['decoder'], region, images=[1])
    listed = numpy.zeros(len(blob), dtype=bool)
    for (a, b) in plan['ranges']:
        listed[a:b] = True
    outside = numpy.flatnonzero(~listed[header['payload_offset']:]) + header['payload_offset']
    assert outside.size > 0.5*(len(blob) - header['payload_offset'])
    mutated = numpy.frombuffer(blob, dtype=numpy.uint8).copy()
    mutated[outside] ^= 0xA5
    assert numpy.array_equal(container.decode_region(mutated.tobytes(), model['decoder'], region, images=[1]), expected)
    f = CountingFile(mutated.tobytes())
    assert numpy.array_equal(container.decode_region(f, model['decoder'], region, images=[1]), expected)
    assert f.nbytes == header['payload_offset'] + sum(b - a for (a, b) in plan['ranges'])
    # a byte of a listed tile
    (a, b) = plan['ranges'][len(plan['ranges'])//2]
    corrupted = numpy.frombuffer(blob, dtype=numpy.uint8).copy()
    corrupted[a:b:16] ^= 0xFF
    try:
        assert not numpy.array_equal(container.decode_region(corrupted.tobytes(), model['decoder'], region, images=[1]), expected)
    except RuntimeError:
        pass
    assert numpy.array_equal(container.decode_region(blob, model['decoder'], region, images=[1]), expected)


def _gather_plan(entries, tiles, pad=0):
    """Plan rows and buffer size for (image, tile) entries laid out in the given order, `pad` symbols between runs."""
    (rows, pos) = ([], 0)
    for (i, t) in entries:
        (r0, c0, nr, nc) = (int(x) for x in tiles[t, :4])
        rows.append((i, r0, c0, nr, nc, pos))
        pos += 128*nr*nc + pad
    return numpy.array(rows, dtype=numpy.int64).reshape(-1, 6), pos


@pytest.mark.parametrize('h, w, coding_tile', [(5, 7, (2, 3)), (17, 25, (4, 6)), (3, 2, (1, 1)), (9, 70, (9, 65))])
def test_the_kernels_equal_numpy_and_dequantize_maps(h, w, coding_tile):
    """Gather against numpy slicing; scatter-dequantise against dequantize_maps + slicing as int32 bit patterns. Several shape
    classes in one launch, entries in a shuffled order and with gaps between the runs."""
    from autoencoder_based_image_compression_amd import container
    from autoencoder_based_image_compression_amd import device as dev
    n = 2
    rng = numpy.random.RandomState(h*w)
    symbols = rng.randint(-300, 300, size=(n, 128, h*w)).astype(numpy.int16)
    (tiles, classes) = container.coding_tile_grid(h, w, coding_tile)
    entries = [(i, t) for i in range(n) for t in range(len(tiles))]
    entries = [entries[k] for k in rng.permutation(len(entries))]
    (plan, total) = _gather_plan(entries, tiles, pad=3)
    buffer = torch.full((total,), -7, dtype=torch.int16, device='cuda')
    symbols_d = torch.from_numpy(symbols).cuda()
    plan_d = torch.from_numpy(plan).cuda()
    dev.tile_symbols_gather(symbols_d, buffer, plan_d, plan, h, w)
    got = buffer.cpu().numpy()
    grid = symbols.reshape(n, 128, h, w)
    for (i, r0, c0, nr, nc, off) in plan.tolist():
        assert numpy.array_equal(got[off:off + 128*nr*nc], grid[i, :, r0:r0 + nr, c0:c0 + nc].reshape(-1))
        assert (got[off + 128*nr*nc:off + 128*nr*nc + 3] == -7).all()
    # dequantise the whole plane from the tiles, and a sub-plane that cuts through tiles, against dequantize_maps
    bw = torch.from_numpy(rng.uniform(0.01, 3., size=128).astype(numpy.float32)).cuda()
    mean = torch.from_numpy(rng.normal(size=128).astype(numpy.float32)).cuda()
    reference = dev.dequantize_maps(symbols_d, bw, mean)['shifted'].view(n, h, w, 128)
    reference_no_mean = dev.dequantize_maps(symbols_d, bw, None)['shifted'].view(n, h, w, 128)
    out = torch.full((n, h, w, 128), float('nan'), device='cuda')
    dev.tile_symbols_dequantize(buffer, plan_d, plan, bw, mean, out)
    assert torch.equal(out.view(torch.int32), reference.view(torch.int32))
    out = torch.full((n, h, w, 128), float('nan'), device='cuda')
    dev.tile_symbols_dequantize(buffer, plan_d, plan, bw, None, out)
    assert torch.equal(out.view(torch.int32), reference_no_mean.view(torch.int32))
    (r0, r1, c0, c1) = (h//3, max(h//3 + 1, h - 1), w//4, max(w//4 + 1, w - 2))
    sub_plan = plan.copy()
    sub_plan[:, 0] = 1 - sub_plan[:, 0]                        # image order reversed in the output
    sub_plan[:, 1] -= r0
    sub_plan[:, 2] -= c0
    sub = torch.full((n, r1 - r0, c1 - c0, 128), 5., device='cuda')
    dev.tile_symbols_dequantize(buffer, torch.from_numpy(sub_plan).cuda(), sub_plan, bw, mean, sub)
    assert torch.equal(sub.view(torch.int32), reference.flip(0)[:, r0:r1, c0:c1].contiguous().view(torch.int32))
    # malformed plans are refused on the host, before any launch
    for (row, col, value) in ((0, 0, n), (0, 1, h), (0, 3, 0), (0, 5, total)):
        bad = plan.copy()
        bad[row, col] = value
        with pytest.raises(dev.HipError):
            dev.tile_symbols_gather(symbols_d, buffer, torch.from_numpy(bad).cuda(), bad, h, w)
        if col != 1:
            with pytest.raises(dev.HipError):
                dev.tile_symbols_dequantize(buffer, torch.from_numpy(bad).cuda(), bad, bw, mean, out)
    torch.cuda.synchronize()
    assert len(classes) >= 1


def test_the_gather_reaches_past_2_gb():
    """A symbol plane of 2.16 GB (1 x 128 x 4112 x 2048 int16): tiles of the last maps at its far end are read through the 64-bit
    offsets, and dequantised back into a sub-plane."""
    from autoencoder_based_image_compression_amd import device as dev
    (h, w, k) = (4112, 2048, 37)
    symbols = torch.zeros((1, 128, h*w), dtype=torch.int16, device='cuda')
    assert symbols.numel()*2 > 2**31
    far = torch.randint(-999, 999, (128, k, k), dtype=torch.int16, device='cuda')
    symbols.view(1, 128, h, w)[0, :, h - k:, w - k:] = far
    plan = numpy.array([[0, h - k, w - k, k, k, 0], [0, h - k, 0, k, 3, 128*k*k]], dtype=numpy.int64)
    buffer = torch.empty(128*k*(k + 3), dtype=torch.int16, device='cuda')
    dev.tile_symbols_gather(symbols, buffer, torch.from_numpy(plan).cuda(), plan, h, w)
    assert torch.equal(buffer[:128*k*k].view(128, k, k), far)
    assert torch.equal(buffer[128*k*k:].view(128, k, 3), symbols.view(1, 128, h, w)[0, :, h - k:, :3])
    bw = torch.full((128,), 0.5, device='cuda')
    out = torch.empty((1, k, k, 128), device='cuda')
    rows = plan[:1].copy()
    rows[0, 1:3] = 0
    dev.tile_symbols_dequantize(buffer, torch.from_numpy(rows).cuda(), rows, bw, None, out)
    assert torch.equal(out[0], far.permute(1, 2, 0).float()*0.5)


def test_a_large_image_with_coding_tiles():
    """16384 x 8192 with transform windows and coding tiles of 64: the full decode equals the in-memory reconstruction, a 512 x 512
    interior region equals its crop, and the coding stage's peak allocation stays within one group of streams + workspace."""
    from autoencoder_based_image_compression_amd import _native
    from autoencoder_based_image_compression_amd import container
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd import pipeline
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    (H, W, tile, per_call) = (16384, 8192, (64, 64), 32)
    v = var.random_variables(1., False, seed=0, bias_std=0.01)
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    encoder = pipeline.DeviceEncoder(v, False)
    decoder = pipeline.DeviceDecoder(v, False)
    x = _images(51, (1, H, W))
    rng = numpy.random.RandomState(52)
    bw = numpy.ones(128, dtype=numpy.float32)
    mean = (rng.standard_normal(128)*0.05).astype(numpy.float32)
    probabilities = numpy.clip(rng.rand(128, 10), 0.05, 0.95)
    xd = torch.from_numpy(x).cuda()
    y = encoder(xd, tile=tile)
    q = dev.quantize_maps(y, torch.from_numpy(bw).cuda(), torch.from_numpy(mean).cuda(), want_shifted=True, want_symbols=True)
    (_, rec, _) = decoder(q['shifted'], tile=tile)
    rec = rec.cpu().numpy()
    del q, y
    # the coding stage alone: symbols in, blob out
    symbols = dev.quantize_maps(encoder(xd, tile=tile), torch.from_numpy(bw).cuda(), torch.from_numpy(mean).cuda(),
                                want_symbols=True)['symbols']
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fields = container._fields(False, 1, H, W, -1, bw, mean, probabilities, numpy.zeros((0, 10)), coding_tile=tile)
    (blob, _) = container._encode_entries(symbols, fields, per_call)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    lib = _native.hip()
    size = tile[0]*tile[1]
    group = per_call*128*(int(lib.eae_hip_coder_stream_stride_bytes(size, 10)) + 2*size + 2*size) + \
        int(lib.eae_hip_coder_workspace_bytes(per_call*128, size, 10))
    slack = 8 << 20
    assert 0 < peak <= group + slack, (peak, group)
    del symbols
    (blob_api, _) = container.encode_images(x, encoder, bw, mean, probabilities, -1, tile=tile, coding_tile=tile, tiles_per_call=per_call)
    assert blob_api == blob
    assert numpy.array_equal(container.decode_images(blob, decoder, tile=tile, tiles_per_call=per_call), rec)
    region = (7000, 3000, 512, 512)
    f = CountingFile(blob)
    out = container.decode_region(f, decoder, region, tile=tile)
    assert numpy.array_equal(out, rec[:, 7000:7512, 3000:3512])
    assert f.nbytes < len(blob)//20
