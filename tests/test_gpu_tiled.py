"""Tiled encode / decode (pipeline.tile_plan, csrc/hip/tile.hip): bit-identical to the oracle and to the
untiled path, sensitive to a halo one latent short, and past the untiled path's 67-megapixel limit with memory bounded by one group
of windows."""
import numpy
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _guarded_buffers():
    """Every test of this module runs on poisoned buffers between guard bands: what device.py / pipeline.py allocate holds 0xFF bytes
    (NaN, -1) until a kernel writes it, and a byte written outside a tensor fails the test (tests/guarded.py)."""
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), 0xFF):
        yield


def _image(seed, n, h, w):
    rng = numpy.random.RandomState(seed)
    x = rng.randint(16, 236, size=(n, h, w)).astype(numpy.float32)
    for _ in range(3):
        x = (x + numpy.roll(x, 1, 1) + numpy.roll(x, -1, 1) + numpy.roll(x, 1, 2) + numpy.roll(x, -1, 2))/numpy.float32(5.)
    return numpy.round(x).astype(numpy.uint8)


def _model(learned=False):
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    v = var.random_variables(1., learned, seed=0, bias_std=0.01)
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    return v


def _host_sse(a, b):
    """Per-image squared error of two uint8 stacks, in row blocks (int64 sums)."""
    out = numpy.zeros(a.shape[0], dtype=numpy.int64)
    for i in range(a.shape[0]):
        for r in range(0, a.shape[1], 1024):
            d = a[i, r:r + 1024].astype(numpy.int32) - b[i, r:r + 1024].astype(numpy.int32)
            out[i] += int((d*d).sum(dtype=numpy.int64))
    return out


@pytest.mark.parametrize('learned', [False, True])
def test_tiled_path_equals_the_oracle(learned):
    """3 images of 272 x 400 (17 x 25 latents, not multiples of the tile) with tile = (4, 6): latents, uint8 reconstruction and
    per-image squared error equal the CPU oracle's."""
    import torch
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd import pipeline
    from oracle import transforms as T
    v = _model(learned)
    x = _image(31, 3, 272, 400)
    xd = torch.from_numpy(x).cuda()
    encoder = pipeline.DeviceEncoder(v, learned)
    decoder = pipeline.DeviceDecoder(v, learned)
    bw = numpy.full(128, 0.5, dtype=numpy.float32)
    y = encoder(xd, tile=(4, 6))
    y_ref = T.encoder(x.astype(numpy.float32)[..., None], v, learned)
    assert numpy.array_equal(y.cpu().numpy(), y_ref)
    shifted = dev.quantize_maps(y, torch.from_numpy(bw).cuda(), None, want_shifted=True)['shifted']
    (rec_f32, rec_u8, sse) = decoder(shifted, reference_uint8=xd, tile=(4, 6))
    assert rec_f32 is None
    q_ref = bw*numpy.round(y_ref/bw)
    rec_ref = numpy.round(T.decoder(q_ref, v, learned)[..., 0].clip(min=16., max=235.)).astype(numpy.uint8)
    assert numpy.array_equal(rec_u8.cpu().numpy(), rec_ref)
    assert numpy.array_equal(sse.cpu().numpy(), _host_sse(x, rec_ref))
    # the squared error alone (no uint8 output), into a caller's accumulator
    acc = torch.full((3,), 5, dtype=torch.int64, device='cuda')
    (none_f32, none_u8, sse_only) = decoder(shifted, want_uint8=False, reference_uint8=xd, sse=acc, tile=(4, 6), tiles_per_launch=5)
    assert none_f32 is None and none_u8 is None and sse_only is acc
    assert numpy.array_equal(acc.cpu().numpy(), _host_sse(x, rec_ref) + 5)
    encoder.check()
    decoder.check()
    for bad in ((0, 4), (4,), 4, (4, 2.5)):
        with pytest.raises(ValueError):
            encoder(xd, tile=bad)
        with pytest.raises(ValueError):
            decoder(shifted, tile=bad)
    with pytest.raises(ValueError):
        encoder(xd, tile=(4, 4), tiles_per_launch=0)


@pytest.fixture(scope='module')
def square():
    """One 2048 x 2048 image through the untiled path: latents, symbols, float and uint8 reconstructions, squared error."""
    import torch
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd import pipeline
    v = _model()
    x = _image(41, 1, 2048, 2048)
    xd = torch.from_numpy(x).cuda()
    rng = numpy.random.RandomState(42)
    bw = torch.ones(128, dtype=torch.float32, device='cuda')
    mean = torch.from_numpy((rng.standard_normal(128)*0.05).astype(numpy.float32)).cuda()
    encoder = pipeline.DeviceEncoder(v, False)
    decoder = pipeline.DeviceDecoder(v, False)
    y = encoder(xd)
    q = dev.quantize_maps(y, bw, mean, want_shifted=True, want_symbols=True)
    (rec_f32, rec_u8, sse) = decoder(q['shifted'], want_float=True, reference_uint8=xd)
    return {'x': x, 'xd': xd, 'bw': bw, 'mean': mean, 'encoder': encoder, 'decoder': decoder, 'y': y, 'q': q, 'rec_f32': rec_f32,
            'rec_u8': rec_u8, 'sse': sse, 'probabilities': numpy.clip(rng.rand(128, 10), 0.05, 0.95)}


def test_tiled_path_equals_the_untiled_path(square):
    """2048 x 2048 with tile = (32, 32) and 3 windows per launch (16 windows: a partial last group): latents, symbols, float and
    uint8 reconstructions and squared error are those of tile=None, bit for bit."""
    import torch
    from autoencoder_based_image_compression_amd import device as dev
    s = square
    y = s['encoder'](s['xd'], tile=(32, 32), tiles_per_launch=3)
    assert torch.equal(y, s['y'])
    q = dev.quantize_maps(y, s['bw'], s['mean'], want_shifted=True, want_symbols=True)
    assert torch.equal(q['symbols'], s['q']['symbols'])
    (rec_f32, rec_u8, sse) = s['decoder'](s['q']['shifted'], want_float=True, reference_uint8=s['xd'], tile=(32, 32), tiles_per_launch=3)
    assert torch.equal(rec_f32, s['rec_f32']) and torch.equal(rec_u8, s['rec_u8']) and torch.equal(sse, s['sse'])
    # into a caller's output tensor
    out = torch.empty_like(s['rec_u8'])
    (_, rec_into, _) = s['decoder'](s['q']['shifted'], out_uint8=out, tile=(61, 7))
    assert rec_into is out and torch.equal(out, s['rec_u8'])
    s['encoder'].check()
    s['decoder'].check()


def test_the_container_writes_the_same_bytes_tiled(square):
    from autoencoder_based_image_compression_amd import container
    s = square
    (bw, mean) = (s['bw'].cpu().numpy(), s['mean'].cpu().numpy())
    (blob, _) = container.encode_images(s['x'], s['encoder'], bw, mean, s['probabilities'], 5)
    (blob_tiled, _) = container.encode_images(s['x'], s['encoder'], bw, mean, s['probabilities'], 5, tile=(32, 32))
    assert blob_tiled == blob
    rec = container.decode_images(blob, s['decoder'])
    assert numpy.array_equal(container.decode_images(blob, s['decoder'], tile=(32, 32)), rec)


@pytest.mark.parametrize('side, halo', [('encoder', (0, 2)), ('encoder', (1, 1)), ('decoder', (1, 1)), ('decoder', (2, 0))])
def test_a_halo_one_latent_short_changes_the_result(square, side, halo):
    """The comparison above can see a wrong halo: with one latent less before or after the tiles, the results differ."""
    import torch
    from autoencoder_based_image_compression_amd import pipeline
    s = square
    obj = s[side]
    assert obj.tile_halo == (pipeline.ENCODER_HALO if side == 'encoder' else pipeline.DECODER_HALO)
    obj.tile_halo = halo
    try:
        if side == 'encoder':
            assert not torch.equal(obj(s['xd'], tile=(32, 32), tiles_per_launch=3), s['y'])
        else:
            (_, rec_u8, _) = obj(s['q']['shifted'], tile=(32, 32), tiles_per_launch=3)
            assert not torch.equal(rec_u8, s['rec_u8'])
    finally:
        obj.tile_halo = pipeline.ENCODER_HALO if side == 'encoder' else pipeline.DECODER_HALO


def test_an_image_past_the_untiled_limit():
    """One 16384 x 8192 image (134 Mpx, twice what the untiled path accepts): tiled encode -> container -> tiled decode. The squared
    error the stitch kernel reports is that of the returned image; the blob round trip equals the in-memory path; untiled crops
    equal the tiled latents inside their exact zones; memory beyond the full planes stays within one group of windows."""
    import torch
    from autoencoder_based_image_compression_amd import _native
    from autoencoder_based_image_compression_amd import container
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd import pipeline
    (H, W, C, tile, per_launch) = (16384, 8192, 1024, (64, 64), 16)
    v = _model()
    x = _image(51, 1, H, W)
    xd = torch.from_numpy(x).cuda()
    encoder = pipeline.DeviceEncoder(v, False)
    decoder = pipeline.DeviceDecoder(v, False)
    with pytest.raises(dev.HipError):
        encoder(xd)                                     # the untiled path refuses it
    (_, (wh, ww)) = pipeline.tile_plan(1, H//16, W//16, tile, *pipeline.ENCODER_HALO)
    lib = _native.hip()
    # encode: peak allocation beyond the input and the latent plane
    y = torch.empty((1, H//16, W//16, 128), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    encoder(xd, out=y, tile=tile, tiles_per_launch=per_launch)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    group = per_launch*(256*wh*ww + 512*wh*ww) + int(lib.eae_hip_encode_scratch_bytes(per_launch, 16*wh, 16*ww))
    slack = 8 << 20                                     # the plan, status words, the allocator's rounding
    assert 0 < peak <= group + slack, (peak, group)
    encoder.check()
    # untiled crops against the tiled latents, inside the crops' exact zones
    (before, after) = pipeline.ENCODER_HALO
    for (r0, c0) in ((0, 0), (H - C, W - C), (H - C, 0), (0, W - C), (7168, 3072)):
        y_crop = encoder(xd[:, r0:r0 + C, c0:c0 + C].contiguous())
        (lo_r, hi_r) = (0 if r0 == 0 else before, C//16 - (0 if r0 + C == H else after))
        (lo_c, hi_c) = (0 if c0 == 0 else before, C//16 - (0 if c0 + C == W else after))
        assert torch.equal(y[:, r0//16 + lo_r:r0//16 + hi_r, c0//16 + lo_c:c0//16 + hi_c], y_crop[:, lo_r:hi_r, lo_c:hi_c]), (r0, c0)
    # in memory: quantise, tiled decode with the squared error
    rng = numpy.random.RandomState(52)
    bw = numpy.ones(128, dtype=numpy.float32)
    mean = (rng.standard_normal(128)*0.05).astype(numpy.float32)
    probabilities = numpy.clip(rng.rand(128, 10), 0.05, 0.95)
    shifted = dev.quantize_maps(y, torch.from_numpy(bw).cuda(), torch.from_numpy(mean).cuda(), want_shifted=True)['shifted']
    (dh, dw) = pipeline.tile_plan(1, H//16, W//16, tile, *pipeline.DECODER_HALO)[1]
    rec = torch.empty_like(xd)
    sse = torch.zeros(1, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    decoder(shifted, reference_uint8=xd, sse=sse, out_uint8=rec, tile=tile, tiles_per_launch=per_launch)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    group = per_launch*(512*dh*dw + 256*dh*dw) + int(lib.eae_hip_decode_scratch_bytes(per_launch, dh, dw))
    assert 0 < peak <= group + slack, (peak, group)
    decoder.check()
    rec_host = rec.cpu().numpy()
    assert int(sse[0]) == int(_host_sse(x, rec_host)[0])
    # through the container, both ways tiled
    (blob, _) = container.encode_images(x, encoder, bw, mean, probabilities, -1, tile=tile)
    assert numpy.array_equal(container.decode_images(blob, decoder, tile=tile), rec_host)


@pytest.mark.parametrize('kind', ['u8_pixels', 'latents', 'f32_pixels', 'int16_x8'])
def test_the_copy_kernel_equals_torch_slicing(kind):
    """eae_hip_tile_copy in both directions against torch slicing, for every element size the path uses (and one more), and
    eae_hip_tile_stitch_u8 against torch for the uint8 reconstruction (interiors and squared error)."""
    import torch
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd import pipeline
    (n, h, w) = (2, 17, 25)
    (unit, make) = {'u8_pixels': (16, lambda *s: torch.randint(0, 256, s, dtype=torch.uint8)),
                    'latents': (1, lambda *s: torch.randn(*s, 128)),
                    'f32_pixels': (16, lambda *s: torch.randn(*s)),
                    'int16_x8': (1, lambda *s: torch.randint(-9999, 9999, s + (8,), dtype=torch.int16))}[kind]
    plane = make(n, unit*h, unit*w).cuda()
    (plan, (wh, ww)) = pipeline.tile_plan(n, h, w, (4, 6), 2, 1)
    plan_d = torch.from_numpy(plan).cuda()
    windows = make(len(plan), unit*wh, unit*ww).cuda()
    dev.tile_copy(plane, windows, plan_d, plan, unit, True)
    for (g, (img, wr, wc, ir, ic, orow, ocol, er, ec)) in enumerate(plan.tolist()):
        assert torch.equal(windows[g], plane[img, unit*wr:unit*(wr + wh), unit*wc:unit*(wc + ww)]), g
    # stitch fresh windows into a copy of the plane: the interiors come from the windows, every element is written
    windows = make(len(plan), unit*wh, unit*ww).cuda()
    stitched = torch.zeros_like(plane)
    expected = torch.zeros_like(plane)
    for (g, (img, wr, wc, ir, ic, orow, ocol, er, ec)) in enumerate(plan.tolist()):
        expected[img, unit*orow:unit*(orow + er), unit*ocol:unit*(ocol + ec)] = windows[g, unit*ir:unit*(ir + er), unit*ic:unit*(ic + ec)]
    dev.tile_copy(stitched, windows, plan_d, plan, unit, False)
    assert torch.equal(stitched, expected)
    if kind == 'u8_pixels':
        image = torch.zeros_like(plane)
        sse = dev.tile_stitch_u8(windows, plan_d, plan, image=image, ref_u8=plane)
        assert torch.equal(image, expected)
        d = expected.to(torch.int64) - plane.to(torch.int64)
        assert torch.equal(sse, (d*d).sum(dim=(1, 2)))
        assert torch.equal(dev.tile_stitch_u8(windows, plan_d, plan, ref_u8=plane), sse)


def test_the_copy_kernel_reaches_past_2_gb():
    """A latent plane of 2.16 GB (1 x 2056 x 2048 x 128 float32): windows at its far end are read and written through the 64-bit
    plane offsets."""
    import torch
    from autoencoder_based_image_compression_amd import device as dev
    (h, w, k) = (2056, 2048, 35)
    plane = torch.zeros((1, h, w, 128), dtype=torch.float32, device='cuda')
    assert plane.numel()*4 > 2**31
    far = torch.randn((k, k, 128), device='cuda')
    plane[0, h - k:, w - k:] = far
    plan = numpy.array([[0, h - k, w - k, 0, 0, h - k, w - k, k, k], [0, h - k, 0, 0, 0, h - k, 0, k, k]], dtype=numpy.int32)
    plan_d = torch.from_numpy(plan).cuda()
    windows = torch.empty((2, k, k, 128), dtype=torch.float32, device='cuda')
    dev.tile_copy(plane, windows, plan_d, plan, 1, True)
    assert torch.equal(windows[0], far) and torch.equal(windows[1], plane[0, h - k:, :k])
    # and back, 3 x 3 interiors into the last rows
    windows.fill_(7.)
    small = numpy.array([[0, h - k, w - k, k - 3, k - 3, h - 3, w - 3, 3, 3]], dtype=numpy.int32)
    dev.tile_copy(plane, windows[:1], torch.from_numpy(small).cuda(), small, 1, False)
    torch.cuda.synchronize()
    assert bool((plane[0, h - 3:, w - 3:] == 7.).all())
    assert torch.equal(plane[0, h - k:h - 3, w - k:], far[:k - 3])
