"""The latent-side helpers of csrc/hip/quantize.hip and csrc/hip/container.hip called directly through their device.py
wrappers: the generic quantiser (every C != 128), nonzero_flags, cast_int16, map_minmax, floor_histograms, dequantize_maps
and the stream pack / unpack kernels. Each is compared with a plain numpy restatement of the reference expression written
out here, at the values that decide something in the reference (a rounding tie, a histogram edge, the sign of a zero, the
1.5e-10 bound of its "quantization was omitted" assertion, NaN and inf) and at sizes that make the grid-stride loops run."""
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


GRID_CAP = 8192*256            # elements one launch of grid_for() covers without looping (csrc/hip/quantize.hip)
F32 = numpy.float32
FLT_MAX = numpy.finfo(F32).max
DENORMAL = numpy.float32(1e-45)


@pytest.fixture(scope='module')
def T():
    import torch
    return torch


@pytest.fixture(scope='module')
def dev():
    from autoencoder_based_image_compression_amd import device
    return device


def _cuda(T, a):
    return T.from_numpy(numpy.ascontiguousarray(a)).cuda()


# ---- quantize_maps, generic kernel -----------------------------------------------------------------------------------------

def _quantize_reference(y, bw, mean):
    """reconstructing_eae_kodak.py:178-192 + tools.py:927-929 + compression.py:142 in float32, with the three counters of
    include/eae_hip.h in the kernel's exact expressions."""
    centered = y - mean
    r = numpy.round(centered/bw)
    cq = bw*r
    rs = numpy.round(cq/bw)
    sym = rs.astype(numpy.int64).astype(numpy.int16)          # (int16_t)(int)rs: the low 16 bits
    checks = [int((~(numpy.abs(rs) < F32(32768.))).sum()),
              int((~(numpy.abs(cq.astype(numpy.float64) - centered.astype(numpy.float64)) < 1.5e-10)).sum()),
              int((~(sym.astype(F32)*bw == centered)).sum())]
    return centered, cq, sym, checks


def _latents(n, hw, c, seed):
    """Laplace latents plus, per map, the values where the quantiser decides something: half-way ties, deviations from a
    multiple of the bin width just below and just above 1.5e-10, exact multiples, and symbols past the int16 range."""
    rng = numpy.random.RandomState(seed)
    bw = rng.uniform(0.25, 2., size=c).astype(F32)
    bw[::3] = F32(2.**-20)                                   # small enough for deviations of ~1e-10 to be representable
    bw[1::3] = F32(0.5)
    mean = (rng.standard_normal(c)*0.1).astype(F32)
    mean[::3] = 0.
    y = (rng.laplace(size=(n, hw, c))*3.).astype(F32)*bw.reshape(1, 1, c)*F32(4.)
    j = rng.randint(-40, 41, size=(n, hw, c)).astype(F32)
    kind = rng.randint(0, 8, size=(n, hw, c))
    b = bw.reshape(1, 1, c)
    dev_ = numpy.array([1.4e-10, 1.6e-10, -1.4e-10, -1.6e-10, 1e-9, 0.], dtype=numpy.float64)
    pick = dev_[rng.randint(0, dev_.size, size=(n, hw, c))]
    y = numpy.where(kind == 0, (j + F32(0.5))*b + mean, y)                       # ties
    y = numpy.where(kind == 1, (j*b).astype(numpy.float64) + pick, y).astype(F32)   # near multiples (mean 0 on those maps)
    y = numpy.where(kind == 2, j*b + mean, y).astype(F32)
    y[0, 0, :] = F32(40000.)*bw                              # past int16: checks[0]
    y[-1, -1, :] = F32(-32770.)*bw
    return y.astype(F32), bw, mean


@pytest.mark.parametrize('c', [1, 3, 127, 129, 200])
def test_quantize_maps_generic(T, dev, c):
    (n, hw) = (2, (GRID_CAP + 4099)//(2*c) + 1) if c == 129 else (3, 257)
    (y, bw, mean) = _latents(n, hw, c, seed=c)
    res = dev.quantize_maps(_cuda(T, y), _cuda(T, bw), _cuda(T, mean), want_cq=True, want_shifted=True, want_symbols=True,
                            want_flags=True)
    (centered, cq, sym, checks) = _quantize_reference(y, bw, mean)
    assert numpy.array_equal(res['cq'].cpu().numpy(), cq)
    assert numpy.array_equal(res['shifted'].cpu().numpy(), cq + mean)
    assert numpy.array_equal(res['symbols'].cpu().numpy(), numpy.ascontiguousarray(sym.transpose(0, 2, 1)))
    assert res['checks'].cpu().tolist() == checks
    assert checks[0] == 2*c and checks[1] > 0 and checks[2] > 0
    # both sides of the 1.5e-10 bound are present on the maps of bin width 2^-20
    dist = numpy.abs(cq.astype(numpy.float64) - centered.astype(numpy.float64))[:, :, ::3]
    assert ((dist > 1.3e-10) & (dist < 1.5e-10)).any() and ((dist >= 1.5e-10) & (dist < 1.5e-9)).any()
    flags = (cq != 0).any(axis=1).astype(numpy.int32)
    assert numpy.array_equal(res['nonzero_flags'].cpu().numpy(), flags)
    # quantised input (the tools.py:372-375 path): cq passes as already quantised, and nothing is altered
    ok = dev.quantize_maps(_cuda(T, cq[:, 1:-1]), _cuda(T, bw), None, want_symbols=True)
    assert ok['checks'].cpu().tolist() == [0, 0, 0] == _quantize_reference(cq[:, 1:-1], bw, F32(0.))[3]


def test_quantize_maps_generic_dead_maps(T, dev):
    """nonzero_flags of the generic kernel: dead maps (all |x| < bw / 2), a map whose only non-zero symbol is the first or
    the last element of the image."""
    (n, hw, c) = (3, 200, 5)
    y = numpy.zeros((n, hw, c), dtype=F32)
    y[:, :, 1] = F32(0.4)
    y[0, 0, 2] = F32(1.)
    y[2, hw - 1, 3] = F32(-1.)
    y[1, :, 4] = F32(-0.)
    res = dev.quantize_maps(_cuda(T, y), _cuda(T, numpy.ones(c, dtype=F32)), None, want_flags=True)
    expected = numpy.zeros((n, c), dtype=numpy.int32)
    (expected[0, 2], expected[2, 3]) = (1, 1)
    assert numpy.array_equal(res['nonzero_flags'].cpu().numpy(), expected)
    assert res['checks'].cpu().tolist() == [0, n*hw, n*hw]    # 0.4 is neither quantised nor kept


# ---- cast_int16 --------------------------------------------------------------------------------------------------------------

def test_cast_int16(T, dev):
    """tls.cast_float_to_int16 (tools.py:126-133): int16(round_half_even(x)), AssertionError when some |round(x)| >= 32768
    (numpy.testing.assert_array_less: NaN and inf fail it too)."""
    rng = numpy.random.RandomState(2)
    ties = numpy.arange(-300, 300, dtype=F32) + F32(0.5)
    specials = numpy.array([32767.5, -32767.5, 32768., -32768., 32767., -32767., 32766.5, -32766.5, 0., -0., numpy.nan,
                            numpy.inf, -numpy.inf, 1e-45, -1e-45, 0.49999997, -0.49999997, 1e30], dtype=F32)
    x = numpy.concatenate([ties, specials, rng.uniform(-33000., 33000., size=GRID_CAP + 9000).astype(F32), specials])
    (out, range_error) = dev.cast_int16(_cuda(T, x))
    (out, range_error) = (out.cpu().numpy(), int(range_error.item()))
    rounded = numpy.round(x)
    with numpy.errstate(invalid='ignore'):
        inside = numpy.abs(rounded) < F32(32768.)
    assert range_error == int((~inside).sum()) > 0
    assert numpy.array_equal(out[inside], rounded[inside].astype(numpy.int16))
    assert numpy.array_equal(out[:ties.size], numpy.round(ties).astype(numpy.int16))
    assert (out[:ties.size] % 2 == 0).all()                   # every tie to the even neighbour
    with pytest.raises(AssertionError):
        numpy.testing.assert_array_less(numpy.absolute(rounded), 32768.)
    # within range: nothing counted, and the reference's assertion passes
    good = x[inside]
    (out, range_error) = dev.cast_int16(_cuda(T, good))
    assert int(range_error.item()) == 0 and numpy.array_equal(out.cpu().numpy(), numpy.round(good).astype(numpy.int16))
    numpy.testing.assert_array_less(numpy.absolute(numpy.round(good)), 32768.)
    for bad in (F32(32767.5), F32(-32767.5), F32(numpy.nan), F32(numpy.inf), F32(-numpy.inf)):
        (_, range_error) = dev.cast_int16(_cuda(T, numpy.array([1., bad, -2.], dtype=F32)))
        assert int(range_error.item()) == 1, bad


# ---- nonzero_flags -----------------------------------------------------------------------------------------------------------

def test_nonzero_flags(T, dev):
    """tls.count_nb_deads (tools.py:318-320): a map is dead when sum(|x|) == 0. +-0 everywhere else; the one non-zero value
    of a live map sits at its first or its last element; NaN makes sum(|x|) NaN, so such a map is not dead."""
    (n, hw, c) = (5, (GRID_CAP + 5000)//(5*50) + 1, 50)
    rng = numpy.random.RandomState(9)
    x = numpy.where(rng.rand(n, hw, c) < 0.5, F32(0.), F32(-0.)).astype(F32)
    x[0, 0, 1] = F32(3.)
    x[1, hw - 1, 2] = F32(-1e-45)
    x[2, 0, 3] = F32(numpy.nan)
    x[3, hw - 1, 4] = F32(numpy.inf)
    x[4, hw - 1, c - 1] = F32(1.)
    x[4, 0, 0] = F32(-2.)
    flags = dev.nonzero_flags(_cuda(T, x)).cpu().numpy()
    dead = numpy.sum(numpy.absolute(x), axis=1) == 0
    assert numpy.array_equal(flags, (~dead).astype(numpy.int32))
    assert flags.sum() == 6
    from autoencoder_based_image_compression_amd.kodak.tools import tools as tls
    assert numpy.array_equal(tls.count_nb_deads(x.reshape(n, hw, 1, c)), numpy.sum(dead, axis=1))


# ---- map_minmax ---------------------------------------------------------------------------------------------------------------

def _special_maps(y, rng):
    """Per map, one of the values where ordering through integer keys can go wrong, placed in the last rows (which only
    the grid-stride loop reaches)."""
    (rows, c) = y.shape
    for m in range(c):
        kind = (m + c) % 6
        if kind == 0:
            y[-1, m] = -numpy.inf
        elif kind == 1:
            y[-1, m] = numpy.inf
            y[-2, m] = -FLT_MAX
        elif kind == 2:
            y[:, m] = numpy.where(rng.rand(rows) < 0.5, F32(0.), F32(-0.))
        elif kind == 3:
            y[:, m] = rng.randint(-1000, 1000, size=rows).astype(F32)*DENORMAL
            y[-1, m] = F32(1001.)*DENORMAL
        elif kind == 4:
            y[-1, m] = FLT_MAX
            y[-3, m] = -FLT_MAX
        else:
            y[-1, m] = F32(1000.)
            y[-2, m] = F32(-1000.)
    return y


@pytest.mark.parametrize('c', [1, 3, 100, 128, 256])
def test_map_minmax(T, dev, c):
    per_block = 256//c
    rows = 1024*64*per_block + 3*per_block*64 + 17           # past the 1024-block cap: the grid-stride loop must run
    rng = numpy.random.RandomState(c)
    y = _special_maps(rng.standard_normal((rows, c)).astype(F32), rng)
    minmax = dev.map_minmax(_cuda(T, y)).cpu().numpy()
    assert numpy.array_equal(minmax[0], numpy.amin(y, axis=0))      # -0 == +0
    assert numpy.array_equal(minmax[1], numpy.amax(y, axis=0))


def test_map_minmax_nan(T, dev):
    """numpy.amin / amax of stats.py:103-104 return NaN for a map that holds a NaN, whatever its sign bit."""
    rng = numpy.random.RandomState(1)
    y = rng.standard_normal((70000, 6)).astype(F32)
    y[123, 1] = F32(numpy.nan)
    y[-1, 2] = -F32(numpy.nan)
    y[0, 3] = F32(numpy.nan)
    y[5, 3] = F32(numpy.inf)
    y[6, 4] = -F32(numpy.inf)
    y[69998, 4] = -F32(numpy.nan)
    minmax = dev.map_minmax(_cuda(T, y)).cpu().numpy()
    assert numpy.array_equal(minmax[0], numpy.amin(y, axis=0), equal_nan=True)
    assert numpy.array_equal(minmax[1], numpy.amax(y, axis=0), equal_nan=True)
    assert numpy.isnan(minmax[:, 1:5]).all() and not numpy.isnan(minmax[:, [0, 5]]).any()


# ---- floor_histograms ---------------------------------------------------------------------------------------------------------

def _floor_reference(y, radius):
    f = numpy.floor(y)
    with numpy.errstate(invalid='ignore'):
        inside = (f >= -radius) & (f <= radius)
    c = y.shape[1]
    hist = numpy.zeros((c, 2*radius + 1), dtype=numpy.int64)
    for m in range(c):
        hist[m] = numpy.bincount(f[inside[:, m], m].astype(numpy.int64) + radius, minlength=2*radius + 1)
    return hist, (~inside).sum(axis=0)


@pytest.mark.parametrize('radius', [0, 1, 5, 300])
def test_floor_histograms(T, dev, radius):
    rng = numpy.random.RandomState(radius + 1)
    c = 3
    rows = 200003
    y = (rng.standard_normal((rows, c))*(radius + 1.5)).astype(F32)
    r = F32(radius)
    specials = numpy.array([r, -r, r + F32(1.), -r - F32(1.), numpy.nextafter(r + F32(1.), F32(0.)), numpy.nextafter(-r, F32(-1e9)),
                            -0., 0., -1e-45, -1e-30, 1e-45, numpy.nan, numpy.inf, -numpy.inf, -FLT_MAX, FLT_MAX, -2.5, 2.5,
                            -0.5], dtype=F32)
    for m in range(c):
        y[-specials.size:, m] = numpy.roll(specials, m)
        y[:specials.size, m] = specials[::-1]
    (hist, overflow) = dev.floor_histograms(_cuda(T, y), radius)
    (hist_ref, overflow_ref) = _floor_reference(y, radius)
    assert numpy.array_equal(hist.cpu().numpy(), hist_ref)
    assert numpy.array_equal(overflow.cpu().numpy(), overflow_ref)
    assert (hist_ref.sum(axis=1) + overflow_ref == rows).all()


def test_unit_interval_counts(T, dev):
    """stats._unit_interval_counts against numpy.histogram(map, bins=arange(floor(min), ceil(max) + 1)) per map -- the
    histogram compute_probabilities_intervals(map, 1.) takes (stats.py:70-134), whose last interval is closed."""
    from autoencoder_based_image_compression_amd.kodak.lossless import stats
    rng = numpy.random.RandomState(8)
    (n, h, w, c) = (2, 40, 24, 10)
    y = (rng.standard_normal((n, h, w, c))*3.).astype(F32)
    y[1, 3, 4, 0] = F32(7.)                                   # maximum exactly an integer: the closed last bin
    y[0, 0, 0, 1] = F32(-6.)                                  # minimum exactly an integer
    y[..., 2] = F32(3.)                                       # constant integer map: no interval at all
    y[..., 3] = F32(-2.5)                                     # constant map between two integers
    y[..., 4] = numpy.round(y[..., 4])                        # integers only
    y[..., 5] = numpy.abs(y[..., 5]) + F32(1e-30)             # positive only
    y[..., 6] = -numpy.abs(y[..., 6]) - F32(1e-30)            # negative only, tiny magnitudes floor to -1
    y[0, 0, 0, 7] = F32(-0.)
    y[..., 8] = numpy.where(y[..., 8] > 0, F32(0.), F32(-0.))   # +-0 only
    y[-1, -1, -1, 9] = F32(12.)
    out = stats._unit_interval_counts(y)
    assert len(out) == c
    for m in range(c):
        data = y[..., m]
        (lo, hi) = (numpy.floor(numpy.amin(data)), numpy.ceil(numpy.amax(data)))
        expected = numpy.histogram(data, bins=numpy.arange(lo, hi + 1.))[0]
        assert (out[m][0], out[m][1]) == (int(lo), int(hi)), m
        assert numpy.array_equal(out[m][2], expected), m
        assert out[m][2].sum() == (data.size if hi > lo else 0)


# ---- dequantize_maps ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('hw', [1, 63, 64, 65, 1000])
def test_dequantize_maps(T, dev, hw):
    """The inverse of compression.py:142 and reconstructing_eae_kodak.py:192: cq = bw * float32(symbol), shifted = cq + mean,
    float32, from the planar int16 symbols, int16 extremes included."""
    rng = numpy.random.RandomState(hw)
    n = 3
    symbols = rng.randint(-32768, 32768, size=(n, 128, hw)).astype(numpy.int16)
    symbols[0, :, 0] = -32768
    symbols[-1, :, -1] = 32767
    symbols[1, ::2, :] = 0
    bw = rng.uniform(0.01, 3., size=128).astype(F32)
    bw[0] = F32(2.**-20)
    mean = (rng.standard_normal(128)*2.).astype(F32)
    out = dev.dequantize_maps(_cuda(T, symbols), _cuda(T, bw), _cuda(T, mean), want_cq=True, want_shifted=True)
    nhwc = symbols.transpose(0, 2, 1).astype(F32)
    cq = bw*nhwc
    assert numpy.array_equal(out['cq'].cpu().numpy(), cq)
    assert numpy.array_equal(out['shifted'].cpu().numpy(), cq + mean)
    no_mean = dev.dequantize_maps(_cuda(T, symbols), _cuda(T, bw), None, want_cq=False, want_shifted=True)
    assert no_mean['cq'] is None and numpy.array_equal(no_mean['shifted'].cpu().numpy(), cq)
    # the round trip with the quantiser: dequantised symbols quantise back to the same symbols
    q = dev.quantize_maps(out['cq'], _cuda(T, bw), None, want_symbols=True)
    assert numpy.array_equal(q['symbols'].cpu().numpy(), symbols)


# ---- coder_pack_streams / coder_unpack_streams ----------------------------------------------------------------------------------

def test_pack_unpack_streams(T, dev):
    """container.hip: map m's ceil(bits / 8) valid bytes of each stream (BAC at +0, bypass at +stride/2) to and from a
    payload at the offsets the caller chose; bit counts 0, 1, 7, 8, 9 and a full half-region."""
    (map_size, length) = (64, 10)
    counts = [0, 1, 7, 8, 9]
    probe = dev.CoderStreams(1, map_size, length, 'cuda')
    half = probe.stride//2
    full = 8*half
    pairs = [(a, b) for a in counts + [full] for b in counts + [full]]
    n_maps = len(pairs)
    streams = dev.CoderStreams(n_maps, map_size, length, 'cuda')
    rng = numpy.random.RandomState(6)
    raw = rng.randint(0, 256, size=(n_maps, streams.stride)).astype(numpy.uint8)
    streams.streams.copy_(_cuda(T, raw))
    bac = numpy.array([a for (a, _) in pairs], dtype=numpy.int32)
    bypass = numpy.array([b for (_, b) in pairs], dtype=numpy.int32)
    streams.bac_bits.copy_(_cuda(T, bac))
    streams.bypass_bits.copy_(_cuda(T, bypass))
    nbytes = numpy.stack([(bac + 7)//8, (bypass + 7)//8], axis=1).astype(numpy.int64)
    # bypass piece first, a gap of 3 bytes between pieces: the kernel must follow the offsets, not assume an order
    offsets = numpy.zeros((n_maps, 2), dtype=numpy.int64)
    at = 0
    for m in range(n_maps):
        offsets[m, 1] = at
        at += nbytes[m, 1] + 3
        offsets[m, 0] = at
        at += nbytes[m, 0] + 3
    payload = dev.coder_pack_streams(streams, _cuda(T, offsets), at).cpu().numpy()
    expected = numpy.zeros(at, dtype=numpy.uint8)
    for m in range(n_maps):
        expected[offsets[m, 0]:offsets[m, 0] + nbytes[m, 0]] = raw[m, :nbytes[m, 0]]
        expected[offsets[m, 1]:offsets[m, 1] + nbytes[m, 1]] = raw[m, half:half + nbytes[m, 1]]
    assert numpy.array_equal(payload, expected)
    back = dev.coder_unpack_streams(_cuda(T, payload), _cuda(T, offsets), _cuda(T, bac), _cuda(T, bypass), map_size, length)
    got = back.streams.cpu().numpy()
    for m in range(n_maps):
        assert numpy.array_equal(got[m, :nbytes[m, 0]], raw[m, :nbytes[m, 0]]), m
        assert numpy.array_equal(got[m, half:half + nbytes[m, 1]], raw[m, half:half + nbytes[m, 1]]), m
    assert numpy.array_equal(back.bac_bits.cpu().numpy(), bac) and numpy.array_equal(back.bypass_bits.cpu().numpy(), bypass)
    assert numpy.array_equal(dev.coder_pack_streams(back, _cuda(T, offsets), at).cpu().numpy(), expected)


# ---- symbol_histograms (one map per block, no stride) and the host hand-off kernels ----------------------------------------------

@pytest.mark.parametrize('radius', [0, 40, 9000])
def test_symbol_histograms_unstrided(T, dev, radius):
    """eae_hip_symbol_histograms (the entry point without first_map / map_step): hist[m][s + radius] per map, the rest in
    overflow[m]; 9000 takes the global-atomics form (more bins than the LDS holds)."""
    from autoencoder_based_image_compression_amd import _native
    rng = numpy.random.RandomState(radius)
    (n_maps, map_size) = (37, 3001)
    symbols = numpy.round(rng.laplace(size=(n_maps, map_size))*(radius + 2)).clip(-32768, 32767).astype(numpy.int16)
    symbols[0, 0] = -32768
    symbols[-1, -1] = 32767
    symbols[1, :] = radius
    symbols[2, :] = -radius - 1
    s = _cuda(T, symbols)
    hist = T.zeros((n_maps, 2*radius + 1), dtype=T.int32, device='cuda')
    overflow = T.zeros(n_maps, dtype=T.int32, device='cuda')
    assert _native.hip().eae_hip_symbol_histograms(dev._p(s), dev._p(hist), radius, dev._p(overflow), n_maps, map_size, dev._stream(s)) == 0
    flat = symbols.astype(numpy.int64)
    inside = numpy.abs(flat) <= radius
    expected = numpy.stack([numpy.bincount(flat[m][inside[m]] + radius, minlength=2*radius + 1) for m in range(n_maps)])
    assert numpy.array_equal(hist.cpu().numpy(), expected)
    assert numpy.array_equal(overflow.cpu().numpy(), (~inside).sum(axis=1))
    (hist2, overflow2) = dev.symbol_histograms(s, radius)
    assert numpy.array_equal(hist2.cpu().numpy(), expected) and numpy.array_equal(overflow2.cpu().numpy(), (~inside).sum(axis=1))


def test_publish_to_host_and_sequence(T, dev):
    """eae_hip_publish_to_host copies device bytes into pinned host memory in stream order; eae_hip_publish_sequence bumps a
    device counter and leaves each new value in a pinned word."""
    src = T.arange(1001, dtype=T.int32, device='cuda')*7 - 3
    dst = T.zeros(1001, dtype=T.int32).pin_memory()
    dev.publish_to_host(src, dst)
    T.cuda.synchronize()
    assert numpy.array_equal(dst.numpy(), numpy.arange(1001, dtype=numpy.int32)*7 - 3)
    counter = T.zeros(1, dtype=T.int32, device='cuda')
    word = T.zeros(1, dtype=T.int32).pin_memory()
    for i in (1, 2, 3):
        dev.publish_sequence(counter, word)
        T.cuda.synchronize()
        assert int(word[0]) == i
    assert int(counter.item()) == 3
