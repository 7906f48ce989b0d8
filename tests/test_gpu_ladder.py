"""eae_hip_ladder_histograms (csrc/hip/ladder.hip) through device.ladder_histograms, on poisoned buffers between guard bands under
both poisons (tests/guarded.py): the clipped histograms of |symbol|, the bypass bit counts and the range errors of K rate points from
one pass, against (a) a float32 numpy restatement of the quantiser's symbol, rint(bw * rint((y - m) / bw) / bw), and (b) the two-pass
route the statistics take today, quantize_maps -> symbol_histograms, folded here. Shapes: one pixel, fewer pixels than a block, a
ragged block edge over several images, several blocks per image."""
import functools

import numpy
import pytest

pytestmark = pytest.mark.gpu

F32 = numpy.float32
SHAPES = [(1, 1), (1, 24), (3, 65), (2, 1536)]
LENGTHS = [1, 4, 10]


@pytest.fixture(autouse=True, params=[0xFF, 0x7F], ids=['poison_ff', 'poison_7f'])
def guard(request):
    """Every test runs twice, on buffers poisoned with 0xFF and with 0x7F bytes, inputs included: an element the kernel does not
    write, a write outside a tensor or a read outside an input that reaches an output fails the exact comparisons below."""
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


@pytest.fixture(scope='module')
def dev():
    from autoencoder_based_image_compression_amd import device
    return device


@functools.lru_cache(maxsize=None)
def inputs(n, hw, k_points, length, with_mean, seed=0):
    """(y [n, hw, 128], bin widths [K, 128], mean or None). Point 0 is the finest; point k is 1 + k / 2 times as wide. Every element
    is built from a target symbol j at point 0 that sweeps 0 .. L + 2 with both signs, so that every bin is hit; a quarter are exact
    half-way cases (j + 0.5) * bw, some are large (up to 32767), and three per image sit at or beyond 32768 at point 0 only."""
    rng = numpy.random.RandomState(seed + 1000*n + hw + 7*k_points + length)
    bw0 = rng.uniform(0.25, 2., size=128).astype(F32)
    bw0[::5] = F32(0.5)
    bw = (bw0[None, :]*(1. + 0.5*numpy.arange(k_points, dtype=numpy.float64))[:, None]).astype(F32)
    mean = (rng.standard_normal(128)*0.2).astype(F32) if with_mean else None
    m = mean if with_mean else F32(0.)
    j = rng.randint(-(length + 2), length + 3, size=(n, hw, 128)).astype(F32)
    kind = rng.randint(0, 8, size=(n, hw, 128))
    y = (rng.laplace(size=(n, hw, 128))*3.).astype(F32)*bw0
    y = numpy.where(kind <= 1, (j + F32(0.5))*bw0 + m, y)                    # ties: round half to even decides
    y = numpy.where(kind == 2, j*bw0 + m, y)
    factor = rng.randint(1, 24000//(length + 2), size=j.shape)                # |j| * factor stays inside int16
    y = numpy.where(kind == 3, (j*factor).astype(F32)*bw0 + m, y)           # suffixes of every length
    y = y.astype(F32)
    flat = y.reshape(n, -1)
    for i in range(n):
        spots = rng.choice(flat.shape[1], size=min(6, flat.shape[1]), replace=False)
        values = [32767., -32767., 16384., 32768., -40000., 32768.5]        # the last three: range errors at point 0 only
        for (s, v) in zip(spots, values):
            c = s % 128
            flat[i, s] = F32(v)*bw0[c] + (mean[c] if with_mean else F32(0.))
    return y, bw, mean


def suffix_bits(magnitudes, length):
    """(s != 0) + (|s| >= L ? 2 * floor(log2(|s| - L + 1)) + 1 : 0), the floor counted by comparisons."""
    v = numpy.maximum(magnitudes - length + 1, 1)
    log2 = sum((v >= (1 << e)).astype(numpy.int64) for e in range(1, 17))
    return (magnitudes != 0).astype(numpy.int64) + numpy.where(magnitudes >= length, 2*log2 + 1, 0)


@functools.lru_cache(maxsize=None)
def reference(n, hw, k_points, length, with_mean):
    (y, bw, mean) = inputs(n, hw, k_points, length, with_mean)
    centered = y - mean if with_mean else y - F32(0.)
    hist = numpy.zeros((n, k_points, 128, length + 1), dtype=numpy.int64)
    bits = numpy.zeros((n, k_points, 128), dtype=numpy.int64)
    errors = numpy.zeros(k_points, dtype=numpy.int64)
    for k in range(k_points):
        rs = numpy.rint(bw[k]*numpy.rint(centered/bw[k])/bw[k])
        assert rs.dtype == F32
        good = numpy.abs(rs) < F32(32768.)
        magnitudes = numpy.where(good, numpy.abs(rs), 0).astype(numpy.int64)
        clipped = numpy.minimum(magnitudes, length)
        for b in range(length + 1):
            hist[:, k, :, b] = (good & (clipped == b)).sum(axis=1)
        bits[:, k] = (suffix_bits(magnitudes, length)*good).sum(axis=1)
        errors[k] = (~good).sum()
    return hist, bits, errors


def points_for(dev, kind, length):
    return {'one': 1, 'three': 3, 'most': dev.ladder_max_points(length)}[kind]


def run(dev, guard, n, hw, k_points, length, with_mean, **kwargs):
    (y, bw, mean) = inputs(n, hw, k_points, length, with_mean)
    out = dev.ladder_histograms(guard.upload(y), guard.upload(bw), guard.upload(mean) if with_mean else None, length, **kwargs)
    return tuple(t.cpu().numpy() for t in out)


def test_max_points_is_what_the_lds_holds(dev):
    assert [dev.ladder_max_points(length) for length in (1, 4, 10, 125, 126, 255)] == [32, 18, 9, 1, 0, 0]
    assert [dev.ladder_max_points(length) for length in (0, -1, 256)] == [0, 0, 0]


@pytest.mark.parametrize('with_mean', [False, True], ids=['no_mean', 'mean'])
@pytest.mark.parametrize('kind', ['one', 'three', 'most'])
@pytest.mark.parametrize('length', LENGTHS)
@pytest.mark.parametrize('n, hw', SHAPES)
def test_against_the_numpy_symbols(dev, guard, n, hw, kind, length, with_mean):
    k_points = points_for(dev, kind, length)
    (hist, bits, errors) = run(dev, guard, n, hw, k_points, length, with_mean)
    (hist_ref, bits_ref, errors_ref) = reference(n, hw, k_points, length, with_mean)
    assert errors_ref[0] == 3*n and not errors_ref[1:].any()
    if hw >= 24:
        assert (hist_ref[:, 0].sum(axis=(0, 1)) > 0).all()          # every bin is hit at the finest point
    assert hist.shape == hist_ref.shape and bits.shape == bits_ref.shape
    assert numpy.array_equal(errors, errors_ref)
    assert numpy.array_equal(hist, hist_ref)
    assert numpy.array_equal(bits, bits_ref)


@pytest.mark.parametrize('length', LENGTHS)
@pytest.mark.parametrize('n, hw', SHAPES)
def test_against_the_two_pass_route(dev, guard, n, hw, length):
    """hist[:, k] is the fold of symbol_histograms(quantize_maps(...)['symbols']) for every point without a range error."""
    import torch
    k_points = 3
    (y, bw, mean) = inputs(n, hw, k_points, length, True)
    (hist, _, errors) = run(dev, guard, n, hw, k_points, length, True)
    y_device = torch.from_numpy(y).cuda()
    folded = 0
    for k in range(k_points):
        if errors[k]:
            continue
        q = dev.quantize_maps(y_device, torch.from_numpy(bw[k]).cuda(), torch.from_numpy(mean).cuda(), want_symbols=True)
        assert int(q['checks'][0].item()) == 0
        (full, overflow) = dev.symbol_histograms(q['symbols'], length)         # bins -L .. L, everything beyond in `overflow`
        full = full.cpu().numpy().astype(numpy.int64).reshape(n, 128, 2*length + 1)
        fold = full[:, :, length:].copy()
        fold[:, :, 1:] += full[:, :, :length][:, :, ::-1]
        fold[:, :, length] += overflow.cpu().numpy().astype(numpy.int64).reshape(n, 128)
        assert numpy.array_equal(hist[:, k], fold)
        folded += 1
    assert folded == 2


def test_outputs_accumulate_over_two_calls(dev, guard):
    import torch
    (n, hw, k_points, length) = (3, 65, 3, 4)
    out = (torch.zeros((n, k_points, 128, length + 1), dtype=torch.int32, device='cuda'),
           torch.zeros((n, k_points, 128), dtype=torch.int64, device='cuda'), torch.zeros(k_points, dtype=torch.int32, device='cuda'))
    run(dev, guard, n, hw, k_points, length, True, out=out)
    (hist, bits, errors) = run(dev, guard, n, hw, k_points, length, True, out=out)
    (hist_ref, bits_ref, errors_ref) = reference(n, hw, k_points, length, True)
    assert numpy.array_equal(hist, 2*hist_ref) and numpy.array_equal(bits, 2*bits_ref) and numpy.array_equal(errors, 2*errors_ref)


def test_bypass_bits_and_range_errors_are_optional(dev, guard):
    import torch
    from autoencoder_based_image_compression_amd import _native
    (n, hw, k_points, length) = (1, 24, 3, 4)
    (y, bw, mean) = inputs(n, hw, k_points, length, False)
    hist = torch.zeros((n, k_points, 128, length + 1), dtype=torch.int32, device='cuda')
    (y_d, bw_d) = (guard.upload(y), guard.upload(bw))
    assert _native.hip().eae_hip_ladder_histograms(y_d.data_ptr(), None, bw_d.data_ptr(), k_points, length, hist.data_ptr(), None, None, n, hw,
                                                   None) == 0
    torch.cuda.synchronize()
    assert numpy.array_equal(hist.cpu().numpy(), reference(n, hw, k_points, length, False)[0])


def test_bad_arguments_are_refused(dev, guard):
    import torch
    from autoencoder_based_image_compression_amd import _native
    lib = _native.hip()
    (n, hw, length) = (1, 24, 10)
    most = dev.ladder_max_points(length)
    (y, bw, _) = inputs(n, hw, most, length, False)
    (y_d, bw_d) = (guard.upload(y), guard.upload(bw))
    hist = torch.zeros((n, most, 128, length + 1), dtype=torch.int32, device='cuda')
    (yp, bp, hp) = (y_d.data_ptr(), bw_d.data_ptr(), hist.data_ptr())
    call = lib.eae_hip_ladder_histograms
    assert call(None, None, bp, 1, length, hp, None, None, n, hw, None) == -1
    assert call(yp, None, None, 1, length, hp, None, None, n, hw, None) == -1
    assert call(yp, None, bp, 1, length, None, None, None, n, hw, None) == -1
    for k_points in (0, -1, most + 1):
        assert call(yp, None, bp, k_points, length, hp, None, None, n, hw, None) == -1
    for bad_length in (0, -3, 256):
        assert call(yp, None, bp, 1, bad_length, hp, None, None, n, hw, None) == -1
    assert call(yp, None, bp, 1, 255, hp, None, None, n, hw, None) == -1          # no point fits at L = 255
    assert call(yp, None, bp, 1, length, hp, None, None, 0, hw, None) == -1
    assert call(yp, None, bp, 1, length, hp, None, None, n, 0, None) == -1
    torch.cuda.synchronize()
    assert not hist.any().item()                                                   # nothing was launched
    with pytest.raises(ValueError):
        dev.ladder_histograms(y_d, bw_d, None, 0)
    with pytest.raises(dev.HipError):
        dev.ladder_histograms(y_d, bw_d[:, :64].contiguous(), None, length)
    with pytest.raises(dev.HipError):
        dev.ladder_histograms(y_d.double(), bw_d, None, length)


def test_a_ladder_longer_than_a_launch_is_split(dev, guard):
    (n, hw, length) = (3, 65, 10)
    k_points = dev.ladder_max_points(length) + 1
    (hist, bits, errors) = run(dev, guard, n, hw, k_points, length, True)
    (hist_ref, bits_ref, errors_ref) = reference(n, hw, k_points, length, True)
    assert numpy.array_equal(hist, hist_ref) and numpy.array_equal(bits, bits_ref) and numpy.array_equal(errors, errors_ref)


def test_a_length_no_launch_takes_goes_the_two_pass_route(dev, guard):
    """L = 255: eae_hip_ladder_max_points is 0 and every point is quantised and counted by the existing kernels; the same arrays come
    back -- at the finest point, whose symbols leave int16, and at the next, whose symbols reach beyond the first histogram radius."""
    (n, hw, k_points, length) = (3, 65, 2, 255)
    assert dev.ladder_max_points(length) == 0
    (hist, bits, errors) = run(dev, guard, n, hw, k_points, length, True)
    (hist_ref, bits_ref, errors_ref) = reference(n, hw, k_points, length, True)
    assert errors_ref[0] and not errors_ref[1]
    assert numpy.array_equal(hist, hist_ref) and numpy.array_equal(bits, bits_ref) and numpy.array_equal(errors, errors_ref)
