"""eae_hip_latent_quantize_rdo (csrc/hip/latent_rows.hip, device.latent_quantize_rdo) on poisoned buffers between guard bands under both
poisons (tests/guarded.py). Every comparison is exact:

* the choice of every symbol against ratecontrol.rdo_quantize_numpy, element for element;
* everything behind the choice -- symbols, shifted, t, dead-map flags -- against device.latent_quantize_rows fed with the latents
  that round to the chosen symbols, y2 = bw r + mean (the test asserts that they do), and the three checks against their statements
  written out in numpy;
* thresholds of zeros (lambda = 0) against device.latent_quantize_rows on the same latents, bit for bit, the checks included;
* every optional output absent in turn; the refusals.

Shapes (n, hw): (1, 1), (3, 33) and (2, 143): in the last two a tile of 32 positions straddles images and the last tile is ragged.
K = 1, and K = 3 with points that are mixed, beyond K and negative. L = 1, 3, 10, 40. Maps 3, 35, 67 and 99 (one per wavefront) have a
power-of-two bin width and a zero mean, so that x = y / bw is exact, and thresholds set by hand: they carry, for every magnitude 1 .. 17
and both signs, a latent whose 2 u + 1 is exactly the threshold, the float of x below and the one above; the half-way cases
u = -0.5 and u = +0.5; a NaN, both infinities and a quotient beyond int16."""
import functools

import numpy
import pytest

pytestmark = pytest.mark.gpu

F32 = numpy.float32
NB_MAPS = 128
CRAFTED_MAPS = (3, 35, 67, 99)
EXCEPTION_MAP = 7
SHAPES = [(1, 1), (3, 33), (2, 143)]
POINTS = {1: {1: (0,), 3: (0, 0, 0), 2: (0, 0)}, 3: {1: (7,), 3: (-3, 7, 1), 2: (1, -2)}}     # [K][n]
LENGTHS = [1, 3, 10, 40]


@pytest.fixture(autouse=True, params=[0xFF, 0x7F], ids=['poison_ff', 'poison_7f'])
def guard(request):
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


@pytest.fixture(scope='module')
def dev():
    from autoencoder_based_image_compression_amd import device
    return device


def crafted_quotients():
    """The x of the crafted latents, float32, exact: see the module's docstring. The hand-set threshold of magnitude a is
    0.75 + a / 64, so 2 u + 1 equals it at u = -1/8 + a / 128."""
    values = []
    for a in range(1, 18):
        at = F32(a) + F32(-0.125) + F32(a)/F32(128.)
        for sign in (F32(1.), F32(-1.)):
            values += [sign*at, sign*numpy.nextafter(at, F32(0.)), sign*numpy.nextafter(at, F32(100.))]
    for j in range(0, 18):
        values += [F32(j) + F32(0.5), -(F32(j) + F32(0.5))]
    values += [F32(numpy.nan), F32(numpy.inf), F32(-numpy.inf), F32(40000.), F32(-32768.), F32(32767.)]
    return numpy.array(values, dtype=F32)


@functools.lru_cache(maxsize=None)
def case(n, hw, length, k_points):
    """Inputs and the numpy reference of one case, made once and shared by the tests and the two poisons (read only)."""
    from autoencoder_based_image_compression_amd import ratecontrol as rc
    points = POINTS[k_points][n]
    rng = numpy.random.RandomState(1000*n + hw + 7*k_points + length)
    bw0 = rng.uniform(0.25, 2., size=NB_MAPS).astype(F32)
    mean = (rng.standard_normal(NB_MAPS)*0.2).astype(F32)
    for c in CRAFTED_MAPS:
        (bw0[c], mean[c]) = (F32(0.5), F32(0.))
    bw = (bw0[None, :]*(2.**numpy.arange(k_points))[:, None]).astype(F32)
    p = rng.uniform(0.05, 0.95, size=(k_points, NB_MAPS, length))
    thresholds = rc.rdo_thresholds(bw, p, 0.25, idx_map_exception=EXCEPTION_MAP)
    for c in CRAFTED_MAPS:                                          # all 16 columns, also those beyond L: the kernel must not read them
        thresholds[:, c, :] = (F32(0.75) + numpy.arange(1, 17, dtype=F32)/F32(64.))[None, :]
    clamped = numpy.clip(numpy.asarray(points), 0, k_points - 1)
    own = bw[clamped][:, None, :]                                   # (n, 1, 128): every image's own row
    y = ((rng.laplace(size=(n, hw, NB_MAPS))*3.).astype(F32)*own + mean).astype(F32)
    y[:, :, 9] = mean[9] + F32(1e-3)*own[:, :, 9]                   # a dead map
    y[:, :, EXCEPTION_MAP] = (F32(1.2)*own[:, :, EXCEPTION_MAP] + mean[EXCEPTION_MAP]).astype(F32)   # magnitude 1 everywhere, never lowered
    quotients = crafted_quotients()
    flat = y.reshape(n*hw, NB_MAPS)
    own_flat = numpy.broadcast_to(own, (n, hw, NB_MAPS)).reshape(n*hw, NB_MAPS)
    for (j, x) in enumerate(quotients[:n*hw*len(CRAFTED_MAPS)]):
        (row, c) = (j//len(CRAFTED_MAPS), CRAFTED_MAPS[j % len(CRAFTED_MAPS)])
        flat[row, c] = x*own_flat[row, c]
    gamma = rng.uniform(2e-5, 0.01, size=(NB_MAPS, NB_MAPS)).astype(F32)
    beta = rng.uniform(0.5, 2., size=NB_MAPS).astype(F32)
    # the reference: the rule per image with its own rows, then the statements behind the choice
    r = numpy.stack([rc.rdo_quantize_numpy(y[i], bw[clamped[i]], mean, thresholds[clamped[i]], length) for i in range(n)])
    with numpy.errstate(invalid='ignore', over='ignore'):
        nearest = numpy.rint((y - mean)/own)
        centered = y - mean
        cq = (own*r).astype(F32)
        rs = numpy.rint(cq/own)
        y2 = (cq + mean).astype(F32)
        bad = ~(numpy.abs(rs) < F32(32768.))
        not_quantized = ~(numpy.abs(cq.astype(numpy.float64) - centered.astype(numpy.float64)) < 1.5e-10)
        # (float)(int16_t)(int)rs: the conversion to int saturates (and gives 0 for a NaN), the one to int16 wraps. -32768 survives
        # both, so that element is out of range and yet not altered; an infinite or NaN `centered` equals no product
        as_int = numpy.where(numpy.isfinite(rs), numpy.clip(rs, -2.**31, 2.**31 - 1.), 0.).astype(numpy.int64)
        as_int16 = (as_int + 32768) % 65536 - 32768
        altered = ~((as_int16.astype(F32)*own).astype(F32) == centered)
        usable = numpy.isfinite(r) & (numpy.abs(r) < 32768.)
        # y2 rounds to the chosen symbol: `latent_quantize_rows` on it runs the statements behind the choice on the same r
        assert numpy.array_equal(numpy.rint((y2 - mean)/own)[usable], r[usable])
    checks = numpy.array([bad.sum(), not_quantized.sum(), altered.sum()], dtype=numpy.int64)
    return {'points': numpy.asarray(points, dtype=numpy.int32), 'bw': bw, 'mean': mean, 'thresholds': thresholds, 'y': y, 'y2': y2, 'r': r,
            'nearest': nearest.astype(F32), 'usable': usable, 'checks': checks, 'gamma': gamma, 'beta': beta}


def bits_of(tensor):
    """A float32 tensor as its bit patterns: NaNs compare like everything else."""
    return tensor.cpu().numpy().view(numpy.int32)


def assert_same_outputs(a, b, what):
    import torch
    assert torch.equal(a['symbols'], b['symbols']), what
    assert torch.equal(a['nonzero_flags'], b['nonzero_flags']), what
    assert numpy.array_equal(bits_of(a['shifted']), bits_of(b['shifted'])), what
    assert (a['t'] is None) == (b['t'] is None)
    if a['t'] is not None:
        assert numpy.array_equal(bits_of(a['t']), bits_of(b['t'])), what


def upload(guard, dev, c, learned):
    igdn = None if learned else (dev.pack_gamma(guard.upload(c['gamma'])), guard.upload(c['beta']))
    return (guard.upload(c['y']), guard.upload(c['bw']), guard.upload(c['thresholds']), guard.upload(c['points']), guard.upload(c['mean']), igdn)


@pytest.mark.parametrize('learned', [False, True], ids=['igdn', 'no_igdn'])
@pytest.mark.parametrize('length', LENGTHS)
@pytest.mark.parametrize('k_points', [1, 3])
@pytest.mark.parametrize('n, hw', SHAPES)
def test_kernel_equals_the_rule_and_the_rows_quantiser_behind_it(dev, guard, n, hw, k_points, length, learned):
    c = case(n, hw, length, k_points)
    (y_d, bw_d, thr_d, point_d, mean_d, igdn) = upload(guard, dev, c, learned)
    out = dev.latent_quantize_rdo(y_d, bw_d, thr_d, point_d, length, mean_d, igdn_out=igdn, want_shifted=True, want_flags=True)
    assert (out['t'] is None) == learned
    # the choice
    symbols = out['symbols'].cpu().numpy().reshape(n, NB_MAPS, hw).transpose(0, 2, 1)
    usable = c['usable']
    assert numpy.array_equal(symbols[usable], c['r'][usable].astype(numpy.int16))
    # behind the choice
    rows = dev.latent_quantize_rows(guard.upload(c['y2']), bw_d, point_d, mean_d, igdn_out=igdn, want_shifted=True, want_flags=True)
    assert_same_outputs(out, rows, 'against latent_quantize_rows on the chosen symbols')
    assert numpy.array_equal(out['checks'].cpu().numpy(), c['checks'])
    assert int(rows['checks'][0].item()) == c['checks'][0]
    assert int(out['nonzero_flags'][:, 9].sum()) == 0
    if n*hw >= 36:
        # every crafted latent is in: NaN, two infinities, 40000 and -32768 leave int16; symbols were lowered, by one, towards zero
        assert c['checks'][0] == 5
        moved = c['r'] != c['nearest']
        moved &= usable
        assert moved[..., list(CRAFTED_MAPS)].any() and (length == 1 or moved[..., 20:30].any())
        assert numpy.array_equal(c['r'][moved], c['nearest'][moved] - numpy.sign(c['nearest'][moved]))
        assert not moved[..., EXCEPTION_MAP].any() and numpy.abs(c['nearest'][moved]).max() <= min(length, 16)


@pytest.mark.parametrize('learned', [False, True], ids=['igdn', 'no_igdn'])
@pytest.mark.parametrize('length', [1, 10])
@pytest.mark.parametrize('k_points', [1, 3])
@pytest.mark.parametrize('n, hw', SHAPES)
def test_zero_thresholds_equal_the_rows_quantiser_bit_for_bit(dev, guard, n, hw, k_points, length, learned):
    c = case(n, hw, length, k_points)
    (y_d, bw_d, thr_d, point_d, mean_d, igdn) = upload(guard, dev, c, learned)
    out = dev.latent_quantize_rdo(y_d, bw_d, guard.upload(numpy.zeros_like(c['thresholds'])), point_d, length, mean_d, igdn_out=igdn,
                                  want_shifted=True, want_flags=True)
    rows = dev.latent_quantize_rows(y_d, bw_d, point_d, mean_d, igdn_out=igdn, want_shifted=True, want_flags=True)
    assert_same_outputs(out, rows, 'thresholds of zeros')
    assert numpy.array_equal(out['checks'].cpu().numpy(), rows['checks'].cpu().numpy())


@pytest.mark.parametrize('absent', ['shifted', 't', 'symbols', 'nonzero_flags', 'checks'])
def test_every_optional_output_absent_in_turn(dev, guard, absent):
    import torch
    from autoencoder_based_image_compression_amd import _native
    (n, hw, length, k_points) = (3, 33, 10, 3)
    c = case(n, hw, length, k_points)
    (y_d, bw_d, thr_d, point_d, mean_d, igdn) = upload(guard, dev, c, False)
    full = dev.latent_quantize_rdo(y_d, bw_d, thr_d, point_d, length, mean_d, igdn_out=igdn, want_shifted=True, want_flags=True)
    if absent == 'checks':                                           # the wrapper always counts: the C entry point itself
        part = {name: (torch.zeros_like(t) if name == 'nonzero_flags' else torch.empty_like(t)) for (name, t) in full.items() if name != 'checks'}
        ptr = lambda t: t.data_ptr()
        assert _native.hip().eae_hip_latent_quantize_rdo(ptr(y_d), ptr(mean_d), ptr(bw_d), ptr(thr_d), ptr(point_d), k_points, length,
                                                         ptr(igdn[0]), ptr(igdn[1]), ptr(part['shifted']), ptr(part['t']), ptr(part['symbols']),
                                                         ptr(part['nonzero_flags']), None, n, hw, None) == 0
        torch.cuda.synchronize()
        part['checks'] = None
    else:
        part = dev.latent_quantize_rdo(y_d, bw_d, thr_d, point_d, length, mean_d, igdn_out=None if absent == 't' else igdn,
                                       want_shifted=absent != 'shifted', want_symbols=absent != 'symbols', want_flags=absent != 'nonzero_flags')
    assert part[absent] is None
    for name in ('shifted', 't', 'symbols', 'nonzero_flags', 'checks'):
        if name == absent:
            continue
        if full[name].dtype == torch.float32:
            assert numpy.array_equal(bits_of(part[name]), bits_of(full[name])), name
        else:
            assert torch.equal(part[name], full[name]), name


def test_refusals(dev, guard):
    import torch
    from autoencoder_based_image_compression_amd import _native
    (n, hw, length, k) = (2, 143, 10, 3)
    c = case(n, hw, length, k)
    (y_d, bw_d, thr_d, point_d, mean_d, _) = upload(guard, dev, c, True)
    (g_d, b_d) = (guard.upload(c['gamma']), guard.upload(c['beta']))
    symbols = torch.full((n, NB_MAPS, hw), -7, dtype=torch.int16, device='cuda')
    t = torch.full((n, hw, NB_MAPS), -7., dtype=torch.float32, device='cuda')
    call = _native.hip().eae_hip_latent_quantize_rdo
    good = [y_d.data_ptr(), None, bw_d.data_ptr(), thr_d.data_ptr(), point_d.data_ptr(), k, length, g_d.data_ptr(), b_d.data_ptr(), None,
            t.data_ptr(), symbols.data_ptr(), None, None, n, hw, None]
    # NULL y / bin widths / thresholds / point; gamma without beta, beta without gamma, no t_out
    for position in (0, 2, 3, 4, 7, 8, 10):
        assert call(*(good[:position] + [None] + good[position + 1:])) == -1, position
    # K, L, n, hw out of range; y, bin widths, thresholds, t_out misaligned
    for (position, value) in ((5, 0), (6, 0), (6, 256), (6, -1), (14, 0), (15, 0), (0, good[0] + 4), (2, good[2] + 8), (3, good[3] + 4),
                              (3, good[3] + 8), (10, good[10] + 4)):
        assert call(*(good[:position] + [value] + good[position + 1:])) == -1, (position, value)
    assert call(*(good[:15] + [(1 << 21) + 1] + good[16:])) == -2
    torch.cuda.synchronize()
    assert bool((symbols == -7).all().item()) and bool((t == -7.).all().item())          # nothing was launched
    for (position, value) in ((6, 1), (6, 255)):                                         # the ends of L's range are taken
        assert call(*(good[:position] + [value] + good[position + 1:])) == 0, (position, value)
    torch.cuda.synchronize()
    with pytest.raises(dev.HipError):
        dev.latent_quantize_rdo(y_d, bw_d, thr_d[:, :, :8].contiguous(), point_d, length, mean_d)
    with pytest.raises(dev.HipError):
        dev.latent_quantize_rdo(y_d, bw_d, thr_d[:1].contiguous(), point_d, length, mean_d)
    with pytest.raises(dev.HipError):
        dev.latent_quantize_rdo(y_d, bw_d, thr_d.double(), point_d, length, mean_d)
    with pytest.raises(dev.HipError):
        dev.latent_quantize_rdo(y_d, bw_d, thr_d, point_d.long(), length, mean_d)
    with pytest.raises(dev.HipError):
        dev.latent_quantize_rdo(y_d, bw_d, thr_d, point_d, 0, mean_d)
