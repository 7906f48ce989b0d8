"""The SVHN kernels (csrc/hip/svhn.hip) called directly through their device.py wrappers, at the shapes and values where
they can go wrong: every row-block and column-block edge of `dense_f64_kernel` (ROWS = 8 rows, 256 columns, 256 k per LDS
pass), the grid-stride loops behind the 4096-block cap of the element-wise kernels, half-way ties, the range limits of the
casts, and the NaN / inf rules of the reference's numpy assertions. Each result is compared with a plain float64 numpy
restatement of the reference expression written out here and, for the dense layers, bit for bit with oracle/svhn_oracle.c.
The whole model runs end to end at the hidden / latent sizes of the reference's own tests (svhn/test_eae.py) and at its
evaluation batch of 250 images (svhn/reconstructing_eae_svhn.py)."""
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


GRID_CAP = 4096*256          # elements one launch of grid_for() covers without looping (csrc/hip/svhn.hip)
# every layer of 3072-300-200 (BASELINE.json configs[0]), 3072-15-12 and 3072-32-16 (svhn/test_eae.py), encoder then decoder
LAYERS = sorted({(3072, h) for h in (300, 15, 32)} | {(h, 3072) for h in (300, 15, 32)}
                | {(300, 200), (200, 300), (15, 12), (12, 15), (32, 16), (16, 32)})
EDGES = [(k, m) for k in (1, 255, 256, 257) for m in (1, 255, 256, 257, 513)]
ROWS = (1, 7, 8, 9, 250, 1001)


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


def _close(a, b, rel=1e-12):
    return numpy.abs(a - b).max() <= rel*max(1., numpy.abs(b).max())


def _leaky(v):
    """svhn/tools/tools.py:676-694: coefficients 0.1 where v < 0, 1 elsewhere."""
    coefficients = numpy.ones(v.shape)
    coefficients[v < 0.] = 0.1
    return coefficients*v


# ---- svhn_dense ---------------------------------------------------------------------------------------------------------

def _dense_inputs(n, k, m, seed):
    rng = numpy.random.RandomState(seed)
    x = rng.standard_normal((n, k))
    w = rng.standard_normal((k, m))*(1./numpy.sqrt(k))
    b = rng.standard_normal(m)*0.5
    return x, w, b


@pytest.mark.parametrize('km', LAYERS + EDGES, ids=lambda km: '{}x{}'.format(*km))
def test_dense_matches_oracle_and_float64(T, dev, km):
    from oracle import svhn as orc
    (k, m) = km
    for n in ROWS:
        (x, w, b) = _dense_inputs(n, k, m, seed=n*7 + k*3 + m)
        (xd, wd, bd) = (_cuda(T, x), _cuda(T, w), _cuda(T, b))
        linear = dev.svhn_dense(xd, wd, bd, False).cpu().numpy()
        leaky = dev.svhn_dense(xd, wd, bd, True).cpu().numpy()
        assert numpy.array_equal(linear, orc.dense(x, w, b, False)), (n, k, m)
        assert numpy.array_equal(leaky, orc.dense(x, w, b, True)), (n, k, m)
        reference = x.dot(w) + b.reshape(1, m)
        assert _close(linear, reference), (n, k, m)
        assert _close(leaky, _leaky(reference)), (n, k, m)
        # the activation is applied to exactly the value the linear layer returns
        assert numpy.array_equal(leaky, _leaky(linear)), (n, k, m)


@pytest.mark.parametrize('leaky', [False, True])
def test_dense_exact_zero_and_negative_preactivations(T, dev, leaky):
    """Dyadic inputs make every product and partial sum exact, so the pre-activations are known exactly: zero in every
    even column of every row whose bias cancels the dot product, negative and positive elsewhere. LeakyReLU keeps 0 (not
    < 0) and scales only the negatives (tools.py:692-694)."""
    from oracle import svhn as orc
    rng = numpy.random.RandomState(21)
    for (n, k, m) in ((9, 300, 257), (17, 257, 300), (250, 15, 12), (1001, 32, 513)):
        x = rng.randint(-4, 5, size=(n, k))/4.
        w = rng.randint(-4, 5, size=(k, m))/8.
        exact = x.dot(w)                                   # exact: every term and sum is a small multiple of 1/32
        b = rng.randint(-8, 9, size=m)/4.
        b[::2] = -exact[n - 1, ::2]                        # the last row (in the last, partial row block) is 0 there
        out = dev.svhn_dense(_cuda(T, x), _cuda(T, w), _cuda(T, b), leaky).cpu().numpy()
        pre = exact + b
        assert (pre[n - 1, ::2] == 0.).all() and (pre < 0.).any() and (pre > 0.).any()
        expected = _leaky(pre) if leaky else pre
        assert numpy.array_equal(out, expected), (n, k, m)
        assert numpy.array_equal(out, orc.dense(x, w, b, leaky))
        assert not numpy.signbit(out[n - 1, ::2]).any()   # +0, not -0 (0.1 * -0 would be -0)


# ---- svhn_quantize ------------------------------------------------------------------------------------------------------

def _quantization(y, bw):
    """svhn/tools/tools.py:1095."""
    return bw*numpy.round(y/bw)


def _omitted(y, bw):
    """Element-wise count of what makes numpy.testing.assert_almost_equal(quantization(y), y, decimal=10) fail
    (tools.py:214-217): NaN and +-inf compare by position (quantization keeps them in place), every other element fails
    when |quantization(y) - y| >= 1.5 * 10**-10."""
    q = _quantization(y, bw)
    with numpy.errstate(invalid='ignore'):
        passes = numpy.isnan(y) | (q == y) | (numpy.abs(q - y) < 1.5e-10)
    return int((~passes).sum())


def _assertion_fails(y, bw):
    try:
        numpy.testing.assert_almost_equal(_quantization(y, bw), y, decimal=10)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('bw', [1., 0.5, 0.25, 2.**-10, 0.3, 3.])
def test_quantize_ties_and_symbols(T, dev, bw):
    rng = numpy.random.RandomState(int(bw*1024) + 1)
    j = numpy.arange(-600, 600, dtype=numpy.float64)
    ties = (j + 0.5)*bw                                   # exact half-way cases when bw is a power of two
    y = numpy.concatenate([ties, j*bw, rng.standard_normal(GRID_CAP + 4099)*40.*bw])
    (q, symbols, checks) = dev.svhn_quantize(_cuda(T, y), bw, want_q=True, want_symbols=True)
    (q, symbols, checks) = (q.cpu().numpy(), symbols.cpu().numpy(), checks.cpu().tolist())
    q_ref = _quantization(y, bw)
    assert numpy.array_equal(q, q_ref)
    assert numpy.array_equal(symbols, numpy.round(q_ref/bw).astype(numpy.int64))
    if bw in (1., 0.5, 0.25, 2.**-10):
        assert numpy.array_equal(symbols[:j.size], numpy.round(j + 0.5).astype(numpy.int64))   # half to even
        assert numpy.array_equal(symbols[j.size:2*j.size], j.astype(numpy.int64))
    assert checks[0] == 0
    assert checks[1] == _omitted(y, bw) > 0
    # already quantised samples pass the assertion and count nothing
    (_, _, checks) = dev.svhn_quantize(_cuda(T, q_ref), bw, want_q=False)
    assert checks.cpu().tolist() == [0, 0] and not _assertion_fails(q_ref, bw)


def test_quantize_symbol_range(T, dev):
    """checks[0]: symbols round(q / bw) whose magnitude reaches 2^31 do not fit the int32 symbols."""
    for bw in (1., 0.5, 2.**-20):
        s = numpy.array([2.**31 - 1, 2.**31 - 1.5, 2.**31 - 0.5, 2.**31, -(2.**31 - 1), -(2.**31 - 0.5), -2.**31, 3.5, -2.**40])
        y = s*bw
        (_, symbols, checks) = dev.svhn_quantize(_cuda(T, y), bw, want_q=False, want_symbols=True)
        r = numpy.round(_quantization(y, bw)/bw)
        assert checks.cpu().tolist()[0] == int((~(numpy.abs(r) < 2.**31)).sum()) == 5
        fits = numpy.abs(r) < 2.**31
        assert numpy.array_equal(symbols.cpu().numpy()[fits], r[fits].astype(numpy.int64))


def test_quantize_omitted_rule(T, dev):
    """checks[1] against the 1.5e-10 bound of assert_almost_equal(decimal=10), with deviations just below and just above
    it around zero and around non-zero multiples of several bin widths, on quantised and unquantised inputs."""
    rng = numpy.random.RandomState(5)
    for bw in (2.**-20, 1e-3, 0.5):
        base = rng.randint(-50, 51, size=4096)*bw
        d = numpy.array([0., 1e-11, 1.4e-10, 1.49e-10, 1.5e-10, 1.51e-10, 1.6e-10, 1e-9, 1e-6])
        y = (base.reshape(-1, 1) + numpy.concatenate([d, -d]).reshape(1, -1)).ravel()
        (_, _, checks) = dev.svhn_quantize(_cuda(T, y), bw, want_q=False)
        expected = _omitted(y, bw)
        assert checks.cpu().tolist() == [0, expected]
        assert expected > 0 and _assertion_fails(y, bw)
        # deviations strictly between 1.5e-10 and 1.5e-9 alone: counted, and numpy raises
        mid = base + 4e-10
        (_, _, checks) = dev.svhn_quantize(_cuda(T, mid), bw, want_q=False)
        assert checks.cpu().tolist()[1] == _omitted(mid, bw) == mid.size and _assertion_fails(mid, bw)
        # deviations below the bound alone: nothing counted, and numpy passes
        low = base + 1.2e-10
        (_, _, checks) = dev.svhn_quantize(_cuda(T, low), bw, want_q=False)
        assert checks.cpu().tolist() == [0, _omitted(low, bw)] == [0, 0] and not _assertion_fails(low, bw)


def test_quantize_nan_and_inf(T, dev):
    """NaN and +-inf pass the reference's "quantization was omitted" assertion (numpy compares them by position), so they
    count in checks[1] only if the finite part fails; they never give a symbol (checks[0]), and count_symbols raises the
    ValueError the reference raises there (int(numpy.round(nan)) in tools.py:221) instead of the AssertionError."""
    from autoencoder_based_image_compression_amd.svhn.tools import tools as tls
    y = numpy.array([1., numpy.nan, numpy.inf, -numpy.inf, -2., 0.])
    assert not _assertion_fails(y, 1.) and _omitted(y, 1.) == 0
    (q, _, checks) = dev.svhn_quantize(_cuda(T, y), 1., want_q=True, want_symbols=True)
    assert checks.cpu().tolist() == [3, 0]
    assert numpy.array_equal(q.cpu().numpy(), _quantization(y, 1.), equal_nan=True)
    y2 = numpy.concatenate([y, [0.25]])
    (_, _, checks) = dev.svhn_quantize(_cuda(T, y2), 1., want_q=False)
    assert checks.cpu().tolist() == [3, 1] and _omitted(y2, 1.) == 1 and _assertion_fails(y2, 1.)
    with pytest.raises(ValueError):
        tls.count_symbols(numpy.array([0., numpy.nan, 2.]), 1.)
    with pytest.raises(AssertionError):
        tls.count_symbols(numpy.array([0., numpy.nan, 2.5]), 1.)


# ---- svhn_symbol_histogram -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['negative', 'straddle', 'single', 'wide'])
def test_symbol_histogram(T, dev, kind):
    rng = numpy.random.RandomState(len(kind))
    size = GRID_CAP + 12345
    if kind == 'negative':
        s = rng.randint(-40, -2, size=size)
        s[-1] = -41                                       # the minimum only in the very last element
    elif kind == 'straddle':
        s = numpy.round(rng.laplace(size=size)*6.).astype(numpy.int64)
        s[-1] = s.max() + 3                               # the maximum only in the very last element
    elif kind == 'single':
        s = numpy.full(size, -7)
    else:
        s = rng.randint(-3, 4, size=size)
        s[0] = -70000
        s[-1] = 70000
    (hist, lo) = dev.svhn_symbol_histogram(_cuda(T, s.astype(numpy.int32)))
    assert lo == s.min()
    assert hist.dtype == numpy.int64 and numpy.array_equal(hist, numpy.bincount(s - s.min()))
    assert hist.sum() == size


# ---- svhn_preprocess / svhn_postprocess ----------------------------------------------------------------------------------

def test_preprocess(T, dev):
    """svhn/svhn/svhn.py:210, (uint8 - mean) / std in float64, over more elements than one grid covers."""
    rng = numpy.random.RandomState(3)
    (n, d) = (400, 3072)
    images = rng.randint(0, 256, size=(n, d)).astype(numpy.uint8)
    images[0] = 0
    images[-1] = 255
    mean = rng.uniform(0., 255., size=(1, d))
    mean[0, :4] = (0., 255., 127.5, 128.)
    for std in (61.3, 1., 0.1):
        out = dev.svhn_preprocess(_cuda(T, images), _cuda(T, mean.reshape(-1)), std).cpu().numpy()
        expected = (images - numpy.tile(mean, (n, 1)))/std
        assert numpy.array_equal(out, expected)


def test_postprocess_edges(T, dev):
    """svhn/eae/utils.py:71-74 + tools.py:166: uint8(round_half_even(clip(rec * std + mean, 0, 255))) and the squared
    error of tools.py:857-859 as an int64 sum. The targets land on 0 and 255, just outside, and on every .5 tie."""
    rng = numpy.random.RandomState(4)
    (n, d) = (250, 3072)
    std = 2.
    mean = numpy.round(rng.uniform(0., 255., size=d)*4.)/4.          # dyadic: rec * std + mean is exact
    target = rng.uniform(-20., 275., size=(n, d))
    specials = numpy.concatenate([[0., 255., -0., -0.5, 255.5, -1e-9, 255. + 1e-9, 0.5, 254.5, 1e-300, -1e300, 1e300],
                                  numpy.arange(0, 256) + 0.5, numpy.arange(-3, 259)])
    target[0, :specials.size] = specials
    target[n - 1, d - specials.size:] = specials[::-1]
    rec = (numpy.round(target*4.)/4. - mean)/std                      # exact values whose rescaled form is known
    rec[0, :12] = (specials[:12] - mean[:12])/std
    ref = rng.randint(0, 256, size=(n, d)).astype(numpy.uint8)
    (out, sse) = dev.svhn_postprocess(_cuda(T, rec), std, _cuda(T, mean), _cuda(T, ref))
    (out, sse) = (out.cpu().numpy(), sse.cpu().numpy())
    rescaled = rec*std + numpy.tile(mean, (n, 1))
    expected = numpy.round(rescaled.clip(min=0., max=255.)).astype(numpy.uint8)
    assert numpy.array_equal(out, expected)
    assert numpy.array_equal(sse, ((ref.astype(numpy.int64) - expected.astype(numpy.int64))**2).sum(axis=1))
    # the ties really are ties, and they round to even
    ties = rescaled[0, 12:12 + 256]
    assert numpy.array_equal(ties, numpy.arange(0, 256) + 0.5)
    assert numpy.array_equal(out[0, 12:12 + 255], (numpy.arange(0, 255) + 1)//2*2)
    (out_only, none) = dev.svhn_postprocess(_cuda(T, rec), std, _cuda(T, mean))
    assert none is None and numpy.array_equal(out_only.cpu().numpy(), expected)


# ---- the whole model ------------------------------------------------------------------------------------------------------

def _images(n, seed):
    rng = numpy.random.RandomState(seed)
    images = rng.randint(0, 256, size=(n, 3072)).astype(numpy.uint8)
    mean = images.astype(numpy.float64).mean(axis=0).reshape(1, 3072)
    return images, mean, float(images.astype(numpy.float64).std())


def _count_symbols(q, bw):
    """svhn/tools/tools.py:214-231, restated."""
    numpy.testing.assert_almost_equal(_quantization(q, bw), q, decimal=10)
    (minimum, maximum) = (numpy.amin(q), numpy.amax(q))
    nb_edges = int(numpy.round((maximum - minimum)/bw)) + 2
    edges = numpy.linspace(minimum - 0.5*bw, maximum + 0.5*bw, num=nb_edges)
    return numpy.histogram(q, bins=edges)[0]


def _rate_psnr(images, mean, std, parameters, nb_y, bw):
    """svhn/eae/utils.py:54-74 with tools.py:289-341 and :857-865, restated on the oracle's encoder / decoder."""
    from oracle import svhn as orc
    x = (images - numpy.tile(mean, (images.shape[0], 1)))/std
    (hidden, y) = orc.encoder(x, parameters)
    q = _quantization(y, bw)
    hist = _count_symbols(q, bw)
    nz = numpy.extract(hist != 0, hist)
    frequency = nz.astype(numpy.float64)/numpy.sum(nz)
    rate = nb_y*(-numpy.sum(frequency*numpy.log2(frequency)))/images.shape[1]
    (hidden_d, rec) = orc.decoder(q, parameters)
    rec_u8 = numpy.round((rec*std + numpy.tile(mean, (images.shape[0], 1))).clip(min=0., max=255.)).astype(numpy.uint8)
    mse = numpy.mean((images.astype(numpy.float64) - rec_u8.astype(numpy.float64))**2, axis=1)
    psnr = numpy.mean(10.*numpy.log10((255.**2)/mse))
    return {'x': x, 'hidden': hidden, 'y': y, 'q': q, 'hidden_d': hidden_d, 'rec': rec, 'rec_u8': rec_u8, 'rate': rate,
            'psnr': psnr, 'hist': hist}


@pytest.mark.parametrize('arch', [(300, 200), (15, 12), (32, 16)], ids=lambda a: '3072-{}-{}'.format(*a))
def test_entropy_autoencoder_end_to_end(arch):
    from autoencoder_based_image_compression_amd.svhn.eae import utils
    from autoencoder_based_image_compression_amd.svhn.eae.EntropyAutoencoder import EntropyAutoencoder
    from autoencoder_based_image_compression_amd.svhn.svhn import svhn
    from autoencoder_based_image_compression_amd.svhn.tools import tools as tls
    (nb_hidden, nb_y) = arch
    numpy.random.seed(nb_hidden + nb_y)
    ae = EntropyAutoencoder(3072, nb_hidden, nb_y, 1., 15., False)
    (images, mean, std) = _images(250, seed=nb_y)
    for bw in (0.02, 0.1):
        expected = _rate_psnr(images, mean, std, ae.get_parameters(), nb_y, bw)
        assert expected['hist'].size >= 3                 # a few symbols, not a degenerate rate
        x = svhn.preprocess_svhn(images, mean, std)
        assert numpy.array_equal(x, expected['x'])
        (hidden, y) = ae.encoder(x)
        assert numpy.array_equal(hidden, expected['hidden']) and numpy.array_equal(y, expected['y'])
        q = tls.quantization(y, bw)
        assert numpy.array_equal(q, expected['q'])
        assert numpy.array_equal(tls.count_symbols(q, bw), expected['hist'])
        (hidden_d, rec) = ae.decoder(q)
        assert numpy.array_equal(hidden_d, expected['hidden_d']) and numpy.array_equal(rec, expected['rec'])
        (rate, psnr, rec_u8) = utils.compute_rate_psnr(images, mean, std, ae, bw, 1, None, return_reconstruction=True)
        assert numpy.array_equal(rec_u8, expected['rec_u8'])
        assert rate == expected['rate'] and psnr == expected['psnr']
