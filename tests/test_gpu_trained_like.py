"""Every GDN / IGDN path of the library on parameters like a TRAINED model's (tests/model_cases.py): an asymmetric `gamma` and
one `beta` per channel, against the CPU oracle on the same parameters, bit for bit (tolerance ZERO, the project's contract).

The other GPU tests take their models from `variables.random_variables` -- the reference's initialisation, `gamma` symmetric and
`beta` = 1 -- so none of them can tell gamma[k][c] from gamma[c][k], or `beta` in the natural channel order from `beta` in the
kernels' packed order. The denominator d[c] = sum_k x[k]^2 * gamma[k][c] + beta[c] has four device implementations
(`gdn_denominator`, `wave_epilogue`, `wave_gdn_inplace`, `quarter_denominator` + `squares_for_mfma`) behind a dozen entry points;
each is launched here. That the oracle itself is oriented correctly, and that either mistake moves more than 95 % of the
elements by 250 times the float32 tolerance, is pinned on the CPU (tests/test_oracle_transforms.py); each comparison below also
asserts that the oracle with `gamma` TRANSPOSED differs from the result at half the elements or more, so that a later edit of
the data cannot quietly make it symmetric again."""
import numpy
import pytest
import torch

import model_cases
from test_gpu_codec import reference_shaped_path
from test_gpu_kernels import FORMS, _assert_handed_over, _image, _select_form

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _guarded_buffers():
    """Every test of this module runs on poisoned buffers between guard bands: what device.py / pipeline.py allocate holds 0xFF bytes
    (NaN, -1) until a kernel writes it, and a byte written outside a tensor fails the test (tests/guarded.py)."""
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), 0xFF):
        yield


GDN_REL = 4e-6        # against the float64 definition: derived in tests/test_oracle_transforms.py


@pytest.fixture(scope='module')
def dev():
    from autoencoder_based_image_compression_amd import device
    return device


@pytest.fixture(scope='module')
def orc():
    from oracle import transforms
    return transforms


def _vars(seed, learned=False, scale_weights_6=False):
    v = model_cases.trained_like_variables(1., learned, seed=seed)
    if scale_weights_6:        # leave the clip floor so that the cast is exercised
        v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    return v


def _transposed(v):
    return {name: (model_cases.gamma_transposed(a) if '/gamma_' in name else a) for (name, a) in v.items()}


def _cuda(a):
    return torch.from_numpy(numpy.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _differs_at_half_or_more(got, other):
    return numpy.mean(numpy.asarray(got) != numpy.asarray(other)) >= 0.5


_cache = {}


def _once(key, make):
    """An oracle result computed once and shared by the cases of a parametrised test; nobody writes to it."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- eae_hip_gdn (gdn.hip: gdn_denominator<4> in 32- and 128-row blocks) and its numpy-shaped call surface --------------------
@pytest.mark.parametrize('rows', [1000, 32801])           # 32-row blocks; 128-row blocks with a ragged last block
@pytest.mark.parametrize('inverse', [False, True])
def test_gdn(dev, orc, rows, inverse):
    v = _vars(10)
    (g, b) = (v['encoder/gamma_3'], v['encoder/beta_3'])
    x = numpy.random.RandomState(11).standard_normal(size=(rows, 128)).astype(numpy.float32)*3
    got = _host(dev.gdn(_cuda(x), dev.pack_gamma(_cuda(g)), _cuda(b), inverse=inverse))
    assert numpy.array_equal(got, orc.gdn(x, g, b, inverse=inverse))
    assert _differs_at_half_or_more(got, orc.gdn(x, model_cases.gamma_transposed(g), b, inverse=inverse))
    ref = model_cases.gdn_float64(x, g, b, inverse)
    assert numpy.all(numpy.abs(got - ref) <= GDN_REL*numpy.abs(ref))


def test_pack_gamma_permutes_the_columns_only(dev):
    """eae_hip_pack_gamma: row k stays row k (the contracted channel), column c moves to its packed place."""
    g = _vars(10)['encoder/gamma_3']
    expect = numpy.empty_like(g)
    expect[:, model_cases.packed_channel_order()] = g
    assert numpy.array_equal(_host(dev.pack_gamma(_cuda(g))), expect)
    assert numpy.array_equal(model_cases.packed_channel_order(), dev.packed_channel_order())


def test_tfutils_gdn_and_inverse_gdn(orc):
    """kodak/tfutils: the reference's call surface (numpy in, numpy out), against the oracle and the float64 definition."""
    from autoencoder_based_image_compression_amd.kodak.tfutils import tfutils
    v = _vars(12)
    (g, b) = (v['decoder/gamma_5'], v['decoder/beta_5'])
    x = numpy.random.RandomState(13).standard_normal(size=(2, 4, 6, 128)).astype(numpy.float32)*3
    for (inverse, fn) in ((False, tfutils.gdn), (True, tfutils.inverse_gdn)):
        got = fn(x, g, b)
        ref = model_cases.gdn_float64(x, g, b, inverse)
        assert got.dtype == numpy.float32 and got.shape == x.shape
        assert numpy.all(numpy.abs(got - ref) <= GDN_REL*numpy.abs(ref))
        assert numpy.array_equal(got, orc.gdn(x, g, b, inverse=inverse))
        assert model_cases.fraction_beyond(model_cases.gdn_float64(x, model_cases.gamma_transposed(g), b, inverse), got) >= 0.5


# ---- conv_1 with the gdn_1 epilogue (conv1.hip: wave_epilogue) ------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 48, 80), (1, 36, 100)])          # (1, 36, 100): the last tile of a row is ragged
def test_conv1_gdn1(dev, orc, shape):
    v = _vars(1)
    x = _image(numpy.random.RandomState(2), *shape)
    raw = orc.conv2d_same(x.astype(numpy.float32)[..., None], v['encoder/weights_1'], 4, v['encoder/biases_1'])
    got = _host(dev.conv9x9s4_u8(_cuda(x), dev.pack_conv9x9s4_weights(_cuda(v['encoder/weights_1'])), _cuda(v['encoder/biases_1']),
                                 dev.pack_gamma(_cuda(v['encoder/gamma_1'])), _cuda(v['encoder/beta_1'])))
    assert numpy.array_equal(got, orc.gdn(raw, v['encoder/gamma_1'], v['encoder/beta_1']))
    assert _differs_at_half_or_more(got, orc.gdn(raw, model_cases.gamma_transposed(v['encoder/gamma_1']), v['encoder/beta_1']))


# ---- conv_2 / transpose_conv_1 with their normalisations, every form of the conv GEMM ------------------------------------------
def _conv2_reference(orc, shape):
    v = _vars(3)
    x = numpy.random.RandomState(4).standard_normal(size=shape + (128,)).astype(numpy.float32)
    raw = orc.conv2d_same(x, v['encoder/weights_2'], 2, v['encoder/biases_2'])
    return (v, x, orc.gdn(raw, v['encoder/gamma_2'], v['encoder/beta_2']),
            orc.gdn(raw, model_cases.gamma_transposed(v['encoder/gamma_2']), v['encoder/beta_2']))


def _tconv1_reference(orc, shape):
    v = _vars(5)
    x = numpy.random.RandomState(6).standard_normal(size=shape + (128,)).astype(numpy.float32)
    raw = orc.conv2d_transpose_same(x, v['decoder/weights_4'], 2, v['decoder/biases_4'])
    return (v, x, orc.gdn(raw, v['decoder/gamma_5'], v['decoder/beta_5'], inverse=True),
            orc.gdn(raw, model_cases.gamma_transposed(v['decoder/gamma_5']), v['decoder/beta_5'], inverse=True))


def _run_conv2(dev, v, x, ws):
    return _host(dev.conv5x5s2(_cuda(x), dev.pack_conv_weights(_cuda(v['encoder/weights_2'])), _cuda(v['encoder/biases_2']), dev.NORM_GDN,
                               dev.pack_gamma(_cuda(v['encoder/gamma_2'])), _cuda(v['encoder/beta_2']), workspace=ws))


def _run_tconv1(dev, v, x, ws):
    return _host(dev.tconv5x5s2(_cuda(x), dev.pack_tconv_weights(_cuda(v['decoder/weights_4'])), _cuda(v['decoder/biases_4']), dev.NORM_IGDN,
                                dev.pack_gamma(_cuda(v['decoder/gamma_5'])), _cuda(v['decoder/beta_5']), workspace=ws))


@pytest.mark.parametrize('form,tile', FORMS)
@pytest.mark.parametrize('shape', [(1, 6, 10), (2, 16, 24)])
def test_conv5x5s2_gdn_in_every_form(dev, orc, shape, form, tile, launch_options):
    _select_form(launch_options, form, tile)
    (v, x, ref, ref_transposed) = _once(('conv2', shape), lambda: _conv2_reference(orc, shape))
    ws = dev.conv_workspace('cuda') if form.startswith(('cut', 'one')) else None      # a cut launch needs a workspace, and its owner collects
    got = _run_conv2(dev, v, x, ws)
    assert numpy.array_equal(got, ref)
    _assert_handed_over(torch, dev, ws)
    assert _differs_at_half_or_more(got, ref_transposed)


@pytest.mark.parametrize('form,tile', FORMS)
@pytest.mark.parametrize('shape', [(1, 3, 5), (2, 8, 12)])
def test_tconv5x5s2_igdn_in_every_form(dev, orc, shape, form, tile, launch_options):
    _select_form(launch_options, form, tile)
    (v, x, ref, ref_transposed) = _once(('tconv1', shape), lambda: _tconv1_reference(orc, shape))
    ws = dev.conv_workspace('cuda') if form.startswith(('cut', 'one')) else None
    got = _run_tconv1(dev, v, x, ws)
    assert numpy.array_equal(got, ref)
    _assert_handed_over(torch, dev, ws)
    assert _differs_at_half_or_more(got, ref_transposed)


@pytest.mark.parametrize('with_workspace', [False, True])
def test_conv_and_tconv_as_the_product_library_launches_them(dev, orc, with_workspace):
    """The same comparisons on whatever library the package loads (the product one unless EAE_HIP_LIB says otherwise), in the
    forms its launch picks by itself, with and without a workspace."""
    for shape in ((1, 6, 10), (2, 16, 24)):
        (v, x, ref, ref_transposed) = _once(('conv2', shape), lambda: _conv2_reference(orc, shape))
        ws = dev.conv_workspace('cuda') if with_workspace else None
        got = _run_conv2(dev, v, x, ws)
        assert numpy.array_equal(got, ref) and _differs_at_half_or_more(got, ref_transposed)
        _assert_handed_over(torch, dev, ws)
    for shape in ((1, 3, 5), (2, 8, 12)):
        (v, x, ref, ref_transposed) = _once(('tconv1', shape), lambda: _tconv1_reference(orc, shape))
        ws = dev.conv_workspace('cuda') if with_workspace else None
        got = _run_tconv1(dev, v, x, ws)
        assert numpy.array_equal(got, ref) and _differs_at_half_or_more(got, ref_transposed)
        _assert_handed_over(torch, dev, ws)


# ---- the latent stage: gdn_3 -> quantiser -> inverse_gdn_4 (latent.hip, latent_body.h) ------------------------------------------
def _latent_inputs(shape):
    rng = numpy.random.RandomState(shape[1]*7)
    x = (rng.laplace(size=shape + (128,))*rng.uniform(0.1, 6., size=128)).astype(numpy.float32)
    x[:, :, :, 9] = 1e-3                         # a dead map after quantisation
    bw = rng.uniform(0.4, 2., size=128).astype(numpy.float32)
    mean = rng.normal(scale=0.2, size=128).astype(numpy.float32)
    mean[9] = 0.
    return (x, bw, mean)


def _stage_reference(orc, v, x, bw, mean, sides):
    """oracle gdn_3 -> numpy quantiser -> oracle inverse_gdn_4, with either normalisation left out as `sides` says; the second
    dict is the same chain with both gamma matrices transposed."""
    chains = []
    for variables in (v, _transposed(v)):
        y = orc.gdn(x, variables['encoder/gamma_3'], variables['encoder/beta_3']) if 'in' in sides else x
        q = model_cases.quantize(y, bw, mean if mean is not None else numpy.zeros(128, dtype=numpy.float32))
        t = orc.gdn(q['shifted'], variables['decoder/gamma_4'], variables['decoder/beta_4'], inverse=True) if 'out' in sides else None
        chains.append({'y': y, 'shifted': q['shifted'], 'symbols': q['symbols'], 'nonzero_flags': q['nonzero_flags'],
                       'checks': q['checks'], 't': t})
    return tuple(chains)


def _assert_stage_equals(got, ref, sides, where=None):
    for key in ('y', 'shifted', 'symbols', 'nonzero_flags'):
        assert numpy.array_equal(_host(got[key]).reshape(ref[key].shape), ref[key]), (key, where)
    assert got['checks'].cpu().tolist() == ref['checks'], where
    if 'out' in sides:
        assert numpy.array_equal(_host(got['t']).reshape(ref['t'].shape), ref['t']), ('t', where)
    else:
        assert got['t'] is None


def _assert_stage_sees_a_transposition(got, wrong, sides):
    if 'in' in sides:
        assert _differs_at_half_or_more(_host(got['y']).reshape(wrong['y'].shape), wrong['y'])
    if 'out' in sides:
        assert _differs_at_half_or_more(_host(got['t']).reshape(wrong['t'].shape), wrong['t'])


@pytest.mark.parametrize('shape', [(3, 5, 7), (2, 32, 48)])           # (3, 5, 7): tiles that straddle images
@pytest.mark.parametrize('sides', ['in+out', 'in', 'out'])
@pytest.mark.parametrize('form', ['q', 'w', 'l'])
def test_latent_stage(dev, orc, shape, sides, form, launch_options):
    """EAE_HIP_LATENT = q: four waves per tile (quarter_denominator + squares_for_mfma); w: one wave per tile (wave_gdn_inplace);
    l: the block-cooperative LDS kernel (gdn_denominator<4>). With both normalisations, and with gdn_3 or inverse_gdn_4 alone: the
    two one-sided template instances that eae_hip_latent_stage also launches."""
    launch_options.delenv('EAE_HIP_LATENT_LDS', raising=False)
    launch_options.setenv('EAE_HIP_LATENT', form)
    v = _vars(30)
    (x, bw, mean) = _latent_inputs(shape)
    (ref, wrong) = _once(('stage', shape, sides), lambda: _stage_reference(orc, v, x, bw, mean, sides))
    gdn_in = (dev.pack_gamma(_cuda(v['encoder/gamma_3'])), _cuda(v['encoder/beta_3'])) if 'in' in sides else None
    igdn_out = (dev.pack_gamma(_cuda(v['decoder/gamma_4'])), _cuda(v['decoder/beta_4'])) if 'out' in sides else None
    got = dev.latent_stage(_cuda(x), _cuda(bw), _cuda(mean), gdn_in=gdn_in, igdn_out=igdn_out, want_y=True, want_shifted=True, want_flags=True)
    _assert_stage_equals(got, ref, sides)
    _assert_stage_sees_a_transposition(got, wrong, sides)
    dead = (ref['nonzero_flags'] == 0).sum(axis=1)
    assert dead.min() >= 1 and dead.max() < 64 and int(numpy.abs(ref['symbols']).max()) > 2     # the quantiser is exercised
    assert ref['checks'][0] == 0 and ref['checks'][1] > 0


@pytest.mark.parametrize('form', ['q', 'w', 'l'])
def test_latent_stage_without_a_map_mean(dev, orc, form, launch_options):
    launch_options.delenv('EAE_HIP_LATENT_LDS', raising=False)
    launch_options.setenv('EAE_HIP_LATENT', form)
    v = _vars(30)
    shape = (3, 5, 7)
    (x, bw, _) = _latent_inputs(shape)
    bw = bw*numpy.float32(0.1)          # finer: without a mean a symbol 0 is a latent 0, whose inverse_gdn_4 is 0 whatever gamma is
    (ref, wrong) = _once(('stage', shape, 'no mean'), lambda: _stage_reference(orc, v, x, bw, None, 'in+out'))
    got = dev.latent_stage(_cuda(x), _cuda(bw), None, gdn_in=(dev.pack_gamma(_cuda(v['encoder/gamma_3'])), _cuda(v['encoder/beta_3'])),
                           igdn_out=(dev.pack_gamma(_cuda(v['decoder/gamma_4'])), _cuda(v['decoder/beta_4'])), want_y=True,
                           want_shifted=True, want_flags=True)
    _assert_stage_equals(got, ref, 'in+out')
    _assert_stage_sees_a_transposition(got, wrong, 'in+out')


def test_latent_stage_as_the_product_library_launches_it(dev, orc):
    """On whatever library the package loads, in the form its launch picks: all three sides."""
    v = _vars(30)
    shape = (3, 5, 7)
    (x, bw, mean) = _latent_inputs(shape)
    for sides in ('in+out', 'in', 'out'):
        (ref, wrong) = _once(('stage', shape, sides), lambda: _stage_reference(orc, v, x, bw, mean, sides))
        gdn_in = (dev.pack_gamma(_cuda(v['encoder/gamma_3'])), _cuda(v['encoder/beta_3'])) if 'in' in sides else None
        igdn_out = (dev.pack_gamma(_cuda(v['decoder/gamma_4'])), _cuda(v['decoder/beta_4'])) if 'out' in sides else None
        got = dev.latent_stage(_cuda(x), _cuda(bw), _cuda(mean), gdn_in=gdn_in, igdn_out=igdn_out, want_y=True, want_shifted=True,
                               want_flags=True)
        _assert_stage_equals(got, ref, sides, sides)
        _assert_stage_sees_a_transposition(got, wrong, sides)


# ---- conv_3 with the latent stage behind it (conv_gemm.hip: eae_hip_conv5x5s2_latent; conv_gemm_split.hip: NORM_LATENT) --------
def _conv3_inputs(shape):
    rng = numpy.random.RandomState(62 + shape[1])
    x = rng.standard_normal(size=shape + (128,)).astype(numpy.float32)
    bw = rng.uniform(0.05, 0.5, size=128).astype(numpy.float32)
    mean = rng.normal(scale=0.05, size=128).astype(numpy.float32)
    return (x, bw, mean)


def _conv3_reference(orc, v, shape):
    (x, bw, mean) = _conv3_inputs(shape)
    raw = orc.conv2d_same(x, v['encoder/weights_3'], 2, v['encoder/biases_3'])
    return _stage_reference(orc, v, raw, bw, mean, 'in+out')


@pytest.mark.parametrize('shape,form', [((1, 6, 10), ''), ((1, 6, 10), 's'), ((2, 16, 24), 'u'), ((2, 16, 24), 's')])
def test_conv3_with_the_latent_stage_as_its_epilogue(dev, orc, shape, form, launch_options):
    """'' : as the launch decides (a small layer: the convolution, then the stage in place on its output); 'u' / 's': the fused
    kernel with whole tiles / with every tile cut. Against oracle conv_3 -> oracle gdn_3 -> numpy quantiser -> oracle
    inverse_gdn_4; the workspace is all zero afterwards."""
    launch_options.clear()
    v = _vars(61)
    (x, bw, mean) = _conv3_inputs(shape)
    (ref, wrong) = _once(('conv3', shape), lambda: _conv3_reference(orc, v, shape))
    if form:
        launch_options.setenv('EAE_HIP_GEMM', form)
    ws = dev.conv_workspace('cuda')
    got = dev.conv5x5s2_latent(_cuda(x), dev.pack_conv_weights(_cuda(v['encoder/weights_3'])), _cuda(v['encoder/biases_3']), _cuda(bw), _cuda(mean),
                               gdn_in=(dev.pack_gamma(_cuda(v['encoder/gamma_3'])), _cuda(v['encoder/beta_3'])),
                               igdn_out=(dev.pack_gamma(_cuda(v['decoder/gamma_4'])), _cuda(v['decoder/beta_4'])),
                               want_y=True, want_shifted=True, want_flags=True, workspace=ws)
    _assert_stage_equals(got, ref, 'in+out')
    _assert_handed_over(torch, dev, ws)
    _assert_stage_sees_a_transposition(got, wrong, 'in+out')
    assert int(numpy.abs(ref['symbols']).max()) > 2


def test_conv3_latent_refuses_one_normalisation_without_the_other(dev):
    """The one-sided stage is reachable through eae_hip_latent_stage only. eae_hip_conv5x5s2_latent refuses gdn_3 without
    inverse_gdn_4 and the reverse with EAE_HIP_BAD_ARGUMENT (-1: `device.HipError` for whoever checks the status as the package
    does) before it launches anything, and the Python wrapper refuses the same with ValueError before it reaches the library."""
    from autoencoder_based_image_compression_amd import _native
    v = _vars(61)
    (x, bw, mean) = _conv3_inputs((1, 6, 10))
    (x, bw, mean) = (_cuda(x), _cuda(bw), _cuda(mean))
    (w3, b3) = (dev.pack_conv_weights(_cuda(v['encoder/weights_3'])), _cuda(v['encoder/biases_3']))
    gdn_in = (dev.pack_gamma(_cuda(v['encoder/gamma_3'])), _cuda(v['encoder/beta_3']))
    igdn_out = (dev.pack_gamma(_cuda(v['decoder/gamma_4'])), _cuda(v['decoder/beta_4']))
    for sides in ({'gdn_in': gdn_in}, {'igdn_out': igdn_out}):
        with pytest.raises(ValueError):
            dev.conv5x5s2_latent(x, w3, b3, bw, mean, **sides)
    outputs = [torch.full((1, 3, 5, 128), 7., device='cuda') for _ in range(3)]
    symbols = torch.full((1, 128, 15), 7, dtype=torch.int16, device='cuda')
    checks = torch.zeros(3, dtype=torch.int32, device='cuda')
    ws = dev.conv_workspace('cuda')
    stream = torch.cuda.current_stream().cuda_stream
    for (g_in, b_in, g_out, b_out) in ((gdn_in[0], gdn_in[1], None, None), (None, None, igdn_out[0], igdn_out[1])):
        pointers = [None if t is None else t.data_ptr() for t in (g_in, b_in, mean, bw, g_out, b_out)]
        status = _native.hip().eae_hip_conv5x5s2_latent(x.data_ptr(), w3.data_ptr(), b3.data_ptr(), pointers[0], pointers[1], pointers[2],
                                                        pointers[3], pointers[4], pointers[5], outputs[0].data_ptr(), outputs[1].data_ptr(),
                                                        outputs[2].data_ptr(), symbols.data_ptr(), None, checks.data_ptr(), 1, 6, 10,
                                                        ws.data_ptr(), stream)
        assert status == -1
        with pytest.raises(dev.HipError):
            dev._check(status, 'eae_hip_conv5x5s2_latent')
    torch.cuda.synchronize()
    assert all(bool((t == 7.).all()) for t in outputs) and bool((symbols == 7).all())       # nothing was launched
    assert int(torch.count_nonzero(ws).item()) == 0 and int(torch.count_nonzero(checks).item()) == 0


# ---- whole models: the C ABI (model.hip), the pipeline objects, the codec and the containers ------------------------------------
def _model_case(orc, learned, shape):
    """(variables, images, oracle latents, quantised latents, oracle reconstruction float32 and uint8, the two with every gamma
    transposed) of one model and image set; bin width 0.05."""
    def make():
        v = _vars(20, learned, scale_weights_6=True)
        x = _image(numpy.random.RandomState(21), *shape)
        bw = numpy.full(128, 0.05, dtype=numpy.float32)
        mean = numpy.random.RandomState(22).normal(scale=0.05, size=128).astype(numpy.float32)
        y = orc.encoder(x.astype(numpy.float32)[..., None], v, learned)
        q = model_cases.quantize(y, bw, mean)
        # what a decoder gets back from the symbols (eae_hip_dequantize_maps): the same floats as the quantiser's own output
        dequantised = q['symbols'].transpose(0, 2, 1).reshape(y.shape).astype(numpy.float32)*bw + mean
        assert numpy.array_equal(dequantised, q['shifted'])
        rec = orc.decoder(dequantised, v, learned)[..., 0]
        swapped = _transposed(v)
        y_wrong = orc.encoder(x.astype(numpy.float32)[..., None], swapped, learned)
        rec_wrong = orc.decoder(q['shifted'], swapped, learned)[..., 0]
        return {'v': v, 'x': x, 'bw': bw, 'mean': mean, 'y': y, 'q': q, 'rec': rec, 'rec_u8': _bt601(rec), 'y_wrong': y_wrong,
                'symbols_wrong': model_cases.quantize(y_wrong, bw, mean)['symbols'], 'rec_wrong': rec_wrong, 'rec_u8_wrong': _bt601(rec_wrong)}
    return _once(('model', learned, shape), make)


def _bt601(rec):
    return numpy.round(rec.clip(min=16., max=235.)).astype(numpy.uint8)


@pytest.mark.parametrize('learned', [False, True])
@pytest.mark.parametrize('shape', [(1, 16, 16), (2, 64, 96)])
def test_model_encode_and_decode(dev, orc, learned, shape):
    """device.Model: eae_hip_model_create's upload and packing of the TensorFlow-layout variables, eae_hip_encode, eae_hip_decode."""
    c = _model_case(orc, learned, shape)
    model = dev.Model(c['v'], learned)
    try:
        y = _host(model.encode(_cuda(c['x'])))
        assert numpy.array_equal(y, c['y'])
        (f32, u8, sse) = model.decode(_cuda(c['q']['shifted']), want_f32=True, want_u8=True, ref_u8=_cuda(c['x']))
        model.check(wait=True)
        assert numpy.array_equal(_host(f32), c['rec'])
        assert numpy.array_equal(_host(u8), c['rec_u8'])
        expected = ((c['x'].astype(numpy.int64) - c['rec_u8'].astype(numpy.int64))**2).reshape(shape[0], -1).sum(axis=1)
        assert numpy.array_equal(_host(sse), expected)
        assert _differs_at_half_or_more(y, c['y_wrong']) and _differs_at_half_or_more(_host(f32), c['rec_wrong'])
    finally:
        model.close()


@pytest.mark.parametrize('learned', [False, True])
@pytest.mark.parametrize('tile', [None, (2, 3)])
def test_pipeline_encoder_and_decoder(orc, learned, tile):
    """pipeline.DeviceEncoder / DeviceDecoder, whole and through windows of 2 x 3 latents: latents, float reconstruction and uint8."""
    from autoencoder_based_image_compression_amd import pipeline
    c = _model_case(orc, learned, (2, 64, 96))
    encoder = pipeline.DeviceEncoder(c['v'], learned)
    decoder = pipeline.DeviceDecoder(c['v'], learned)
    y = _host(encoder(_cuda(c['x']), tile=tile))
    assert numpy.array_equal(y, c['y'])
    (f32, u8, _) = decoder(_cuda(c['q']['shifted']), want_float=True, want_uint8=True, tile=tile)
    encoder.check()
    decoder.check()
    assert numpy.array_equal(_host(f32), c['rec'])
    assert numpy.array_equal(_host(u8), c['rec_u8'])
    assert len(numpy.unique(c['rec_u8'])) > 4                       # the data exercises the cast, not only the clip floor
    assert _differs_at_half_or_more(y, c['y_wrong']) and _differs_at_half_or_more(_host(f32), c['rec_wrong'])
    assert numpy.mean(c['rec_u8'] != c['rec_u8_wrong']) > 0.1


def _probabilities():
    import os
    with numpy.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coder_golden.npz')) as g:
        return g['real_probabilities_1']


@pytest.mark.parametrize('learned', [False, True])
@pytest.mark.parametrize('graphs', [False, True])
def test_batch_codec(orc, tmp_path, learned, graphs):
    """codec.BatchCodec, launch by launch and replaying its captured graphs: bits, squared error and dead maps per image equal the
    image-by-image host path of tests/test_gpu_codec.py, and the reconstruction is the oracle's."""
    from autoencoder_based_image_compression_amd import codec
    c = _model_case(orc, learned, (2, 64, 96))
    probabilities = _probabilities()
    path = str(tmp_path/'binary_probabilities.npy')
    numpy.save(path, probabilities)
    (nb_bits, nb_deads, rec, _) = _once(('host path', learned),
                                        lambda: reference_shaped_path(c['v'], learned, c['x'], c['bw'], c['mean'], path, 67)[:3] + (None,))
    assert numpy.array_equal(rec, c['rec_u8'])
    sse = ((c['x'].astype(numpy.int64) - rec.astype(numpy.int64))**2).reshape(2, -1).sum(axis=1)
    bc = codec.BatchCodec(c['v'], learned, c['bw'], c['mean'], probabilities, 67, 2, 64, 96, keep_reconstruction=True, use_graphs=graphs)
    try:
        images = _cuda(c['x'])
        for _ in range(3 if graphs else 1):                            # with graphs: the capture, then replays
            ticket = bc.submit(images)
            r = ticket.result()
            assert numpy.array_equal(r['nb_bits'], nb_bits)
            assert numpy.array_equal(r['sse'], sse)
            assert numpy.array_equal(r['nb_deads'], nb_deads)
            assert numpy.array_equal(_host(ticket.reconstruction_uint8), c['rec_u8'])
    finally:
        bc.close()
    # uint8 pixels, part of them on the clip floor either way: a transposed gamma moves fewer than half, but far more than none
    assert nb_bits.min() > 0 and numpy.mean(c['rec_u8'] != c['rec_u8_wrong']) > 0.1


@pytest.mark.parametrize('learned', [False, True])
def test_container_round_trip(orc, learned):
    """container.encode_images -> decode_images: the symbols in the blob are the numpy quantiser's on the oracle's latents, and the
    decoded images are the oracle decoder's uint8 on the dequantised symbols."""
    from autoencoder_based_image_compression_amd import container, pipeline
    c = _model_case(orc, learned, (2, 64, 96))
    encoder = pipeline.DeviceEncoder(c['v'], learned)
    decoder = pipeline.DeviceDecoder(c['v'], learned)
    (blob, info) = container.encode_images(c['x'], encoder, c['bw'], c['mean'], _probabilities(), 67)
    (_, symbols) = container.decode_symbols(blob, decoder.device)
    symbols = _host(symbols).reshape(c['q']['symbols'].shape)
    assert numpy.array_equal(symbols, c['q']['symbols'])
    assert _differs_at_half_or_more(symbols, c['symbols_wrong'])
    decoded = container.decode_images(blob, decoder)
    assert numpy.array_equal(decoded, c['rec_u8'])
    assert numpy.mean(decoded != c['rec_u8_wrong']) > 0.1           # uint8 pixels: part of the image sits on the clip floor either way
    assert info['nb_bits'].shape == (2, 128) and int(info['nb_bits'].sum()) > 0
