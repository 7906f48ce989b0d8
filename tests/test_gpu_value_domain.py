"""GPU == oracle with tolerance 0, over VALUES: the transform kernels at float32's edges.

The rest of the suite holds that claim over shapes, launch forms, grids and buffers with inputs within a few binades of 1. Here
the inputs come from tests/value_domain_cases.py (the oracle is held against exact arithmetic out there on the CPU,
tests/test_oracle_value_domain.py):

A1 .. A6   accumulators that are subnormal, straddle the normal / subnormal line, meet a subnormal or an absorbing bias, overflow
           inside the chain, are already infinite while products beyond 2^128 keep arriving, or meet inf / NaN / -0 / 2^-149 /
           FLT_MAX in the input (two of them next to an image corner: a padded tap is a zero the kernel multiplies and the oracle
           skips; the weights stay finite, a padded 0 * inf is outside the contract);
G          the range guard of `gdn_tile` (csrc/hip/common.h) bound by bound: a tile wholly inside, ONE element exactly on a bound,
           ONE element one ulp beyond it -- in lane 0 and lane 63, the first and the last register, a lane outside the image, one
           wavefront of several --, and x = 0, subnormal x, subnormal / negative / infinite a, infinite x;
teeth      for every bound, far-side operands for which the short form gives other bits than the full one (the test build's
           eae_hip_debug_check_mid_forms): without one, a wrong bound could not be seen;
L          the luma cast and its squared error at 15.5, 16, 16.5, 234.5, 235, 235.5, +-inf and +-FLT_MAX.

Comparisons are exact: NaNs by position, everything else `==` (-0 == +0, as everywhere in the suite). Every case asserts from the
oracle's own intermediates that it populates the class it claims."""
import ctypes

import numpy
import pytest
import torch

import model_cases
import value_domain_cases as vd
from test_gpu_kernels import FORMS, _assert_handed_over, _select_form

pytestmark = pytest.mark.gpu

F32 = numpy.float32
C = 128


@pytest.fixture(autouse=True)
def guard():
    """Every test of this module runs on poisoned buffers between guard bands (tests/guarded.py): outputs hold NaN until a kernel
    writes them, inputs go between bands through `guard.upload`, and a byte written outside a tensor fails the test."""
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), 0xFF) as g:
        yield g


@pytest.fixture(scope='module')
def dev():
    from autoencoder_based_image_compression_amd import device
    return device


@pytest.fixture(scope='module')
def orc():
    from oracle import transforms
    return transforms


def _host(t):
    return t.cpu().numpy()


def _difference(got, ref):
    """'' when `got` equals `ref` (vd.same), else a line that says how: counts per kind of value and the first differing element."""
    got = numpy.asarray(got).reshape(numpy.asarray(ref).shape)
    if vd.same(got, ref):
        return ''
    with numpy.errstate(invalid='ignore'):
        differs = ~((got == ref) | (numpy.isnan(got) & numpy.isnan(ref)))
    first = tuple(int(i) for i in numpy.argwhere(differs)[0])
    sub = (numpy.abs(ref) > 0) & (numpy.abs(ref) < vd.TINY)
    return '{0} of {1} differ ({2} where the oracle is subnormal, {3} where it is not finite, {4} NaN only in the result); first at {5}: got {6!r} ' \
           '(0x{7:08X}), oracle {8!r} (0x{9:08X})'.format(int(differs.sum()), differs.size, int((differs & sub).sum()), int((differs & ~numpy.isfinite(ref)).sum()),
                                                         int((numpy.isnan(got) & ~numpy.isnan(ref)).sum()), first, got[first], vd.bits(got[first]),
                                                         ref[first], vd.bits(ref[first]))


def _report(failures):
    assert not failures, '{0} case(s) differ from the oracle:\n  '.format(len(failures)) + '\n  '.join(failures)


_cache = {}


def _once(key, make):
    """An oracle result computed once and shared by the forms of a parametrised test; nobody writes to it."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _optional(up, a):
    return up(a) if a is not None else None


# ---- A classes: conv5x5s2 / tconv5x5s2, with and without normalisation, every form -------------------------------------------------
CONV_SHAPES = [('conv', (1, 6, 10)), ('conv', (1, 16, 24)), ('tconv', (1, 3, 5)), ('tconv', (1, 8, 12))]


def _run_a_classes(guard, dev, kind, shape, workspace):
    up = guard.upload
    failures = []
    for cls in vd.A_CLASSES:
        case = vd.a_case(kind, cls, shape)
        vd.assert_population(cls, case['raw'])
        (pack, launch, norm) = ((dev.pack_conv_weights, dev.conv5x5s2, dev.NORM_GDN) if kind == 'conv'
                                else (dev.pack_tconv_weights, dev.tconv5x5s2, dev.NORM_IGDN))
        (x, wp, bias) = (up(case['x']), pack(up(case['w'])), _optional(up, case['bias']))
        (gp, beta) = (dev.pack_gamma(up(case['gamma'])), up(case['beta']))
        for (normalised, ref) in ((False, case['raw']), (True, case['normed'])):
            ws = dev.conv_workspace('cuda') if workspace else None
            got = _host(launch(x, wp, bias, norm if normalised else dev.NORM_NONE, gp if normalised else None, beta if normalised else None,
                               workspace=ws))
            _assert_handed_over(torch, dev, ws)
            how = _difference(got, ref)
            if how:
                failures.append('{0} {1} {2} {3}: {4}'.format(kind, shape, cls, 'normalised' if normalised else 'plain', how))
            if cls == 'A5' and not normalised:
                assert not numpy.isnan(got).any()          # a product rounded before it is added would show here
    return failures


@pytest.mark.parametrize('form,tile', FORMS)
@pytest.mark.parametrize('kind,shape', CONV_SHAPES)
def test_a_classes_in_every_form(guard, dev, kind, shape, form, tile, launch_options):
    """The smallest shapes with a ragged wave tile ((1, 6, 10) -> 15 positions, (1, 3, 5) -> 60) and with whole ones; the forms that
    cut tiles ('cut*', 'one*') run through eae_hip_conv5x5s2_ws / eae_hip_tconv5x5s2_ws."""
    _select_form(launch_options, form, tile)
    _report(_run_a_classes(guard, dev, kind, shape, form.startswith(('cut', 'one'))))


@pytest.mark.parametrize('with_workspace', [False, True])
@pytest.mark.parametrize('kind,shape', CONV_SHAPES)
def test_a_classes_as_the_library_launches_them(guard, dev, kind, shape, with_workspace):
    """On whatever library the package loads (the product one unless EAE_HIP_LIB says otherwise), in the form its launch picks: the
    plain entry points and the ones with a workspace."""
    _report(_run_a_classes(guard, dev, kind, shape, with_workspace))


# ---- the latent stage: oracle gdn_3 -> numpy quantiser -> oracle inverse_gdn_4 ------------------------------------------------------
def _stage_reference(orc, raw, bw, mean, gdn_in, igdn_out):
    """raw [n, h, w, 128] through the stage; each normalisation a (gamma, beta) pair. Where the rounded quotient is not a finite int16
    the symbol is whatever the cast gives (include/eae_hip.h: checks[0] counts them): `symbol_defined` leaves those out."""
    with numpy.errstate(all='ignore'):
        y = orc.gdn(raw, *gdn_in)
        q = model_cases.quantize(y, bw, mean)
        t = orc.gdn(q['shifted'], *igdn_out, inverse=True)
        tiled = numpy.broadcast_to(bw.reshape(1, 1, 1, C), y.shape)
        rounded = numpy.round(q['cq']/tiled)
        defined = numpy.abs(rounded) < F32(32768.)
    defined = numpy.ascontiguousarray(defined.reshape(y.shape[0], -1, C).transpose(0, 2, 1))
    return {'y': y, 'shifted': q['shifted'], 't': t, 'symbols': q['symbols'], 'symbol_defined': defined, 'nonzero_flags': q['nonzero_flags'],
            'checks': q['checks']}


def _stage_differences(got, ref, tag):
    failures = []
    for key in ('y', 'shifted', 't'):
        how = _difference(_host(got[key]), ref[key])
        if how:
            failures.append('{0} {1}: {2}'.format(tag, key, how))
    sym = _host(got['symbols']).reshape(ref['symbols'].shape)
    if not numpy.array_equal(sym[ref['symbol_defined']], ref['symbols'][ref['symbol_defined']]):
        failures.append('{0} symbols: {1} differ'.format(tag, int((sym != ref['symbols'])[ref['symbol_defined']].sum())))
    if not numpy.array_equal(_host(got['nonzero_flags']), ref['nonzero_flags']):
        failures.append('{0} nonzero_flags differ'.format(tag))
    if got['checks'].cpu().tolist() != ref['checks']:
        failures.append('{0} checks: got {1}, oracle {2}'.format(tag, got['checks'].cpu().tolist(), ref['checks']))
    return failures


def _stage_vectors():
    rng = numpy.random.RandomState(62)
    return (rng.uniform(0.05, 0.5, size=C).astype(F32), rng.normal(scale=0.05, size=C).astype(F32))


def _latent_forms(launch_options, gemm, stage):
    launch_options.clear()
    if gemm:
        launch_options.setenv('EAE_HIP_GEMM', gemm)
    launch_options.setenv('EAE_HIP_LATENT', stage)


@pytest.mark.parametrize('stage', ['q', 'w', 'l'])
@pytest.mark.parametrize('gemm', ['', 'u', 's'])
def test_a_classes_conv3_with_the_latent_stage(guard, dev, orc, gemm, stage, launch_options):
    """eae_hip_conv5x5s2_latent: as the launch decides (small layers: the convolution, then the stage in place, in each of its three
    forms), with whole tiles ('u') and with every tile cut ('s': the stage fused behind the split conv GEMM)."""
    _latent_forms(launch_options, gemm, stage)
    up = guard.upload
    (bw, mean) = _stage_vectors()
    (gamma, beta) = vd.norm_parameters()
    (gamma_out, beta_out) = vd.norm_parameters(6)
    failures = []
    for shape in ((1, 6, 10), (1, 16, 24)):
        for cls in vd.A_CLASSES:
            case = vd.a_case('conv', cls, shape)
            ref = _once(('a latent', cls, shape), lambda: _stage_reference(orc, case['raw'], bw, mean, (gamma, beta), (gamma_out, beta_out)))
            ws = dev.conv_workspace('cuda')
            got = dev.conv5x5s2_latent(up(case['x']), dev.pack_conv_weights(up(case['w'])), _optional(up, case['bias']), up(bw), up(mean),
                                       gdn_in=(dev.pack_gamma(up(gamma)), up(beta)), igdn_out=(dev.pack_gamma(up(gamma_out)), up(beta_out)),
                                       want_y=True, want_shifted=True, want_flags=True, workspace=ws)
            _assert_handed_over(torch, dev, ws)
            failures += _stage_differences(got, ref, '{0} {1}'.format(cls, shape))
    _report(failures)


# ---- A classes: conv_1 on pixels, transpose_conv_3 -----------------------------------------------------------------------------------
@pytest.mark.parametrize('image_name', vd.IMAGES_U8)
@pytest.mark.parametrize('cls', vd.A_CLASSES_U8)
def test_a_classes_conv9x9s4_u8(guard, dev, cls, image_name):
    """(1, 36, 100): the last tile of a row is ragged. All 0 (every product a zero), all 255, a 0 / 255 checkerboard, the usual image."""
    up = guard.upload
    case = vd.a_case_conv1(cls, image_name)
    if image_name == 'zeros':                # every product is a zero: the output is the bias
        assert numpy.all(case['raw'] == (0. if case['bias'] is None else case['bias']))
    elif cls == 'A1' and image_name != 'usual':
        # 81 products of ONE pixel value (or of 0 and 255) with weights of +-2^-148: about 3 % of the sums cancel to exactly 0 on the
        # 2^-149 grid; the rest is subnormal
        s = vd.shares(case['raw'])
        assert s['subnormal'] >= 0.9 and s['subnormal'] + s['zero'] == 1.0, s
    else:
        vd.assert_population(cls, case['raw'])
    (x, wp, bias) = (up(case['x']), dev.pack_conv9x9s4_weights(up(case['w'])), _optional(up, case['bias']))
    failures = []
    for (normalised, ref) in ((False, case['raw']), (True, case['normed'])):
        got = _host(dev.conv9x9s4_u8(x, wp, bias, dev.pack_gamma(up(case['gamma'])) if normalised else None, up(case['beta']) if normalised else None))
        how = _difference(got, ref)
        if how:
            failures.append('{0} {1} {2}: {3}'.format(cls, image_name, 'normalised' if normalised else 'plain', how))
    _report(failures)


@pytest.mark.parametrize('cls', ['A1', 'A2', 'A4', 'A5', 'A6'])
def test_a_classes_tconv9x9s4_luma(guard, dev, cls):
    """float32 output only (the cast has its own test below). No bias in this layer: A3 does not exist here.

    A6 is where the contract ends ("Value domain"): this kernel multiplies every input site of an output's 3 x 3
    site neighbourhood, with a ZERO WEIGHT where the tap does not exist, and 0 * inf = NaN; the oracle skips those taps. Measured on
    an MI355X: 66 of the 560 outputs are NaN where the oracle is finite, exactly the ones `vd.tconv3_structural_nan` names (three
    non-finite inputs, each spoiling its 12 x 12 block instead of the 9 x 9 of its taps). Everything else equals the oracle, and
    that model is asserted so that a change is noticed."""
    up = guard.upload
    case = vd.a_case_tconv3(cls)
    vd.assert_population(cls, case['raw'])
    ref = case['raw']
    if cls == 'A6':
        beyond_the_taps = vd.tconv3_structural_nan(case['x'], ref.shape)
        assert int((beyond_the_taps & ~numpy.isnan(ref)).sum()) == 66
        ref = numpy.where(beyond_the_taps, F32(numpy.nan), ref)
    else:
        assert numpy.isfinite(case['x']).all()
    (f32, _, _) = dev.tconv9x9s4_luma(up(case['x']), dev.pack_tconv9x9s4_weights(up(case['w'])), want_f32=True, want_u8=False)
    _report([how for how in [_difference(_host(f32), ref)] if how])


# ---- G: the guard of gdn_tile, bound by bound ------------------------------------------------------------------------------------------
def _g_reference(orc, raw, gamma, beta, inverse, expectation, name):
    with numpy.errstate(all='ignore'):
        a = orc.gdn_denominators(raw, gamma, beta)
        assert vd.g_expectation_holds(a.reshape(-1, C), raw.reshape(-1, C), inverse, expectation), name
        return orc.gdn(raw, gamma, beta, inverse=inverse)


# tconv5x5s2, (1, 8, 12) in, 24 outputs per row: the element of input (p, q) = row 12 p + q lands on output (2p, 2q) -- lane 0, lane 22 (the
# last even position of the first tile's first row), position 48 = lane 16 of the second tile -- or, with the ODD weights, on output
# (2p + 1, 2q + 1): input (0, 3) -> output (1, 7) = position 31, lane 63's (and lane 31's) position of the first tile.
TCONV_PLACES = [('lane0_first', 0, 0), ('lane0_last', 0, 123), ('lane22_first', 11, 4), ('lane22_last', 11, 127), ('second_tile_only', 12, 77)]
TCONV_PLACES_ODD = [('lane63_first', 3, 4), ('lane63_last', 3, 127)]
TCONV_OTHERS = F32(2.)**30          # what the three outputs beside the element's are multiplied by: 2^-70 -> 2^-40, whose square is inside


def _g_conv_cases(orc, kind):
    """[(name, input, weights, bias, gamma, beta, reference)] on the shapes with whole tiles only. One-tap identity weights: the
    un-normalised output IS the chosen values (asserted from the oracle's convolution), the biases are null.
    'conv': (1, 16, 24) in, 96 positions out = the rows of `vd.g_cases`. 'tconv': (1, 8, 12) in, 384 out; input (p, q) goes to the
    output (2p, 2q) as it is and to its three neighbours (2p + 1, 2q), ... times 2^30, so that ONE output is on or beyond the bound;
    a second set of weights leaves (2p + 1, 2q + 1) as it is instead, which reaches lane 63 (TCONV_PLACES_ODD)."""
    def make():
        cases = []
        inverse = kind == 'tconv'
        if kind == 'conv':
            w = vd.identity_conv_weights()
            g = vd.g_cases(96, False)
        else:
            (w, w_odd) = (vd.identity_tconv_weights(), vd.identity_tconv_weights())
            for (u, v) in ((1, 1), (1, 2), (2, 1), (2, 2)):
                (w if (u, v) != (1, 1) else w_odd)[u, v] *= TCONV_OTHERS
                if (u, v) in ((1, 2), (2, 1)):
                    w_odd[u, v] *= TCONV_OTHERS
            g = vd.g_cases(96, True, TCONV_PLACES)
            odd = [case for case in vd.g_cases(96, True, TCONV_PLACES_ODD) if case[0].endswith(('lane63_first', 'lane63_last'))]
            g = [case + (w,) for case in g] + [case + (w_odd,) for case in odd]
        for case in g:
            (name, values, gamma, beta, expectation) = case[:5]
            if kind == 'tconv':
                w = case[5]
                (same_phase, other_phase) = (slice(0, None, 2), slice(1, None, 2)) if w is not w_odd else (slice(1, None, 2), slice(0, None, 2))
            x = vd.identity_conv_input((1, 8, 12), values) if kind == 'conv' else values.reshape(1, 8, 12, C)
            with numpy.errstate(all='ignore'):
                raw = (orc.conv2d_same if kind == 'conv' else orc.conv2d_transpose_same)(x, w, 2, None)
            if not numpy.isfinite(values).all():
                pass                       # an infinite input meets the zero weights of its neighbours' taps: NaN around it, on both sides
            elif kind == 'conv':
                assert vd.same(raw.reshape(-1, C), values), name
            else:
                with numpy.errstate(over='ignore'):
                    assert vd.same(raw[0, same_phase, same_phase].reshape(-1, C), values), name
                    assert vd.same(raw[0, other_phase, other_phase].reshape(-1, C), values*TCONV_OTHERS), name
            cases.append((name, x, w, None, gamma, beta, _g_reference(orc, raw, gamma, beta, inverse, expectation, name)))
        return cases
    return _once(('g conv', kind), make)


def _g_ragged_cases(orc, kind):
    """The ragged shapes ((1, 6, 10) -> 15 positions, (1, 3, 5) -> 60): a lane outside the image takes part in the guard's ballot
    with acc = bias. Null and zero biases put |x| = 0 there (below 2^-60: what a real model with the reference's zero biases does);
    a bias of 2^-60 puts them exactly on the bound, its predecessor one ulp beyond; with beta = pred(2^-40) (pred(2^-96) for IGDN)
    in a channel whose gamma[c][c] = 1, only the lanes outside have a = beta beyond the bound. Inside, x + bias == x."""
    def make():
        cases = []
        inverse = kind == 'tconv'
        positions = (1, 3, 5)
        values = vd.base_x(15, 7)
        zero = numpy.zeros((C, C), dtype=F32)
        one = numpy.ones(C, dtype=F32)
        diagonal = zero.copy()
        diagonal[33, 33] = 1.
        bound = vd.two(-96) if inverse else vd.two(-40)

        def beta_at(v):
            b = one.copy()
            b[33] = v
            return b
        table = [('null_bias', None, zero, one), ('zero_bias', numpy.zeros(C, dtype=F32), zero, one),
                 ('bias_inside', numpy.full(C, 0.125, dtype=F32), zero, one),
                 ('bias_on_x_min', numpy.full(C, vd.two(-60), dtype=F32), zero, one),
                 ('bias_beyond_x_min', numpy.full(C, vd.below(vd.two(-60)), dtype=F32), zero, one),
                 ('outside_a_on_bound', numpy.full(C, vd.two(-60), dtype=F32), diagonal, beta_at(bound)),
                 ('outside_a_beyond_bound', numpy.full(C, vd.two(-60), dtype=F32), diagonal, beta_at(vd.below(bound)))]
        if kind == 'conv':
            (x, w) = (vd.identity_conv_input(positions, values), vd.identity_conv_weights())
        else:
            (x, w) = (values.reshape(positions + (C,)), vd.identity_tconv_weights())
        for (name, bias, gamma, beta) in table:
            with numpy.errstate(all='ignore'):
                raw = (orc.conv2d_same if kind == 'conv' else orc.conv2d_transpose_same)(x, w, 2, bias)
                a = orc.gdn_denominators(raw, gamma, beta)
            if name != 'bias_inside':
                expected = values if kind == 'conv' else numpy.repeat(numpy.repeat(values.reshape(3, 5, C), 2, axis=0), 2, axis=1).reshape(-1, C)
                assert vd.same(raw.reshape(-1, C), expected), name                                  # x + bias == x inside the image
            assert vd.g_expectation_holds(a.reshape(-1, C), raw.reshape(-1, C), inverse, 'inside'), name    # all that leaves the range is outside the image
            with numpy.errstate(all='ignore'):
                cases.append((name, x, w, bias, gamma, beta, orc.gdn(raw, gamma, beta, inverse=inverse)))
        return cases
    return _once(('g ragged', kind), make)


def _run_g_conv(guard, dev, kind, cases, workspace):
    up = guard.upload
    (pack, launch, norm) = ((dev.pack_conv_weights, dev.conv5x5s2, dev.NORM_GDN) if kind == 'conv'
                            else (dev.pack_tconv_weights, dev.tconv5x5s2, dev.NORM_IGDN))
    packed = {}
    failures = []
    for (name, x, w, bias, gamma, beta, ref) in cases:
        if id(w) not in packed:
            packed[id(w)] = pack(up(w))
        wp = packed[id(w)]
        ws = dev.conv_workspace('cuda') if workspace else None
        got = _host(launch(up(x), wp, _optional(up, bias), norm, dev.pack_gamma(up(gamma)), up(beta), workspace=ws))
        _assert_handed_over(torch, dev, ws)
        how = _difference(got, ref)
        if how:
            failures.append('{0} {1}: {2}'.format(kind, name, how))
    return failures


@pytest.mark.parametrize('form,tile', FORMS)
@pytest.mark.parametrize('kind', ['conv', 'tconv'])
def test_guard_bounds_in_every_form(guard, dev, orc, kind, form, tile, launch_options):
    """conv5x5s2 + GDN (four bounds) and tconv5x5s2 + IGDN (one), every form: 'lds' normalises with `gdn_apply` (no short forms) and
    must agree all the same."""
    _select_form(launch_options, form, tile)
    workspace = form.startswith(('cut', 'one'))
    _report(_run_g_conv(guard, dev, kind, _g_conv_cases(orc, kind), workspace) + _run_g_conv(guard, dev, kind, _g_ragged_cases(orc, kind), workspace))


@pytest.mark.parametrize('kind', ['conv', 'tconv'])
def test_guard_bounds_as_the_library_launches_them(guard, dev, orc, kind):
    _report(_run_g_conv(guard, dev, kind, _g_conv_cases(orc, kind), False) + _run_g_conv(guard, dev, kind, _g_ragged_cases(orc, kind), True))


@pytest.mark.parametrize('rows', [1, 127, 1000])
@pytest.mark.parametrize('inverse', [False, True])
def test_guard_bounds_gdn(guard, dev, orc, rows, inverse):
    """eae_hip_gdn normalises with `gdn_apply` (hipcc's full sqrtf and `/`): the same cases, x given directly."""
    up = guard.upload
    failures = []
    for (name, x, gamma, beta, expectation) in vd.g_cases(rows, inverse):
        ref = _g_reference(orc, x, gamma, beta, inverse, expectation, name)
        how = _difference(_host(dev.gdn(up(x), dev.pack_gamma(up(gamma)), up(beta), inverse=inverse)), ref)
        if how:
            failures.append('{0}: {1}'.format(name, how))
    _report(failures)


# conv_1: pixels in. With a one-tap filter w and a bias b, the un-normalised output of channel c is b[c] where the pixel is 0 -- and
# in the lanes outside the image -- and w[c] + b[c] (one rounding, exact here) where it is 1: ONE pixel is 1.
# Where it is: conv_1's block is 8 x 16 outputs and each of its waves owns 2 x 16 of them (csrc/hip/conv1.hip), so on the 9 x 25
# outputs of this image the places are named by output (row, column) and what they are to the kernel: the first and the last position
# of the first wave's tile, one in its middle, one in the second wave of the same block, one in the ragged block to the right and the
# last output of all (the ragged block at the bottom right, one row and nine columns of it inside the image).
CONV1_PLACES = [('r0c0_ch0', 0, 0), ('r0c0_ch123', 0, 123), ('r1c15_ch4', 40, 4), ('r1c15_ch127', 40, 127), ('r1c6_ch77', 31, 77),
                ('r2c3_ch9', 53, 9), ('r0c20_ch77', 20, 77), ('r8c24_ch64', 224, 64)]


def _g_conv1_cases(orc):
    def make():
        (h, w) = (9, 25)
        cases = []
        two = vd.two
        # bound -> (b, w on the bound, w one ulp beyond it, gamma[c][c] on, gamma[c][c] beyond)
        table = {'x_min': (F32(1.5)*two(-60), -two(-61), -vd.above(two(-61)), None, None),
                 'x_max': (two(59) + two(37), two(59) - two(37), two(59), None, None),
                 'a_min': (F32(1.5)*two(-20), -two(-21), -two(-21), F32(1.), vd.below(1.)),
                 'a_max': (two(39), two(39), two(39), F32(1.), vd.above(1.))}

        def build(name, place, ch, b_c, w_c, gamma_cc, expectation, bias=True, beta_c=None, pixel=1):
            image = numpy.zeros((1, 4*h, 4*w), dtype=numpy.uint8)
            if place is not None:
                image[0, 4*(place//w) + 2, 4*(place % w) + 2] = pixel
            weights = numpy.zeros((9, 9, 1, C), dtype=F32)
            weights[4, 4, 0, :] = 1.
            b = numpy.ones(C, dtype=F32)
            (gamma, beta) = (numpy.zeros((C, C), dtype=F32), numpy.ones(C, dtype=F32))
            if ch is not None:
                (weights[4, 4, 0, ch], b[ch]) = (w_c, b_c)
                if gamma_cc is not None:
                    (gamma[ch, ch], beta[ch]) = (gamma_cc, 0.)
                if beta_c is not None:
                    beta[ch] = beta_c
            with numpy.errstate(all='ignore'):
                raw = orc.conv2d_same(image.astype(F32)[..., None], weights, 4, b if bias else None)
            cases.append((name, image, weights, b if bias else None, gamma, beta, _g_reference(orc, raw, gamma, beta, False, expectation, name)))
            return raw

        build('inside', 30, None, None, None, None, 'inside')
        for (bound, (b_c, w_on, w_beyond, g_on, g_beyond)) in table.items():
            for (place_name, row, ch) in CONV1_PLACES:
                raw = build('{0}_on_{1}'.format(bound, place_name), row, ch, b_c, w_on, g_on, 'inside')
                value = vd.BOUNDS[bound][0]
                if g_on is None:
                    assert abs(raw.reshape(-1, C)[row, ch]) == value, (bound, place_name)
                build('{0}_beyond_{1}'.format(bound, place_name), row, ch, b_c, w_beyond, g_beyond, 'beyond')
        # ONE element with teeth at every place (as vd.PLACED_TEETH): x = 2^120 + 1 over sqrt(beta) = 2^-20 overflows (the rest of the channel
        # is 1 over 2^-20); a = (1 + 2^60)^2 * 2^10 = inf under an x on its bound (the rest: a = 2^10). A tiny a under an x in range would
        # need w + b = 2^-60 beside a b whose square stays above 2^-20: not to be had with one tap, so a_min's teeth stay with the extras.
        for (place_name, row, ch) in CONV1_PLACES:
            build('teeth_x_max_' + place_name, row, ch, F32(1.), two(120), None, None, beta_c=two(-40))
            build('teeth_a_max_' + place_name, row, ch, F32(1.), two(60), two(10), 'beyond')
        build('null_bias', 30, None, None, None, None, None, bias=False)                    # the lanes outside the image hold |x| = 0
        build('x_zero', 30, 50, F32(1.), F32(-1.), None, None)
        build('x_inf', 30, 50, F32(1.), two(121), None, None, pixel=255)                     # 255 * 2^121 overflows: the only way to an infinite x here
        build('x_subnormal', 30, 50, two(-140), two(-140), None, None)
        (x_teeth, a_teeth) = vd.FAR_SIDE_TEETH['x_min_subnormal_numerator']                  # a pair div_mid gets wrong; the rest of the channel holds 0
        build('x_min_subnormal_numerator', 30, 50, F32(0.), x_teeth, None, None, beta_c=a_teeth)
        build('a_inf', 30, 50, two(39), two(100), F32(1.), None)
        build('a_subnormal', 30, 50, two(-70), two(-70), F32(1.), None)
        build('a_negative', 30, 50, F32(1.), F32(1.), None, None, beta_c=F32(-8.))
        return cases
    return _once('g conv1', make)


def test_guard_bounds_conv9x9s4_u8(guard, dev, orc):
    """(1, 36, 100): 25 positions per row, so every row ends in a ragged tile whose outside lanes hold the bias."""
    up = guard.upload
    failures = []
    for (name, image, weights, bias, gamma, beta, ref) in _g_conv1_cases(orc):
        got = _host(dev.conv9x9s4_u8(up(image), dev.pack_conv9x9s4_weights(up(weights)), _optional(up, bias), dev.pack_gamma(up(gamma)), up(beta)))
        how = _difference(got, ref)
        if how:
            failures.append('{0}: {1}'.format(name, how))
    _report(failures)


# ---- G through the latent stage: n = 3, hw = 33 ------------------------------------------------------------------------------------
def _g_latent_cases(orc):
    """[(name, x [3, 3, 11, 128], bw, mean, (gamma_in, beta_in), (gamma_out, beta_out), reference)]. GDN in: the cases of `vd.g_cases`
    with inverse_gdn_4 the identity (gamma = 0, beta = 1). IGDN out (`wave_gdn_inplace<true>`, the second guard of the stage): gdn_3 is
    the identity, the element's channel is quantised with a bin width of 2^-48 and holds 1000 * 2^-48 everywhere but in ONE element,
    2^-48: a = shifted^2 gamma[c][c] is 2^-96 there (on the bound) or one ulp below it (gamma[c][c] = 1 - ulp); and, since `sqrt_mid`
    still gives sqrtf's bits one ulp out, the same with a = 2^-140 in ONE element, where it does not. Each at every place of
    `vd.placements`: lane 0 and lane 63, first and last register, the second tile alone."""
    def make():
        rows = 99
        zero = numpy.zeros((C, C), dtype=F32)
        one = numpy.ones(C, dtype=F32)
        bw = numpy.full(C, 0.25, dtype=F32)
        mean = numpy.zeros(C, dtype=F32)
        cases = []
        for (name, x, gamma, beta, expectation) in vd.g_cases(rows, False):
            with numpy.errstate(all='ignore'):
                assert vd.g_expectation_holds(orc.gdn_denominators(x, gamma, beta), x, False, expectation), name
            cases.append(('in_' + name, x, bw, mean, (gamma, beta), (zero, one)))
        x0 = vd.base_x(rows, 40 + rows)

        def out_case(name, row, ch, unit, others, element, gamma_cc, expectation):
            x = x0.copy()
            x[:, ch] = F32(others)*unit
            x[row, ch] = F32(element)*unit
            (bw_c, gamma_out, beta_out) = (bw.copy(), zero.copy(), one.copy())
            (bw_c[ch], gamma_out[ch, ch], beta_out[ch]) = (unit, gamma_cc, 0.)
            with numpy.errstate(all='ignore'):
                shifted = model_cases.quantize(x.reshape(3, 3, 11, C), bw_c, mean)['shifted'].reshape(-1, C)
            assert numpy.array_equal(shifted[:, ch], x[:, ch]), name      # the quantiser hands the multiples of the bin width through
            assert vd.g_expectation_holds(orc.gdn_denominators(shifted, gamma_out, beta_out), shifted, True, expectation), name
            cases.append((name, x, bw_c, mean, (zero, one), (gamma_out, beta_out)))

        out_case('out_inside', 40, 77, vd.two(-48), 1000., 1000., 1., 'inside')
        for (place, row, ch) in vd.placements(rows):
            out_case('out_on_the_bound_' + place, row, ch, vd.two(-48), 1000., 1., 1., 'inside')
            out_case('out_beyond_the_bound_' + place, row, ch, vd.two(-48), 1000., 1., vd.below(1.), 'beyond')
            # with teeth: the bin width is 2^-70, ONE element holds symbol 1 (a = 2^-140, vd.PLACED_TEETH['teeth_a_min_igdn']) and the rest
            # of the channel 2^30 bin widths (a = 2^-80; symbols beyond int16, which checks[0] counts and `symbol_defined` leaves out)
            out_case('out_teeth_' + place, row, ch, vd.two(-70), 2.**30, 1., 1., 'beyond')
        return [case + (_stage_reference(orc, case[1].reshape(3, 3, 11, C), *case[2:]),) for case in cases]
    return _once('g latent', make)


@pytest.mark.parametrize('stage', ['q', 'w', 'l'])
def test_guard_bounds_latent_stage(guard, dev, orc, stage, launch_options):
    """EAE_HIP_LATENT = w runs `wave_gdn_inplace` (the guard, twice per tile); q normalises quarter tiles with the full forms and l
    with `gdn_apply`: all three against the same reference. 99 rows: three whole tiles and a ragged one whose outside lanes hold 0."""
    _latent_forms(launch_options, '', stage)
    up = guard.upload
    failures = []
    for (name, x, bw, mean, gdn_in, igdn_out, ref) in _g_latent_cases(orc):
        got = dev.latent_stage(up(x.reshape(3, 3, 11, C)), up(bw), up(mean), gdn_in=(dev.pack_gamma(up(gdn_in[0])), up(gdn_in[1])),
                               igdn_out=(dev.pack_gamma(up(igdn_out[0])), up(igdn_out[1])), want_y=True, want_shifted=True, want_flags=True)
        failures += _stage_differences(got, ref, name)
    _report(failures)


@pytest.mark.parametrize('stage', ['q', 'w', 'l'])
@pytest.mark.parametrize('gemm', ['', 'u', 's'])
def test_guard_bounds_conv3_with_the_latent_stage(guard, dev, orc, gemm, stage, launch_options):
    """The same cases as the output of conv_3 (one-tap identity weights, (3, 6, 22) in): the stage in place behind the convolution,
    and fused behind the split conv GEMM ('u', 's')."""
    _latent_forms(launch_options, gemm, stage)
    up = guard.upload
    wp = dev.pack_conv_weights(up(vd.identity_conv_weights()))
    failures = []
    for (name, x, bw, mean, gdn_in, igdn_out, ref) in _g_latent_cases(orc):
        ws = dev.conv_workspace('cuda')
        got = dev.conv5x5s2_latent(up(vd.identity_conv_input((3, 3, 11), x)), wp, None, up(bw), up(mean),
                                   gdn_in=(dev.pack_gamma(up(gdn_in[0])), up(gdn_in[1])), igdn_out=(dev.pack_gamma(up(igdn_out[0])), up(igdn_out[1])),
                                   want_y=True, want_shifted=True, want_flags=True, workspace=ws)
        _assert_handed_over(torch, dev, ws)
        if not numpy.isfinite(x).all():     # an infinite input meets the zero weights of its neighbours' taps: the reference goes through conv_3
            with numpy.errstate(all='ignore'):
                ref = _once(('g latent conv', name), lambda: _stage_reference(
                    orc, orc.conv2d_same(vd.identity_conv_input((3, 3, 11), x), vd.identity_conv_weights(), 2, None), bw, mean, gdn_in, igdn_out))
        failures += _stage_differences(got, ref, name)
    _report(failures)


def test_the_identity_convolution_of_the_latent_cases(orc):
    """What test_guard_bounds_conv3_with_the_latent_stage relies on: the oracle's conv_3 of the one-tap input IS the case's x."""
    for (name, x, _, _, _, _, _) in _g_latent_cases(orc)[::7]:
        if not numpy.isfinite(x).all():
            continue
        with numpy.errstate(all='ignore'):
            raw = orc.conv2d_same(vd.identity_conv_input((3, 3, 11), x), vd.identity_conv_weights(), 2, None)
        assert vd.same(raw.reshape(-1, C), x), name


# ---- teeth: what the short forms do on the far side of each bound ---------------------------------------------------------------------
def _differs(mode, first):
    from autoencoder_based_image_compression_amd import _native
    out = torch.zeros(2, dtype=torch.int64, device='cuda')
    assert _native.hip().eae_hip_debug_check_mid_forms(mode, first, 1, 0, ctypes.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    return int(out[0].item()) == 1


def _sqrt_differs(a):
    return _differs(0, vd.bits(a))


def _div_differs(x, s):
    return _differs(2, (vd.bits(x) << 32) | vd.bits(s))


def _s(a):
    return numpy.sqrt(F32(a))


def _pair(name):
    """(x, s) of a G case that carries a far-side operand (vd.FAR_SIDE_TEETH)."""
    (x, a) = vd.FAR_SIDE_TEETH[name]
    return (x, _s(a))


# bound -> far-side operands: (what it is, x, s) for div_mid(x, s) against x / s, s = sqrtf(a); for the IGDN bound (what, a) for
# sqrt_mid(a) against sqrtf(a). The first entries are one ulp beyond the bound with the other operand at each end of ITS range -- what
# the 'beyond' cases above put into one element; the rest lie further out and are what the extras above hold.
FAR_SIDE = {
    'a_min': [('a one ulp below 2^-40, x = 2^-60', vd.two(-60), _s(vd.below(vd.two(-40)))), ('a one ulp below, x = 1', F32(1.), _s(vd.below(vd.two(-40)))),
              ('a one ulp below, x = 2^60', vd.two(60), _s(vd.below(vd.two(-40)))),
              ('a = 2^-140 (subnormal), x = 1', F32(1.), _s(vd.two(-140))),
              ('a = 2^-140, x = 2^60: the quotient overflows (G case a_min_quotient_overflows)',) + _pair('a_min_quotient_overflows')],
    'a_max': [('a one ulp above 2^80, x = 2^-60', vd.two(-60), _s(vd.above(vd.two(80)))), ('a one ulp above, x = 1', F32(1.), _s(vd.above(vd.two(80)))),
              ('a one ulp above, x = 2^60', vd.two(60), _s(vd.above(vd.two(80)))),
              ('a = FLT_MAX, x = 1.2345 * 2^-60', F32(1.2345)*vd.two(-60), _s(vd.FLT_MAX)), ('a = +inf, x = 1', F32(1.), F32(vd.INF)),
              ('a = +inf, x = 2^100 (G case a_inf)', vd.two(100), F32(vd.INF))],
    'x_min': [('x one ulp below 2^-60, s = 2^-20', vd.below(vd.two(-60)), vd.two(-20)), ('x one ulp below, s = 1', vd.below(vd.two(-60)), F32(1.)),
              ('x one ulp below, s = 2^40', vd.below(vd.two(-60)), vd.two(40)),
              ('x = 0', F32(0.), F32(1.)), ('x = 2^-140 (subnormal), s = 1', vd.two(-140), F32(1.)),
              ('x = 1.2345 * 2^-100, s = 1.5 * 2^39: a subnormal quotient', F32(1.2345)*vd.two(-100), F32(1.5)*vd.two(39)),
              ('x = 0x1.82p-140 (subnormal), s = 0x1.e0a78p-9 (G case x_min_subnormal_numerator)',) + _pair('x_min_subnormal_numerator'),
              ('x = -0x1.4df78p-131, s = 0x1.a553d8p-7', F32(float.fromhex('-0x1.4df78p-131')), F32(float.fromhex('0x1.a553d8p-7')))],
    'x_max': [('x one ulp above 2^60, s = 2^-20', vd.above(vd.two(60)), vd.two(-20)), ('x one ulp above, s = 1', vd.above(vd.two(60)), F32(1.)),
              ('x one ulp above, s = 2^40', vd.above(vd.two(60)), vd.two(40)),
              ('x = 2^120, s = 2^-20: the quotient overflows (G case x_max_quotient_overflows)',) + _pair('x_max_quotient_overflows'), ('x = +inf', F32(vd.INF), F32(1.)), ('x = -inf', F32(-vd.INF), F32(1.))],
    'a_min_igdn': [('a one ulp below 2^-96', vd.below(vd.two(-96))), ('a = 1.5 * 2^-100', F32(1.5)*vd.two(-100)), ('a = 2^-126', vd.two(-126)),
                   ('a = 2^-140 (subnormal)', vd.two(-140)), ('a = 2^-149', vd.two(-149)), ('a = -1', F32(-1.))],
}
# Measured on an MI355X: ONE ulp beyond any single bound, with the other operand anywhere in its own range, both forms still give the
# same bits -- each bound is conservative by itself, and an element one ulp out only proves that the fallback is taken and right. What
# the guard exists for lies further out (and is what the G extras hold): a quotient that overflows (`/` gives inf, the unscaled Newton
# steps NaN), an infinite x or a, a subnormal numerator over a divisor that is no power of two (v_div_scale would have scaled it;
# 1095 of 6000 random such pairs differ, and 0 of 6000 with 2^-100 <= |x| < 2^-60 whose quotient is subnormal), and for IGDN a
# denominator below 2^-126 (v_sqrt_f32 flushes a subnormal operand; 2^-126 itself differs too, 1.5 * 2^-100 does not).
ONE_ULP_OPERANDS = {'a_min': 3, 'a_max': 3, 'x_min': 3, 'x_max': 3, 'a_min_igdn': 1}     # the leading entries of FAR_SIDE


@pytest.mark.parametrize('bound', sorted(FAR_SIDE))
def test_every_bound_has_a_far_side_operand_the_short_form_gets_wrong(test_library, bound):
    """Without such an operand a G case proves nothing about the bound: both paths would give the oracle's bits."""
    observed = []
    for operand in FAR_SIDE[bound]:
        with numpy.errstate(all='ignore'):
            observed.append(_sqrt_differs(operand[1]) if bound == 'a_min_igdn' else _div_differs(operand[1], operand[2]))
    print('far side of {0}: '.format(bound) + '; '.join('{0}: {1}'.format(operand[0], 'DIFFERS' if d else 'same bits')
                                                           for (operand, d) in zip(FAR_SIDE[bound], observed)))
    assert any(observed), bound
    assert not any(observed[:ONE_ULP_OPERANDS[bound]]), bound          # conservative by one ulp: see above
    for (operand, differs) in zip(FAR_SIDE[bound], observed):
        if 'G case' in operand[0]:
            assert differs, operand[0]                                  # the extras of `vd.g_cases` do carry operands with teeth


def test_the_placed_operands_have_teeth(test_library):
    """vd.PLACED_TEETH (and their likes in the conv_1 and latent-stage cases): the operand of the ONE element that leaves the range is one
    the short form gets wrong, so a lane or a register missing from the guard's vote gives other bits than the oracle's."""
    with numpy.errstate(all='ignore'):
        assert _div_differs(vd.two(120), _s(vd.two(-40)))                                                 # teeth_x_max
        assert _div_differs(*_pair('x_min_subnormal_numerator'))                                          # teeth_x_min
        assert _div_differs(vd.two(60), _s(F32(vd.two(60)*vd.two(60))*vd.two(10)))                         # teeth_a_max: s = sqrt(inf)
        (x, gamma_cc) = vd.PLACED_TEETH['teeth_a_min'][1:3]
        assert F32(x*x)*gamma_cc == vd.two(-140) and _sqrt_differs(vd.two(-140))                          # teeth_a_min
        x = vd.PLACED_TEETH['teeth_a_min_igdn'][1]
        assert F32(x*x) == vd.two(-140)                                                                   # teeth_a_min_igdn, out_teeth_*


def test_on_the_bounds_the_short_forms_hold(test_library):
    """The near side, at the corners: every bound itself with the other operand at each end of its range (the exhaustive and the
    sampled proofs are in tests/test_gpu_kernels.py)."""
    for a in (vd.two(-40), vd.two(80)):
        for x in (vd.two(-60), -vd.two(60), F32(1.)):
            assert not _div_differs(x, _s(a)), (a, x)
    assert not _sqrt_differs(vd.two(-96)) and not _sqrt_differs(F32(vd.INF))


# ---- L: the luma cast -------------------------------------------------------------------------------------------------------------------
LUMA_TARGETS = (15.5, 16., 16.5, 234.5, 235., 235.5)


def test_luma_cast_at_its_edges(guard, dev, orc):
    """transpose_conv_3's uint8 output and its squared error aimed at the half-way points next to both clip levels, at +-inf and at
    +-FLT_MAX, through a single nonzero tap (output (4p, 4q) = x[p][q][0] * w; every other output is 0 -> 16). The infinities come from
    FLT_MAX * +-4, so no 0 * inf (NaN, whose uint8 is undefined in numpy too) arises anywhere. Against round(clip(.)) in numpy."""
    up = guard.upload
    shape = (1, 5, 7)
    target = vd.image(numpy.random.RandomState(9), 1, 20, 28)
    for (tap, values) in ((F32(1.), LUMA_TARGETS + (-3., 300.)), (vd.FLT_MAX, (4., -4., 1., -1., 0., 0.5, -0.5, 2.))):
        x = numpy.zeros(shape + (C,), dtype=F32)
        for (k, v) in enumerate(values):
            x[0, 1 + 2*(k//4), 1 + k % 4, 0] = v
        w = numpy.zeros((9, 9, 1, C), dtype=F32)
        w[2, 2, 0, 0] = tap
        with numpy.errstate(all='ignore'):
            ref = orc.conv2d_transpose_same(x, w, 4, None)[..., 0]
        assert not numpy.isnan(ref).any()
        if tap == 1.:
            assert set(LUMA_TARGETS) <= set(ref.ravel().tolist())
        else:
            assert {vd.INF, -vd.INF, float(vd.FLT_MAX), -float(vd.FLT_MAX)} <= set(ref.ravel().tolist())
        ref_u8 = numpy.round(ref.clip(min=16., max=235.)).astype(numpy.uint8)
        (f32, u8, sse) = dev.tconv9x9s4_luma(up(x), dev.pack_tconv9x9s4_weights(up(w)), want_f32=True, want_u8=True, ref_u8=up(target))
        assert vd.same(_host(f32), ref)
        assert numpy.array_equal(_host(u8), ref_u8)
        assert _host(sse).tolist() == [int(((target.astype(numpy.int64) - ref_u8.astype(numpy.int64))**2).sum())]
    assert numpy.round(F32(15.5).clip(16., 235.)) == 16 and numpy.round(F32(16.5)) == 16 and numpy.round(F32(234.5)) == 234 and numpy.round(F32(235.5).clip(16., 235.)) == 235
