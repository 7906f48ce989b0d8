"""The oracle at float32's value edges (tests/value_domain_cases.py), against exact arithmetic -- CPU only.

oracle/transforms_oracle.c is the reference of every GPU parity test, so it must itself be right where accumulators are subnormal,
overflow or are already infinite, and where the operands of the normalisations leave the middle of the range -- inside a process
that has imported torch (which may change the floating-point environment of the threads it starts: flush-to-zero would go
unnoticed by every other test). Sampled outputs of each case are recomputed as the documented chain in `fractions.Fraction`, every
step rounded to float32 once (ties to even, gradual underflow, overflow to inf), the square root correctly rounded through
`math.isqrt`. Going through float64 would round twice and is not a reference."""
from fractions import Fraction

import numpy
import pytest
import torch  # noqa: F401  (on purpose: the oracle has to be right in the processes the GPU tests run in)

import value_domain_cases as vd

SAMPLES = 16


@pytest.fixture(scope='module')
def orc():
    from oracle import transforms
    return transforms


def _sample_indices(shape, seed):
    rng = numpy.random.RandomState(seed)
    return [tuple(int(rng.randint(s)) for s in shape) for _ in range(SAMPLES)]


def test_round_f32_is_float32_rounding():
    """The reference's own rounding, on the cases float32 defines: ties to even, the subnormal quantum, the overflow threshold."""
    one = Fraction(1)
    ulp = Fraction(1, 2**23)
    assert vd.round_f32(one + ulp/2) == one and vd.round_f32(one + 3*ulp/2) == one + 2*ulp              # ties to even
    assert vd.round_f32(one + ulp/2 + Fraction(1, 2**80)) == one + ulp
    tiny = Fraction(1, 2**149)
    assert vd.round_f32(tiny/2) == 0 and vd.round_f32(3*tiny/2) == 2*tiny and vd.round_f32(tiny*Fraction(3, 4)) == tiny
    assert vd.round_f32(Fraction(1, 2**126) - tiny/4) == Fraction(1, 2**126)
    flt_max = Fraction(float(vd.FLT_MAX))
    assert vd.round_f32(flt_max + Fraction(2)**103 - 1) == flt_max and vd.round_f32(flt_max + Fraction(2)**103) == vd.INF
    assert vd.round_f32(-(flt_max + Fraction(2)**103)) == -vd.INF
    rng = numpy.random.RandomState(0)
    for v in numpy.ldexp(rng.standard_normal(size=200), rng.randint(-160, 135, size=200)):               # float64 -> float32 rounds once
        with numpy.errstate(over='ignore'):
            assert vd.equals_exact(numpy.float32(v), vd.round_f32(Fraction(float(v))))
    for a in (2., 3., float(vd.two(-149)), float(vd.two(-126)), float(vd.below(vd.two(-96))), 1. + 2.**-23, float(vd.FLT_MAX)):
        assert vd.equals_exact(numpy.sqrt(numpy.float32(a)), vd.sqrt(Fraction(a)))


@pytest.mark.parametrize('cls', ['A1', 'A2', 'A3tiny', 'A3one', 'A4', 'A5', 'A6'])
@pytest.mark.parametrize('kind,shape', [('conv', (1, 6, 10)), ('tconv', (1, 3, 5))])
def test_conv_chains_are_exact(kind, shape, cls):
    case = vd.a_case(kind, cls, shape)
    vd.assert_population(cls, case['raw'])
    for index in _sample_indices(case['raw'].shape, 11):
        exact = vd.conv_chain(case['x'], case['w'], case['bias'], kind, 2, index)
        assert vd.equals_exact(case['raw'][index], exact), (index, case['raw'][index], exact)


def test_the_fused_chain_keeps_infinity():
    """A5: once an accumulator is +inf, a product whose exact value is beyond -2^128 leaves it +inf in a fused chain; rounding the
    product first gives -inf and the sum NaN. The oracle returns all inf and no NaN, and so does the exact chain."""
    for (kind, shape) in (('conv', (1, 6, 10)), ('tconv', (1, 3, 5))):
        raw = vd.a_case(kind, 'A5', shape)['raw']
        assert numpy.all(numpy.isinf(raw)) and not numpy.any(numpy.isnan(raw))
    assert vd.fma(Fraction(2)**100, -Fraction(2)**100, vd.INF) == vd.INF


@pytest.mark.parametrize('cls', ['A1', 'A2', 'A4', 'A5'])
def test_conv1_and_tconv3_chains_are_exact(cls):
    case = vd.a_case_conv1(cls, 'usual')
    x = case['x'].astype(numpy.float32)[..., None]
    for index in _sample_indices(case['raw'].shape, 12):
        exact = vd.conv_chain(x, case['w'], case['bias'], 'conv', 4, index)
        assert vd.equals_exact(case['raw'][index], exact), (index, case['raw'][index], exact)
    case = vd.a_case_tconv3(cls)
    for index in _sample_indices(case['raw'].shape, 13):
        exact = vd.conv_chain(case['x'], case['w'], None, 'tconv', 4, index + (0,))
        assert vd.equals_exact(case['raw'][index], exact), (index, case['raw'][index], exact)


@pytest.mark.parametrize('inverse', [False, True])
def test_gdn_chains_are_exact_on_the_guard_cases(orc, inverse):
    """Every G case (each bound of gdn_tile's guard: inside, on it, one ulp beyond; zero, subnormal and infinite x; subnormal,
    negative and infinite a): the element the case is about and 15 others, through the exact chain."""
    rows = 99
    for (name, x, gamma, beta, expectation) in vd.g_cases(rows, inverse):
        with numpy.errstate(all='ignore'):
            (a, y) = (orc.gdn_denominators(x, gamma, beta), orc.gdn(x, gamma, beta, inverse=inverse))
        assert vd.g_expectation_holds(a, x, inverse, expectation), name
        changed = numpy.argwhere((x != vd.base_x(rows, 40 + rows)) | (beta != 1.)[None, :])
        picked = [tuple(changed[0])] if len(changed) else []
        for (row, ch) in picked + _sample_indices(x.shape, 15)[:SAMPLES - len(picked)]:
            (a_exact, y_exact) = vd.gdn_chain(x[row], gamma, beta, inverse, ch)
            assert vd.equals_exact(a[row, ch], a_exact), (name, row, ch, a[row, ch], a_exact)
            assert vd.equals_exact(y[row, ch], y_exact), (name, row, ch, y[row, ch], y_exact)


@pytest.mark.parametrize('cls', ['A1', 'A2', 'A4', 'A6'])
@pytest.mark.parametrize('kind,shape', [('conv', (1, 6, 10)), ('tconv', (1, 3, 5))])
def test_gdn_chains_are_exact_on_the_a_classes(kind, shape, cls):
    """Dense gamma, per-channel beta, on subnormal, straddling, overflowed and special un-normalised values."""
    case = vd.a_case(kind, cls, shape)
    raw = case['raw'].reshape(-1, vd.C)
    for (row, ch) in _sample_indices(raw.shape, 14):
        (a_exact, y_exact) = vd.gdn_chain(raw[row], case['gamma'], case['beta'], kind == 'tconv', ch)
        assert vd.equals_exact(case['a'].reshape(-1, vd.C)[row, ch], a_exact), (row, ch)
        assert vd.equals_exact(case['normed'].reshape(-1, vd.C)[row, ch], y_exact), (row, ch, case['normed'].reshape(-1, vd.C)[row, ch], y_exact)
