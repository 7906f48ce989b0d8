"""Seeded inputs at float32's VALUE edges, shared by the CPU tests of the oracle out there (tests/test_oracle_value_domain.py) and
the GPU parity tests (tests/test_gpu_value_domain.py). Every other float input of the suite lies within a few binades of 1.

A classes: plain `standard_normal` tensors x0, w0 scaled by powers of two (no model initialiser), so that the accumulators of a conv
or transposed conv are subnormal (A1), straddle the normal / subnormal line (A2), meet a bias (A3), overflow inside the chain (A4),
are +-inf while products beyond 2^128 keep arriving (A5: a fused chain stays inf, anything that rounds the product first gives NaN)
or meet special values in the input (A6). G classes: the five bounds of `gdn_tile`'s range guard (csrc/hip/common.h), one element
at a time. Each builder returns its inputs together with the oracle's own intermediates -- the un-normalised output `raw`, the
denominators `a` = sum_k x_k^2 gamma[k][c] + beta[c] -- so that a test asserts that its case populates the class it claims
(`shares`). Also here: the exact float32 arithmetic in `fractions.Fraction` that the CPU tests hold the oracle against."""
import functools
import math
from fractions import Fraction

import numpy

F32 = numpy.float32
C = 128
INF = float('inf')
FLT_MAX = numpy.finfo(F32).max
TINY = numpy.finfo(F32).tiny                 # 2^-126, the smallest normal


def two(e):
    return F32(math.ldexp(1., e))


def below(v):
    """The float32 one ulp nearer to 0."""
    return numpy.nextafter(F32(v), F32(0.))


def above(v):
    """The float32 one ulp further from 0."""
    return numpy.nextafter(F32(v), F32(numpy.copysign(INF, v)))


def bits(v):
    return int(numpy.asarray(v, dtype=F32).view(numpy.uint32))


def shares(t):
    """Fractions of the elements of `t` that are subnormal, normal, zero, inf and NaN."""
    t = numpy.asarray(t, dtype=F32)
    mag = numpy.abs(t)
    with numpy.errstate(invalid='ignore'):
        return {'subnormal': float(numpy.mean((mag > 0) & (mag < TINY))), 'normal': float(numpy.mean((mag >= TINY) & numpy.isfinite(t))),
                'zero': float(numpy.mean(mag == 0)), 'inf': float(numpy.mean(numpy.isinf(t))), 'nan': float(numpy.mean(numpy.isnan(t)))}


def same(got, ref):
    """The suite's exact comparison, out here: NaNs by position, everything else `==` (so -0 == +0, inf == inf)."""
    got = numpy.asarray(got)
    ref = numpy.asarray(ref)
    if got.shape != ref.shape:
        return False
    (gn, rn) = (numpy.isnan(got), numpy.isnan(ref))
    return bool(numpy.array_equal(gn, rn) and numpy.array_equal(got[~gn], ref[~rn]))


def image(rng, n, h, w):
    """The usual 16..235 image of the kernel tests (3x box blur)."""
    x = rng.randint(16, 236, size=(n, h, w)).astype(numpy.float64)
    for _ in range(3):
        x = (x + numpy.roll(x, 1, 1) + numpy.roll(x, -1, 1) + numpy.roll(x, 1, 2) + numpy.roll(x, -1, 2))/5.
    return numpy.round(x).astype(numpy.uint8)


def _orc():
    from oracle import transforms
    return transforms


# ---- A classes ------------------------------------------------------------------------------------------------------------------
# class -> (log2 of the scale of x0, of w0). A3 and A6 are built on these below.
A_SCALES = {'A1': (-40, -103), 'A2': (-20, -110), 'A4': (70, 52), 'A5': (70, 57), 'A6': (0, -3)}
A_CLASSES = ('A1', 'A2', 'A3tiny', 'A3one', 'A4', 'A5', 'A6')
# conv_1 reads pixels, not floats: the filter carries both scales, less what a pixel of ~2^7 and the 81-tap sum add (2^5 in A1 / A2, so
# that the sums sit where the class wants them; A4: sums of ~2^10 sigma against 2^128; A5: one product 2^7 * 2^125 is beyond 2^128).
A_SCALES_U8 = {'A1': -148, 'A2': -136, 'A4': 117, 'A5': 125}
A_CLASSES_U8 = ('A1', 'A2', 'A3tiny', 'A3one', 'A4', 'A5')
IMAGES_U8 = ('zeros', 'full', 'checkerboard', 'usual')
SPECIALS = (INF, -INF, float('nan'), -0.0, float(two(-149)), float(FLT_MAX))


def _bias(cls, seed):
    if cls == 'A3tiny':            # +-2^-130: subnormal biases on subnormal sums
        return (numpy.where(numpy.random.RandomState(seed).uniform(size=C) < 0.5, -1., 1.)*two(-130)).astype(F32)
    if cls == 'A3one':             # a normal bias absorbs a subnormal sum
        return numpy.ones(C, dtype=F32)
    return None


def norm_parameters(seed=5):
    """A dense asymmetric gamma and a per-channel beta from plain generators: for the A classes through a normalisation."""
    rng = numpy.random.RandomState(seed)
    return (numpy.abs(rng.standard_normal(size=(C, C))*0.01).astype(F32), (0.5 + numpy.abs(rng.standard_normal(size=C))).astype(F32))


def _with_specials(x, seed):
    """A6: six elements of x become +inf, -inf, NaN, -0.0, 2^-149 and FLT_MAX; the first within two positions of the top left corner
    and the last within two of the bottom right one, so that their taps meet the padding. The WEIGHTS stay finite: a padded tap is a
    zero that the kernel multiplies and the oracle skips, and 0 * inf is outside that contract."""
    (n, h, w, c) = x.shape
    rng = numpy.random.RandomState(seed)
    places = [(0, 0, min(1, w - 1)), (0, h - 1, max(w - 2, 0))] + [(0, int(rng.randint(h)), int(rng.randint(w))) for _ in range(4)]
    order = (0, 5, 1, 2, 3, 4)                                                # +inf and FLT_MAX take the two corners
    for (k, place) in zip(order, places):
        x[place + (int(rng.randint(c)),)] = F32(SPECIALS[k])
    return x


@functools.lru_cache(maxsize=None)
def a_case(kind, cls, shape):
    """kind 'conv' (5x5, stride 2, SAME) or 'tconv' (its transpose) at input positions `shape`: dict with x, w (TF layout), bias (or
    None), raw = the oracle's output with the bias, and its normalisation `normed` (GDN for 'conv', IGDN for 'tconv') with `a`."""
    orc = _orc()
    base = {'A3tiny': 'A1', 'A3one': 'A1'}.get(cls, cls)
    (sx, sw) = A_SCALES[base]
    rng = numpy.random.RandomState(1000 + 7*shape[1] + shape[2] + (0 if kind == 'conv' else 500))
    x = (rng.standard_normal(size=shape + (C,)).astype(F32)*two(sx)).astype(F32)
    w = (rng.standard_normal(size=(5, 5, C, C)).astype(F32)*two(sw)).astype(F32)
    if cls == 'A6':
        x = _with_specials(x, 77)
    bias = _bias(cls, 3)
    with numpy.errstate(all='ignore'):
        raw = (orc.conv2d_same if kind == 'conv' else orc.conv2d_transpose_same)(x, w, 2, bias)
        (gamma, beta) = norm_parameters()
        case = {'x': x, 'w': w, 'bias': bias, 'raw': raw, 'gamma': gamma, 'beta': beta, 'a': orc.gdn_denominators(raw, gamma, beta),
                'normed': orc.gdn(raw, gamma, beta, inverse=kind == 'tconv')}
    return case                      # shared by every test that asks for it: nobody writes to it


def assert_population(cls, raw):
    """What each A class claims about the oracle's un-normalised output."""
    s = shares(raw)
    if cls == 'A1':
        assert s['subnormal'] >= 0.99 and s['inf'] == 0 and s['nan'] == 0, s
    elif cls == 'A2':
        assert s['subnormal'] >= 0.10 and s['normal'] >= 0.10 and s['inf'] == 0 and s['nan'] == 0, s
    elif cls == 'A3tiny':
        assert s['subnormal'] >= 0.99 and s['nan'] == 0, s
    elif cls == 'A3one':
        assert s['normal'] == 1.0 and numpy.all(numpy.asarray(raw) == F32(1.)), s           # the bias absorbs every subnormal sum
    elif cls == 'A4':
        assert s['inf'] >= 0.01 and s['normal'] >= 0.01, s
    elif cls == 'A5':
        assert s['inf'] == 1.0 and s['nan'] == 0, s
    elif cls == 'A6':
        assert s['nan'] > 0 and s['inf'] > 0 and s['normal'] > 0.25, s
    return s


def images_u8(name, shape=(1, 36, 100)):
    (n, h, w) = shape
    if name == 'zeros':
        return numpy.zeros(shape, dtype=numpy.uint8)
    if name == 'full':
        return numpy.full(shape, 255, dtype=numpy.uint8)
    if name == 'checkerboard':
        return (((numpy.arange(h)[:, None] + numpy.arange(w)[None, :]) % 2)*255).astype(numpy.uint8)[None].repeat(n, axis=0)
    return image(numpy.random.RandomState(5), n, h, w)


@functools.lru_cache(maxsize=None)
def a_case_conv1(cls, image_name):
    """conv_1 (9x9, stride 4, uint8 pixels in) on a (1, 36, 100) image with a filter at the class's scale."""
    orc = _orc()
    base = {'A3tiny': 'A1', 'A3one': 'A1'}.get(cls, cls)
    x = images_u8(image_name)
    w = (numpy.random.RandomState(2000).standard_normal(size=(9, 9, 1, C)).astype(F32)*two(A_SCALES_U8[base])).astype(F32)
    bias = _bias(cls, 4)
    with numpy.errstate(all='ignore'):
        raw = orc.conv2d_same(x.astype(F32)[..., None], w, 4, bias)
        (gamma, beta) = norm_parameters()
        case = {'x': x, 'w': w, 'bias': bias, 'raw': raw, 'gamma': gamma, 'beta': beta, 'a': orc.gdn_denominators(raw, gamma, beta),
                'normed': orc.gdn(raw, gamma, beta)}
    return case


@functools.lru_cache(maxsize=None)
def a_case_tconv3(cls, shape=(1, 5, 7)):
    """transpose_conv_3 (9x9, stride 4, 128 -> 1), float32 output."""
    orc = _orc()
    (sx, sw) = A_SCALES[cls]
    rng = numpy.random.RandomState(3000)
    x = (rng.standard_normal(size=shape + (C,)).astype(F32)*two(sx)).astype(F32)
    w = (rng.standard_normal(size=(9, 9, 1, C)).astype(F32)*two(sw)).astype(F32)
    if cls == 'A6':
        x = _with_specials(x, 78)
    with numpy.errstate(all='ignore'):
        return {'x': x, 'w': w, 'raw': orc.conv2d_transpose_same(x, w, 4, None)[..., 0]}


# ---- G classes: the range guard of gdn_tile, bound by bound ----------------------------------------------------------------------
# bound -> (its value, the direction of the far side, which normalisation has it, 'x' or 'a')
BOUNDS = {'a_min': (two(-40), 'below', False, 'a'), 'a_max': (two(80), 'above', False, 'a'),
          'x_min': (two(-60), 'below', False, 'x'), 'x_max': (two(60), 'above', False, 'x'),
          'a_min_igdn': (two(-96), 'below', True, 'a')}


def base_x(rows, seed):
    """[rows, 128] with every |x| a multiple of 2^-10 in [1, 7): wholly inside every bound, and x + b == x for a bias b <= 2^-60."""
    rng = numpy.random.RandomState(seed)
    mag = 1. + rng.randint(0, 6*1024, size=(rows, C))/1024.
    return (mag*numpy.where(rng.uniform(size=(rows, C)) < 0.5, -1., 1.)).astype(F32)


def placements(rows):
    """(row, channel) of the ONE element, named after where it sits in a 32-position wave tile over rows in raster order
    (csrc/hip/common.h: wave_epilogue -- register r of tile t at lane l holds channel 32 t + (r & 3) + 8 (r >> 2) + 4 (l >> 5) of
    position l & 31): lane 0 and lane 63, each with the first and the last register; and one element in the second tile alone, so
    that only one of the launch's wavefronts leaves the range. Fewer than 32 rows: the last row stands in for lane 63's."""
    last = min(31, rows - 1)
    places = [('lane0_first', 0, 0), ('lane0_last', 0, 123), ('lane63_first', last, 4), ('lane63_last', last, 127)]
    if rows > 40:
        places.append(('second_tile_only', 40, 77))
    return places


def g_cases(rows, inverse, places=None):
    """List of (name, x [rows, 128] un-normalised, gamma, beta, expectation) for one normalisation direction; expectation is 'inside'
    (every a and |x| within the bounds), 'beyond' (at least one outside) or None (the extras: not asserted). gamma = 0 and beta = 1
    except in the channel of an `a` element, where gamma[c][c] = 1 (1 -+ ulp for the far side) and beta[c] = 0: a = x^2 gamma[c][c]
    exactly, and it moves with the data."""
    x0 = base_x(rows, 40 + rows)
    zero = numpy.zeros((C, C), dtype=F32)
    one = numpy.ones(C, dtype=F32)
    cases = [('inside', x0, zero, one, 'inside')]

    def with_element(row, ch, value, a_channel, gamma_cc=1.):
        x = x0.copy()
        x[row, ch] = value
        (gamma, beta) = (zero, one)
        if a_channel:
            (gamma, beta) = (zero.copy(), one.copy())
            gamma[ch, ch] = gamma_cc
            beta[ch] = 0.
        return (x, gamma, beta)

    for (bound, (value, far, inv, operand)) in BOUNDS.items():
        if inv != inverse:
            continue
        for (i, (place, row, ch)) in enumerate(places if places is not None else placements(rows)):
            sign = F32(-1.) if i % 2 else F32(1.)
            if operand == 'a':           # x = the bound's exact root (2^-20, 2^40, 2^-48): a = x^2 gamma[c][c] is the bound, or 1 ulp beyond it
                root = F32(math.sqrt(float(value)))
                beyond_cc = below(1.) if far == 'below' else above(1.)
                assert F32(root*root)*F32(1.) == value and F32(root*root)*beyond_cc == (below(value) if far == 'below' else above(value))
                on = with_element(row, ch, sign*root, True)
                beyond = with_element(row, ch, sign*root, True, beyond_cc)
            else:
                on = with_element(row, ch, sign*value, False)
                beyond = with_element(row, ch, sign*(below(value) if far == 'below' else above(value)), False)
            cases.append(('{0}_on_{1}'.format(bound, place),) + on + ('inside',))
            cases.append(('{0}_beyond_{1}'.format(bound, place),) + beyond + ('beyond',))
    # operands with TEETH (the short forms give other bits for them on an MI355X, PLACED_TEETH below), ONE element each, at every place:
    # a lane or a register left out of the guard's min / max chains or of its ballot shows here, not in the one-ulp cases above
    for (name, (inv, value, gamma_cc, beta_c)) in PLACED_TEETH.items():
        if inv != inverse:
            continue
        for (place, row, ch) in (places if places is not None else placements(rows)):
            (x, gamma, beta) = with_element(row, ch, value, gamma_cc is not None, gamma_cc)
            if beta_c is not None:
                beta = beta.copy()
                beta[ch] = beta_c
            cases.append(('{0}_{1}'.format(name, place), x, gamma, beta, None if name == 'teeth_x_max' else 'beyond'))
    (row, ch) = (min(5, rows - 1), 50)
    for (name, value, a_channel) in (('x_zero', 0., False), ('x_subnormal', two(-140), False), ('x_plus_inf', INF, False),
                                     ('x_minus_inf', -INF, False), ('a_subnormal', two(-70), True), ('a_inf', two(100), True)):
        cases.append((name,) + with_element(row, ch, value, a_channel) + (None,))
    # far-side operands that the short forms get WRONG on an MI355X (FAR_SIDE_TEETH below): beta[c] sets s = sqrt(a) for the channel
    for (name, (value, beta_c)) in FAR_SIDE_TEETH.items():
        (x, gamma, beta) = with_element(row, ch, value, False)
        beta = beta.copy()
        beta[ch] = beta_c
        cases.append((name, x, gamma, beta, None))
    negative = one.copy()
    negative[ch] = -1.                                                        # a < 0: NaN on both sides
    cases.append(('a_negative', x0, zero, negative, None))
    return cases


def square_root_operand(s):
    """A float32 a with sqrtf(a) == s (two neighbouring a share most s; numpy's float32 sqrt is correctly rounded, like sqrtf)."""
    a = F32(s)*F32(s)
    for candidate in (a, below(a), above(a), below(below(a)), above(above(a))):
        if numpy.sqrt(candidate) == F32(s):
            return candidate
    raise AssertionError('no float32 has the square root {0!r}'.format(s))


# name -> (x of ONE element, beta of its channel with gamma = 0, so a = beta): operands far beyond a bound, where hipcc's full division
# does what div_mid leaves out -- the quotient overflows (x / s = 2^140, 2^130: `/` gives inf, the unscaled Newton steps NaN), or the
# numerator is subnormal and the divisor not a power of two (v_div_scale would have scaled it: the pair below is one that a search on
# an MI355X found to differ; 16 others with s = sqrt(1.5 * 2^-30) did not). tests/test_gpu_value_domain.py asks the test build's hook
# about exactly these pairs.
FAR_SIDE_TEETH = {'x_max_quotient_overflows': (two(120), two(-40)), 'a_min_quotient_overflows': (two(60), two(-140)),
                  'x_min_subnormal_numerator': (F32(float.fromhex('0x1.82p-140')), square_root_operand(float.fromhex('0x1.e0a78p-9')))}


# name -> (IGDN?, x of the ONE element, gamma[c][c] or None, beta[c] or None): exactly one element of the tile leaves the range, and far enough
# for the short forms to go wrong. teeth_x_max: 2^120 / sqrt(2^-40) overflows (no |x| <= 2^64 has teeth, and the square of this one is
# inf, so inf * gamma = NaN takes its whole position -- one lane, every register -- out of range: the one case here that is not ONE element). teeth_x_min: the subnormal numerator of FAR_SIDE_TEETH.
# teeth_a_max: a = 2^120 * 2^10 = +inf under an x on its bound (div_mid(x, inf) is NaN, x / inf is 0). teeth_a_min: a = 2^-120 * 2^-20 =
# 2^-140, a subnormal that v_sqrt_f32 flushes, under an x on its bound. teeth_a_min_igdn: a = (2^-70)^2, the same for IGDN.
PLACED_TEETH = {'teeth_x_max': (False, two(120), None, two(-40)),
                'teeth_x_min': (False,) + (FAR_SIDE_TEETH['x_min_subnormal_numerator'][0], None, FAR_SIDE_TEETH['x_min_subnormal_numerator'][1]),
                'teeth_a_max': (False, two(60), two(10), None), 'teeth_a_min': (False, two(-60), two(-20), None),
                'teeth_a_min_igdn': (True, two(-70), F32(1.), None)}


def g_expectation_holds(a, x, inverse, expectation):
    """Does the oracle's own (a, x) populate what the case claims about gdn_tile's guard?"""
    with numpy.errstate(invalid='ignore'):
        mag = numpy.abs(x)
        inside = bool(numpy.all(a >= two(-96))) if inverse else bool(
            numpy.all(a >= two(-40)) and numpy.all(a <= two(80)) and numpy.all(mag >= two(-60)) and numpy.all(mag <= two(60)))
    if expectation == 'inside':
        return inside
    if expectation == 'beyond':
        if inverse:
            outside = int(numpy.sum(~(a >= two(-96))))
        else:
            outside = int(numpy.sum(~((a >= two(-40)) & (a <= two(80)) & (mag >= two(-60)) & (mag <= two(60)))))
        return outside == 1                                                   # ONE element, and it is 1 ulp out (checked by the builder)
    return True


def identity_conv_input(out_positions, values):
    """Input [n, 2h, 2w, 128] of conv5x5s2 whose output under `identity_conv_weights` is `values` [n, h, w, 128] exactly: the centre
    tap of output (i, j) is input (2i + 1, 2j + 1); every other input is 0, and so is every other weight."""
    (n, h, w) = out_positions
    x = numpy.zeros((n, 2*h, 2*w, C), dtype=F32)
    x[:, 1::2, 1::2, :] = values.reshape(n, h, w, C)
    return x


def identity_conv_weights():
    w = numpy.zeros((5, 5, C, C), dtype=F32)
    w[2, 2] = numpy.eye(C, dtype=F32)
    return w


def identity_tconv_weights():
    """tconv5x5s2 with these copies input (p, q) to the outputs (2p + a, 2q + b), a, b in {0, 1}: taps u, v in {1, 2}, one tap each."""
    w = numpy.zeros((5, 5, C, C), dtype=F32)
    for u in (1, 2):
        for v in (1, 2):
            w[u, v] = numpy.eye(C, dtype=F32)
    return w


# ---- exact float32 arithmetic in fractions.Fraction ------------------------------------------------------------------------------
# A value is a Fraction (finite; the sign of a zero is not kept: the suite compares -0 == +0) or a Python float inf / -inf / nan.
def to_exact(v):
    v = float(v)
    return v if (math.isinf(v) or math.isnan(v)) else Fraction(v)


def round_f32(v):
    """A real number to the nearest float32: ties to even, gradual underflow (quantum 2^-149 below 2^-126), overflow to inf from
    2^128 - 2^103 on (the halfway point between FLT_MAX and 2^128, which rounds up, its neighbour being odd)."""
    if isinstance(v, float) or v == 0:
        return v
    mag = abs(v)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()             # floor(log2(mag)) is e or e - 1
    if Fraction(2)**e > mag:
        e -= 1
    quantum = Fraction(2)**(max(e, -126) - 23)
    scaled = mag/quantum
    n = scaled.numerator//scaled.denominator
    rest = scaled - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    out = n*quantum
    if out >= Fraction(2)**128:
        return INF if v > 0 else -INF
    return out if v > 0 else -out


def _sign(v):
    return v if isinstance(v, float) else float((v > 0) - (v < 0))


def _special(result):
    """The result of an operation that had an inf or a NaN among its operands, computed on signs: inf, -inf, NaN or 0."""
    return result if (math.isinf(result) or math.isnan(result)) else Fraction(0)


def fma(a, b, c):
    if isinstance(a, float) or isinstance(b, float) or isinstance(c, float):
        with numpy.errstate(invalid='ignore'):
            product = float(numpy.float64(_sign(a))*numpy.float64(_sign(b)))
            return _special(float(numpy.float64(product) + numpy.float64(_sign(c))))
    return round_f32(a*b + c)


def add(a, b):
    return fma(a, Fraction(1), b)


def mul(a, b):
    return fma(a, b, Fraction(0))


def div(a, b):
    if isinstance(a, float) or isinstance(b, float) or b == 0:
        with numpy.errstate(all='ignore'):
            return _special(float(numpy.float64(_sign(a))/numpy.float64(_sign(b))))       # x / +0 = +-inf, 0 / 0 = NaN, x / inf = 0
    return round_f32(a/b)


def sqrt(a):
    """Correctly rounded: an integer square root of a * 4^k with more bits than float32 holds; an inexact one is moved to the middle
    of its unit interval, which lies on the same side of every rounding boundary as the true root."""
    if isinstance(a, float):
        return a if a > 0 else float('nan')                                    # sqrt(+inf) = +inf, sqrt(-inf) = sqrt(NaN) = NaN
    if a < 0:
        return float('nan')
    if a == 0:
        return a
    m = a*Fraction(2)**150                                                     # a float32 is a multiple of 2^-149
    assert m.denominator == 1
    k = 64
    value = m.numerator << (2*k)
    r = math.isqrt(value)
    root = Fraction(r) if r*r == value else Fraction(2*r + 1, 2)
    return round_f32(root/Fraction(2)**(75 + k))


def conv_chain(x, w, bias, kind, stride, out_index):
    """One output element of the oracle's conv ('conv') or transposed conv ('tconv') as its documented chain: +0, then channel blocks
    of 32, kernel row, kernel column, channel within the block, skipping padded taps; the bias added afterwards."""
    (b, i, j, co) = out_index
    (n, h, wd, cin) = x.shape
    k = w.shape[0]

    def pad_before(size):
        out = -(-size//stride)
        return max((out - 1)*stride + k - size, 0)//2

    acc = Fraction(0)
    if kind == 'conv':
        (pbh, pbw) = (pad_before(h), pad_before(wd))
    else:
        (pbh, pbw) = (pad_before(h*stride), pad_before(wd*stride))
    for c0 in range(0, cin, 32):
        for u in range(k):
            for v in range(k):
                if kind == 'conv':
                    (r, c) = (i*stride + u - pbh, j*stride + v - pbw)
                    if r < 0 or r >= h or c < 0 or c >= wd:
                        continue
                else:
                    (pn, qn) = (i + pbh - u, j + pbw - v)
                    if pn < 0 or pn % stride or qn < 0 or qn % stride:
                        continue
                    (r, c) = (pn//stride, qn//stride)
                    if r >= h or c >= wd:
                        continue
                for ci in range(c0, min(c0 + 32, cin)):
                    wv = w[u, v, ci, co] if kind == 'conv' else w[u, v, co, ci]
                    acc = fma(to_exact(x[b, r, c, ci]), to_exact(wv), acc)
    return add(acc, to_exact(bias[co])) if bias is not None else acc


def gdn_chain(xrow, gamma, beta, inverse, c):
    """Channel c of one row through tfuls.gdn / inverse_gdn as the oracle orders it; returns (a, y)."""
    d = Fraction(0)
    for k in range(len(xrow)):
        xk = to_exact(xrow[k])
        d = fma(mul(xk, xk), to_exact(gamma[k, c]), d)
    a = add(d, to_exact(beta[c]))
    s = sqrt(a)
    xc = to_exact(xrow[c])
    return (a, mul(xc, s) if inverse else div(xc, s))


def equals_exact(value, exact):
    """A float32 of the oracle against an exact value: NaN with NaN, otherwise equal as numbers (-0 == +0)."""
    value = float(value)
    if isinstance(exact, float):
        return (math.isnan(value) and math.isnan(exact)) or value == exact
    return (not math.isnan(value)) and (not math.isinf(value)) and Fraction(value) == exact


def tconv3_structural_nan(x, out_shape):
    """Where transpose_conv_3's kernel gives NaN for a non-finite input although the oracle's chain never meets it: output pixel
    (4p' + a, 4q' + b) reads ALL nine sites (p' + dr, q' + dc), dr, dc in {-1, 0, 1}, with a zero weight where the tap u = a + 2 - 4 dr,
    v = b + 2 - 4 dc does not exist (csrc/hip/tconv3.hip), and 0 * inf = 0 * NaN = NaN. The oracle skips those taps."""
    (n, H, W) = out_shape
    mask = numpy.zeros(out_shape, dtype=bool)
    for (b, p, q, _) in numpy.argwhere(~numpy.isfinite(x)):
        for i in range(max(4*(p - 1), 0), min(4*(p + 2), H)):
            for j in range(max(4*(q - 1), 0), min(4*(q + 2), W)):
                (u, v) = (i % 4 + 2 - 4*(p - i//4), j % 4 + 2 - 4*(q - j//4))
                if not (0 <= u <= 8 and 0 <= v <= 8):
                    mask[b, i, j] = True
    return mask
