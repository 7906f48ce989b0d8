"""The host side of the rate-distortion optimised quantiser (ratecontrol.py), CPU only:

* magnitude_bits against a loop written here, at L = 1, 3, 10, 40, on random tables and on tables made of the 0.01 / 0.5 / 0.99 clamps;
* rdo_thresholds: zeros at lambda = 0, in the exception map's row and beyond min(L, 16); float32; K points; the refusals;
* rdo_quantize_numpy: every result is the nearest symbol or one step towards zero of it, the nearest symbol at lambda = 0, and
  special values (NaN, infinities, huge quotients) are left alone;
* the rule against brute force: on Laplacian maps with tables fitted on their nearest-rounded symbols, the choice of every eligible
  element is the argmin of (|x| - s)^2 bw^2 + lambda B(s) over s = a and s = a - 1 in float64, except where the two costs are within
  1e-5 bw^2 of each other (float32 against float64 at a tie), which at most 0.01 % of the elements may be."""
import math

import numpy
import pytest

from autoencoder_based_image_compression_amd import ratecontrol as rc

F32 = numpy.float32
NB_MAPS = 128
LENGTHS = [1, 3, 10, 40]


def bits_by_loop(p, a):
    """B(a) under the row p, one term at a time."""
    length = len(p)
    bits = 0.
    for i in range(min(a, length)):
        bits += -math.log2(1. - p[i])
    if a < length:
        bits += -math.log2(p[a])
    else:
        bits += 2*int(math.floor(math.log2(a - length + 1))) + 1          # Exp-Golomb order 0 of a - L
    if a > 0:
        bits += 1.
    return bits


def tables(length, seed):
    """(6, L): random rows, and rows made of the clamps `probabilities_from_counts` leaves."""
    rng = numpy.random.RandomState(seed)
    rows = [rng.uniform(0.02, 0.98, size=length) for _ in range(3)]
    rows.append(numpy.full(length, 0.01))
    rows.append(numpy.full(length, 0.99))
    rows.append(numpy.array([(0.01, 0.5, 0.99)[i % 3] for i in range(length)]))
    return numpy.stack(rows)


@pytest.mark.parametrize('length', LENGTHS)
def test_magnitude_bits_equals_the_loop(length):
    p = tables(length, length)
    bits = rc.magnitude_bits(p)
    assert bits.dtype == numpy.float64 and bits.shape == (p.shape[0], length + 1)
    for (row, out) in zip(p, bits):
        expected = numpy.array([bits_by_loop(row, a) for a in range(length + 1)])
        assert numpy.allclose(out, expected, rtol=1e-13, atol=0.)
    # leading axes pass through
    assert numpy.array_equal(rc.magnitude_bits(p.reshape(2, 3, length)), bits.reshape(2, 3, length + 1))


def point(length, seed, k_points=None):
    rng = numpy.random.RandomState(seed)
    shape = (NB_MAPS,) if k_points is None else (k_points, NB_MAPS)
    bw = rng.uniform(0.25, 3., size=shape).astype(F32)
    p = rng.uniform(0.02, 0.98, size=shape + (length,))
    return bw, p


@pytest.mark.parametrize('length', LENGTHS)
def test_thresholds(length):
    (bw, p) = point(length, 10 + length)
    used = min(length, rc.RDO_MAGNITUDES)
    t = rc.rdo_thresholds(bw, p, 0.3, idx_map_exception=5)
    assert t.dtype == F32 and t.shape == (NB_MAPS, rc.RDO_MAGNITUDES) and rc.RDO_MAGNITUDES == 16
    assert not t[5].any() and not t[:, used:].any()
    bits = rc.magnitude_bits(p)
    saved = bits[:, 1:used + 1] - bits[:, :used]
    expected = numpy.where(saved > 0., 0.3*saved/(bw.astype(numpy.float64)**2)[:, None], 0.).astype(F32)
    expected[5] = 0.
    assert numpy.array_equal(t[:, :used], expected)
    assert (t[:, :used] > 0.).any() and (t >= 0.).all()
    assert not rc.rdo_thresholds(bw, p, 0., idx_map_exception=5).any()
    assert rc.rdo_thresholds(bw, p, 0.).dtype == F32
    # no exception map: every row of a busy table has a threshold
    free = rc.rdo_thresholds(bw, p, 0.3)
    assert free[5].any() and numpy.array_equal(numpy.delete(free, 5, axis=0), numpy.delete(t, 5, axis=0))
    assert numpy.array_equal(rc.rdo_thresholds(bw, p, 0.3, idx_map_exception=NB_MAPS), free)


def test_thresholds_where_a_step_saves_nothing():
    """B(1) - B(0) is what lowering a 1 to a 0 saves. With p[0] = 0.01 a zero costs 6.6 bits and a one 2.0 (0.01 + 1 + the sign):
    the step saves nothing and its threshold is 0, while the step from 2 to 1 still has one."""
    p = numpy.full((NB_MAPS, 3), 0.5)
    p[:, 0] = 0.01
    bits = rc.magnitude_bits(p)
    assert (bits[:, 1] < bits[:, 0]).all()
    t = rc.rdo_thresholds(numpy.ones(NB_MAPS, dtype=F32), p, 1.)
    assert not t[:, 0].any() and (t[:, 1] > 0.).all()


def test_thresholds_take_points():
    (bw, p) = point(10, 3, k_points=4)
    t = rc.rdo_thresholds(bw, p, 0.7, idx_map_exception=100)
    assert t.shape == (4, NB_MAPS, 16) and t.dtype == F32
    for k in range(4):
        assert numpy.array_equal(t[k], rc.rdo_thresholds(bw[k], p[k], 0.7, idx_map_exception=100))


@pytest.mark.parametrize('value', [-1e-9, -1., float('nan'), float('inf'), -float('inf')])
def test_thresholds_refuse(value):
    (bw, p) = point(10, 4)
    with pytest.raises(ValueError):
        rc.rdo_thresholds(bw, p, value)


def laplacian_case(length, bin_width, seed, size=2048):
    """(y (size, 128), bw, mean, tables fitted on the nearest-rounded symbols): map c has scale 0.3 .. 20 bins."""
    rng = numpy.random.RandomState(seed)
    scales = numpy.exp(numpy.linspace(numpy.log(0.3), numpy.log(20.), NB_MAPS))
    bw = numpy.full(NB_MAPS, bin_width, dtype=F32)
    mean = (rng.standard_normal(NB_MAPS)*0.1).astype(F32)
    y = (rng.laplace(size=(size, NB_MAPS))*scales*bin_width).astype(F32) + mean
    nearest = numpy.rint((y - mean)/bw)
    clipped = numpy.minimum(numpy.abs(nearest), length).astype(numpy.int64)
    hist = numpy.stack([numpy.bincount(clipped[:, c], minlength=length + 1) for c in range(NB_MAPS)])
    (zeros, ones) = rc.decision_counts(hist)
    return y, bw, mean, rc.probabilities_from_counts(zeros, ones), nearest.astype(F32)


@pytest.mark.parametrize('length', LENGTHS)
def test_every_result_is_the_nearest_symbol_or_one_step_towards_zero(length):
    (y, bw, mean, p, nearest) = laplacian_case(length, 1., 20 + length)
    assert numpy.array_equal(rc.rdo_quantize_numpy(y, bw, mean, rc.rdo_thresholds(bw, p, 0.), length), nearest)
    r = rc.rdo_quantize_numpy(y, bw, mean, rc.rdo_thresholds(bw, p, 0.5), length)
    assert r.dtype == F32
    moved = r != nearest
    assert moved.any()
    assert numpy.array_equal(r[moved], nearest[moved] - numpy.sign(nearest[moved]))
    magnitude = numpy.abs(nearest[moved])
    assert magnitude.min() >= 1 and magnitude.max() <= min(length, 16)
    assert ((numpy.sign(r[moved]) == numpy.sign(nearest[moved])) | (r[moved] == 0.)).all()


def test_special_values_are_left_alone():
    bw = numpy.ones(NB_MAPS, dtype=F32)
    t = numpy.full((NB_MAPS, 16), 100., dtype=F32)                  # every eligible element is lowered
    y = numpy.zeros((2, NB_MAPS), dtype=F32)
    y[0, :8] = [numpy.nan, numpy.inf, -numpy.inf, 40000., -40000., 3e38, 17., -16.]
    r = rc.rdo_quantize_numpy(y, bw, None, t, 40)
    assert numpy.isnan(r[0, 0]) and numpy.array_equal(r[0, 1:8], numpy.array([numpy.inf, -numpy.inf, 40000., -40000., 3e38, 17., -15.], dtype=F32))
    assert not r[1].any()


def test_the_rule_against_brute_force():
    """Figures of one run: 3,145,728 elements, 1,885,528 eligible of which 493,273 lowered, 18 left out as ties, 0 disagreements."""
    (total, eligible_total, left_out, wrong, lowered) = (0, 0, 0, 0, 0)
    length = 10
    for (seed, bin_width) in enumerate((0.37, 1., 2.5)):
        (y, bw, mean, p, nearest) = laplacian_case(length, bin_width, 40 + seed)
        bits = rc.magnitude_bits(p)                                  # (128, L + 1)
        x = numpy.abs((y.astype(numpy.float64) - mean)/bw)
        a = numpy.abs(nearest).astype(numpy.int64)
        eligible = (a >= 1) & (a <= min(length, 16))
        index = numpy.where(eligible, a, 1)
        maps = numpy.arange(NB_MAPS)
        width2 = float(bin_width)**2
        for rdo_lambda in (0.01, 0.1, 0.5, 3.):
            r = rc.rdo_quantize_numpy(y, bw, mean, rc.rdo_thresholds(bw, p, rdo_lambda), length)
            stay = (x - index)**2*width2 + rdo_lambda*bits[maps, index]
            step = (x - (index - 1))**2*width2 + rdo_lambda*bits[maps, index - 1]
            tie = numpy.abs(stay - step) <= 1e-5*width2
            chose_step = numpy.abs(r) == numpy.abs(nearest) - 1.
            assert numpy.array_equal(r[~eligible], nearest[~eligible])
            judged = eligible & ~tie
            wrong += int((chose_step != (step < stay))[judged].sum())
            left_out += int((eligible & tie).sum())
            eligible_total += int(eligible.sum())
            lowered += int(chose_step[eligible].sum())
            total += y.size
    print('elements {0}, eligible {1}, left out {2}, disagreements {3}, lowered {4}'.format(total, eligible_total, left_out, wrong, lowered))
    assert total >= 3000000 and lowered > eligible_total//100
    assert wrong == 0
    assert left_out <= total//10000
