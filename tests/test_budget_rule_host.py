"""The integer selection rule of `codec.BudgetCodec` on the host (ratecontrol.fixed_costs, log2_tables, upper_bounds_fixed,
select_by_upper_bound: DESIGN.md section 19), and the inventory of `codec._BudgetSlot` against tests/budget_slot_buffers.py.
CPU only, numpy only.

The bound that is asserted: 0 <= upper_bounds_fixed - blob_byte_bounds(...)[1] <= 128 bytes per blob. Every cost of the fixed-point
rule is rounded up by less than 2^-20 bit per decision, i.e. by less than one bit per map while map_size * L <= 2^19 (the largest case
here: 16384 * 33 = 2^19.04, two bits at most), which the rounding of the stream to whole bytes turns into one byte per map at most."""
import functools
import os

import numpy
import pytest

import budget_slot_buffers
import ratecontrol_slot_buffers
import slot_buffers
from test_slot_inventory import _with_one_more_buffer, assigned_attributes

from autoencoder_based_image_compression_amd import ratecontrol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODEC = os.path.join(ROOT, 'autoencoder_based_image_compression_amd', 'codec.py')
NB_MAPS = 128
LENGTHS = (1, 3, 10, 33)
MAP_SIZES = (12, 143, 16384)
K = 3


def clipped_histograms(magnitudes, length):
    """int64 (..., map_size) magnitudes -> (..., L + 1) histograms clipped at L."""
    clipped = numpy.minimum(magnitudes, length)
    return numpy.stack([(clipped == b).sum(axis=-1) for b in range(length + 1)], axis=-1).astype(numpy.int64)


@functools.lru_cache(maxsize=None)
def case(length, map_size, exception):
    """(ladder, hist (N, K, 128, L + 1), bypass bits): seeded Laplacian symbols at scales from 0.05 to 6 over the maps, the points
    1 / 2 / 4 times as coarse; tables fitted on the counts of all images (`probabilities_from_counts`: clamps included).
    Map 3 of image 0 is all zeros at every point. The exception map (7) of image 0 has no zero at decision 0 (zeros == 0, point 0), of
    image 1 only zeros and ones (ones == 0 at decision 1; t == 0 from decision 2 on), of image 2 Laplacian symbols."""
    rng = numpy.random.RandomState(1000*length + map_size + (7 if exception >= 0 else 0))
    n = 3
    scales = numpy.geomspace(0.05, 6., NB_MAPS)[None, None, :, None]/numpy.array([1., 2., 4.])[None, :, None, None]
    magnitudes = numpy.abs(numpy.rint(rng.laplace(size=(n, 1, NB_MAPS, map_size))*scales)).astype(numpy.int64)
    magnitudes[0, :, 3] = 0
    if exception >= 0:
        magnitudes[0, 0, exception] = 1 + rng.randint(0, 3, size=map_size)
        magnitudes[1, :, exception] = rng.randint(0, 2, size=map_size)
    hist = clipped_histograms(magnitudes, length)
    suffix = numpy.maximum(magnitudes - length + 1, 1)
    bypass = ((magnitudes != 0) + numpy.where(magnitudes >= length, 2*numpy.floor(numpy.log2(suffix)).astype(numpy.int64) + 1, 0)).sum(axis=-1)
    (zeros, ones) = ratecontrol.decision_counts(hist.sum(axis=0))
    tables = ratecontrol.probabilities_from_counts(zeros, ones)
    ladder = ratecontrol.RateLadder(numpy.ones((K, NB_MAPS), dtype=numpy.float32)*numpy.array([[1.], [2.], [4.]], dtype=numpy.float32),
                                    tables, numpy.zeros(NB_MAPS, dtype=numpy.float32), exception)
    return ladder, hist, bypass


@pytest.mark.parametrize('exception', [-1, 7], ids=['no_exception', 'exception'])
@pytest.mark.parametrize('map_size', MAP_SIZES)
@pytest.mark.parametrize('length', LENGTHS)
def test_upper_bounds_fixed_against_the_float_bound(length, map_size, exception):
    (ladder, hist, bypass) = case(length, map_size, exception)
    assert not hist[0, :, 3, 1:].any() and (hist[0, :, 3, 0] == map_size).all()          # the all-zero map
    if exception >= 0:
        (zeros, ones) = ratecontrol.decision_counts(hist[:, :, exception])
        assert zeros[0, 0, 0] == 0 and ones[0, 0, 0] > 0                                 # zeros == 0
        if length > 1:
            assert ones[1, 0, 1] == 0 and zeros[1, 0, 1] > 0                             # ones == 0
        if length > 2:
            assert zeros[1, 0, 2] == 0 and ones[1, 0, 2] == 0                            # t == 0
    fixed = ratecontrol.upper_bounds_fixed(hist, bypass, ladder, map_size)
    reference = ratecontrol.blob_byte_bounds(hist, bypass, ladder, 16, 16*map_size)[1]
    assert fixed.dtype == numpy.int64 and fixed.shape == reference.shape == (3, K)
    difference = fixed - reference
    print('L', length, 'map_size', map_size, 'difference', difference.min(), difference.max())
    assert difference.min() >= 0
    assert difference.max() <= NB_MAPS


def test_upper_bounds_fixed_refuses_what_it_cannot_index():
    (ladder, hist, bypass) = case(3, 12, 7)
    with pytest.raises(ValueError):
        ratecontrol.upper_bounds_fixed(hist, bypass, ladder, 11)
    with pytest.raises(ValueError):
        ratecontrol.upper_bounds_fixed(hist[:, :2], bypass[:, :2], ladder, 12)


def test_fixed_costs_at_the_ends_of_the_interval():
    smallest = numpy.nextafter(0., 1.)
    largest = numpy.nextafter(1., 0.)
    p = numpy.full((1, NB_MAPS, 3), 0.5)
    p[0, 0] = (0.5, smallest, largest)
    ladder = ratecontrol.RateLadder(numpy.ones((1, NB_MAPS), dtype=numpy.float32), p, numpy.zeros(NB_MAPS, dtype=numpy.float32))
    costs = ratecontrol.fixed_costs(ladder)
    assert costs.dtype == numpy.uint32 and costs.shape == (1, NB_MAPS, 3, 2)
    assert costs[0, 0, 0].tolist() == [1 << 20, 1 << 20]
    assert (costs[0, 1:] == 1 << 20).all()
    assert costs[0, 0, 1].tolist() == [1074 << 20, 0]                  # -log2(2^-1074); 1 - p rounds to 1
    assert costs[0, 0, 2].tolist() == [1, 53 << 20]                    # a cost is never rounded down to nothing; 1 - p = 2^-53
    assert int(costs.max()) < 2**32
    assert ratecontrol.C99 == 15204 and ratecontrol.FIXED_ONE == 1 << 20


def test_log2_tables():
    tables = ratecontrol.log2_tables(1025)
    assert tables.dtype == numpy.uint32 and tables.shape == (2, 1026)
    assert tables[:, 0].tolist() == [0, 0] and tables[:, 1].tolist() == [0, 0]
    for e in range(1, 11):
        assert tables[:, 1 << e].tolist() == [e << 20, e << 20]
    others = numpy.array([n for n in range(3, 1026) if n & (n - 1)])
    assert (tables[0, others] == tables[1, others] + 1).all()
    assert (numpy.diff(tables[1].astype(numpy.int64)) >= 0).all()
    assert tables[:, 3].tolist() == [1661954, 1661953]                 # log2(3) * 2^20 = 1661953.6...
    with pytest.raises(ValueError):
        ratecontrol.log2_tables(0)


def test_select_by_upper_bound_at_and_under_every_bound():
    rng = numpy.random.RandomState(5)
    (n, k) = (6, 4)
    upper = numpy.sort(rng.randint(5000, 90000, size=(n, k)), axis=1)[:, ::-1].astype(numpy.int64)      # finest first: the largest
    valid = numpy.ones((n, k), dtype=bool)
    for j in range(k):
        (point, promised) = ratecontrol.select_by_upper_bound(upper, valid, upper[:, j])
        assert point.dtype == numpy.int64 and promised.dtype == bool
        assert numpy.array_equal(point, numpy.full(n, j)) and promised.all()
        (point, promised) = ratecontrol.select_by_upper_bound(upper, valid, upper[:, j] - 1)
        if j + 1 < k:
            assert numpy.array_equal(point, numpy.full(n, j + 1)) and promised.all()
        else:
            assert numpy.array_equal(point, numpy.full(n, k - 1)) and not promised.any()      # no fitting point: the last valid one
    # a scalar budget
    (point, promised) = ratecontrol.select_by_upper_bound(upper, valid, int(upper[:, 1].max()))
    assert (point <= 1).all() and promised.all()


def test_select_by_upper_bound_skips_invalid_points():
    upper = numpy.array([[10, 50, 40, 30], [100, 90, 80, 70], [100, 90, 80, 70], [10, 10, 10, 10]], dtype=numpy.int64)
    valid = numpy.array([[False, True, True, True],        # an invalid point (that would fit) in front of a fitting one
                         [True, True, False, False],       # no fitting point: the last VALID one
                         [True, True, True, True],
                         [False, False, False, False]])    # no valid point: K - 1, not promised
    (point, promised) = ratecontrol.select_by_upper_bound(upper, valid, numpy.array([45, 60, 85, 1000]))
    assert point.tolist() == [2, 1, 2, 3]
    assert promised.tolist() == [True, False, True, False]
    with pytest.raises(ValueError):
        ratecontrol.select_by_upper_bound(upper, valid[:, :3], 10)
    with pytest.raises(ValueError):
        ratecontrol.select_by_upper_bound(upper, valid, numpy.zeros((4, 4)))


def test_the_rule_is_not_select_rate_points():
    """An image with lower <= budget < upper at a point goes one point on, where `select_rate_points` would try the point."""
    lower = numpy.array([[80, 40]])
    upper = numpy.array([[100, 50]])
    valid = numpy.ones((1, 2), dtype=bool)
    tried = ratecontrol.select_rate_points(lower, upper, valid, 90, lambda i, k: (85, 45)[k])
    assert tried['rate_point'].tolist() == [0] and tried['fits'].all()
    (point, promised) = ratecontrol.select_by_upper_bound(upper, valid, 90)
    assert point.tolist() == [1] and promised.all()


# ---- the inventory of codec._BudgetSlot ------------------------------------------------------------------------------------------

def _source():
    with open(CODEC) as f:
        return f.read()


def _unclassified(source):
    known = {slot_buffers.attribute_of(name) for name in budget_slot_buffers.BUDGET_SLOT}
    return sorted(assigned_attributes(source, '_BudgetSlot') - known)


def test_every_attribute_of_the_budget_slot_is_classified():
    assert {'accum', 'hist', 'pinned_budgets', 'select', 'prob_row', 'table', 'exception_rows'} <= assigned_attributes(_source(), '_BudgetSlot')
    assert _unclassified(_source()) == []


def test_every_entry_of_the_budget_slot_exists_and_says_why():
    # (a reason names a line or a step of DESIGN.md section 19's launch table: `needs_digit`)
    ratecontrol_slot_buffers.check_entries(budget_slot_buffers.BUDGET_SLOT, assigned_attributes(_source(), '_BudgetSlot'),
                                           budget_slot_buffers.MUST_BE_SCRATCH, ('budgets_nbytes', 'points_table'), needs_digit=True)
    assert all(entry.alias is None for entry in budget_slot_buffers.BUDGET_SLOT.values())


def test_an_unclassified_buffer_of_the_budget_slot_is_noticed():
    grown = _with_one_more_buffer(_source(), '_BudgetSlot')
    assert _unclassified(grown) == ['extra']


def test_the_slot_itself_did_not_grow():
    """`_BudgetSlot` exists so that `_Slot` keeps its attributes: tests/slot_buffers.py still classifies all of them."""
    known = {slot_buffers.attribute_of(name) for name in slot_buffers.SLOT}
    assert assigned_attributes(_source(), '_Slot') <= known
