"""The integer rule of `codec.QualityCodec` on the host (ratecontrol.max_sse_for_psnr, quality_rounds, select_by_quality: DESIGN.md
section 21), and the inventory of `codec._QualitySlot` against tests/quality_slot_buffers.py. CPU only, numpy only.

`select_by_quality` is held against two statements written here: on tables that do not decrease along the ladder, "the last k >=
first with sse[k] <= max_sse, else first, not met"; on any table, a literal restatement of the loop."""
import os

import numpy
import pytest

import quality_slot_buffers
import ratecontrol_slot_buffers
import slot_buffers
from test_slot_inventory import _with_one_more_buffer, assigned_attributes

from autoencoder_based_image_compression_amd import ratecontrol
from autoencoder_based_image_compression_amd.kodak.tools import tools as tls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODEC = os.path.join(ROOT, 'autoencoder_based_image_compression_amd', 'codec.py')
PIXEL_COUNTS = (1, 176*208, 512*768)


def meets(sse, nb_pixels, target):
    return sse == 0 or tls.psnr_from_sse(sse, nb_pixels) >= target


@pytest.mark.parametrize('nb_pixels', PIXEL_COUNTS)
def test_max_sse_is_the_largest_squared_error_that_keeps_the_target(nb_pixels):
    targets = numpy.sort(numpy.random.RandomState(nb_pixels % 1000).uniform(5., 60., size=200))
    values = ratecontrol.max_sse_for_psnr(targets, nb_pixels)
    assert values.dtype == numpy.int64 and values.shape == (200,)
    for (target, s) in zip(targets.tolist(), values.tolist()):
        assert s >= 0 and meets(s, nb_pixels, target), (target, s)
        assert s == ratecontrol.MAX_SSE_SATURATION or not meets(s + 1, nb_pixels, target), (target, s)
        scalar = ratecontrol.max_sse_for_psnr(target, nb_pixels)
        assert isinstance(scalar, numpy.int64) and int(scalar) == s
    assert (numpy.diff(values) <= 0).all()                     # non-increasing in the target
    assert values[0] > values[-1]
    assert values.max() < ratecontrol.MAX_SSE_SATURATION      # nothing saturates between 5 and 60 dB


def test_max_sse_at_the_ends():
    # one pixel: psnr_from_sse(1, 1) = 20 log10(255) = 48.13 dB, so a target above it is met by a squared error of 0 only
    assert tls.psnr_from_sse(1, 1) < 48.2
    assert int(ratecontrol.max_sse_for_psnr(48.2, 1)) == 0 and int(ratecontrol.max_sse_for_psnr(48.1, 1)) == 1
    assert int(ratecontrol.max_sse_for_psnr(1000., 512*768)) == 0
    assert ratecontrol.max_sse_for_psnr([1000., 1e300], [1, 512*768]).tolist() == [0, 0]
    # a target no image can miss saturates
    assert int(ratecontrol.max_sse_for_psnr(-1000., 1)) == ratecontrol.MAX_SSE_SATURATION == 1 << 62
    # targets and pixel counts broadcast
    both = ratecontrol.max_sse_for_psnr([[30.], [40.]], [100, 200])
    assert both.shape == (2, 2) and both[0, 1] == ratecontrol.max_sse_for_psnr(30., 200)
    for bad in (numpy.nan, numpy.inf, -numpy.inf, [30., numpy.nan]):
        with pytest.raises(ValueError, match='finite'):
            ratecontrol.max_sse_for_psnr(bad, 100)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='nb_pixels'):
            ratecontrol.max_sse_for_psnr(30., bad)


def test_quality_rounds():
    for k in range(1, 65):
        rounds = ratecontrol.quality_rounds(k)
        assert 2**rounds >= k + 1 > 2**(rounds - 1), k        # ceil(log2(k + 1)) without a logarithm
    assert [ratecontrol.quality_rounds(k) for k in (1, 2, 3, 4, 9)] == [1, 2, 2, 3, 4]
    with pytest.raises(ValueError):
        ratecontrol.quality_rounds(0)


def restated_loop(row, first, max_sse):
    """The issue's steps, literally, for one image."""
    k_points = len(row)
    (L, R) = (first - 1, k_points)
    (points, values) = ([], [])
    for _ in range(ratecontrol.quality_rounds(k_points)):
        if R - L > 1:
            mid = (L + R) >> 1
            (points, values) = (points + [mid], values + [row[mid]])
            if row[mid] <= max_sse:
                L = mid
            else:
                R = mid
        else:
            (points, values) = (points + [max(L, first)], values + [row[max(L, first)]])
    return (L if L >= first else first), L >= first, points, values


def thresholds_of(row):
    return sorted({v + d for v in row for d in (-1, 0, 1)})


@pytest.mark.parametrize('k_points', range(1, 10))
def test_select_by_quality_against_the_two_statements(k_points):
    rng = numpy.random.RandomState(40 + k_points)
    tables = []
    for _ in range(6):
        steps = rng.randint(0, 4, size=k_points)              # ties included
        tables.append((True, (10 + numpy.cumsum(steps)).astype(numpy.int64)))
        tables.append((False, rng.randint(0, 30, size=k_points).astype(numpy.int64)))
    checked = 0
    for (monotone, row) in tables:
        cases = [(first, t) for first in range(k_points) for t in thresholds_of(row.tolist())]
        sse = numpy.tile(row, (len(cases), 1))
        first = numpy.array([c[0] for c in cases], dtype=numpy.int64)
        max_sse = numpy.array([c[1] for c in cases], dtype=numpy.int64)
        (point, met, probe_points, probe_sse) = ratecontrol.select_by_quality(sse, first, max_sse)
        assert point.dtype == numpy.int64 and met.dtype == bool and probe_points.dtype == numpy.int64 and probe_sse.dtype == numpy.int64
        assert probe_points.shape == probe_sse.shape == (len(cases), ratecontrol.quality_rounds(k_points))
        for (i, (f, t)) in enumerate(cases):
            assert (point[i], met[i], probe_points[i].tolist(), probe_sse[i].tolist()) == restated_loop(row.tolist(), f, t), (row, f, t)
            assert all(f <= k < k_points for k in probe_points[i].tolist()) and point[i] in probe_points[i], (row, f, t)
            assert probe_sse[i].tolist() == [row[k] for k in probe_points[i].tolist()]
            if monotone:
                fitting = [k for k in range(f, k_points) if row[k] <= t]
                assert (int(point[i]), bool(met[i])) == ((fitting[-1], True) if fitting else (f, False)), (row, f, t)
            else:
                assert not met[i] or row[point[i]] <= t                  # a point that is taken as met did meet the threshold
            checked += 1
    assert checked >= 12*k_points*2


def test_select_by_quality_refuses_what_it_cannot_index():
    sse = numpy.arange(6, dtype=numpy.int64).reshape(2, 3)
    ok = (numpy.zeros(2, dtype=numpy.int64), numpy.zeros(2, dtype=numpy.int64))
    for (first, max_sse) in ((numpy.array([0, 3]), ok[1]), (numpy.array([-1, 0]), ok[1]), (numpy.zeros(3, dtype=numpy.int64), ok[1]),
                             (ok[0], numpy.zeros(2)), (numpy.zeros(2), ok[1])):
        with pytest.raises(ValueError):
            ratecontrol.select_by_quality(sse, first, max_sse)
    with pytest.raises(ValueError):
        ratecontrol.select_by_quality(sse.astype(numpy.float64), *ok)
    with pytest.raises(ValueError):
        ratecontrol.select_by_quality(sse[0], *ok)


def test_a_table_that_is_not_monotone_gives_the_bisection_its_own_outcome():
    """What the docstring promises: a point that met the threshold, though a coarser one does too; or `first`, not met, though a point
    the search did not probe would have met it."""
    assert 'ASSUMED AND NOT CHECKED' in ratecontrol.select_by_quality.__doc__ and 'not monotone' in ratecontrol.select_by_quality.__doc__
    sse = numpy.array([[5, 9, 5, 9, 9, 9, 5, 9, 9]], dtype=numpy.int64)
    (point, met, probe_points, _) = ratecontrol.select_by_quality(sse, numpy.array([0]), numpy.array([5]))
    assert (point.tolist(), met.tolist(), probe_points.tolist()) == ([0], [True], [[4, 1, 0, 0]])           # points 2 and 6 meet it too
    sse = numpy.array([[9, 9, 5, 9, 9, 9, 5, 9, 9]], dtype=numpy.int64)
    (point, met, probe_points, _) = ratecontrol.select_by_quality(sse, numpy.array([0]), numpy.array([5]))
    assert (point.tolist(), met.tolist(), probe_points.tolist()) == ([0], [False], [[4, 1, 0, 0]])          # points 2 and 6 would have met it
    (point, met, probe_points, _) = ratecontrol.select_by_quality(sse, numpy.array([2]), numpy.array([5]))
    assert (point.tolist(), met.tolist(), probe_points.tolist()) == ([2], [True], [[5, 3, 2, 2]])


# ---- the inventory of codec._QualitySlot -----------------------------------------------------------------------------------------

def _source():
    with open(CODEC) as f:
        return f.read()


def _unclassified(source):
    known = {slot_buffers.attribute_of(name) for name in quality_slot_buffers.QUALITY_SLOT}
    return sorted(assigned_attributes(source, '_QualitySlot') - known)


def test_every_attribute_of_the_quality_slot_is_classified():
    assert {'accum', 'select', 'first', 'point', 'met', 'state', 'trace_point', 'trace_sse', 'pinned_max_sse', 'max_sse', 'probe_acc',
            'probe_latent', 'prob_row', 'table'} <= assigned_attributes(_source(), '_QualitySlot')
    assert _unclassified(_source()) == []


def test_every_entry_of_the_quality_slot_exists_and_says_why():
    table = quality_slot_buffers.QUALITY_SLOT
    ratecontrol_slot_buffers.check_entries(table, assigned_attributes(_source(), '_QualitySlot'), quality_slot_buffers.MUST_BE_SCRATCH,
                                           ('budgets_nbytes', 'max_sse_nbytes', 'points_table'))
    assert all(entry.alias is None for entry in table.values())
    assert not any(entry.cls == slot_buffers.CARRIED for entry in table.values())       # a step depends on nothing the last one left


def test_an_unclassified_buffer_of_the_quality_slot_is_noticed():
    assert _unclassified(_with_one_more_buffer(_source(), '_QualitySlot')) == ['extra']


def test_the_other_slots_did_not_grow():
    """`_QualitySlot` exists so that `_Slot` and `_BudgetSlot` keep their attributes: their helpers still classify all of them."""
    import budget_slot_buffers
    assert assigned_attributes(_source(), '_Slot') <= {slot_buffers.attribute_of(name) for name in slot_buffers.SLOT}
    assert assigned_attributes(_source(), '_BudgetSlot') <= {slot_buffers.attribute_of(name) for name in budget_slot_buffers.BUDGET_SLOT}
