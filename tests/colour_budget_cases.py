"""What tests/test_gpu_colour_budget_container.py and tests/test_gpu_colour_budget_codec.py share (a plain helper module: import it, no
fixture lives here): the ladders, the pictures, the numpy statement of the rule of DESIGN.md section 29 on a table of bounds, and the
budgets both modules build from the bounds of a first call.

Pictures of 50 x 83 (Y coded at 64 x 96, chroma 25 x 42 coded at 32 x 48) and of 64 x 96 (no plane needs a pad), the trained-like models
of tests/test_gpu_frame_container.py with fixed and learned bin widths, ladders of K = 2 and 3 points built like the one of
tests/test_gpu_frame_codec.py (the model's bin widths times 1, 2, 4; the same table at every point), L = 10 with exception map 67 and
L = 3 without."""
import numpy

from test_gpu_colour_container import pictures_of
from test_gpu_frame_container import RATES

HEADER = 48
SHARES = (0.25, 0.6, 0.9)
# name: (learned bin widths, rate, K, picture size, N, chroma at doubled bin widths, a ladder with a price)
CONFIGS = {
    'fixed_L10_exception_K3_50x83_N3': (False, 'L10_exception_67', 3, (50, 83), 3, False, False),
    'learned_L3_K2_64x96_N2': (True, 'L3_no_exception', 2, (64, 96), 2, False, False),
    'learned_L10_exception_K2_50x83_N2_chroma_doubled': (True, 'L10_exception_67', 2, (50, 83), 2, True, False),
    'fixed_L3_K3_64x96_N3_priced': (False, 'L3_no_exception', 3, (64, 96), 3, False, True),
}


def ladders_of(models, config):
    """(the luminance ladder, the chroma ladder or None) of a configuration."""
    from autoencoder_based_image_compression_amd import ratecontrol
    (learned, rate, nb_points, _, _, doubled, priced) = CONFIGS[config]
    (length, idx_map_exception) = RATES[rate]
    m = models[learned]
    multipliers = numpy.array([1., 2., 4.][:nb_points], dtype=numpy.float32)
    tables = numpy.stack([models['probabilities'][:, :length]]*nb_points)

    def ladder(scale):
        widths = (m['bin_widths'][None]*(multipliers*numpy.float32(scale))[:, None]).astype(numpy.float32)
        price = 0.02*(multipliers.astype(numpy.float64)*scale)**2 if priced else None
        return ratecontrol.RateLadder(widths, tables, m['map_mean'], idx_map_exception, rdo_lambda=price)

    return (ladder(1.), ladder(2.) if doubled else None)


def pictures(config, seed=0):
    (_, _, _, size, count, _, _) = CONFIGS[config]
    return pictures_of(size, seed, count)


def rule(upper, valid, budgets, share):
    """The rule on bounds alone: upper int64 (N, 3, K) and valid bool (N, 3, K) in the order Y, Cb, Cr -> (rate_point (N, 3),
    plane budgets (N, 3), plane promises (N, 3)), with the functions of ratecontrol.py."""
    from autoencoder_based_image_compression_amd import ratecontrol
    budgets = numpy.broadcast_to(numpy.asarray(budgets, dtype=numpy.int64), (upper.shape[0],))
    c = ratecontrol.colour_chroma_budgets(budgets, share)
    (point_cb, promised_cb) = ratecontrol.select_by_upper_bound(upper[:, 1], valid[:, 1], c)
    (point_cr, promised_cr) = ratecontrol.select_by_upper_bound(upper[:, 2], valid[:, 2], c)
    r = ratecontrol.colour_luma_budgets(budgets, upper[:, 1], point_cb, upper[:, 2], point_cr)
    (point_y, promised_y) = ratecontrol.select_by_upper_bound(upper[:, 0], valid[:, 0], r)
    return (numpy.stack([point_y, point_cb, point_cr], axis=1), numpy.stack([r, c, c], axis=1),
            numpy.stack([promised_y, promised_cb, promised_cr], axis=1))


def exact_budget(upper, valid, i, share, luma_point):
    """For picture i: a budget B = 48 + the three bounds of a triple (luma_point, kcb, kcr) at which the rule takes exactly that
    triple, all three promised, and at B - 1 the same chroma points -> (B, (luma_point, kcb, kcr)), or None when no chroma pair is
    consistent with the budget it makes at this share."""
    nb_points = upper.shape[2]
    one = (upper[i:i + 1], valid[i:i + 1])
    for kcb in range(nb_points):
        for kcr in range(nb_points):
            budget = HEADER + int(upper[i, 0, luma_point]) + int(upper[i, 1, kcb]) + int(upper[i, 2, kcr])
            (points, _, promised) = rule(*one, budget, share)
            (points_under, _, _) = rule(*one, budget - 1, share)
            if points[0].tolist() == [luma_point, kcb, kcr] and promised[0].all() and points_under[0, 1:].tolist() == [kcb, kcr]:
                return (budget, (luma_point, kcb, kcr))
    return None


def exact_budgets(upper, valid, share, shift=0):
    """One budget per picture by `exact_budget`, picture i aiming at luminance point (i + shift) % K -> (budgets int64 (N,), the
    triples), or None when some picture has none at this share."""
    (budgets, triples) = ([], [])
    for i in range(upper.shape[0]):
        found = exact_budget(upper, valid, i, share, (i + shift) % upper.shape[2])
        if found is None:
            return None
        budgets.append(found[0])
        triples.append(found[1])
    return (numpy.array(budgets, dtype=numpy.int64), triples)


def spill_budgets(upper, valid, share):
    """One budget per picture at which the bytes chroma did not use move Y at least one point finer than the even split (Y given
    P - 2 c, whatever chroma took) would: searched among the sums of three bounds and the values just around them -> int64 (N,), or None
    when some picture has none at this share."""
    from autoencoder_based_image_compression_amd import ratecontrol
    nb_points = upper.shape[2]
    out = []
    for i in range(upper.shape[0]):
        one = (upper[i:i + 1], valid[i:i + 1])
        sums = sorted({HEADER + int(upper[i, 0, a]) + int(upper[i, 1, b]) + int(upper[i, 2, c]) + d
                       for a in range(nb_points) for b in range(nb_points) for c in range(nb_points) for d in (0, 1, 64)})
        for budget in sums:
            (points, plane_budgets, _) = rule(*one, budget, share)
            even = max(budget - HEADER, 0) - 2*int(plane_budgets[0, 1])
            (even_point, _) = ratecontrol.select_by_upper_bound(upper[i:i + 1, 0], valid[i:i + 1, 0], even)
            if points[0, 0] < even_point[0]:
                out.append(budget)
                break
        else:
            return None
    return numpy.array(out, dtype=numpy.int64)
