"""Rate ladders: what an image costs at each of K rate points, from counts alone, and the choice of a point for a byte budget
(DESIGN.md section 18). Host side, numpy only; the one device call is `device.ladder_histograms`, made by the callers
(`container.encode_images_to_budget`, `kodak.lossless.stats.compute_binary_probabilities_ladder`), which hand its outputs in here
as numpy arrays. The second half of the file is the rule of `codec.BudgetCodec`: the same upper bound in integer
arithmetic, which `eae_hip_ladder_select` restates on the device element for element, and the choice on that bound alone. The end of
the file is the rule of `codec.QualityCodec`: a PSNR floor as an integer bound on the squared error, and the
bisection of the ladder for the coarsest point that keeps it, which `eae_hip_quality_search` restates round by round. Between the two
stands the rule of `codec.ColourBudgetCodec`: how one byte budget is shared between the planes of a picture;
behind `QualityCodec`'s the rule of `codec.ColourQualityCodec`: how one PSNR floor is.

A rate point is a pair: 128 bin widths and a table of binary probabilities (the reference walks nine, `multipliers` of
reconstructing_eae_kodak.py, and learns a point's cost by quantising and coding at it). The coder's cost is a function of the
histogram of |symbol| clipped at the truncated unary length L, per map:
  * the bypass stream's length is exact: one sign bit per non-zero symbol plus the Exp-Golomb suffix of |s| - L from L on
    (LosslessCoder.cpp:22-37, 58-111, 232-252) -- the kernel sums it;
  * the arithmetic-coded stream's length follows the ideal cost -sum zeros[i] log2 p[i] - sum ones[i] log2(1 - p[i]) of the
    binary decisions of stats.py:181-195: from above to within a constant, from below to within a constant on a table that fits the
    data and to within the rounding of the coder's 16-bit interval on any table (the allowances below).
"""
import numpy

NB_MAPS = 128

# How far the arithmetic-coded stream of the host coder (`interface_cython.encode_flattened_map`: 16-bit interval, E1/E2/E3
# rescaling, `stop_encoding`'s closing bits) was seen from the cost of its decisions. MEASURED, NOT PROVEN: profiles/rate_ladder.md
# holds the sweep (`python profiles/rate_ladder.py --sweep`, CPU only): 6670 Laplacian maps of 1 to 16384 symbols, scales 0 (all-zero
# maps) to 12, L = 1, 4, 10, tables fitted on matched data, on 1.5x, 0.1x and 10x mismatched data and on the map itself (with the
# 0.5 / 0.01 / 0.99 clamps that brings), and tables whose every entry is 0.99, 0.01, 0.999 or 0.001.
#   above:  actual - ceil(ideal) <= +2 bits on every map (actual - ideal <= +2.239)                     -> ALLOWANCE_HIGH = 2 + 1
#   below, tables fitted on matched, 1.5x mismatched or own data:  actual - floor(ideal) >= 0 (actual - ideal >= -0.773)
#                                                                                                       -> ALLOWANCE_LOW = 0 + 1
#   below, any table: NO constant holds. The coder gives decision i the share (floor(p R) + 1) / (R + 1) or (R - floor(p R)) / (R + 1)
#   of its interval, R + 1 >= 2^14 wide after rescaling: up to 2^-14 more than p or 1 - p. A table that calls frequent decisions
#   rare (every entry 0.999 on a busy map) therefore codes BELOW the ideal cost in proportion to the stream: -652 bits on 16384
#   symbols, -44 with a table fitted on 10x finer data. `floor_bits` is the cost at the largest shares, p + 2^-14 and 1 - p + 2^-14:
#   actual - floor(floor_bits) >= +1 on every map of the sweep. The lower bound is built on it, since a point is skipped on the lower
#   bound alone; on fitted tables it is 2.5 bits below the ideal cost at 1536 symbols, 26 at 16384.
# The sizes swept end at 16384 symbols per map (a 2048 x 2048 image). `select_rate_points` codes a point before it takes it whatever
# the bounds say, and counts the points the upper bound promised and the coder did not deliver.
ALLOWANCE_LOW = 1
ALLOWANCE_HIGH = 3
INTERVAL_SHARE_EXCESS = 2.**-14

_FIXED_HEADER_BYTES = 28          # container._HEADER.size: 'EAE1', version, flags, sizes, L, exception map index
_TILE_FIELD_BYTES = 4             # container._TILE_HEADER.size - container._HEADER.size: the coding tile of an EAT1 blob, two u16


class RateLadder(object):
    """K rate points in the caller's order of preference, finest first (no monotonicity is assumed: the selection walks the order).
    bin_widths_points float32 (K, 128); binary_probabilities_points float64 (K, 128, L); map_mean float32 (128,); idx_map_exception:
    the map coded with a probability row of its own (container.py), -1 for none.
    rdo_lambda: None, or the price of a bit at every point, in squared latent units per bit as `codec.BatchCodec(rdo_lambda=...)`
    takes it (DESIGN.md sections 23 and 24): a non-negative finite number, or one per point, array-like (K,) -- c * bw_k**2 keeps the
    price the same in bins at every point. A rate point is then 128 bin widths, a table and a price: the symbols of every point are
    those of the rate-distortion optimised quantiser, and whatever chooses a point from this ladder counts, bounds and probes THOSE
    symbols. `rdo_lambdas` float64 (K,) and `rdo_thresholds_points` float32 (K, 128, 16), row k `rdo_thresholds(bin_widths_points[k],
    binary_probabilities_points[k], rdo_lambdas[k], idx_map_exception)`; both None without. 0.0 is a ladder with a price, of zero:
    it takes every launch of one and gives the bytes of None."""

    def __init__(self, bin_widths_points, binary_probabilities_points, map_mean, idx_map_exception=-1, rdo_lambda=None):
        for (name, array, dtype, ndim) in (('bin_widths_points', bin_widths_points, numpy.float32, 2),
                                           ('binary_probabilities_points', binary_probabilities_points, numpy.float64, 3),
                                           ('map_mean', map_mean, numpy.float32, 1)):
            if not isinstance(array, numpy.ndarray) or array.dtype != dtype or array.ndim != ndim:
                raise TypeError('`{0}` must be a {1}-dimensional numpy array of {2}.'.format(name, ndim, numpy.dtype(dtype).name))
        (nb_points, nb_maps) = bin_widths_points.shape
        if nb_points < 1 or nb_maps != NB_MAPS:
            raise ValueError('`bin_widths_points` must be (K, {}) with K >= 1.'.format(NB_MAPS))
        if binary_probabilities_points.shape[:2] != (nb_points, nb_maps) or map_mean.shape != (nb_maps,):
            raise ValueError('`binary_probabilities_points` must be (K, {0}, L) and `map_mean` ({0},).'.format(NB_MAPS))
        length = binary_probabilities_points.shape[2]
        if length < 1 or length > 255:
            raise ValueError('The truncated unary length does not belong to [1, 255].')
        if not (numpy.isfinite(bin_widths_points).all() and (bin_widths_points > 0.).all()):
            raise ValueError('A quantization bin width is not strictly positive.')
        if not ((binary_probabilities_points > 0.) & (binary_probabilities_points < 1.)).all():
            raise ValueError('A binary probability does not belong to ]0, 1[.')
        if not numpy.isfinite(map_mean).all():
            raise ValueError('`map_mean` is not finite.')
        if isinstance(idx_map_exception, bool) or int(idx_map_exception) != idx_map_exception:
            raise TypeError('`idx_map_exception` must be an integer.')
        self.bin_widths_points = numpy.ascontiguousarray(bin_widths_points)
        self.binary_probabilities_points = numpy.ascontiguousarray(binary_probabilities_points)
        self.map_mean = numpy.ascontiguousarray(map_mean)
        # as `container.encode_images`: an index outside the maps means no exception map
        self.idx_map_exception = int(idx_map_exception) if 0 <= idx_map_exception < nb_maps else -1
        self.nb_points = nb_points
        self.truncated_unary_length = length
        self.rdo_lambdas = None
        self.rdo_thresholds_points = None
        if rdo_lambda is not None:
            try:
                lambdas = numpy.array(rdo_lambda, dtype=numpy.float64)
            except (TypeError, ValueError):
                raise ValueError('`rdo_lambda` must be None, a number or one number per point.')
            if isinstance(rdo_lambda, (bool, numpy.bool_)) or lambdas.ndim > 1 or (lambdas.ndim == 1 and lambdas.shape[0] != nb_points):
                raise ValueError('`rdo_lambda` must be None, a number or one number per point, (K,).')
            lambdas = numpy.ascontiguousarray(numpy.broadcast_to(lambdas, (nb_points,)))
            if not numpy.isfinite(lambdas).all() or (lambdas < 0.).any():
                raise ValueError('`rdo_lambda` must be finite and not negative at every point.')
            self.rdo_lambdas = lambdas
            # (rdo_thresholds defined below: looked up when a ladder is made)
            self.rdo_thresholds_points = numpy.ascontiguousarray(numpy.stack([
                rdo_thresholds(self.bin_widths_points[k], self.binary_probabilities_points[k], lambdas[k], self.idx_map_exception)
                for k in range(nb_points)]))


def decision_counts(hist):
    """Clipped histograms of |symbol| (..., L + 1) (bin L: every |s| >= L) -> (zeros, ones), int64 (..., L): how often decision i of
    the truncated unary prefix is 0 and 1. `stats._decisions_from_hist` of every histogram: a symbol of magnitude a < L is a zero
    of decision a and a one of every decision before it, a symbol from L on a one of all L."""
    hist = numpy.asarray(hist).astype(numpy.int64)
    zeros = hist[..., :-1]
    beyond = numpy.cumsum(hist[..., ::-1], axis=-1)[..., ::-1]          # beyond[..., j] = symbols of magnitude >= j
    return numpy.ascontiguousarray(zeros), numpy.ascontiguousarray(beyond[..., 1:])


def probabilities_from_counts(zeros, ones):
    """stats.py:56-66: zeros / (zeros + ones) in float64, 0 / 0 -> 0.5, 0 -> 0.01, 1 -> 0.99."""
    total = (zeros + ones).astype(numpy.float64)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        p = zeros.astype(numpy.float64)/total
    p[numpy.isnan(p)] = 0.5
    p[p == 0.] = 0.01
    p[p == 1.] = 0.99
    return p


def ideal_bits(zeros, ones, probabilities):
    """-sum zeros[i] log2 p[i] - sum ones[i] log2(1 - p[i]) over the last axis, float64."""
    return -(zeros*numpy.log2(probabilities) + ones*numpy.log2(1. - probabilities)).sum(axis=-1)


def floor_bits(zeros, ones, probabilities):
    """`ideal_bits` with every decision at the largest share of the interval the coder can give it, p + 2^-14 or 1 - p + 2^-14
    (at most 1): what the stream costs at least, up to its closing bits, whatever the table (ALLOWANCE_LOW, above)."""
    share_zero = numpy.minimum(probabilities + INTERVAL_SHARE_EXCESS, 1.)
    share_one = numpy.minimum(1. - probabilities + INTERVAL_SHARE_EXCESS, 1.)
    return -(zeros*numpy.log2(share_zero) + ones*numpy.log2(share_one)).sum(axis=-1)


def _check_counts(hist, bypass_bits, ladder):
    hist = numpy.asarray(hist)
    bypass_bits = numpy.asarray(bypass_bits)
    if hist.ndim != 4 or hist.shape[1:] != (ladder.nb_points, NB_MAPS, ladder.truncated_unary_length + 1):
        raise ValueError('`hist` must be (N, K, {}, L + 1) for the K points and the L of the ladder.'.format(NB_MAPS))
    if bypass_bits.shape != hist.shape[:3]:
        raise ValueError('`bypass_bits` must be (N, K, {}).'.format(NB_MAPS))
    return hist, bypass_bits.astype(numpy.int64)


def estimate_bits(hist, bypass_bits, ladder):
    """Outputs of `device.ladder_histograms` (as numpy) -> (ideal arithmetic-coded bits float64 (N, K, 128), exact bypass bits
    int64 (N, K, 128)). The exception map is costed with the row `container._exception_rows` would form from that very
    histogram, clamps included: it is the row the blob would carry."""
    (zeros, ones, tables, bypass_bits) = _decisions_and_tables(hist, bypass_bits, ladder)
    return ideal_bits(zeros, ones, tables), bypass_bits


def _decisions_and_tables(hist, bypass_bits, ladder):
    """(zeros, ones, the probability row every (image, point, map) is coded with, bypass bits)."""
    (hist, bypass_bits) = _check_counts(hist, bypass_bits, ladder)
    (zeros, ones) = decision_counts(hist)
    tables = numpy.broadcast_to(ladder.binary_probabilities_points[None], zeros.shape).copy()
    e = ladder.idx_map_exception
    if e >= 0:
        tables[:, :, e] = probabilities_from_counts(zeros[:, :, e], ones[:, :, e])
    return zeros, ones, tables, bypass_bits


def nb_coding_tiles(height, width, coding_tile):
    """(tiles of a height x width image cut by coding_tile=(th, tw) latents, the tile clamped to the latent plane): the grid of
    `container.coding_tile_grid`, counted."""
    if height < 1 or width < 1 or height % 16 != 0 or width % 16 != 0:
        raise ValueError('The image sizes are not positive multiples of 16.')
    (th, tw) = (int(coding_tile[0]), int(coding_tile[1]))
    if th < 1 or tw < 1:
        raise ValueError('`coding_tile` must be a pair of positive integers.')
    (h, w) = (height//16, width//16)
    (th, tw) = (min(th, h), min(tw, w))
    return (-(-h//th))*(-(-w//tw)), (th, tw)


def header_bytes(ladder, height=None, width=None, coding_tile=None):
    """Bytes in front of the payload of a single-image EAE1 blob written at a point of the ladder (container.py, layout); with
    coding_tile=(th, tw) latents, of the single-image EAT1 blob of a height x width image: the same fields, the tile, and the index
    u32 [T][128][2]."""
    length = ladder.truncated_unary_length
    common = _FIXED_HEADER_BYTES + 8*NB_MAPS + 8*NB_MAPS*length + (8*length if ladder.idx_map_exception >= 0 else 0)
    if coding_tile is None:
        return common + 8*NB_MAPS
    if height is None or width is None:
        raise ValueError('The header of an EAT1 blob depends on the image sizes.')
    return common + _TILE_FIELD_BYTES + 8*NB_MAPS*nb_coding_tiles(height, width, coding_tile)[0]


def _check_counts_tiles(hist, bypass_bits, ladder):
    hist = numpy.asarray(hist)
    bypass_bits = numpy.asarray(bypass_bits)
    if hist.ndim != 5 or hist.shape[1] != ladder.nb_points or hist.shape[3:] != (NB_MAPS, ladder.truncated_unary_length + 1):
        raise ValueError('`hist` must be (N, K, T, {}, L + 1) for the K points and the L of the ladder.'.format(NB_MAPS))
    if bypass_bits.shape != hist.shape[:4]:
        raise ValueError('`bypass_bits` must be (N, K, T, {}).'.format(NB_MAPS))
    return hist.astype(numpy.int64), bypass_bits.astype(numpy.int64)


def blob_byte_bounds(hist, bypass_bits, ladder, height, width, coding_tile=None):
    """(lower, upper), int64 (N, K): bounds on the size of the single-image EAE1 blob `container.encode_images` would write for
    every image at every point. The header is exact; every map adds its bypass stream, ceil(bits / 8) bytes, exact, and its
    arithmetic-coded stream, between floor(`floor_bits`) - ALLOWANCE_LOW and ceil(`ideal_bits`) + ALLOWANCE_HIGH bits, each rounded up
    to a byte (on a table fitted to the data the two costs are a few bits apart: the comment at ALLOWANCE_LOW).
    height, width: of the images (the histograms must count their (height / 16) * (width / 16) symbols per map, except at a point
    with range errors, which `valid_points` tells apart).
    coding_tile=(th, tw) latents: of the single-image EAT1 blob instead, from the counts per tile `device.ladder_histograms_tiles`
    leaves, hist (N, K, T, 128, L + 1) and bypass_bits (N, K, T, 128). Every (tile, map) is a pair of streams of its own, so the
    same costs and the same allowances apply per tile stream (a tile is a map of 1 to 16,384 symbols: what the allowances were
    measured on); the exception map's row is the one its WHOLE-map counts give, as the blob carries one per image."""
    if coding_tile is not None:
        (hist, bypass_bits) = _check_counts_tiles(hist, bypass_bits, ladder)
        (nb_tiles, _) = nb_coding_tiles(height, width, coding_tile)
        if hist.shape[2] != nb_tiles:
            raise ValueError('The histograms are not those of the {} coding tiles of the image.'.format(nb_tiles))
        if int(hist.sum(axis=(2, -1)).max()) > (height//16)*(width//16):
            raise ValueError('The histograms count more symbols than a map of a {} x {} image holds.'.format(height, width))
        (zeros, ones) = decision_counts(hist)                                       # (N, K, T, 128, L)
        tables = numpy.broadcast_to(ladder.binary_probabilities_points[None, :, None], zeros.shape).copy()
        e = ladder.idx_map_exception
        if e >= 0:
            tables[:, :, :, e] = probabilities_from_counts(zeros[:, :, :, e].sum(axis=2), ones[:, :, :, e].sum(axis=2))[:, :, None]
        fixed = header_bytes(ladder, height, width, coding_tile) + ((bypass_bits + 7)//8).sum(axis=(-1, -2))
        low_bits = numpy.maximum(numpy.floor(floor_bits(zeros, ones, tables)).astype(numpy.int64) - ALLOWANCE_LOW, 0)
        high_bits = numpy.ceil(ideal_bits(zeros, ones, tables)).astype(numpy.int64) + ALLOWANCE_HIGH
        return fixed + ((low_bits + 7)//8).sum(axis=(-1, -2)), fixed + ((high_bits + 7)//8).sum(axis=(-1, -2))
    (zeros, ones, tables, bypass_bits) = _decisions_and_tables(hist, bypass_bits, ladder)
    if height < 1 or width < 1 or height % 16 != 0 or width % 16 != 0:
        raise ValueError('The image sizes are not positive multiples of 16.')
    if int(numpy.asarray(hist).sum(axis=-1).max()) > (height//16)*(width//16):
        raise ValueError('The histograms count more symbols than a map of a {} x {} image holds.'.format(height, width))
    fixed = header_bytes(ladder) + ((bypass_bits + 7)//8).sum(axis=-1)
    low_bits = numpy.maximum(numpy.floor(floor_bits(zeros, ones, tables)).astype(numpy.int64) - ALLOWANCE_LOW, 0)
    high_bits = numpy.ceil(ideal_bits(zeros, ones, tables)).astype(numpy.int64) + ALLOWANCE_HIGH
    return fixed + ((low_bits + 7)//8).sum(axis=-1), fixed + ((high_bits + 7)//8).sum(axis=-1)


def valid_points(hist, map_size):
    """bool (N, K): the points at which every symbol of the image fits int16. An element beyond goes into no bin
    (eae_hip_ladder_histograms), so a valid (image, point) is one whose histograms hold all 128 * map_size symbols."""
    return numpy.asarray(hist).astype(numpy.int64).sum(axis=(-1, -2)) == NB_MAPS*int(map_size)


def select_rate_points(lower, upper, valid, budget_bytes, size_of):
    """The deterministic choice of a rate point per image. lower, upper int (N, K) (`blob_byte_bounds`); valid bool (N, K);
    budget_bytes: a scalar or one value per image; size_of(image, k) -> the real size in bytes of the image coded at point k.
    Per image, in ladder order: a point that is invalid or whose lower bound exceeds the budget is skipped; any other point is
    coded (`size_of`) and taken if its real size fits. If none fits, the last valid point is taken (and coded, if it was not) and
    `fits` is False. An image without a valid point raises the AssertionError of `container.encode_images`.
    -> dict: 'rate_point' int64 (N,), 'blob_bytes' int64 (N,), 'attempts' int64 (N,) (calls of size_of), 'fits' bool (N,),
    'upper_bound_misses': the attempts at a point with upper <= budget whose real size did not fit (expected: 0)."""
    lower = numpy.asarray(lower)
    upper = numpy.asarray(upper)
    valid = numpy.asarray(valid, dtype=bool)
    if lower.ndim != 2 or upper.shape != lower.shape or valid.shape != lower.shape:
        raise ValueError('`lower`, `upper` and `valid` must be (N, K).')
    (nb_images, nb_points) = lower.shape
    budgets = numpy.broadcast_to(numpy.asarray(budget_bytes), (nb_images,)) if numpy.ndim(budget_bytes) <= 1 else None
    if budgets is None:
        raise ValueError('`budget_bytes` must be a scalar or one value per image.')
    out = {'rate_point': numpy.zeros(nb_images, dtype=numpy.int64), 'blob_bytes': numpy.zeros(nb_images, dtype=numpy.int64),
           'attempts': numpy.zeros(nb_images, dtype=numpy.int64), 'fits': numpy.zeros(nb_images, dtype=bool), 'upper_bound_misses': 0}
    for i in range(nb_images):
        budget = budgets[i]
        candidates = numpy.flatnonzero(valid[i])
        if candidates.size == 0:
            raise AssertionError('The rounded array elements cannot be represented as 16-bit signed integers.')
        sizes = {}
        chosen = None
        for k in candidates.tolist():
            if lower[i, k] > budget:
                continue
            sizes[k] = int(size_of(i, k))
            if sizes[k] <= budget:
                chosen = k
                break
            if upper[i, k] <= budget:
                out['upper_bound_misses'] += 1
        out['fits'][i] = chosen is not None
        if chosen is None:
            chosen = int(candidates[-1])
            if chosen not in sizes:
                sizes[chosen] = int(size_of(i, chosen))
        out['rate_point'][i] = chosen
        out['blob_bytes'][i] = sizes[chosen]
        out['attempts'][i] = len(sizes)
    return out


# ---- the rule of `codec.BudgetCodec`: a point per image from its upper bound alone, in integers -----------
# The device reaches the decision below element for element (`eae_hip_ladder_select`), so nothing in it is floating point: every
# logarithm is taken here, once per ladder, rounded against the budget (a cost up, a subtracted term down) and handed over as a table
# of 2^-20 bits.
FIXED_SHIFT = 20
FIXED_ONE = 1 << FIXED_SHIFT
# ceil(-log2(0.99) * 2^20): what a decision costs under the 0.99 clamp of `probabilities_from_counts` (a count of one kind only)
C99 = int(numpy.ceil(-numpy.log2(0.99)*FIXED_ONE))


def fixed_costs(ladder):
    """uint32 (K, 128, L, 2): [..., 0] = ceil(-log2(p) * 2^20), what a zero of the decision costs in 2^-20 bits, [..., 1] =
    ceil(-log2(1 - p) * 2^20), a one. Below 2^32 for every float64 p in ]0, 1[ (the smallest gives 1074 * 2^20)."""
    p = ladder.binary_probabilities_points
    costs = numpy.stack([numpy.ceil(-numpy.log2(p)*FIXED_ONE), numpy.ceil(-numpy.log2(1. - p)*FIXED_ONE)], axis=-1)
    assert costs.min() >= 0. and costs.max() < 2.**32
    return numpy.ascontiguousarray(costs.astype(numpy.uint32))


def log2_tables(map_size):
    """uint32 (2, map_size + 1): [0, n] = ceil(log2(n) * 2^20), [1, n] = floor(log2(n) * 2^20); entry 0 of both is 0 (never
    multiplied by anything but a zero count)."""
    map_size = int(map_size)
    if map_size < 1 or map_size > (1 << 24):
        raise ValueError('`map_size` does not belong to [1, 2^24].')
    tables = numpy.zeros((2, map_size + 1), dtype=numpy.uint32)
    scaled = numpy.log2(numpy.arange(1, map_size + 1, dtype=numpy.float64))*FIXED_ONE
    tables[0, 1:] = numpy.ceil(scaled)
    tables[1, 1:] = numpy.floor(scaled)
    return tables


def upper_bounds_fixed(hist, bypass_bits, ladder, map_size):
    """int64 (N, K): an upper bound on the size of every image's single-image EAE1 blob at every point, in integer arithmetic only
    (64-bit sums of counts times the tables above): what `eae_hip_ladder_select` computes. Per map, fp = sum over the decisions of
    zeros * c0 + ones * c1 (`fixed_costs`); the exception map, coded with the row `probabilities_from_counts` forms from its own
    counts, pays per decision t * Lceil[t] - z * Lfloor[z] - o * Lfloor[o] with t = z + o (`log2_tables`), o * C99 when z == 0,
    z * C99 when o == 0, nothing when t == 0. The stream then takes ((fp + 2^20 - 1) >> 20) + ALLOWANCE_HIGH bits, rounded up to a
    byte; the bypass stream ceil(bits / 8) bytes; the header `header_bytes`.
    Never below `blob_byte_bounds(...)[1]` and at most a byte per map above it while map_size * L <= 2^19 (every cost is rounded up
    by less than 2^-20 bit per decision)."""
    (hist, bypass_bits) = _check_counts(hist, bypass_bits, ladder)
    map_size = int(map_size)
    (zeros, ones) = decision_counts(hist)
    if int(hist.astype(numpy.int64).sum(axis=-1).max()) > map_size:
        raise ValueError('The histograms count more symbols than a map of {} holds.'.format(map_size))
    costs = fixed_costs(ladder).astype(numpy.int64)
    fp = (zeros*costs[None, ..., 0] + ones*costs[None, ..., 1]).sum(axis=-1)              # (N, K, 128)
    e = ladder.idx_map_exception
    if e >= 0:
        tables = log2_tables(map_size).astype(numpy.int64)
        (z, o) = (zeros[:, :, e], ones[:, :, e])
        t = z + o
        own = t*tables[0][t] - z*tables[1][z] - o*tables[1][o]
        own = numpy.where(z == 0, o*C99, numpy.where(o == 0, z*C99, own))
        fp[:, :, e] = own.sum(axis=-1)
    bits = (fp + (FIXED_ONE - 1)) >> FIXED_SHIFT
    stream_bytes = (bits + (ALLOWANCE_HIGH + 7))//8
    return header_bytes(ladder) + (stream_bytes + (bypass_bits + 7)//8).sum(axis=-1)


def upper_bounds_fixed_tiles(hist, bypass_bits, ladder, map_size, header_bytes):
    """int64 (N, K): `upper_bounds_fixed` for the single-image EAT1 blob, from the counts per coding tile hist (N, K, T, 128, L + 1)
    and bypass_bits (N, K, T, 128) (`device.ladder_histograms_tiles`); what `eae_hip_ladder_select_tiles` computes, integers only.
    map_size: symbols of a WHOLE map; header_bytes: `header_bytes(ladder, height, width, coding_tile)`.
    Per (image, point, tile, map), fp = sum over the decisions of z * c0 + o * c1 (`fixed_costs`) on the tile's own counts; the
    stream takes ((fp + 2^20 - 1) >> 20) + ALLOWANCE_HIGH bits, rounded up to a byte, the tile's bypass stream ceil(bits / 8) bytes.
    The exception map keeps ONE row per image, measured on the whole map: with Z, O the whole-map counts of a
    decision (the sums over the tiles) and T_ = Z + O, a tile's z zeros and o ones of it cost z * (Lceil[T_] - Lfloor[Z]) + o *
    (Lceil[T_] - Lfloor[O]), o * C99 when Z == 0, z * C99 when O == 0 -- over the tiles that is `upper_bounds_fixed`'s whole-map
    cost T_ * Lceil[T_] - Z * Lfloor[Z] - O * Lfloor[O].
    Never below `blob_byte_bounds(..., coding_tile)[1]` and at most a byte per stream above it while map_size * L <= 2^19."""
    (hist, bypass_bits) = _check_counts_tiles(hist, bypass_bits, ladder)
    map_size = int(map_size)
    (zeros, ones) = decision_counts(hist)                                                  # (N, K, T, 128, L)
    if int(hist.sum(axis=(2, -1)).max()) > map_size:
        raise ValueError('The histograms count more symbols than a map of {} holds.'.format(map_size))
    costs = fixed_costs(ladder).astype(numpy.int64)
    fp = (zeros*costs[None, :, None, :, :, 0] + ones*costs[None, :, None, :, :, 1]).sum(axis=-1)     # (N, K, T, 128)
    e = ladder.idx_map_exception
    if e >= 0:
        tables = log2_tables(map_size).astype(numpy.int64)
        (z, o) = (zeros[:, :, :, e], ones[:, :, :, e])                                    # (N, K, T, L)
        (whole_z, whole_o) = (z.sum(axis=2), o.sum(axis=2))                               # (N, K, L)
        total = tables[0][whole_z + whole_o]
        cost_zero = numpy.where(whole_z == 0, 0, numpy.where(whole_o == 0, C99, total - tables[1][whole_z]))
        cost_one = numpy.where(whole_z == 0, C99, numpy.where(whole_o == 0, 0, total - tables[1][whole_o]))
        fp[:, :, :, e] = (z*cost_zero[:, :, None] + o*cost_one[:, :, None]).sum(axis=-1)
    bits = (fp + (FIXED_ONE - 1)) >> FIXED_SHIFT
    stream_bytes = (bits + (ALLOWANCE_HIGH + 7))//8
    return int(header_bytes) + (stream_bytes + (bypass_bits + 7)//8).sum(axis=(-1, -2))


def select_by_upper_bound(upper, valid, budgets):
    """-> (rate_point int64 (N,), promised bool (N,)). upper int (N, K); valid bool (N, K); budgets: a scalar or one value per
    image. Per image, in ladder order, the first valid point with upper <= budget (`promised`: the bound says the blob fits); if
    there is none, the last valid point, not promised; if no point is valid, point K - 1, not promised (quantising at it fails the
    range check). Unlike `select_rate_points` nothing is coded to find out: a point is taken on its upper bound alone, so an
    image with lower <= budget < upper at a point goes on to the next one."""
    upper = numpy.asarray(upper)
    valid = numpy.asarray(valid, dtype=bool)
    if upper.ndim != 2 or valid.shape != upper.shape:
        raise ValueError('`upper` and `valid` must be (N, K).')
    (nb_images, nb_points) = upper.shape
    if numpy.ndim(budgets) > 1:
        raise ValueError('`budgets` must be a scalar or one value per image.')
    budgets = numpy.broadcast_to(numpy.asarray(budgets, dtype=numpy.int64), (nb_images,))
    rate_point = numpy.full(nb_images, nb_points - 1, dtype=numpy.int64)
    promised = numpy.zeros(nb_images, dtype=bool)
    for i in range(nb_images):
        candidates = numpy.flatnonzero(valid[i])
        if candidates.size == 0:
            continue
        fitting = candidates[upper[i, candidates] <= budgets[i]]
        promised[i] = fitting.size != 0
        rate_point[i] = fitting[0] if fitting.size else candidates[-1]
    return rate_point, promised


# ---- the rule of `codec.ColourBudgetCodec`: one byte budget for the three planes of a colour picture ----------
# A picture's budget B is that of its single-picture EAC1 blob: the colour header and three plane blobs. With P = max(B - header, 0):
#   1. Cb and Cr each get c = (P * share_q16) >> 17, share_q16 = round(chroma_share * 65536), and take `select_by_upper_bound`'s point
#      for c on their own `upper_bounds_fixed`;
#   2. Y gets r = max(P - ub_cb - ub_cr, 0), ub_x the bound of the point the chroma plane TOOK, promised or not: what chroma did not
#      need goes to the luminance. The device restates this line (`eae_hip_colour_budget_rest`), so that r never visits the host;
#   3. if all three planes are promised, header + ub_y + ub_cb + ub_cr <= B: ub_y <= r = P - ub_cb - ub_cr, and r > 0 or ub_y > 0 = r
#      would not be promised, so P = B - header.
COLOUR_SHARE_SHIFT = 16


def colour_header_bytes():
    """The bytes in front of the three plane blobs of an EAC1 blob: the size of `container`'s colour header struct."""
    from . import container
    return container.COLOUR_HEADER_BYTES


def _colour_payloads(budget_bytes):
    """budget_bytes, a scalar or one value per picture -> P = max(B - header, 0), int64 (N,) (a scalar: (1,))."""
    budgets = numpy.asarray(budget_bytes)
    if budgets.ndim > 1 or budgets.dtype.kind not in 'iuf' or (budgets.dtype.kind == 'f' and not numpy.isfinite(budgets).all()):
        raise ValueError('`budget_bytes` must be a number or one number per picture.')
    if budgets.size and (budgets.max() > (1 << 62) or budgets.min() < -(1 << 62)):
        raise ValueError('`budget_bytes` does not belong to [-2^62, 2^62].')
    return numpy.maximum(numpy.atleast_1d(budgets).astype(numpy.int64) - colour_header_bytes(), 0)


def colour_chroma_budgets(budget_bytes, chroma_share):
    """-> int64 (N,): c, the byte budget of the Cb blob and of the Cr blob of every picture (rule 1 above). budget_bytes: a scalar
    (N = 1) or one value per picture, up to 2^62; chroma_share: the fraction of the payload both chroma planes together may take,
    0 < chroma_share < 1, else ValueError. The product is formed in two halves, so nothing leaves int64."""
    try:
        share = float(chroma_share)
    except (TypeError, ValueError):
        raise ValueError('`chroma_share` must be a number.')
    if isinstance(chroma_share, (bool, numpy.bool_)) or not 0. < share < 1.:
        raise ValueError('`chroma_share` does not belong to ]0, 1[.')
    share_q16 = int(round(share*(1 << COLOUR_SHARE_SHIFT)))
    payload = _colour_payloads(budget_bytes)
    shift = COLOUR_SHARE_SHIFT + 1
    # (P * q) >> 17 with P = high * 2^17 + low: high * q + ((low * q) >> 17), high * q < 2^45 * 2^16
    return (payload >> shift)*share_q16 + (((payload & ((1 << shift) - 1))*share_q16) >> shift)


def colour_luma_budgets(budget_bytes, upper_cb, point_cb, upper_cr, point_cr):
    """-> int64 (N,): r, the byte budget of the Y blob of every picture (rule 2 above): max(P - upper_cb[i, point_cb[i]] -
    upper_cr[i, point_cr[i]], 0). budget_bytes: a scalar or one value per picture, up to 2^62; upper_cb, upper_cr int (N, K), the
    chroma planes' `upper_bounds_fixed`, not negative; point_cb, point_cr int (N,), the points they took. A picture with a point
    outside [0, K) gets 0, as on the device (`device.colour_budget_rest` is this function element for element)."""
    (upper_cb, upper_cr) = (numpy.asarray(upper_cb), numpy.asarray(upper_cr))
    (point_cb, point_cr) = (numpy.asarray(point_cb), numpy.asarray(point_cr))
    if upper_cb.ndim != 2 or upper_cb.shape[1] < 1 or upper_cr.shape != upper_cb.shape or upper_cb.dtype.kind not in 'iu' or upper_cr.dtype.kind not in 'iu':
        raise ValueError('`upper_cb` and `upper_cr` must be integer arrays (N, K) with K >= 1.')
    (nb_images, nb_points) = upper_cb.shape
    if point_cb.shape != (nb_images,) or point_cr.shape != (nb_images,) or point_cb.dtype.kind not in 'iu' or point_cr.dtype.kind not in 'iu':
        raise ValueError('`point_cb` and `point_cr` must be integer arrays (N,).')
    if nb_images and (upper_cb.min() < 0 or upper_cr.min() < 0 or max(int(upper_cb.max()), int(upper_cr.max())) >= (1 << 63)):
        raise ValueError('An upper bound is negative or does not fit int64.')
    payload = _colour_payloads(budget_bytes)
    if payload.shape[0] not in (1, nb_images):
        raise ValueError('`budget_bytes` must be a number or one number per picture.')
    rest = numpy.broadcast_to(payload, (nb_images,)).copy()
    inside = (point_cb >= 0) & (point_cb < nb_points) & (point_cr >= 0) & (point_cr < nb_points)
    rows = numpy.arange(nb_images)
    for (upper, point) in ((upper_cb, point_cb), (upper_cr, point_cr)):
        taken = upper.astype(numpy.int64)[rows, numpy.where(inside, point, 0)]
        rest = numpy.where(rest > taken, rest - taken, 0)          # never below -2^63: both operands are in [0, 2^63)
    return numpy.where(inside, rest, 0).astype(numpy.int64)


# ---- the rule of `codec.QualityCodec`: the coarsest point per image that keeps a PSNR floor, in integers -----
# PSNR >= T is sse <= max_sse for an integer max_sse the host derives once per threshold (`max_sse_for_psnr`); the search itself
# compares integers only, so the device (`eae_hip_quality_search`) reaches the choice below element for element.
MAX_SSE_SATURATION = 1 << 62      # where `max_sse_for_psnr` stops: no image has a squared error near it (255^2 per pixel)


def _psnr_meets(sse, nb_pixels, target_psnr):
    """`tls.psnr_from_sse(sse, nb_pixels) >= target_psnr`, a squared error of 0 meeting every target (psnr_from_sse raises there)."""
    from .kodak.tools import tools as tls
    return sse == 0 or bool(tls.psnr_from_sse(sse, nb_pixels) >= target_psnr)


def max_sse_for_psnr(target_psnr, nb_pixels):
    """The largest integer s >= 0 with `tls.psnr_from_sse(s, nb_pixels) >= target_psnr`, int64; s = 0 meets every target. Scalars
    or arrays (broadcast against each other). The closed form floor(255^2 nb_pixels 10^(-T / 10)) is only the start: s is stepped
    by one until psnr_from_sse, in the float64 expression it has, meets the target at s and misses it at s + 1, so that `sse <= s` and
    `psnr_from_sse(sse) >= T` are the same statement for every integer sse. Saturates at MAX_SSE_SATURATION = 2^62 (a target no
    image can miss). A target that is not finite raises ValueError; one that only s = 0 meets gives 0."""
    targets = numpy.asarray(target_psnr, dtype=numpy.float64)
    pixels = numpy.asarray(nb_pixels)
    if not numpy.isfinite(targets).all():
        raise ValueError('`target_psnr` is not finite.')
    if pixels.dtype.kind not in 'iu' or (pixels < 1).any():
        raise ValueError('`nb_pixels` must be a positive integer.')
    (targets, pixels) = numpy.broadcast_arrays(targets, pixels)
    out = numpy.zeros(targets.shape, dtype=numpy.int64)
    for index in numpy.ndindex(targets.shape):
        (target, n) = (float(targets[index]), int(pixels[index]))
        estimate = (255.**2)*n*(10.**(-target/10.))
        s = MAX_SSE_SATURATION if estimate >= MAX_SSE_SATURATION else int(numpy.floor(estimate))
        while s > 0 and not _psnr_meets(s, n, target):
            s -= 1
        while s < MAX_SSE_SATURATION and _psnr_meets(s + 1, n, target):
            s += 1
        out[index] = s
    return out if out.ndim else out[()]


def quality_rounds(nb_points):
    """ceil(log2(nb_points + 1)): the rounds after which a bisection over nb_points + 1 outcomes (each point, or none) has one left,
    whatever the data: 1, 2, 2, 3, 3, 3, 3, 4, ... and 4 for the reference's nine points."""
    nb_points = int(nb_points)
    if nb_points < 1:
        raise ValueError('`nb_points` must be at least 1.')
    return nb_points.bit_length()


def select_by_quality(sse, first, max_sse):
    """-> (point int64 (N,), met bool (N,), probe_points int64 (N, R), probe_sse int64 (N, R)), R = quality_rounds(K).
    sse int64 (N, K): the squared error of image i at point k; first int64 (N,): the finest point the search may take; max_sse int64
    (N,). Per image a bisection of exactly R rounds from (L, R) = (first - 1, K): a round with R - L > 1 (live) probes mid = (L + R)
    >> 1 and sets L = mid if sse[mid] <= max_sse, else R = mid; a round that is not live probes max(L, first) and changes nothing;
    every round records the point it probed and its sse. At the end point = L and met if L >= first, else point = first, not met.
    MONOTONICITY IS ASSUMED AND NOT CHECKED. Where sse is non-decreasing in k (points are ordered finest first), point is the
    coarsest point >= first with sse <= max_sse -- the smallest blob that keeps the floor --, or `first`, not met, when not even the
    finest allowed point keeps it. On a table that is not monotone the result is the bisection's own outcome: a point >= first
    that was probed and met the threshold (a coarser one that meets it too may exist), or `first`, not met, although some point
    the search did not probe would have met it."""
    sse = numpy.asarray(sse)
    first = numpy.asarray(first)
    max_sse = numpy.asarray(max_sse)
    if sse.ndim != 2 or sse.shape[1] < 1 or sse.dtype.kind not in 'iu':
        raise ValueError('`sse` must be an integer array (N, K) with K >= 1.')
    (nb_images, nb_points) = sse.shape
    if first.shape != (nb_images,) or max_sse.shape != (nb_images,) or first.dtype.kind not in 'iu' or max_sse.dtype.kind not in 'iu':
        raise ValueError('`first` and `max_sse` must be integer arrays (N,).')
    if nb_images and (first.min() < 0 or first.max() >= nb_points):
        raise ValueError('`first` does not belong to [0, K).')
    nb_rounds = quality_rounds(nb_points)
    point = numpy.zeros(nb_images, dtype=numpy.int64)
    met = numpy.zeros(nb_images, dtype=bool)
    probe_points = numpy.zeros((nb_images, nb_rounds), dtype=numpy.int64)
    probe_sse = numpy.zeros((nb_images, nb_rounds), dtype=numpy.int64)
    for i in range(nb_images):
        (point[i], met[i], probe_points[i], probe_sse[i]) = bisect_by_quality(lambda k: int(sse[i, k]), nb_points, int(first[i]), int(max_sse[i]))
    return point, met, probe_points, probe_sse


def bisect_by_quality(sse_of, nb_points, first, max_sse):
    """`select_by_quality` for one image whose squared error at point k is sse_of(k), asked for the points probed only (a point may
    be asked for more than once) -> (point, met, probed points, their sse), the last two lists of quality_rounds(nb_points)."""
    (low, high) = (first - 1, nb_points)
    (points, values) = ([], [])
    for _ in range(quality_rounds(nb_points)):
        live = high - low > 1
        probed = (low + high) >> 1 if live else max(low, first)
        value = int(sse_of(probed))
        points.append(probed)
        values.append(value)
        if live:
            if value <= max_sse:
                low = probed
            else:
                high = probed
    return (low, True, points, values) if low >= first else (first, False, points, values)


# ---- the rule of `codec.ColourQualityCodec`: one PSNR floor for the three planes of a colour picture ----------
# A picture's quality is the PSNR over all S = h w + 2 hc wc samples of its 4:2:0 form, (hc, wc) the chroma size: its error is E = sse_Y +
# sse_Cb + sse_Cr, each over its plane's REAL samples against the split input (for even sides the 4:1:1-weighted YUV PSNR). The
# threshold is M = `max_sse_for_psnr(T, S)`, or a given integer. Then:
#   1. Cb and Cr each get a = (M * share_q16) >> 17, share_q16 = round(chroma_share * 65536), and take `select_by_quality`'s point for
#      a on their own squared errors;
#   2. Y gets max(M - sse_cb - sse_cr, 0), sse_x the REAL squared error of the point the chroma plane TOOK, met or not: the error
#      chroma does not spend goes to the luminance, as unspent bytes do above. The device restates this line
#      (`eae_hip_colour_quality_rest`), so that it never visits the host; Y takes `select_by_quality`'s point for it;
#   3. the picture is met when sse_y + sse_cb + sse_cr <= M, on the three squared errors of the points taken. If all three planes are
#      met it is: sse_y <= M - sse_cb - sse_cr. The converse does not hold (chroma may miss a and Y make up for it).
# `select_by_quality`'s caveat is this rule's: MONOTONICITY IS ASSUMED AND NOT CHECKED. Where a plane's squared error is not
# non-decreasing along its ladder, its point is the bisection's own outcome, not necessarily the coarsest that keeps its threshold.
# The rule is not a joint search: 'sse_rgb' is not separable over the planes, and a coarser triple that keeps M may exist.

def colour_nb_samples(h, w):
    """S = h w + 2 hc wc: the samples of the 4:2:0 form of an h x w picture, (hc, wc) = (ceil(h / 2), ceil(w / 2))
    (`device.chroma_size`)."""
    (h, w) = (int(h), int(w))
    if h < 1 or w < 1:
        raise ValueError('`h` and `w` must be positive.')
    return h*w + 2*((h + 1)//2)*((w + 1)//2)


def _colour_max_sse(max_sse):
    """max_sse, a scalar or one value per picture -> int64 (N,) (a scalar: (1,)), in [0, 2^62]."""
    thresholds = numpy.asarray(max_sse)
    if thresholds.ndim > 1 or thresholds.dtype.kind not in 'iu':
        raise ValueError('`max_sse` must be an integer or one integer per picture.')
    if thresholds.size and (int(thresholds.max()) > MAX_SSE_SATURATION or int(thresholds.min()) < 0):
        raise ValueError('`max_sse` does not belong to [0, 2^62].')
    return numpy.atleast_1d(thresholds).astype(numpy.int64)


def colour_chroma_max_sse(max_sse, chroma_share):
    """-> int64 (N,): a, the squared-error threshold of the Cb plane and of the Cr plane of every picture (rule 1 above). max_sse: a
    scalar (N = 1) or one value per picture, in [0, 2^62]; chroma_share: the fraction of the picture's error both chroma planes
    together may take, 0 < chroma_share < 1, else ValueError (1/3, `codec.ColourQualityCodec`'s default, is the chroma planes' share
    of the samples: a starting value nobody has measured on a trained model). The product is formed in two halves, as in
    `colour_chroma_budgets`, so nothing leaves int64."""
    try:
        share = float(chroma_share)
    except (TypeError, ValueError):
        raise ValueError('`chroma_share` must be a number.')
    if isinstance(chroma_share, (bool, numpy.bool_)) or not 0. < share < 1.:
        raise ValueError('`chroma_share` does not belong to ]0, 1[.')
    share_q16 = int(round(share*(1 << COLOUR_SHARE_SHIFT)))
    thresholds = _colour_max_sse(max_sse)
    shift = COLOUR_SHARE_SHIFT + 1
    # (M * q) >> 17 with M = high * 2^17 + low: high * q + ((low * q) >> 17), high * q <= 2^45 * 2^16
    return (thresholds >> shift)*share_q16 + (((thresholds & ((1 << shift) - 1))*share_q16) >> shift)


def colour_luma_max_sse(max_sse, sse_cb, sse_cr):
    """-> int64 (N,): the squared-error threshold of the Y plane of every picture (rule 2 above): max(M - sse_cb[i] - sse_cr[i], 0).
    max_sse: a scalar or one value per picture, in [0, 2^62]; sse_cb, sse_cr int (N,): the real squared errors of the points the
    chroma planes took, not negative (`device.colour_quality_rest` is this function element for element)."""
    (sse_cb, sse_cr) = (numpy.asarray(sse_cb), numpy.asarray(sse_cr))
    if sse_cb.ndim != 1 or sse_cr.shape != sse_cb.shape or sse_cb.dtype.kind not in 'iu' or sse_cr.dtype.kind not in 'iu':
        raise ValueError('`sse_cb` and `sse_cr` must be integer arrays (N,).')
    nb_images = sse_cb.shape[0]
    if nb_images and (sse_cb.min() < 0 or sse_cr.min() < 0 or max(int(sse_cb.max()), int(sse_cr.max())) >= (1 << 63)):
        raise ValueError('A squared error is negative or does not fit int64.')
    thresholds = _colour_max_sse(max_sse)
    if thresholds.shape[0] not in (1, nb_images):
        raise ValueError('`max_sse` must be an integer or one integer per picture.')
    rest = numpy.broadcast_to(thresholds, (nb_images,)).copy()
    for spent in (sse_cb.astype(numpy.int64), sse_cr.astype(numpy.int64)):
        rest = numpy.where(rest > spent, rest - spent, 0)          # never below -2^63: both operands are in [0, 2^63)
    return rest.astype(numpy.int64)


# ---- the rule of the rate-distortion optimised quantiser --------------------------------------------------------
# Nearest rounding fixes the symbols before the coder's tables are looked at. Here a latent whose nearest symbol has magnitude a >= 1
# is coded at a - 1 instead when the squared error that adds, (2 u + 1) bw^2 with u = |x| - a in [-1/2, 1/2], is below rdo_lambda times
# the bits the coder's static table says it saves. The host forms one threshold per (map, magnitude), `rdo_thresholds`; the device
# (`eae_hip_latent_quantize_rdo`) and `rdo_quantize_numpy` compare 2 u + 1 against it in float32, element for element the same.
RDO_MAGNITUDES = 16               # the magnitudes 1 .. 16 have a threshold; a larger one is never lowered


def magnitude_bits(binary_probabilities):
    """float64 (..., L) -> float64 (..., L + 1): B(a), the bits the coder spends on a symbol of magnitude a = 0 .. L under the static
    table p, p[i] the probability that decision i of the truncated unary prefix is 0: -log2(1 - p[i]) for every decision i < min(a, L)
    that is a one, -log2 p[a] for the closing zero when a < L, the Exp-Golomb suffix of a - L when a >= L (2 floor(log2(a - L + 1))
    + 1 bits, as eae_hip_ladder_histograms counts it: 1 bit at a = L), and the sign bit when a > 0."""
    p = numpy.asarray(binary_probabilities, dtype=numpy.float64)
    if p.ndim < 1 or p.shape[-1] < 1:
        raise ValueError('`binary_probabilities` must be (..., L) with L >= 1.')
    length = p.shape[-1]
    ones = numpy.concatenate([numpy.zeros(p.shape[:-1] + (1,)), numpy.cumsum(-numpy.log2(1. - p), axis=-1)], axis=-1)   # i < a
    bits = ones.copy()
    bits[..., :length] += -numpy.log2(p)
    bits[..., length] += 1.                                # Exp-Golomb order 0 of a - L = 0
    bits[..., 1:] += 1.                                    # the sign
    return bits


def rdo_thresholds(bin_widths, binary_probabilities, rdo_lambda, idx_map_exception=-1):
    """float32 (..., 128, RDO_MAGNITUDES): T[c][a - 1] = rdo_lambda (B(a) - B(a - 1)) / bw[c]^2 for a = 1 .. min(L, 16), formed in
    float64 and cast; 0 where a step saves nothing (B(a) <= B(a - 1)), in the columns beyond min(L, 16), in the whole row of the
    exception map (its probability row is measured on the image's own symbols: a price taken from it would move the symbols it is
    measured on) and everywhere at rdo_lambda = 0. bin_widths float32 (..., 128), binary_probabilities float64 (..., 128, L): one
    point, or (K, 128) and (K, 128, L) for a ladder. rdo_lambda: squared latent units per bit; negative or not finite: ValueError."""
    rdo_lambda = float(rdo_lambda)
    if not numpy.isfinite(rdo_lambda) or rdo_lambda < 0.:
        raise ValueError('`rdo_lambda` must be a finite number that is not negative.')
    bw = numpy.asarray(bin_widths, dtype=numpy.float64)
    p = numpy.asarray(binary_probabilities, dtype=numpy.float64)
    if bw.ndim < 1 or bw.shape[-1] != NB_MAPS or p.shape[:-1] != bw.shape or p.shape[-1] < 1:
        raise ValueError('`bin_widths` must be (..., {0}) and `binary_probabilities` (..., {0}, L).'.format(NB_MAPS))
    used = min(p.shape[-1], RDO_MAGNITUDES)
    thresholds = numpy.zeros(bw.shape + (RDO_MAGNITUDES,), dtype=numpy.float32)
    if rdo_lambda == 0.:
        return thresholds
    bits = magnitude_bits(p)
    saved = (bits[..., 1:] - bits[..., :-1])[..., :used]
    with numpy.errstate(over='ignore'):
        thresholds[..., :used] = numpy.where(saved > 0., rdo_lambda*saved/(bw*bw)[..., None], 0.).astype(numpy.float32)
    if 0 <= idx_map_exception < NB_MAPS:
        thresholds[..., int(idx_map_exception), :] = 0.
    return thresholds


def rdo_quantize_numpy(y, bin_widths, map_mean, thresholds, truncated_unary_length):
    """The choice `eae_hip_latent_quantize_rdo` makes, in numpy float32, statement for statement: y float32 (..., 128) (channels
    last), bin_widths and map_mean float32 (128,) (map_mean None: zeros), thresholds float32 (128, RDO_MAGNITUDES) -> r float32
    of y's shape, the symbol of every latent as a float (what the device multiplies by the bin width).
    centered = y - m; x = centered / bw; r = round_half_even(x); a = |r|; u = |x| - a; where a >= 1 and a <= min(L, 16) -- tested
    in float, so that a NaN, an infinity or a huge a is left alone -- and 2 u + 1 < thresholds[c][a - 1], r = r - copysign(1, r)."""
    f32 = numpy.float32
    y = numpy.asarray(y)
    bw = numpy.asarray(bin_widths)
    mean = numpy.zeros(NB_MAPS, dtype=f32) if map_mean is None else numpy.asarray(map_mean)
    thresholds = numpy.asarray(thresholds)
    if y.dtype != f32 or bw.dtype != f32 or mean.dtype != f32 or thresholds.dtype != f32:
        raise TypeError('`y`, `bin_widths`, `map_mean` and `thresholds` must be float32.')
    if y.shape[-1] != NB_MAPS or bw.shape != (NB_MAPS,) or mean.shape != (NB_MAPS,) or thresholds.shape != (NB_MAPS, RDO_MAGNITUDES):
        raise ValueError('`y` must be (..., {0}), `bin_widths` and `map_mean` ({0},), `thresholds` ({0}, {1}).'.format(NB_MAPS, RDO_MAGNITUDES))
    amax = f32(min(int(truncated_unary_length), RDO_MAGNITUDES))
    with numpy.errstate(invalid='ignore', over='ignore'):
        centered = y - mean
        x = centered/bw
        r = numpy.rint(x)
        a = numpy.abs(r)
        u = numpy.abs(x) - a
        eligible = (a >= f32(1.)) & (a <= amax)
        column = numpy.where(eligible, a, f32(1.)).astype(numpy.int64) - 1
        lower = eligible & (f32(2.)*u + f32(1.) < thresholds[numpy.arange(NB_MAPS), column])
        return numpy.where(lower, r - numpy.copysign(f32(1.), r), r).astype(f32)
