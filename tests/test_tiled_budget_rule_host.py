"""The byte-budget rule for tile-indexed (EAT1) blobs on the host: ratecontrol.header_bytes with a coding
tile, upper_bounds_fixed_tiles and blob_byte_bounds(coding_tile=...), from counts per coding tile. CPU only, numpy only; every
comparison is exact.

The bound that is asserted: 0 <= upper_bounds_fixed_tiles - blob_byte_bounds(..., coding_tile)[1] <= T * 128 bytes per blob. Every
cost of the fixed-point rule is rounded up by less than 2^-20 bit per decision, i.e. by less than one bit per stream while
map_size * L <= 2^19 (here 143 * 33 at the most), which the rounding of a stream to whole bytes turns into one byte per stream at most.

The allowances of ratecontrol.py were measured on maps of 1 to 16,384 symbols; a tile stream is such a map. The last test codes
tile-sized maps with the host coder under a row fitted on a larger map that contains them, and holds the coder's bits against the
per-stream bounds: a check of the allowances on the reference coder, not of code under test."""
import functools

import numpy
import pytest

from test_budget_rule_host import clipped_histograms

from autoencoder_based_image_compression_amd import container
from autoencoder_based_image_compression_amd import ratecontrol

NB_MAPS = 128
K = 3
PLANES = ((11, 13), (32, 48))
TILES = ((4, 4), (8, 8), (16, 16), (64, 64))


def bypass_bits_of(magnitudes, length):
    suffix = numpy.maximum(magnitudes - length + 1, 1)
    return (magnitudes != 0) + numpy.where(magnitudes >= length, 2*numpy.floor(numpy.log2(suffix)).astype(numpy.int64) + 1, 0)


def cut(values, h, w, coding_tile):
    """(..., h * w) per-latent values -> a list of (..., rows * cols), one per coding tile, row-major."""
    (tiles, _) = container.coding_tile_grid(h, w, coding_tile)
    plane = values.reshape(values.shape[:-1] + (h, w))
    return [plane[..., r0:r0 + nr, c0:c0 + nc].reshape(values.shape[:-1] + (nr*nc,)) for (r0, c0, nr, nc, _) in tiles.tolist()]


@functools.lru_cache(maxsize=None)
def tiled_case(length, h, w, coding_tile, exception):
    """(ladder, hist (N, K, T, 128, L + 1), bypass (N, K, T, 128), whole-map hist (N, K, 128, L + 1), whole-map bypass): seeded
    Laplacian magnitudes at scales from 0.05 to 6 over the maps, the points 1 / 2 / 4 times as coarse, tables fitted on the counts
    of all images. Map 3 of image 0 is all zeros. The exception map (7): image 0 has no zero at point 0 (Z == 0 at decision 0);
    image 1 holds zeros and ones only, all of its ones in the first row of the plane (O == 0 at decision 1, T_ == 0 from decision 2
    on, and every tile below the first row of tiles holds no one at all); image 2 is Laplacian with its first coding tile all zero
    (a tile that holds none of the later decisions)."""
    rng = numpy.random.RandomState(1000*length + 17*h + w + 3*coding_tile[0] + (7 if exception >= 0 else 0))
    n = 3
    map_size = h*w
    scales = numpy.geomspace(0.05, 6., NB_MAPS)[None, None, :, None]/numpy.array([1., 2., 4.])[None, :, None, None]
    magnitudes = numpy.abs(numpy.rint(rng.laplace(size=(n, 1, NB_MAPS, map_size))*scales)).astype(numpy.int64)
    magnitudes[0, :, 3] = 0
    if exception >= 0:
        magnitudes[0, 0, exception] = 1 + rng.randint(0, 3, size=map_size)
        magnitudes[1, :, exception] = 0
        magnitudes[1, :, exception, :w] = 1
        first = numpy.zeros((h, w), dtype=bool)
        first[:min(coding_tile[0], h), :min(coding_tile[1], w)] = True
        busy = 1 + numpy.abs(numpy.rint(rng.laplace(size=(K, map_size))*3.)).astype(numpy.int64)
        magnitudes[2, :, exception] = numpy.where(first.reshape(-1)[None, :], 0, busy)
    parts = cut(magnitudes, h, w, coding_tile)
    hist = numpy.stack([clipped_histograms(part, length) for part in parts], axis=2)
    bypass = numpy.stack([bypass_bits_of(part, length).sum(axis=-1) for part in parts], axis=2)
    whole = clipped_histograms(magnitudes, length)
    (zeros, ones) = ratecontrol.decision_counts(whole.sum(axis=0))
    tables = ratecontrol.probabilities_from_counts(zeros, ones)
    ladder = ratecontrol.RateLadder(numpy.ones((K, NB_MAPS), dtype=numpy.float32)*numpy.array([[1.], [2.], [4.]], dtype=numpy.float32),
                                    tables, numpy.zeros(NB_MAPS, dtype=numpy.float32), exception)
    return ladder, hist, bypass, whole, bypass_bits_of(magnitudes, length).sum(axis=-1)


@pytest.mark.parametrize('exception', [-1, 7], ids=['no_exception', 'exception'])
@pytest.mark.parametrize('length', [3, 10])
@pytest.mark.parametrize('coding_tile', TILES)
@pytest.mark.parametrize('h, w', PLANES)
def test_header_bytes_is_the_header_assemble_blob_writes(h, w, coding_tile, length, exception):
    rng = numpy.random.RandomState(1)
    tables = rng.uniform(0.1, 0.9, size=(K, NB_MAPS, length))
    ladder = ratecontrol.RateLadder(numpy.ones((K, NB_MAPS), dtype=numpy.float32), tables, numpy.zeros(NB_MAPS, dtype=numpy.float32), exception)
    (tiles, _) = container.coding_tile_grid(h, w, (min(coding_tile[0], h), min(coding_tile[1], w)))
    rows = numpy.full((1 if exception >= 0 else 0, length), 0.5)
    (blob, header_length) = container.assemble_blob(False, 1, 16*h, 16*w, exception, ladder.bin_widths_points[0], ladder.map_mean, tables[0],
                                                    rows, numpy.zeros((len(tiles)*NB_MAPS, 2), dtype=numpy.uint32), b'', coding_tile=coding_tile)
    assert blob[:4] == b'EAT1' and len(blob) == header_length
    assert ratecontrol.header_bytes(ladder, 16*h, 16*w, coding_tile) == header_length
    assert ratecontrol.nb_coding_tiles(16*h, 16*w, coding_tile)[0] == len(tiles)
    # the EAE1 header is unchanged, and four bytes and (T - 1) index blocks shorter
    assert ratecontrol.header_bytes(ladder) == header_length - 4 - 8*NB_MAPS*(len(tiles) - 1)


def test_header_bytes_of_a_tiled_blob_needs_the_image_sizes():
    (ladder, _, _, _, _) = tiled_case(3, 11, 13, (4, 4), -1)
    with pytest.raises(ValueError):
        ratecontrol.header_bytes(ladder, coding_tile=(4, 4))
    with pytest.raises(ValueError):
        ratecontrol.header_bytes(ladder, 176, 200, (4, 4))
    with pytest.raises(ValueError):
        ratecontrol.header_bytes(ladder, 176, 208, (0, 4))


@pytest.mark.parametrize('exception', [-1, 7], ids=['no_exception', 'exception'])
@pytest.mark.parametrize('length', [1, 3, 10, 33])
def test_one_tile_per_plane_is_the_whole_map_bound(length, exception):
    (h, w) = (11, 13)
    (ladder, hist, bypass, whole, whole_bypass) = tiled_case(length, h, w, (16, 16), exception)
    assert hist.shape[2] == 1 and numpy.array_equal(hist[:, :, 0], whole) and numpy.array_equal(bypass[:, :, 0], whole_bypass)
    header = ratecontrol.header_bytes(ladder, 16*h, 16*w, (16, 16))
    assert header == ratecontrol.header_bytes(ladder) + 4
    tiled = ratecontrol.upper_bounds_fixed_tiles(hist, bypass, ladder, h*w, header)
    assert tiled.dtype == numpy.int64 and tiled.shape == (3, K)
    assert numpy.array_equal(tiled, ratecontrol.upper_bounds_fixed(whole, whole_bypass, ladder, h*w) + 4)
    (low, high) = ratecontrol.blob_byte_bounds(hist, bypass, ladder, 16*h, 16*w, (16, 16))
    (low_whole, high_whole) = ratecontrol.blob_byte_bounds(whole, whole_bypass, ladder, 16*h, 16*w)
    assert numpy.array_equal(low, low_whole + 4) and numpy.array_equal(high, high_whole + 4)


@pytest.mark.parametrize('exception', [-1, 7], ids=['no_exception', 'exception'])
@pytest.mark.parametrize('length', [1, 3, 10, 33])
@pytest.mark.parametrize('coding_tile', [(4, 4), (8, 8), (1, 1)])
def test_upper_bounds_fixed_tiles_against_the_float_bound(coding_tile, length, exception):
    (h, w) = (11, 13)
    (ladder, hist, bypass, whole, whole_bypass) = tiled_case(length, h, w, coding_tile, exception)
    nb_tiles = hist.shape[2]
    assert nb_tiles == ratecontrol.nb_coding_tiles(16*h, 16*w, coding_tile)[0]
    assert numpy.array_equal(hist.sum(axis=2), whole) and numpy.array_equal(bypass.sum(axis=2), whole_bypass)
    if exception >= 0:
        (zeros, ones) = ratecontrol.decision_counts(whole[:, :, exception])
        assert zeros[0, 0, 0] == 0 and ones[0, 0, 0] > 0                                 # Z == 0
        assert zeros[2, 0, 0] > 0 and ones[2, 0, 0] > 0                                  # both non-zero
        if length > 1:
            assert ones[1, 0, 1] == 0 and zeros[1, 0, 1] > 0                             # O == 0
        if length > 2:
            assert zeros[1, 0, 2] == 0 and ones[1, 0, 2] == 0                            # T_ == 0
        (tile_zeros, tile_ones) = ratecontrol.decision_counts(hist[:, :, :, exception])
        assert tile_ones[1, 0, -1, 0] == 0 and ones[1, 0, 0] > 0                         # a tile without a one of a decision the map has
        assert tile_ones[2, 0, 0, 0] == 0 and tile_zeros[2, 0, 0, 0] > 0
        if length > 1:
            assert tile_zeros[2, 0, 0, 1] == 0 and tile_ones[2, 0, 0, 1] == 0            # a tile that holds none of a decision
    header = ratecontrol.header_bytes(ladder, 16*h, 16*w, coding_tile)
    fixed = ratecontrol.upper_bounds_fixed_tiles(hist, bypass, ladder, h*w, header)
    (low, reference) = ratecontrol.blob_byte_bounds(hist, bypass, ladder, 16*h, 16*w, coding_tile)
    assert fixed.dtype == numpy.int64 and fixed.shape == reference.shape == low.shape == (3, K)
    difference = fixed - reference
    print('tile', coding_tile, 'L', length, 'difference', difference.min(), difference.max(), 'streams', nb_tiles*NB_MAPS)
    assert difference.min() >= 0
    assert difference.max() <= nb_tiles*NB_MAPS
    assert (low <= reference).all() and (low >= header).all()
    # tiles cost: never less than the whole maps' streams (each tile pays its own closing bits and byte padding)
    assert (fixed >= ratecontrol.upper_bounds_fixed(whole, whole_bypass, ladder, h*w)).all()
    assert numpy.array_equal(ratecontrol.valid_points(hist.sum(axis=2), h*w), numpy.ones((3, K), dtype=bool))


def test_the_exception_map_sums_to_the_whole_map_cost():
    """Before the rounding to bits, the exception map's cost over the tiles is `upper_bounds_fixed`'s whole-map formula: with every
    other map empty and one tile per symbol row, the two bounds differ by the streams' rounding alone."""
    (length, h, w, coding_tile, e) = (10, 11, 13, (4, 4), 7)
    (ladder, hist, _, whole, _) = tiled_case(length, h, w, coding_tile, e)
    tables = ratecontrol.log2_tables(h*w).astype(numpy.int64)
    (z, o) = ratecontrol.decision_counts(hist[:, :, :, e])
    (whole_z, whole_o) = ratecontrol.decision_counts(whole[:, :, e])
    total = whole_z + whole_o
    expected = total*tables[0][total] - whole_z*tables[1][whole_z] - whole_o*tables[1][whole_o]
    expected = numpy.where(whole_z == 0, whole_o*ratecontrol.C99, numpy.where(whole_o == 0, whole_z*ratecontrol.C99, expected))
    per_tile = numpy.where(whole_z[:, :, None] == 0, o*ratecontrol.C99, numpy.where(
        whole_o[:, :, None] == 0, z*ratecontrol.C99,
        z*(tables[0][total] - tables[1][whole_z])[:, :, None] + o*(tables[0][total] - tables[1][whole_o])[:, :, None]))
    assert numpy.array_equal(per_tile.sum(axis=2), expected)
    # and through the function: only the exception map's streams cost more than their three closing bits
    only = numpy.zeros_like(hist)
    only[:, :, :, e] = hist[:, :, :, e]
    bound = ratecontrol.upper_bounds_fixed_tiles(only, numpy.zeros(hist.shape[:4], dtype=numpy.int64), ladder, h*w, 0)
    streams = ((((per_tile.sum(axis=-1) + ratecontrol.FIXED_ONE - 1) >> 20) + 3 + 7)//8).sum(axis=-1)
    assert numpy.array_equal(bound, streams + (NB_MAPS - 1)*hist.shape[2])


def test_upper_bounds_fixed_tiles_refuses_what_it_cannot_index():
    (ladder, hist, bypass, whole, whole_bypass) = tiled_case(3, 11, 13, (4, 4), 7)
    with pytest.raises(ValueError):
        ratecontrol.upper_bounds_fixed_tiles(hist, bypass, ladder, 142, 0)
    with pytest.raises(ValueError):
        ratecontrol.upper_bounds_fixed_tiles(whole, whole_bypass, ladder, 143, 0)
    with pytest.raises(ValueError):
        ratecontrol.upper_bounds_fixed_tiles(hist, bypass[:, :, :3], ladder, 143, 0)
    with pytest.raises(ValueError):
        ratecontrol.blob_byte_bounds(hist, bypass, ladder, 176, 208, (8, 8))        # the counts of another grid


@pytest.mark.parametrize('length', [3, 10])
def test_the_host_coder_on_tile_sized_maps_stays_inside_the_bounds_of_a_stream(length):
    """Maps of 1, 3, 4, 12, 16, 64 and 256 symbols cut out of a larger map, coded under the row fitted on that larger map (the
    exception map's case) and under a row fitted on other data (every other map's): the arithmetic-coded stream lies between
    floor(floor_bits) - ALLOWANCE_LOW and ceil(ideal_bits) + ALLOWANCE_HIGH, under the fixed-point bound too, and the bypass stream
    is exact."""
    from autoencoder_based_image_compression_amd.kodak.lossless import interface_cython
    rng = numpy.random.RandomState(40 + length)
    checked = 0
    for scale in (0., 0.3, 1., 4., 12.):
        larger = numpy.rint(rng.laplace(size=1536)*scale).astype(numpy.int16)
        other = numpy.rint(rng.laplace(size=1536)*scale*1.5).astype(numpy.int16)
        rows = []
        for fitted_on in (larger, other):
            (zeros, ones) = ratecontrol.decision_counts(clipped_histograms(numpy.abs(fitted_on.astype(numpy.int64)), length))
            rows.append(ratecontrol.probabilities_from_counts(zeros, ones))
        for row in rows:
            cost_zero = numpy.ceil(-numpy.log2(row)*ratecontrol.FIXED_ONE).astype(numpy.int64)
            cost_one = numpy.ceil(-numpy.log2(1. - row)*ratecontrol.FIXED_ONE).astype(numpy.int64)
            for size in (1, 3, 4, 12, 16, 64, 256):
                for start in (0, 700, 1536 - size):
                    symbols = numpy.ascontiguousarray(larger[start:start + size])
                    magnitudes = numpy.abs(symbols.astype(numpy.int64))
                    (zeros, ones) = ratecontrol.decision_counts(clipped_histograms(magnitudes, length))
                    (_, bac_bits, _, bypass_bits) = interface_cython.encode_flattened_map(symbols, row)
                    low = max(int(numpy.floor(ratecontrol.floor_bits(zeros, ones, row))) - ratecontrol.ALLOWANCE_LOW, 0)
                    high = int(numpy.ceil(ratecontrol.ideal_bits(zeros, ones, row))) + ratecontrol.ALLOWANCE_HIGH
                    fixed = ((int((zeros*cost_zero + ones*cost_one).sum()) + ratecontrol.FIXED_ONE - 1) >> 20) + ratecontrol.ALLOWANCE_HIGH
                    assert low <= bac_bits <= high <= fixed, (scale, size, start, low, bac_bits, high, fixed)
                    assert bypass_bits == int(bypass_bits_of(magnitudes, length).sum())
                    checked += 1
    assert checked == 5*2*7*3


# ---- the inventory of codec._TiledBudgetSlot -------------------------------------------------------------------------------------

def _source():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'autoencoder_based_image_compression_amd', 'codec.py')) as f:
        return f.read()


def _unclassified(source):
    import slot_buffers
    import tiled_budget_slot_buffers
    from test_slot_inventory import assigned_attributes
    known = {slot_buffers.attribute_of(name) for name in tiled_budget_slot_buffers.TILED_BUDGET_SLOT}
    return sorted(assigned_attributes(source, '_TiledBudgetSlot') - known)


def test_every_attribute_of_the_tiled_budget_slot_is_classified():
    from test_slot_inventory import assigned_attributes
    assert {'accum', 'hist', 'pinned_budgets', 'select', 'prob_row', 'class_rows', 'table', 'exception_rows'} <= \
        assigned_attributes(_source(), '_TiledBudgetSlot')
    assert _unclassified(_source()) == []


def test_every_entry_of_the_tiled_budget_slot_exists_and_says_why():
    import ratecontrol_slot_buffers
    import tiled_budget_slot_buffers
    from test_slot_inventory import assigned_attributes
    table = tiled_budget_slot_buffers.TILED_BUDGET_SLOT
    ratecontrol_slot_buffers.check_entries(table, assigned_attributes(_source(), '_TiledBudgetSlot'), tiled_budget_slot_buffers.MUST_BE_SCRATCH,
                                           ('budgets_nbytes', 'points_table'))
    assert table['class_rows'].alias == 'prob_row'


def test_an_unclassified_buffer_of_the_tiled_budget_slot_is_noticed():
    from test_slot_inventory import _with_one_more_buffer
    assert _unclassified(_with_one_more_buffer(_source(), '_TiledBudgetSlot')) == ['extra']


def test_the_other_slots_did_not_grow():
    """`_TiledBudgetSlot` exists so that `_Slot` and `_BudgetSlot` keep their attributes: their helpers still classify all of them."""
    import budget_slot_buffers
    import slot_buffers
    from test_slot_inventory import assigned_attributes
    assert assigned_attributes(_source(), '_Slot') <= {slot_buffers.attribute_of(name) for name in slot_buffers.SLOT}
    assert assigned_attributes(_source(), '_BudgetSlot') <= {slot_buffers.attribute_of(name) for name in budget_slot_buffers.BUDGET_SLOT}
