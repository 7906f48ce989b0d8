"""The two launches behind a byte budget for tile-indexed (EAT1) blobs, on poisoned buffers between guard
bands under both poisons (tests/guarded.py):

* eae_hip_ladder_histograms_tiles (device.ladder_histograms_tiles) against numpy on the symbols `quantize_maps` gives, cut with
  `container.coding_tile_grid`, and, summed over the tiles, against device.ladder_histograms: tiles of four shape classes down to
  3 x 1 and 1 x 1, a tile clamped to the plane, and planes of 64 x 64 whose tiles a launch may cut into chunks;
* eae_hip_ladder_select_tiles (device.ladder_select_tiles) against the host rule it restates in integers --
  ratecontrol.upper_bounds_fixed_tiles, valid_points on the counts summed over the tiles, select_by_upper_bound --, with budgets at
  and one byte under every bound, and prob_row in the run order of codec.coding_tile_layout.

Every comparison is exact."""
import functools

import numpy
import pytest

from test_gpu_budget_kernels import budget_sweep, random_latents
from test_gpu_ladder import inputs, suffix_bits
from test_tiled_budget_rule_host import tiled_case

pytestmark = pytest.mark.gpu

F32 = numpy.float32
NB_MAPS = 128


@pytest.fixture(autouse=True, params=[0xFF, 0x7F], ids=['poison_ff', 'poison_7f'])
def guard(request):
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


@pytest.fixture(scope='module')
def dev():
    from autoencoder_based_image_compression_amd import device
    return device


@pytest.fixture(scope='module')
def rc():
    from autoencoder_based_image_compression_amd import ratecontrol
    return ratecontrol


# ---- ladder_histograms_tiles ---------------------------------------------------------------------------------------------------------

def points_for(dev, kind, length):
    return {'one': 1, 'three': 3, 'most': dev.ladder_max_points(length)}[kind]


_REFERENCES = {}


def tile_reference(dev, n, h, w, coding_tile, k_points, length):
    """(hist int64 [N, K, T, 128, L + 1], bypass bits [N, K, T, 128], range errors [K]) from the int16 symbols of `quantize_maps`,
    cut with `coding_tile_grid`; an element whose float32 symbol leaves int16 (its int16 has wrapped) is counted in the range
    errors only. Computed once per shape (on plain buffers) and shared."""
    import torch
    from autoencoder_based_image_compression_amd import container
    key = (n, h, w, coding_tile, k_points, length)
    if key in _REFERENCES:
        return _REFERENCES[key]
    (y, bw, mean) = inputs(n, h*w, k_points, length, True)
    (tiles, _) = container.coding_tile_grid(h, w, (min(coding_tile[0], h), min(coding_tile[1], w)))
    hist = numpy.zeros((n, k_points, len(tiles), NB_MAPS, length + 1), dtype=numpy.int64)
    bits = numpy.zeros((n, k_points, len(tiles), NB_MAPS), dtype=numpy.int64)
    errors = numpy.zeros(k_points, dtype=numpy.int64)
    y_device = torch.from_numpy(y).cuda()
    for k in range(k_points):
        q = dev.quantize_maps(y_device, torch.from_numpy(bw[k]).cuda(), torch.from_numpy(mean).cuda(), want_symbols=True)
        symbols = q['symbols'].cpu().numpy().astype(numpy.int64).reshape(n, NB_MAPS, h, w)
        rs = numpy.rint(bw[k]*numpy.rint((y - mean)/bw[k])/bw[k])
        good = (numpy.abs(rs) < F32(32768.)).reshape(n, h, w, NB_MAPS).transpose(0, 3, 1, 2)
        errors[k] = (~good).sum()
        assert errors[k] == int(q['checks'][0].item())
        magnitudes = numpy.abs(symbols)
        clipped = numpy.minimum(magnitudes, length)
        bypass = suffix_bits(magnitudes, length)*good
        for (t, (r0, c0, nr, nc, _)) in enumerate(tiles.tolist()):
            window = (slice(None), slice(None), slice(r0, r0 + nr), slice(c0, c0 + nc))
            for b in range(length + 1):
                hist[:, k, t, :, b] = (good[window] & (clipped[window] == b)).sum(axis=(2, 3))
            bits[:, k, t] = bypass[window].sum(axis=(2, 3))
    _REFERENCES[key] = (hist, bits, errors)
    return _REFERENCES[key]


def run_tiles(dev, guard, n, h, w, coding_tile, k_points, length, **kwargs):
    (y, bw, mean) = inputs(n, h*w, k_points, length, True)
    y_d = guard.upload(y.reshape(n, h, w, NB_MAPS))
    out = dev.ladder_histograms_tiles(y_d, guard.upload(bw), coding_tile, guard.upload(mean), length, **kwargs)
    return tuple(t.cpu().numpy() for t in out), y_d


def check_tiles(dev, guard, n, h, w, coding_tile, k_points, length):
    ((hist, bits, errors), y_d) = run_tiles(dev, guard, n, h, w, coding_tile, k_points, length)
    (hist_ref, bits_ref, errors_ref) = tile_reference(dev, n, h, w, coding_tile, k_points, length)
    assert errors_ref[0] == 3*n and not errors_ref[1:].any()
    assert hist.shape == hist_ref.shape and bits.shape == bits_ref.shape
    assert numpy.array_equal(errors, errors_ref)
    assert numpy.array_equal(hist, hist_ref)
    assert numpy.array_equal(bits, bits_ref)
    # summed over the tiles: the whole-map kernel's outputs on the same input, element for element
    (_, bw, mean) = inputs(n, h*w, k_points, length, True)
    whole = dev.ladder_histograms(y_d, guard.upload(bw), guard.upload(mean), length)
    assert numpy.array_equal(hist.sum(axis=2), whole[0].cpu().numpy())
    assert numpy.array_equal(bits.sum(axis=2), whole[1].cpu().numpy())
    assert numpy.array_equal(errors, whole[2].cpu().numpy())


@pytest.mark.parametrize('kind', ['one', 'three', 'most'])
@pytest.mark.parametrize('length', [1, 3, 10])
@pytest.mark.parametrize('coding_tile', [(4, 4), (8, 8), (16, 16), (1, 1)])
def test_histograms_per_tile_on_a_plane_of_11_by_13(dev, guard, coding_tile, length, kind):
    """(4, 4): four shape classes, 4 x 4, 3 x 4, 4 x 1 and 3 x 1; (8, 8): 8 x 8, 3 x 8, 8 x 5, 3 x 5; (16, 16): clamped, one tile."""
    from autoencoder_based_image_compression_amd import container
    (tiles, classes) = container.coding_tile_grid(11, 13, (min(coding_tile[0], 11), min(coding_tile[1], 13)))
    assert (len(tiles), len(classes)) == {(4, 4): (12, 4), (8, 8): (4, 4), (16, 16): (1, 1), (1, 1): (143, 1)}[coding_tile]
    check_tiles(dev, guard, 3, 11, 13, coding_tile, points_for(dev, kind, length), length)


@pytest.mark.parametrize('coding_tile', [(64, 64), (32, 64)])
def test_histograms_per_tile_on_tiles_a_launch_may_cut_into_chunks(dev, guard, coding_tile):
    """Two images of 64 x 64 latents, K = 9, L = 10: two and four tiles for some five hundred blocks."""
    check_tiles(dev, guard, 2, 64, 64, coding_tile, 9, 10)


@pytest.mark.parametrize('n, coding_tile, k_points, length', [(4, (1, 1), 3, 10), (5, (1, 1), 9, 10), (13, (2, 2), 3, 3), (30, (2, 2), 9, 10)])
def test_histograms_per_tile_when_a_block_takes_several_whole_tiles(dev, guard, n, coding_tile, k_points, length):
    """More (image, tile) entries than two blocks per compute unit: the launcher deals whole tiles to the blocks, and a block
    that gets two or three of them (572 and 715 entries of one latent; 546 and 1,260 entries of 2 x 2, 1 x 2, 2 x 1 and 1 x 1 latents,
    for 512 blocks on 256 compute units) counts the next tile in the LDS arrays its flush of the last one has cleared. Bins AND
    bypass bits against numpy and against the whole-map kernel."""
    from autoencoder_based_image_compression_amd import container
    (h, w) = (11, 13)
    (tiles, classes) = container.coding_tile_grid(h, w, coding_tile)
    assert len(classes) == (1 if coding_tile == (1, 1) else 4)
    blocks = 2*dev.device_info()['compute_units']
    assert n*len(tiles) > blocks                                    # several tiles per block: the branch this test is about
    assert (n*len(tiles)) % blocks != 0                              # ... and not the same number for every block
    check_tiles(dev, guard, n, h, w, coding_tile, k_points, length)


def test_an_element_beyond_int16_lands_in_the_range_errors_only(dev, guard):
    (n, h, w, length) = (2, 5, 6, 4)
    bw = numpy.stack([numpy.full(NB_MAPS, 0.5, dtype=F32), numpy.full(NB_MAPS, 1., dtype=F32)])
    y = numpy.zeros((n, h, w, NB_MAPS), dtype=F32)
    y[1, 4, 5, 9] = F32(0.5*40000.)                    # symbol 40000 at point 0, 20000 at point 1: in the last tile (3 x 2) of image 1
    (hist, bits, errors) = (t.cpu().numpy() for t in dev.ladder_histograms_tiles(guard.upload(y), guard.upload(bw), (2, 4), None, length))
    assert errors.tolist() == [1, 0]
    sizes = numpy.array([8, 4, 8, 4, 4, 2])
    expected = numpy.zeros((n, 2, 6, NB_MAPS, length + 1), dtype=numpy.int64)
    expected[..., 0] = sizes[None, None, :, None]
    expected[1, :, 5, 9, 0] -= 1
    expected[1, 1, 5, 9, length] = 1
    assert numpy.array_equal(hist, expected)
    expected_bits = numpy.zeros((n, 2, 6, NB_MAPS), dtype=numpy.int64)
    expected_bits[1, 1, 5, 9] = int(suffix_bits(numpy.array([20000]), length)[0])
    assert numpy.array_equal(bits, expected_bits)


def test_the_outputs_accumulate_over_two_calls(dev, guard):
    import torch
    (n, h, w, coding_tile, k_points, length) = (3, 11, 13, (4, 4), 3, 3)
    out = (torch.zeros((n, k_points, 12, NB_MAPS, length + 1), dtype=torch.int32, device='cuda'),
           torch.zeros((n, k_points, 12, NB_MAPS), dtype=torch.int64, device='cuda'), torch.zeros(k_points, dtype=torch.int32, device='cuda'))
    run_tiles(dev, guard, n, h, w, coding_tile, k_points, length, out=out)
    ((hist, bits, errors), _) = run_tiles(dev, guard, n, h, w, coding_tile, k_points, length, out=out)
    (hist_ref, bits_ref, errors_ref) = tile_reference(dev, n, h, w, coding_tile, k_points, length)
    assert numpy.array_equal(hist, 2*hist_ref) and numpy.array_equal(bits, 2*bits_ref) and numpy.array_equal(errors, 2*errors_ref)


def test_a_ladder_longer_than_a_launch_is_split(dev, guard):
    (n, h, w, coding_tile, length) = (3, 11, 13, (8, 8), 10)
    k_points = dev.ladder_max_points(length) + 1
    ((hist, bits, errors), _) = run_tiles(dev, guard, n, h, w, coding_tile, k_points, length)
    (hist_ref, bits_ref, errors_ref) = tile_reference(dev, n, h, w, coding_tile, k_points, length)
    assert numpy.array_equal(hist, hist_ref) and numpy.array_equal(bits, bits_ref) and numpy.array_equal(errors, errors_ref)


def test_a_length_no_launch_takes_is_folded_on_the_host(dev, guard):
    """L = 255: eae_hip_ladder_max_points is 0; the same arrays come back, at the finest point, whose symbols leave int16, too."""
    (n, h, w, coding_tile, k_points, length) = (3, 11, 13, (4, 4), 2, 255)
    assert dev.ladder_max_points(length) == 0
    ((hist, bits, errors), _) = run_tiles(dev, guard, n, h, w, coding_tile, k_points, length)
    (hist_ref, bits_ref, errors_ref) = tile_reference(dev, n, h, w, coding_tile, k_points, length)
    assert errors_ref[0] and not errors_ref[1]
    assert numpy.array_equal(hist, hist_ref) and numpy.array_equal(bits, bits_ref) and numpy.array_equal(errors, errors_ref)


def test_histograms_per_tile_refuses_bad_arguments(dev, guard):
    import torch
    from autoencoder_based_image_compression_amd import _native
    lib = _native.hip()
    (n, h, w, length) = (1, 4, 6, 10)
    most = dev.ladder_max_points(length)
    (y, bw, _) = inputs(n, h*w, most, length, False)
    (y_d, bw_d) = (guard.upload(y.reshape(n, h, w, NB_MAPS)), guard.upload(bw))
    hist = torch.zeros((n, most, 6, NB_MAPS, length + 1), dtype=torch.int32, device='cuda')
    call = lib.eae_hip_ladder_histograms_tiles
    good = [y_d.data_ptr(), None, bw_d.data_ptr(), 1, length, hist.data_ptr(), None, None, n, h, w, 2, 2, None]
    for position in (0, 2, 5):                                                      # NULL y / bin widths / hist
        assert call(*(good[:position] + [None] + good[position + 1:])) == -1, position
    for (position, value) in ((3, 0), (3, -1), (3, most + 1), (4, 0), (4, 256), (4, 255), (8, 0), (9, 0), (10, -1), (11, 0), (12, -2)):
        assert call(*(good[:position] + [value] + good[position + 1:])) == -1, (position, value)
    assert call(*(good[:9] + [1 << 15, 1 << 15] + good[11:])) == -2                 # a plane of 2^30 latents
    assert call(*(good[:8] + [1 << 12, 1 << 10, 1 << 10, 1, 1] + good[13:])) == -2  # 2^32 tiles
    torch.cuda.synchronize()
    assert not hist.any().item()                                                    # nothing was launched
    with pytest.raises(ValueError):
        dev.ladder_histograms_tiles(y_d, bw_d, (2, 2), None, 0)
    with pytest.raises(ValueError):
        dev.ladder_histograms_tiles(y_d, bw_d, (0, 2), None, length)
    with pytest.raises(dev.HipError):
        dev.ladder_histograms_tiles(y_d.view(n, h*w, NB_MAPS), bw_d, (2, 2), None, length)
    with pytest.raises(dev.HipError):
        dev.ladder_histograms_tiles(y_d, bw_d[:, :64].contiguous(), (2, 2), None, length)


# ---- ladder_select_tiles -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def run_order_images(n, h, w, coding_tile, exception):
    """int32 [entries]: the image of every entry of `codec.coding_tile_layout` in RUN order, and the number of shape classes."""
    from autoencoder_based_image_compression_amd import codec
    layout = codec.coding_tile_layout(n, h, w, coding_tile, exception)
    images = numpy.array([layout['entries'][p][0] for p in layout['payload_entry'].tolist()], dtype=numpy.int32)
    # the static rows of the layout name the same images: the exception map of image i takes row 128 + i
    if exception >= 0:
        assert numpy.array_equal(layout['prob_row'].reshape(-1, NB_MAPS)[:, exception], NB_MAPS + images)
    return images, len(layout['runs'])


def expected_selection(rc, hist, bypass, ladder, h, w, coding_tile, budgets, row_base, entry_image):
    """The host rule -> (point int32 (N,), prob_row int32 (entries, 128), upper int64 (N, K), flags int32 (N,))."""
    header = rc.header_bytes(ladder, 16*h, 16*w, coding_tile)
    upper = rc.upper_bounds_fixed_tiles(hist, bypass, ladder, h*w, header)
    valid = rc.valid_points(hist.sum(axis=2), h*w)
    (point, promised) = rc.select_by_upper_bound(upper, valid, budgets)
    flags = promised.astype(numpy.int32) + 2*(~valid.any(axis=1)).astype(numpy.int32)
    prob_row = point[entry_image][:, None]*NB_MAPS + numpy.arange(NB_MAPS)[None, :]
    if ladder.idx_map_exception >= 0:
        prob_row[:, ladder.idx_map_exception] = row_base + entry_image
    return point.astype(numpy.int32), prob_row.astype(numpy.int32), upper, flags


def run_select(dev, rc, guard, hist, bypass, ladder, h, w, coding_tile, seen):
    """`device.ladder_select_tiles` for every row of `budget_sweep` against the host rule; `seen` collects (point, flags) pairs."""
    (n, k_points) = hist.shape[:2]
    row_base = k_points*NB_MAPS
    (entry_image, nb_classes) = run_order_images(n, h, w, coding_tile, ladder.idx_map_exception)
    hist_d = guard.upload(hist.astype(numpy.int32))
    bypass_d = guard.upload(bypass.astype(numpy.int64))
    costs_d = guard.upload(rc.fixed_costs(ladder).view(numpy.int32))
    logs_d = guard.upload(rc.log2_tables(h*w).view(numpy.int32)) if ladder.idx_map_exception >= 0 else None
    images_d = guard.upload(entry_image)
    header = rc.header_bytes(ladder, 16*h, 16*w, coding_tile)
    upper = rc.upper_bounds_fixed_tiles(hist, bypass, ladder, h*w, header)
    for budgets in budget_sweep(upper):
        out = dev.ladder_select_tiles(hist_d, bypass_d, costs_d, logs_d, ladder.idx_map_exception, header, h*w, guard.upload(budgets),
                                      images_d, row_base)
        (point, prob_row, upper_ref, flags) = expected_selection(rc, hist, bypass, ladder, h, w, coding_tile, budgets, row_base, entry_image)
        assert numpy.array_equal(out['upper'].cpu().numpy(), upper_ref)
        assert numpy.array_equal(out['point'].cpu().numpy(), point)
        assert numpy.array_equal(out['flags'].cpu().numpy(), flags)
        assert numpy.array_equal(out['prob_row'].cpu().numpy(), prob_row)
        seen.update(zip(point.tolist(), flags.tolist()))
    return nb_classes


@pytest.mark.parametrize('exception', [-1, 5], ids=['no_exception', 'exception'])
@pytest.mark.parametrize('k_points, length', [(1, 10), (3, 10), (9, 10), (3, 1), (3, 3), (3, 33)])
def test_ladder_select_tiles_on_the_histograms_of_random_latents(dev, rc, guard, k_points, length, exception):
    """Plane 5 x 8 with tiles of (2, 3): four shape classes (2 x 3, 1 x 3, 2 x 2, 1 x 2), nine tiles; images of another entropy each
    take another point at one budget. One element of image 0 leaves int16 at point 0."""
    seen = set()
    (h, w, coding_tile) = (5, 8, (2, 3))
    for n in (1, 3, 5):
        (y, ladder) = random_latents(n, h*w, k_points, length, exception)
        (hist, bypass, errors) = dev.ladder_histograms_tiles(guard.upload(y.reshape(n, h, w, NB_MAPS)), guard.upload(ladder.bin_widths_points),
                                                             coding_tile, guard.upload(ladder.map_mean), length)
        (hist, bypass) = (hist.cpu().numpy().astype(numpy.int64), bypass.cpu().numpy())
        assert errors.cpu().numpy().tolist() == [1] + [0]*(k_points - 1)
        valid = rc.valid_points(hist.sum(axis=2), h*w)
        assert not valid[0, 0] and valid[1:].all()
        assert run_select(dev, rc, guard, hist, bypass, ladder, h, w, coding_tile, seen) == 4
    assert {(k, 1) for k in range(k_points)} <= seen and (k_points - 1, 0) in seen
    assert ((0, 2) in seen) == (k_points == 1)


@pytest.mark.parametrize('length, coding_tile, exception', [(10, (4, 4), 7), (10, (4, 4), -1), (3, (8, 8), 7), (33, (1, 1), 7), (10, (16, 16), 7)])
def test_ladder_select_tiles_on_synthetic_histograms(dev, rc, guard, length, coding_tile, exception):
    """tests/test_tiled_budget_rule_host.py's cases on a plane of 11 x 13 (the exception map with Z == 0, O == 0 and T_ == 0 at some
    decision, tiles that hold none of a decision), with image 1 invalid at point 0 and image 2 at every point (a symbol short)."""
    (h, w) = (11, 13)
    (ladder, hist, bypass, _, _) = tiled_case(length, h, w, coding_tile, exception)
    hist = hist.copy()
    hist[1, 0, 0, 10, 0] -= 1
    hist[2, :, -1, 11, 0] -= 1
    valid = rc.valid_points(hist.sum(axis=2), h*w)
    assert valid.tolist() == [[True]*3, [False, True, True], [False]*3]
    seen = set()
    run_select(dev, rc, guard, hist, bypass, ladder, h, w, coding_tile, seen)
    assert seen == {(0, 1), (1, 1), (2, 1), (2, 0), (2, 2)}       # every point, nothing fits, no valid point


def test_ladder_select_tiles_writes_every_output_element(dev, rc, guard):
    import torch
    (h, w, coding_tile) = (11, 13, (4, 4))
    (ladder, hist, bypass, _, _) = tiled_case(3, h, w, coding_tile, 7)
    (n, k) = hist.shape[:2]
    header = rc.header_bytes(ladder, 16*h, 16*w, coding_tile)
    budgets = rc.upper_bounds_fixed_tiles(hist, bypass, ladder, h*w, header)[:, 1]
    (entry_image, _) = run_order_images(n, h, w, coding_tile, 7)
    args = (guard.upload(hist.astype(numpy.int32)), guard.upload(bypass), guard.upload(rc.fixed_costs(ladder).view(numpy.int32)),
            guard.upload(rc.log2_tables(h*w).view(numpy.int32)), 7, header, h*w, guard.upload(budgets), guard.upload(entry_image), k*NB_MAPS)
    results = []
    for fill in (0x55, 0xAA):
        out = {'point': torch.empty(n, dtype=torch.int32, device='cuda'),
               'prob_row': torch.empty((entry_image.size, NB_MAPS), dtype=torch.int32, device='cuda'),
               'upper': torch.empty((n, k), dtype=torch.int64, device='cuda'), 'flags': torch.empty(n, dtype=torch.int32, device='cuda')}
        for t in out.values():
            t.view(torch.uint8).fill_(fill)
        dev.ladder_select_tiles(*args, out=out)
        results.append({name: t.cpu().numpy() for (name, t) in out.items()})
    for name in results[0]:
        assert numpy.array_equal(results[0][name], results[1][name]), name
    assert results[0]['point'].tolist() == [1, 1, 1]


def test_ladder_select_tiles_refuses_bad_arguments(dev, rc, guard):
    import torch
    from autoencoder_based_image_compression_amd import _native
    lib = _native.hip()
    (h, w, coding_tile, length) = (11, 13, (8, 8), 3)
    (ladder, hist, bypass, _, _) = tiled_case(length, h, w, coding_tile, 7)
    (n, k, nb_tiles) = hist.shape[:3]
    (entry_image, _) = run_order_images(n, h, w, coding_tile, 7)
    tensors = (guard.upload(hist.astype(numpy.int32)), guard.upload(bypass), guard.upload(rc.fixed_costs(ladder).view(numpy.int32)),
               guard.upload(rc.log2_tables(h*w).view(numpy.int32)), guard.upload(numpy.full(n, 10**6, dtype=numpy.int64)),
               guard.upload(entry_image))
    (hp, bp, cp, lp, gp, ep) = (t.data_ptr() for t in tensors)
    outs = (torch.full((n,), -7, dtype=torch.int32, device='cuda'), torch.full((entry_image.size, NB_MAPS), -7, dtype=torch.int32, device='cuda'),
            torch.full((n, k), -7, dtype=torch.int64, device='cuda'), torch.full((n,), -7, dtype=torch.int32, device='cuda'))
    (pp, rp, up, fp) = (t.data_ptr() for t in outs)
    call = lib.eae_hip_ladder_select_tiles
    good = [hp, bp, cp, lp, k, length, 7, 1000, h*w, nb_tiles, gp, ep, int(entry_image.size), k*NB_MAPS, pp, rp, up, fp, n, None]
    for position in (0, 1, 2, 10, 11, 14, 15, 16, 17):            # a NULL among the required pointers
        assert call(*(good[:position] + [None] + good[position + 1:])) == -1, position
    assert call(*(good[:3] + [None] + good[4:])) == -1            # an exception map without log tables
    for (position, value) in ((4, 0), (4, dev.ladder_max_points(length) + 1), (5, 0), (5, 256), (6, 128), (7, -1), (8, 0), (9, 0), (12, 0),
                              (13, -1), (18, 0), (2, cp + 4), (16, up + 4)):
        assert call(*(good[:position] + [value] + good[position + 1:])) == -1, (position, value)
    assert call(*(good[:8] + [(1 << 24) + 1] + good[9:])) == -2   # EAE_HIP_BAD_SHAPE: a map beyond the tables
    assert call(*(good[:9] + [h*w + 1] + good[10:])) == -2        # more tiles than a map has symbols
    torch.cuda.synchronize()
    assert all(bool((t == -7).all().item()) for t in outs)        # nothing was launched
    with pytest.raises(dev.HipError):
        dev.ladder_select_tiles(tensors[0][:, :, 0], tensors[1], tensors[2], tensors[3], 7, 1000, h*w, tensors[4], tensors[5], k*NB_MAPS)
    with pytest.raises(dev.HipError):
        dev.ladder_select_tiles(tensors[0], tensors[1], tensors[2], tensors[3], 7, 1000, h*w, tensors[4], tensors[5].long(), k*NB_MAPS)
