"""The selection of csrc/hip/budget.hip and the quantiser of csrc/hip/latent_rows.hip that takes its points, on poisoned buffers between
guard bands under both poisons (tests/guarded.py):

* eae_hip_ladder_select (device.ladder_select) against the host rule it restates in integers -- ratecontrol.upper_bounds_fixed,
  valid_points, select_by_upper_bound --, element for element: on the histograms device.ladder_histograms leaves for random latents,
  and on synthetic histograms uploaded directly (maps of 16,384 symbols: the 64-bit sums; invalid points; the exception map's corner
  cases), with budgets at and one byte under every bound;
* eae_hip_latent_quantize_rows (device.latent_quantize_rows) against device.latent_stage image by image, bit for bit: tiles of 32
  positions that straddle two and three images, a ragged last tile, every image at another point; every optional output absent in turn.

Every comparison is exact."""
import functools

import numpy
import pytest

from test_budget_rule_host import case

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


# ---- ladder_select -----------------------------------------------------------------------------------------------------------------

def expected_selection(rc, hist, bypass, ladder, map_size, budgets, row_base):
    """The host rule -> (point int32 (N,), prob_row int32 (N, 128), upper int64 (N, K), flags int32 (N,))."""
    upper = rc.upper_bounds_fixed(hist, bypass, ladder, map_size)
    valid = rc.valid_points(hist, map_size)
    (point, promised) = rc.select_by_upper_bound(upper, valid, budgets)
    flags = promised.astype(numpy.int32) + 2*(~valid.any(axis=1)).astype(numpy.int32)
    prob_row = point[:, None]*NB_MAPS + numpy.arange(NB_MAPS)[None, :]
    if ladder.idx_map_exception >= 0:
        prob_row[:, ladder.idx_map_exception] = row_base + numpy.arange(hist.shape[0])
    return point.astype(numpy.int32), prob_row.astype(numpy.int32), upper, flags


def budget_sweep(upper):
    """Budgets at and one byte under every bound, then one nothing fits and one everything fits: int64 (2 K + 2, N)."""
    rows = []
    for j in range(upper.shape[1]):
        rows += [upper[:, j], upper[:, j] - 1]
    rows += [numpy.zeros(upper.shape[0], dtype=numpy.int64), upper.max(axis=1) + 1]
    return numpy.stack(rows).astype(numpy.int64)


def run_select(dev, rc, guard, hist, bypass, ladder, map_size, seen):
    """`device.ladder_select` for every row of `budget_sweep` against the host rule; `seen` collects (point, flags) pairs."""
    (n, k_points) = hist.shape[:2]
    row_base = k_points*NB_MAPS
    hist_d = guard.upload(hist.astype(numpy.int32))
    bypass_d = guard.upload(bypass.astype(numpy.int64))
    costs_d = guard.upload(rc.fixed_costs(ladder).view(numpy.int32))
    logs_d = guard.upload(rc.log2_tables(map_size).view(numpy.int32)) if ladder.idx_map_exception >= 0 else None
    upper = rc.upper_bounds_fixed(hist, bypass, ladder, map_size)
    for budgets in budget_sweep(upper):
        out = dev.ladder_select(hist_d, bypass_d, costs_d, logs_d, ladder.idx_map_exception, rc.header_bytes(ladder), map_size,
                                guard.upload(budgets), row_base)
        (point, prob_row, upper_ref, flags) = expected_selection(rc, hist, bypass, ladder, map_size, budgets, row_base)
        assert numpy.array_equal(out['upper'].cpu().numpy(), upper_ref)
        assert numpy.array_equal(out['point'].cpu().numpy(), point)
        assert numpy.array_equal(out['flags'].cpu().numpy(), flags)
        assert numpy.array_equal(out['prob_row'].cpu().numpy(), prob_row)
        seen.update(zip(point.tolist(), flags.tolist()))


@functools.lru_cache(maxsize=None)
def random_latents(n, hw, k_points, length, exception):
    """(y [n, hw, 128], ladder): Laplacian latents, the points 1, 1.5, 2, ... times as coarse, a seeded table; one element of image 0
    leaves int16 at point 0 only (every coarser point is at least 1.5 times as wide)."""
    from autoencoder_based_image_compression_amd import ratecontrol
    rng = numpy.random.RandomState(100*n + 10*k_points + length)
    bw0 = rng.uniform(0.25, 2., size=NB_MAPS).astype(F32)
    bw = (bw0[None, :]*(1. + 0.5*numpy.arange(k_points, dtype=numpy.float64))[:, None]).astype(F32)
    mean = (rng.standard_normal(NB_MAPS)*0.2).astype(F32)
    y = ((rng.laplace(size=(n, hw, NB_MAPS))*rng.uniform(0.1, 8., size=NB_MAPS)).astype(F32)*bw0 + mean).astype(F32)
    y[0, 1, 17] = F32(40000.)*bw0[17] + mean[17]
    # (one table for every point, a zero cheaper than a one: a coarser point then costs less, and the sweep below reaches every point)
    tables = numpy.tile(rng.uniform(0.5, 0.98, size=(1, NB_MAPS, length)), (k_points, 1, 1))
    return y, ratecontrol.RateLadder(bw, tables, mean, exception)


@pytest.mark.parametrize('exception', [-1, 5], ids=['no_exception', 'exception'])
@pytest.mark.parametrize('k_points, length', [(1, 10), (3, 10), (9, 10), (3, 1), (3, 3), (3, 33)])
def test_ladder_select_on_the_histograms_of_random_latents(dev, rc, guard, k_points, length, exception):
    seen = set()
    hw = 40
    for n in range(1, 6):
        (y, ladder) = random_latents(n, hw, k_points, length, exception)
        (hist, bypass, errors) = dev.ladder_histograms(guard.upload(y), guard.upload(ladder.bin_widths_points), guard.upload(ladder.map_mean), length)
        (hist, bypass) = (hist.cpu().numpy(), bypass.cpu().numpy())
        assert errors.cpu().numpy().tolist() == [1] + [0]*(k_points - 1)
        assert not rc.valid_points(hist, hw)[0, 0] and rc.valid_points(hist, hw)[1:].all()
        run_select(dev, rc, guard, hist, bypass, ladder, hw, seen)
    # every point was taken with its promise kept, the last one also without (nothing fitted), and with K = 1 image 0 had no valid point
    assert {(k, 1) for k in range(k_points)} <= seen and (k_points - 1, 0) in seen
    assert ((0, 2) in seen) == (k_points == 1)


@pytest.mark.parametrize('length, map_size, exception', [(10, 16384, 7), (10, 16384, -1), (3, 143, 7), (33, 12, 7)])
def test_ladder_select_on_synthetic_histograms(dev, rc, guard, length, map_size, exception):
    """tests/test_budget_rule_host.py's cases (an all-zero map; the exception map with zeros == 0, ones == 0 and t == 0 at some
    decision), with image 1 invalid at point 0 and image 2 at every point (a symbol short: an element that left int16)."""
    (ladder, hist, bypass) = case(length, map_size, exception)
    hist = hist.copy()
    hist[1, 0, 10, 0] -= 1
    hist[2, :, 11, 0] -= 1
    valid = rc.valid_points(hist, map_size)
    assert valid.tolist() == [[True]*3, [False, True, True], [False]*3]
    if map_size == 16384:
        assert int(rc.upper_bounds_fixed(hist, bypass, ladder, map_size).max()) > 500000      # sums of 2^-20 bits far beyond 32 bits
    seen = set()
    run_select(dev, rc, guard, hist, bypass, ladder, map_size, seen)
    assert seen == {(0, 1), (1, 1), (2, 1), (2, 0), (2, 2)}       # every point, nothing fits, no valid point


def test_ladder_select_writes_every_output_element(dev, rc, guard):
    """Outputs that held the other poison come back the same: nothing depends on what the buffers held (the autouse fixture's
    two poisons check the same for the wrapper's own allocations)."""
    import torch
    (ladder, hist, bypass) = case(3, 143, 7)
    (n, k) = hist.shape[:2]
    budgets = rc.upper_bounds_fixed(hist, bypass, ladder, 143)[:, 1]
    args = (guard.upload(hist.astype(numpy.int32)), guard.upload(bypass), guard.upload(rc.fixed_costs(ladder).view(numpy.int32)),
            guard.upload(rc.log2_tables(143).view(numpy.int32)), 7, rc.header_bytes(ladder), 143, guard.upload(budgets), k*NB_MAPS)
    results = []
    for fill in (0x55, 0xAA):
        out = {'point': torch.empty(n, dtype=torch.int32, device='cuda'), 'prob_row': torch.empty((n, NB_MAPS), dtype=torch.int32, device='cuda'),
               'upper': torch.empty((n, k), dtype=torch.int64, device='cuda'), 'flags': torch.empty(n, dtype=torch.int32, device='cuda')}
        for t in out.values():
            t.view(torch.uint8).fill_(fill)
        dev.ladder_select(*args, out=out)
        results.append({name: t.cpu().numpy() for (name, t) in out.items()})
    for name in results[0]:
        assert numpy.array_equal(results[0][name], results[1][name]), name
    assert results[0]['point'].tolist() == [1, 1, 1]


def test_ladder_select_refuses_bad_arguments(dev, rc, guard):
    import torch
    from autoencoder_based_image_compression_amd import _native
    lib = _native.hip()
    (ladder, hist, bypass) = case(3, 12, 7)
    (n, k, length, map_size) = (3, 3, 3, 12)
    tensors = (guard.upload(hist.astype(numpy.int32)), guard.upload(bypass), guard.upload(rc.fixed_costs(ladder).view(numpy.int32)),
               guard.upload(rc.log2_tables(map_size).view(numpy.int32)), guard.upload(numpy.full(n, 10**6, dtype=numpy.int64)))
    (hp, bp, cp, lp, gp) = (t.data_ptr() for t in tensors)
    outs = (torch.full((n,), -7, dtype=torch.int32, device='cuda'), torch.full((n, NB_MAPS), -7, dtype=torch.int32, device='cuda'),
            torch.full((n, k), -7, dtype=torch.int64, device='cuda'), torch.full((n,), -7, dtype=torch.int32, device='cuda'))
    (pp, rp, up, fp) = (t.data_ptr() for t in outs)
    call = lib.eae_hip_ladder_select
    good = [hp, bp, cp, lp, k, length, 7, 1000, map_size, gp, k*NB_MAPS, pp, rp, up, fp, n, None]
    for position in (0, 1, 2, 9, 11, 12, 13, 14):                 # a NULL among the required pointers
        assert call(*(good[:position] + [None] + good[position + 1:])) == -1, position
    assert call(*(good[:3] + [None] + good[4:])) == -1            # an exception map without log tables
    for (position, value) in ((4, 0), (4, dev.ladder_max_points(length) + 1), (5, 0), (5, 256), (6, 128), (7, -1), (8, 0), (10, -1), (15, 0),
                              (2, cp + 4), (13, up + 4)):
        assert call(*(good[:position] + [value] + good[position + 1:])) == -1, (position, value)
    assert call(*(good[:8] + [(1 << 24) + 1] + good[9:])) == -2   # EAE_HIP_BAD_SHAPE
    torch.cuda.synchronize()
    assert all(bool((t == -7).all().item()) for t in outs)        # nothing was launched
    assert call(*(good[:3] + [None] + good[4:6] + [-1] + good[7:])) == 0       # no exception map: the log tables may be NULL
    torch.cuda.synchronize()
    with pytest.raises(dev.HipError):
        dev.ladder_select(tensors[0], tensors[1], tensors[2][:, :64].contiguous(), tensors[3], 7, 1000, map_size, tensors[4], k*NB_MAPS)
    with pytest.raises(dev.HipError):
        dev.ladder_select(tensors[0], tensors[1], tensors[2], tensors[3], 7, 1000, map_size, tensors[4][:2].contiguous(), k*NB_MAPS)


# ---- latent_quantize_rows ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def quantiser_inputs(n, hw, k_points, points):
    """(y, bin widths [K, 128], mean, gamma, beta): a quarter of the elements are exact half-way cases (j + 0.5) * bw + m of the
    image's OWN point, one element of image 0 leaves int16, map 9 is dead everywhere."""
    rng = numpy.random.RandomState(1000*n + hw + 7*k_points + sum(points))
    bw0 = rng.uniform(0.25, 2., size=NB_MAPS).astype(F32)
    bw0[::5] = F32(0.5)
    bw = (bw0[None, :]*(2.**numpy.arange(k_points))[:, None]).astype(F32)
    mean = (rng.standard_normal(NB_MAPS)*0.2).astype(F32)
    y = (rng.laplace(size=(n, hw, NB_MAPS))*3.).astype(F32)*bw0 + mean
    j = rng.randint(-12, 13, size=(n, hw, NB_MAPS)).astype(F32)
    own = bw[numpy.clip(numpy.asarray(points), 0, k_points - 1)][:, None, :]
    y = numpy.where(rng.randint(0, 4, size=y.shape) == 0, (j + F32(0.5))*own + mean, y).astype(F32)
    y[:, :, 9] = mean[9] + F32(1e-3)
    y[0, hw//2, 17] = F32(40000.)*own[0, 0, 17] + mean[17]
    gamma = rng.uniform(2e-5, 0.01, size=(NB_MAPS, NB_MAPS)).astype(F32)
    beta = rng.uniform(0.5, 2., size=NB_MAPS).astype(F32)
    return y, bw, mean, gamma, beta


def bits_of(tensor):
    """A float32 tensor as its bit patterns: NaNs compare like everything else."""
    return tensor.cpu().numpy().view(numpy.int32)


CASES = [(3, 143, 3, (2, 0, 1)), (3, 143, 3, (1, 1, 1)), (3, 143, 1, (0, 0, 0)),        # tiles straddle images, the last one is ragged
         (5, 12, 3, (2, 0, 1, 1, 2)), (5, 12, 3, (0, 0, 0, 0, 0)), (5, 12, 1, (0, 0, 0, 0, 0)),      # one tile spans three images
         (2, 64, 3, (1, 0)), (2, 64, 3, (2, 2)), (2, 64, 1, (0, 0)),
         (3, 143, 3, (-3, 7, 1))]                                                          # outside [0, K): clamped to 0 and K - 1


@pytest.mark.parametrize('learned', [False, True], ids=['fixed', 'learned'])
@pytest.mark.parametrize('n, hw, k_points, points', CASES)
def test_latent_quantize_rows_equals_latent_stage_image_by_image(dev, guard, n, hw, k_points, points, learned):
    import torch
    (y, bw, mean, gamma, beta) = quantiser_inputs(n, hw, k_points, points)
    (y_d, bw_d, mean_d) = (guard.upload(y), guard.upload(bw), guard.upload(mean))
    igdn = None if learned else (dev.pack_gamma(guard.upload(gamma)), guard.upload(beta))
    rows = dev.latent_quantize_rows(y_d, bw_d, guard.upload(numpy.asarray(points, dtype=numpy.int32)), mean_d, igdn_out=igdn,
                                    want_shifted=True, want_flags=True)
    assert (rows['t'] is None) == learned
    checks = numpy.zeros(3, dtype=numpy.int64)
    for i in range(n):
        k = min(max(points[i], 0), k_points - 1)
        one = dev.latent_stage(y_d[i:i + 1], bw_d[k], mean_d, gdn_in=None, igdn_out=igdn, want_shifted=True, want_flags=True)
        assert torch.equal(rows['symbols'][i], one['symbols'][0]), i
        assert torch.equal(rows['nonzero_flags'][i], one['nonzero_flags'][0]), i
        assert numpy.array_equal(bits_of(rows['shifted'][i]), bits_of(one['shifted'][0])), i
        if not learned:
            assert numpy.array_equal(bits_of(rows['t'][i]), bits_of(one['t'][0])), i
        checks += one['checks'].cpu().numpy()
    assert numpy.array_equal(rows['checks'].cpu().numpy(), checks)
    assert checks[0] == 1                                          # the one element outside int16
    assert int(rows['nonzero_flags'][:, 9].sum()) == 0 and int(rows['nonzero_flags'].sum()) > n*100


def test_the_points_matter(dev, guard):
    """The comparison above has teeth: with every image at point 0 the symbols of an image that belongs at point 2 differ."""
    import torch
    (n, hw, k_points, points) = CASES[0]
    (y, bw, mean, _, _) = quantiser_inputs(n, hw, k_points, points)
    (y_d, bw_d, mean_d) = (guard.upload(y), guard.upload(bw), guard.upload(mean))
    own = dev.latent_quantize_rows(y_d, bw_d, guard.upload(numpy.asarray(points, dtype=numpy.int32)), mean_d)
    first = dev.latent_quantize_rows(y_d, bw_d, guard.upload(numpy.zeros(n, dtype=numpy.int32)), mean_d)
    assert torch.equal(own['symbols'][1], first['symbols'][1]) and not torch.equal(own['symbols'][0], first['symbols'][0])


@pytest.mark.parametrize('absent', ['shifted', 'symbols', 'nonzero_flags', 'checks'])
@pytest.mark.parametrize('learned', [False, True], ids=['fixed', 'learned'])
def test_latent_quantize_rows_every_optional_output_absent_in_turn(dev, guard, learned, absent):
    """The null-output branches of the four-wave body (csrc/hip/quarter_body.h). n = 3, hw = 33: the tiles of 32 positions straddle
    images (the per-lane flag path) or lie inside one (the packed path), and the last tile is ragged."""
    import torch
    (n, hw, k_points, points) = (3, 33, 3, (2, 0, 1))
    (y, bw, mean, gamma, beta) = quantiser_inputs(n, hw, k_points, points)
    (y_d, bw_d, mean_d, point_d) = (guard.upload(y), guard.upload(bw), guard.upload(mean), guard.upload(numpy.asarray(points, dtype=numpy.int32)))
    igdn = None if learned else (dev.pack_gamma(guard.upload(gamma)), guard.upload(beta))
    full = dev.latent_quantize_rows(y_d, bw_d, point_d, mean_d, igdn_out=igdn, want_shifted=True, want_symbols=True, want_flags=True,
                                    want_checks=True)
    part = dev.latent_quantize_rows(y_d, bw_d, point_d, mean_d, igdn_out=igdn, want_shifted=absent != 'shifted',
                                    want_symbols=absent != 'symbols', want_flags=absent != 'nonzero_flags', want_checks=absent != 'checks')
    assert part[absent] is None and (full['t'] is None) == learned
    assert int(full['checks'][0]) == 1 and int(full['nonzero_flags'][:, 9].sum()) == 0 and int(full['nonzero_flags'].sum()) > n*100
    for name in ('shifted', 't', 'symbols', 'nonzero_flags', 'checks'):
        if name != absent and full[name] is not None:
            assert torch.equal(part[name], full[name]), name


def test_latent_quantize_rows_refuses_bad_arguments(dev, guard):
    import torch
    from autoencoder_based_image_compression_amd import _native
    lib = _native.hip()
    (n, hw, k) = (2, 64, 3)
    (y, bw, mean, gamma, beta) = quantiser_inputs(n, hw, k, (1, 0))
    (y_d, bw_d, g_d, b_d) = (guard.upload(y), guard.upload(bw), guard.upload(gamma), guard.upload(beta))
    point = guard.upload(numpy.zeros(n, dtype=numpy.int32))
    symbols = torch.full((n, NB_MAPS, hw), -7, dtype=torch.int16, device='cuda')
    t = torch.full((n, hw, NB_MAPS), -7., dtype=torch.float32, device='cuda')
    call = lib.eae_hip_latent_quantize_rows
    good = [y_d.data_ptr(), None, bw_d.data_ptr(), point.data_ptr(), k, g_d.data_ptr(), b_d.data_ptr(), None, t.data_ptr(), symbols.data_ptr(),
            None, None, n, hw, None]
    for position in (0, 2, 3, 5, 6, 8):                           # NULL y / bin widths / point; gamma without beta, beta without gamma, no t_out
        assert call(*(good[:position] + [None] + good[position + 1:])) == -1, position
    for (position, value) in ((4, 0), (12, 0), (13, 0), (0, good[0] + 4), (2, good[2] + 8), (8, good[8] + 4)):
        assert call(*(good[:position] + [value] + good[position + 1:])) == -1, (position, value)
    assert call(*(good[:13] + [(1 << 21) + 1] + good[14:])) == -2
    torch.cuda.synchronize()
    assert bool((symbols == -7).all().item()) and bool((t == -7.).all().item())          # nothing was launched
    with pytest.raises(dev.HipError):
        dev.latent_quantize_rows(y_d, bw_d, point.long(), None)
    with pytest.raises(dev.HipError):
        dev.latent_quantize_rows(y_d, bw_d[:, :64].contiguous(), point, None)
    with pytest.raises(dev.HipError):
        dev.latent_quantize_rows(y_d.double(), bw_d, point, None)
