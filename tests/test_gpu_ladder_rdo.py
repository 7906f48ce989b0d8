"""eae_hip_ladder_histograms_rdo and eae_hip_ladder_histograms_rdo_tiles (csrc/hip/ladder.hip) through device.ladder_histograms_rdo
and device.ladder_histograms_rdo_tiles, on poisoned buffers between guard bands under both poisons (tests/guarded.py): the ladder's
counts of the symbols the rate-distortion optimised quantiser chooses, against

(a) numpy float32: ratecontrol.rdo_quantize_numpy per point, then rint(bw * r / bw), the bins and the bits of test_gpu_ladder.py;
(b) device.ladder_histograms[_tiles] on the same input, word for word, with thresholds of zero;
(c) device.latent_quantize_rdo with point == k followed by symbol_histograms: the symbols counted are the symbols coded;
(d) the tiles form summed over the tiles against the whole-map form.

The inputs are test_gpu_ladder.py's (ties, exact multiples, large symbols, range errors at point 0) with elements placed just below,
at and just above a threshold: |x| = a + (t - 1) / 2 and its two float32 neighbours, both signs. Every comparison is exact."""
import functools

import numpy
import pytest

from test_gpu_ladder import inputs, suffix_bits

pytestmark = pytest.mark.gpu

F32 = numpy.float32
NB_MAPS = 128
MAGNITUDES = 16
SHAPES = [(1, 1), (1, 24), (3, 65), (2, 1536)]
LENGTHS = [1, 4, 10, 20]                # 20: only 16 magnitudes have a threshold
PLANES = [(2, 5, 7, (2, 3)), (2, 11, 13, (4, 4)), (2, 11, 13, (16, 16)), (2, 32, 48, (16, 16))]
#          ^ ragged tiles            ^ four shape classes    ^ clamped: one tile     ^ 12 tiles for ~512 blocks: cut into chunks


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


@functools.lru_cache(maxsize=None)
def rdo_inputs(n, hw, k_points, length, with_mean, table='random'):
    """(y [n, hw, 128], bin widths [K, 128], mean or None, thresholds [K, 128, 16]). table: 'random' -- per point, uniform in
    (0.05, 1.95) in the min(L, 16) columns a magnitude can have, a tenth of them 0 (a step that saves nothing) --, 'zero', or 'three'
    (3.0 in all 16 columns: above every 2 u + 1, and what lies beyond min(L, 16) must not be read as a threshold of a magnitude
    > L). With 'random', an eighth of the elements (at most 1200) sit on a threshold: for a point k, a magnitude a and a map c with
    t = thresholds[k, c, a - 1] > 0, |x| = a + (t - 1) / 2 or one of its two float32 neighbours, either sign."""
    (y, bw, mean) = inputs(n, hw, k_points, length, with_mean)
    y = y.copy()
    rng = numpy.random.RandomState(77 + 1000*n + hw + 7*k_points + length)
    used = min(length, MAGNITUDES)
    thresholds = numpy.zeros((k_points, NB_MAPS, MAGNITUDES), dtype=F32)
    if table == 'three':
        thresholds[:] = F32(3.)
    elif table == 'random':
        thresholds[:, :, :used] = rng.uniform(0.05, 1.95, size=(k_points, NB_MAPS, used)).astype(F32)
        thresholds[rng.rand(k_points, NB_MAPS, MAGNITUDES) < 0.1] = F32(0.)
        flat = y.reshape(n*hw, NB_MAPS)
        m = mean if with_mean else numpy.zeros(NB_MAPS, dtype=F32)
        for _ in range(min(n*hw*NB_MAPS//24, 400)):
            (k, a, c) = (rng.randint(k_points), rng.randint(1, used + 1), rng.randint(NB_MAPS))
            t = thresholds[k, c, a - 1]
            if t == 0.:
                continue
            on = F32(a) + (t - F32(1.))/F32(2.)
            sign = F32(1.) if rng.rand() < 0.5 else F32(-1.)
            for x in (numpy.nextafter(on, F32(0.)), on, numpy.nextafter(on, F32(64.))):
                flat[rng.randint(n*hw), c] = sign*F32(x)*bw[k, c] + m[c]
    return y, bw, mean, thresholds


@functools.lru_cache(maxsize=None)
def rdo_symbols(n, hw, k_points, length, with_mean, table='random'):
    """Per point, in numpy float32: (magnitudes int64 [K, n, hw, 128], 0 where the symbol leaves int16; good bool: where it does not;
    eligible, lowered bool: what the rule could lower and what it lowered)."""
    from autoencoder_based_image_compression_amd import ratecontrol
    (y, bw, mean, thresholds) = rdo_inputs(n, hw, k_points, length, with_mean, table)
    centered = y - mean if with_mean else y - F32(0.)
    amax = F32(min(length, MAGNITUDES))
    (magnitudes, good, eligible, lowered) = ([], [], [], [])
    for k in range(k_points):
        with numpy.errstate(all='ignore'):
            nearest = numpy.rint(centered/bw[k])
            r = ratecontrol.rdo_quantize_numpy(y, bw[k], mean, thresholds[k], length)
            rs = numpy.rint(bw[k]*r/bw[k])
        assert r.dtype == F32 and rs.dtype == F32
        good.append(numpy.abs(rs) < F32(32768.))
        magnitudes.append(numpy.where(good[-1], numpy.abs(rs), 0).astype(numpy.int64))
        eligible.append((numpy.abs(nearest) >= F32(1.)) & (numpy.abs(nearest) <= amax))
        lowered.append(r != nearest)
        assert not (lowered[-1] & ~eligible[-1]).any() and (numpy.abs(r[lowered[-1]]) == numpy.abs(nearest[lowered[-1]]) - 1).all()
    return numpy.stack(magnitudes), numpy.stack(good), numpy.stack(eligible), numpy.stack(lowered)


def lowered_shares(n, hw, k_points, length, with_mean, table='random'):
    (_, _, eligible, lowered) = rdo_symbols(n, hw, k_points, length, with_mean, table)
    return [lowered[k].sum()/max(int(eligible[k].sum()), 1) for k in range(k_points)]


@functools.lru_cache(maxsize=None)
def reference(n, hw, k_points, length, with_mean, table='random'):
    """(hist int64 [n, K, 128, L + 1], bypass bits [n, K, 128], range errors [K]) of the RDO symbols."""
    (magnitudes, good, _, _) = rdo_symbols(n, hw, k_points, length, with_mean, table)
    hist = numpy.zeros((n, k_points, NB_MAPS, length + 1), dtype=numpy.int64)
    clipped = numpy.minimum(magnitudes, length)
    for b in range(length + 1):
        hist[..., b] = (good & (clipped == b)).sum(axis=2).transpose(1, 0, 2)
    bits = (suffix_bits(magnitudes, length)*good).sum(axis=2).transpose(1, 0, 2)
    return hist, bits, (~good).sum(axis=(1, 2, 3))


@functools.lru_cache(maxsize=None)
def tile_reference(n, h, w, coding_tile, k_points, length, table='random'):
    """The same per coding tile: (hist [n, K, T, 128, L + 1], bits [n, K, T, 128], range errors [K])."""
    from autoencoder_based_image_compression_amd import container
    (magnitudes, good, _, _) = rdo_symbols(n, h*w, k_points, length, True, table)
    (tiles, _) = container.coding_tile_grid(h, w, (min(coding_tile[0], h), min(coding_tile[1], w)))
    (magnitudes, good) = (magnitudes.reshape(k_points, n, h, w, NB_MAPS), good.reshape(k_points, n, h, w, NB_MAPS))
    clipped = numpy.minimum(magnitudes, length)
    bypass = suffix_bits(magnitudes, length)*good
    hist = numpy.zeros((n, k_points, len(tiles), NB_MAPS, length + 1), dtype=numpy.int64)
    bits = numpy.zeros((n, k_points, len(tiles), NB_MAPS), dtype=numpy.int64)
    for (t, (r0, c0, nr, nc, _)) in enumerate(tiles.tolist()):
        window = (slice(None), slice(None), slice(r0, r0 + nr), slice(c0, c0 + nc))
        for b in range(length + 1):
            hist[:, :, t, :, b] = (good[window] & (clipped[window] == b)).sum(axis=(2, 3)).transpose(1, 0, 2)
        bits[:, :, t] = bypass[window].sum(axis=(2, 3)).transpose(1, 0, 2)
    return hist, bits, (~good).sum(axis=(1, 2, 3, 4))


def uploaded(guard, n, hw, k_points, length, with_mean, table='random', plane=None):
    (y, bw, mean, thresholds) = rdo_inputs(n, hw, k_points, length, with_mean, table)
    y_d = guard.upload(y if plane is None else y.reshape((n,) + plane + (NB_MAPS,)))
    return y_d, guard.upload(bw), guard.upload(mean) if with_mean else None, guard.upload(thresholds)


def run(dev, guard, n, hw, k_points, length, with_mean, table='random', **kwargs):
    (y_d, bw_d, mean_d, thr_d) = uploaded(guard, n, hw, k_points, length, with_mean, table)
    return tuple(t.cpu().numpy() for t in dev.ladder_histograms_rdo(y_d, bw_d, thr_d, mean_d, length, **kwargs))


def equal(got, expected):
    return all(g.shape == e.shape and numpy.array_equal(g, e) for (g, e) in zip(got, expected)) and len(got) == len(expected)


# ---- the whole-map form ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_mean', [False, True], ids=['no_mean', 'mean'])
@pytest.mark.parametrize('k_points', [1, 3])
@pytest.mark.parametrize('length', LENGTHS)
@pytest.mark.parametrize('n, hw', SHAPES)
def test_against_the_numpy_symbols(dev, guard, n, hw, k_points, length, with_mean):
    expected = reference(n, hw, k_points, length, with_mean)
    # the reference is one RDO moves: at some point it lowers between a tenth and nine tenths of what it could lower
    shares = lowered_shares(n, hw, k_points, length, with_mean)
    assert any(0.1 <= share <= 0.9 for share in shares), shares
    if hw >= 24:
        assert expected[2][0] > 0 and not expected[2][1:].any()          # range errors at the finest point only
    if k_points > 1:
        (_, _, _, thresholds) = rdo_inputs(n, hw, k_points, length, with_mean)
        assert not numpy.array_equal(thresholds[0], thresholds[1])         # per-point tables that differ
    assert equal(run(dev, guard, n, hw, k_points, length, with_mean), expected)


@pytest.mark.parametrize('length', LENGTHS)
@pytest.mark.parametrize('n, hw', SHAPES)
def test_thresholds_of_zero_give_the_words_of_nearest_rounding(dev, guard, n, hw, length):
    (y_d, bw_d, mean_d, thr_d) = uploaded(guard, n, hw, 3, length, True, 'zero')
    assert not thr_d.any().item()
    got = dev.ladder_histograms_rdo(y_d, bw_d, thr_d, mean_d, length)
    nearest = dev.ladder_histograms(y_d, bw_d, mean_d, length)
    for (a, b) in zip(got, nearest):
        assert a.dtype == b.dtype and a.shape == b.shape and numpy.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert got[0].any().item()


@pytest.mark.parametrize('length', LENGTHS)
@pytest.mark.parametrize('n, hw', SHAPES)
def test_thresholds_above_every_cost_lower_every_eligible_symbol(dev, guard, n, hw, length):
    """3.0 > 2 u + 1 for every u in [-1/2, 1/2]: every magnitude 1 .. min(L, 16) goes down by one, 1 becomes 0 and loses its sign
    bit; a magnitude beyond min(L, 16) stays although its column of the table holds 3.0 too."""
    (_, _, eligible, lowered) = rdo_symbols(n, hw, 3, length, True, 'three')
    assert eligible.any() and numpy.array_equal(eligible, lowered)
    expected = reference(n, hw, 3, length, True, 'three')
    nearest = reference(n, hw, 3, length, True, 'zero')
    assert expected[1].sum() < nearest[1].sum() and expected[0][..., 0].sum() > nearest[0][..., 0].sum()
    assert equal(run(dev, guard, n, hw, 3, length, True, 'three'), expected)


def test_outputs_accumulate_into_what_they_hold(dev, guard):
    import torch
    (n, hw, k_points, length) = (3, 65, 3, 4)
    rng = numpy.random.RandomState(5)
    start = (rng.randint(0, 1000, size=(n, k_points, NB_MAPS, length + 1)).astype(numpy.int32),
             rng.randint(0, 1 << 40, size=(n, k_points, NB_MAPS)).astype(numpy.int64), rng.randint(0, 1000, size=k_points).astype(numpy.int32))
    out = tuple(torch.from_numpy(a).cuda() for a in start)
    run(dev, guard, n, hw, k_points, length, True, out=out)
    got = run(dev, guard, n, hw, k_points, length, True, out=out)
    expected = reference(n, hw, k_points, length, True)
    assert equal(got, tuple(s.astype(numpy.int64) + 2*e for (s, e) in zip(start, expected)))


@pytest.mark.parametrize('length', [4, 10, 20])
@pytest.mark.parametrize('n, hw', [(3, 65), (2, 1536)])
def test_the_symbols_counted_are_the_symbols_the_quantiser_writes(dev, guard, n, hw, length):
    """hist[:, k] and bypass_bits[:, k] are those of latent_quantize_rdo's symbols with point == k, for every point without a range
    error (there the int16 symbols have wrapped)."""
    import torch
    k_points = 3
    (y_d, bw_d, mean_d, thr_d) = uploaded(guard, n, hw, k_points, length, True)
    (hist, bits, errors) = (t.cpu().numpy() for t in dev.ladder_histograms_rdo(y_d, bw_d, thr_d, mean_d, length))
    radius = 32768
    folded = 0
    for k in range(k_points):
        if errors[k]:
            continue
        point = torch.full((n,), k, dtype=torch.int32, device='cuda')
        q = dev.latent_quantize_rdo(y_d, bw_d, thr_d, point, length, mean_d, want_symbols=True)
        assert int(q['checks'][0].item()) == 0
        magnitudes = numpy.abs(q['symbols'].cpu().numpy().astype(numpy.int64)).reshape(n, NB_MAPS, hw)
        # through the device's own histogram too: bins -L .. L, everything beyond in `overflow`
        (full, overflow) = dev.symbol_histograms(q['symbols'], length)
        full = full.cpu().numpy().astype(numpy.int64).reshape(n, NB_MAPS, 2*length + 1)
        fold = full[:, :, length:].copy()
        fold[:, :, 1:] += full[:, :, :length][:, :, ::-1]
        fold[:, :, length] += overflow.cpu().numpy().astype(numpy.int64).reshape(n, NB_MAPS)
        assert numpy.array_equal(hist[:, k], fold)
        assert numpy.array_equal(bits[:, k], suffix_bits(magnitudes, length).sum(axis=2))
        assert magnitudes.max() < radius
        folded += 1
    assert folded == 2


def test_a_ladder_longer_than_a_launch_is_split(dev, guard):
    (n, hw, length) = (3, 65, 10)
    k_points = dev.ladder_max_points(length) + 1
    assert equal(run(dev, guard, n, hw, k_points, length, True), reference(n, hw, k_points, length, True))


def test_a_length_no_launch_takes_goes_the_two_pass_route(dev, guard):
    """L = 255: eae_hip_ladder_max_points is 0; the quantiser and the histogram passes give the same arrays, at the finest point,
    whose symbols leave int16, too."""
    (n, hw, k_points, length) = (3, 65, 2, 255)
    assert dev.ladder_max_points(length) == 0
    expected = reference(n, hw, k_points, length, True)
    assert expected[2][0] and not expected[2][1]
    assert equal(run(dev, guard, n, hw, k_points, length, True), expected)


def test_the_table_by_magnitude_may_be_handed_in(dev, guard):
    (n, hw, k_points, length) = (3, 65, 3, 10)
    (y_d, bw_d, mean_d, thr_d) = uploaded(guard, n, hw, k_points, length, True)
    by_magnitude = dev.rdo_thresholds_by_magnitude(thr_d)
    assert tuple(by_magnitude.shape) == (k_points, MAGNITUDES, NB_MAPS) and by_magnitude.is_contiguous()
    assert numpy.array_equal(by_magnitude.cpu().numpy(), rdo_inputs(n, hw, k_points, length, True)[3].transpose(0, 2, 1))
    got = tuple(t.cpu().numpy() for t in dev.ladder_histograms_rdo(y_d, bw_d, thr_d, mean_d, length, by_magnitude=by_magnitude))
    assert equal(got, reference(n, hw, k_points, length, True))
    with pytest.raises(dev.HipError):
        dev.ladder_histograms_rdo(y_d, bw_d, thr_d, mean_d, length, by_magnitude=thr_d)
    with pytest.raises(dev.HipError):
        dev.ladder_histograms_rdo(y_d, bw_d, thr_d, mean_d, length, by_magnitude=by_magnitude[:2])


# ---- the tiles form ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('length', [4, 10, 20])
@pytest.mark.parametrize('n, h, w, coding_tile', PLANES)
def test_tiles_against_numpy_and_the_whole_map_form(dev, guard, n, h, w, coding_tile, length):
    k_points = 3
    assert any(0.1 <= share <= 0.9 for share in lowered_shares(n, h*w, k_points, length, True))
    (y_d, bw_d, mean_d, thr_d) = uploaded(guard, n, h*w, k_points, length, True, plane=(h, w))
    got = tuple(t.cpu().numpy() for t in dev.ladder_histograms_rdo_tiles(y_d, bw_d, thr_d, coding_tile, mean_d, length))
    assert equal(got, tile_reference(n, h, w, coding_tile, k_points, length))
    whole = tuple(t.cpu().numpy() for t in dev.ladder_histograms_rdo(y_d, bw_d, thr_d, mean_d, length))
    assert equal((got[0].sum(axis=2), got[1].sum(axis=2), got[2]), whole)
    assert equal(whole, reference(n, h*w, k_points, length, True))


@pytest.mark.parametrize('n, h, w, coding_tile', PLANES)
def test_tiles_with_thresholds_of_zero_give_the_words_of_nearest_rounding(dev, guard, n, h, w, coding_tile):
    (y_d, bw_d, mean_d, thr_d) = uploaded(guard, n, h*w, 3, 10, True, 'zero', plane=(h, w))
    got = dev.ladder_histograms_rdo_tiles(y_d, bw_d, thr_d, coding_tile, mean_d, 10)
    nearest = dev.ladder_histograms_tiles(y_d, bw_d, coding_tile, mean_d, 10)
    for (a, b) in zip(got, nearest):
        assert a.dtype == b.dtype and a.shape == b.shape and numpy.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_tiles_accumulate_and_take_the_most_points(dev, guard):
    import torch
    (n, h, w, coding_tile, length) = (2, 11, 13, (4, 4), 10)
    k_points = dev.ladder_max_points(length)
    expected = tile_reference(n, h, w, coding_tile, k_points, length)
    rng = numpy.random.RandomState(6)
    start = (rng.randint(0, 1000, size=expected[0].shape).astype(numpy.int32), rng.randint(0, 1 << 40, size=expected[1].shape).astype(numpy.int64),
             rng.randint(0, 1000, size=k_points).astype(numpy.int32))
    out = tuple(torch.from_numpy(a).cuda() for a in start)
    (y_d, bw_d, mean_d, thr_d) = uploaded(guard, n, h*w, k_points, length, True, plane=(h, w))
    dev.ladder_histograms_rdo_tiles(y_d, bw_d, thr_d, coding_tile, mean_d, length, out=out)
    assert equal(tuple(t.cpu().numpy() for t in out), tuple(s.astype(numpy.int64) + e for (s, e) in zip(start, expected)))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch(dev, guard):
    import torch
    from autoencoder_based_image_compression_amd import _native
    lib = _native.hip()
    (n, h, w, length) = (1, 4, 6, 10)
    hw = h*w
    most = dev.ladder_max_points(length)
    (y_d, bw_d, _, thr_d) = uploaded(guard, n, hw, most, length, False)
    by_magnitude = dev.rdo_thresholds_by_magnitude(thr_d)
    hist = torch.zeros((n, most, NB_MAPS, length + 1), dtype=torch.int32, device='cuda')
    (yp, bp, tp, hp) = (y_d.data_ptr(), bw_d.data_ptr(), by_magnitude.data_ptr(), hist.data_ptr())
    assert tp % 16 == 0

    def whole(y=yp, bw=bp, thresholds=tp, k_points=1, length=length, hist=hp, n=n, hw=hw):
        return lib.eae_hip_ladder_histograms_rdo(y, None, bw, thresholds, k_points, length, hist, None, None, n, hw, None)

    def tiles(y=yp, bw=bp, thresholds=tp, k_points=1, length=length, hist=hp, n=n, h=h, w=w, th=2, tw=2):
        return lib.eae_hip_ladder_histograms_rdo_tiles(y, None, bw, thresholds, k_points, length, hist, None, None, n, h, w, th, tw, None)

    for call in (whole, tiles):
        for bad in (dict(y=None), dict(bw=None), dict(hist=None), dict(thresholds=None), dict(thresholds=tp + 4), dict(thresholds=tp + 8),
                    dict(k_points=0), dict(k_points=-1), dict(k_points=most + 1), dict(length=0), dict(length=-3), dict(length=256),
                    dict(length=255), dict(n=0)):
            assert call(**bad) == -1, bad
    assert whole(hw=0) == -1
    for bad in (dict(h=0), dict(w=0), dict(th=0), dict(tw=0), dict(th=-1)):
        assert tiles(**bad) == -1, bad
    torch.cuda.synchronize()
    assert not hist.any().item()                                                   # nothing was launched
    for call in (lambda **k: dev.ladder_histograms_rdo(k.pop('y', y_d), k.pop('bw', bw_d), k.pop('thr', thr_d), None, k.pop('length', length)),
                 lambda **k: dev.ladder_histograms_rdo_tiles(k.pop('y', y_d).view(n, h, w, NB_MAPS), k.pop('bw', bw_d), k.pop('thr', thr_d),
                                                             (2, 2), None, k.pop('length', length))):
        with pytest.raises(ValueError):
            call(length=0)
        with pytest.raises(dev.HipError):
            call(bw=bw_d[:, :64].contiguous())
        with pytest.raises(dev.HipError):
            call(y=y_d.double())
        with pytest.raises(dev.HipError):
            call(thr=thr_d[:, :, :8].contiguous())
        with pytest.raises(dev.HipError):
            call(thr=thr_d[:1].contiguous())
        with pytest.raises(dev.HipError):
            call(thr=thr_d.double())
        with pytest.raises(dev.HipError):
            call(thr=by_magnitude)
    with pytest.raises(dev.HipError):
        dev.ladder_histograms_rdo_tiles(y_d, bw_d, thr_d, (2, 2), None, length)           # y is not a plane
