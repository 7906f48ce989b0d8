"""The four rate-control codecs and the two host loops on a ladder with a price, `ratecontrol.RateLadder(..., rdo_lambda=...)` (DESIGN.md
section 24): the step counts, bounds, probes and codes the symbols of the rate-distortion optimised quantiser.

tests/test_gpu_budget_codec.py's inputs (none of it imported): three 176 x 208 images of three entropies (an 11 x 13 latent plane),
`trained_like_variables` with `decoder/weights_6` scaled, a ladder at 1, 2 and 4 times the bin widths with the tables of
`stats.compute_binary_probabilities_ladder`; L = 10 with an exception map, L = 3 without, the learned-bin-width model once; launch by
launch and replayed as hipGraphs; 2 x nb_slots + 1 steps whose budgets or thresholds change every step. The price is
rdo_lambda = 2 * mean(bw_k ** 2) per point. Coding tiles are 4 x 4: twelve tiles of four shape classes.

Nothing expected comes from code under test:
* `container.encode_images(..., rdo_lambda=lambda_k)` of every image at every point, whole and in tiles, gives the blobs, the bit counts and
  the sizes; `container.decode_images` of that blob the reconstruction and the squared error;
* the counts are those of numpy float32 -- `ratecontrol.rdo_quantize_numpy` per point, rint(bw * r / bw), folded here --, not the new
  kernel's; the host rule of ratecontrol.py (`upper_bounds_fixed[_tiles]`, `valid_points`, `select_by_upper_bound`, `select_by_quality`)
  on them gives the bounds, the points, `promised` and the probes;
* the image-by-image functions of `kodak/` on bw * r give the exception map's cost and the dead maps.

The reference is held to three conditions where it is built: every RDO blob is within its RDO bound; some (image, point) has an RDO
bound strictly below its nearest-rounding bound; and some step sets a budget between the two, where the codec must take that point,
promised, and the same ladder without a price takes the next one. Every comparison is exact."""
import contextlib

import numpy
import pytest
import torch

import model_cases
from test_gpu_ladder import suffix_bits

pytestmark = pytest.mark.gpu

F32 = numpy.float32
SHAPE = (176, 208)
(H_MAP, W_MAP) = (11, 13)
MAP_SIZE = H_MAP*W_MAP
BATCH = 3
K = 3
MULTIPLIERS = (1., 2., 4.)
EXCEPTION = 5
TILE = (4, 4)
NB_STEPS = 9                              # 2 x nb_slots + 1
NO_BUDGET = 1 << 62
MODES = {'launches': {}, 'graphs': {'use_graphs': True}}
# (model kind, truncated unary length, exception map)
CASES = {'fixed_L10_exception': (False, 10, EXCEPTION), 'fixed_L3': (False, 3, -1), 'learned_L10_exception': (True, 10, EXCEPTION)}
BUDGET_KEYS = ('rate_point', 'upper_bound_bytes', 'budget_bytes', 'blob_bytes', 'promised', 'fits', 'nb_bits', 'coder_bits', 'exception_bits',
               'sse', 'nb_deads', 'container_bytes')
QUALITY_KEYS = BUDGET_KEYS + ('first_point', 'met', 'max_sse', 'probe_points', 'probe_sse')
FORMS = {'budget': 'whole', 'tiled_budget': 'tiles', 'quality': 'whole', 'tiled_quality': 'tiles'}


def _images():
    """Noise, a noisy ramp and a nearly flat image: three different entropies."""
    rng = numpy.random.RandomState(2)
    (h, w) = SHAPE
    noise = rng.randint(16, 236, size=(h, w))
    ramp = numpy.clip(numpy.broadcast_to(16 + 219*numpy.arange(w)/(w - 1), (h, w)) + rng.randint(-4, 5, size=(h, w)), 16, 235)
    flat = rng.randint(16, 236, size=(h, w))//8 + 100
    return numpy.stack([noise, ramp, flat]).astype(numpy.uint8)


@pytest.fixture(scope='module')
def references(tmp_path_factory):
    return {'directory': tmp_path_factory.mktemp('rdo_ratecontrol')}


def _counts(rs, length, tiles):
    """Symbols as float32 rs [K][N, h, w, 128] -> (hist int64 [N, K, T, 128, L + 1], bypass bits [N, K, T, 128]) per coding tile."""
    hist = numpy.zeros((BATCH, K, len(tiles), 128, length + 1), dtype=numpy.int64)
    bits = numpy.zeros((BATCH, K, len(tiles), 128), dtype=numpy.int64)
    for k in range(K):
        good = numpy.abs(rs[k]) < F32(32768.)
        magnitudes = numpy.where(good, numpy.abs(rs[k]), 0).astype(numpy.int64)
        clipped = numpy.minimum(magnitudes, length)
        bypass = suffix_bits(magnitudes, length)*good
        for (t, (r0, c0, nr, nc, _)) in enumerate(tiles.tolist()):
            window = (slice(None), slice(r0, r0 + nr), slice(c0, c0 + nc))
            for b in range(length + 1):
                hist[:, k, t, :, b] = (good[window] & (clipped[window] == b)).sum(axis=(1, 2))
            bits[:, k, t] = bypass[window].sum(axis=(1, 2))
    return hist, bits


def reference(cache, name):
    """Once per case: the ladders, the numpy counts and the host rule's bounds on them, and for every (image, point), whole and in
    tiles, what `container.encode_images(..., rdo_lambda=...)` and `container.decode_images` give."""
    if name in cache:
        return cache[name]
    from autoencoder_based_image_compression_amd import container, pipeline, ratecontrol
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    from autoencoder_based_image_compression_amd.kodak.lossless import compression, stats as lossless_stats
    from autoencoder_based_image_compression_amd.kodak.tools import tools as tls
    (learned, length, exception) = CASES[name]
    v = model_cases.trained_like_variables(0.05, learned, seed=11 + int(learned))
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    encoder = pipeline.DeviceEncoder(v, learned)
    decoder = pipeline.DeviceDecoder(v, learned)
    images = _images()
    base = v[var.BIN_WIDTHS_NAME] if not learned else numpy.random.RandomState(17).uniform(0.04, 0.06, size=128).astype(numpy.float32)
    bin_widths_points = (numpy.array(MULTIPLIERS, dtype=numpy.float32)[:, None]*base[None, :]).astype(numpy.float32)
    y = encoder(torch.from_numpy(images).cuda()).cpu().numpy().reshape(BATCH, H_MAP, W_MAP, 128)
    map_mean = lossless_stats.compute_map_mean(y)
    tables = lossless_stats.compute_binary_probabilities_ladder(y, bin_widths_points, map_mean, length)
    lambdas = 2.*(bin_widths_points.astype(numpy.float64)**2).mean(axis=1)
    ladder = ratecontrol.RateLadder(bin_widths_points, tables, map_mean, exception, rdo_lambda=lambdas)
    plain = ratecontrol.RateLadder(bin_widths_points, tables, map_mean, exception)
    zero = ratecontrol.RateLadder(bin_widths_points, tables, map_mean, exception, rdo_lambda=0.)
    assert numpy.array_equal(ladder.rdo_lambdas, lambdas)

    # the symbols of both rules in numpy float32, and their counts per tile and per map
    (r, rs, rs_nearest) = ([], [], [])
    for k in range(K):
        thresholds = ratecontrol.rdo_thresholds(bin_widths_points[k], tables[k], lambdas[k], exception)
        r.append(ratecontrol.rdo_quantize_numpy(y, bin_widths_points[k], map_mean, thresholds, length))
        rs.append(numpy.rint(bin_widths_points[k]*r[k]/bin_widths_points[k]))
        rs_nearest.append(numpy.rint(bin_widths_points[k]*numpy.rint((y - map_mean)/bin_widths_points[k])/bin_widths_points[k]))
        assert rs[k].dtype == F32 and rs_nearest[k].dtype == F32
    moved = sum(int((rs[k] != rs_nearest[k]).sum()) for k in range(K))
    nonzero = sum(int((rs_nearest[k] != 0).sum()) for k in range(K))
    print(name, 'non-zero nearest-rounded symbols', nonzero, 'lowered', moved)
    assert moved >= nonzero//100                                 # the price moves symbols: no case passes on nearest rounding
    (tiles, _) = container.coding_tile_grid(H_MAP, W_MAP, TILE)
    one_tile = numpy.array([[0, 0, H_MAP, W_MAP, 0]])
    out = {'variables': v, 'learned': learned, 'length': length, 'exception': exception, 'images': images, 'ladder': ladder, 'plain': plain,
           'zero': zero, 'encoder': encoder, 'decoder': decoder, 'whole': {}, 'tiles': {}}
    for (form, grid, coding_tile) in (('whole', one_tile, None), ('tiles', tiles, TILE)):
        f = out[form]
        f['coding_tile'] = coding_tile
        f['header_bytes'] = ratecontrol.header_bytes(ladder, SHAPE[0], SHAPE[1], coding_tile)
        for (key, symbols) in (('upper', rs), ('upper_nearest', rs_nearest)):
            (hist, bits) = _counts(symbols, length, grid)
            if form == 'whole':
                f[key] = ratecontrol.upper_bounds_fixed(hist[:, :, 0], bits[:, :, 0], ladder, MAP_SIZE)
            else:
                f[key] = ratecontrol.upper_bounds_fixed_tiles(hist, bits, ladder, MAP_SIZE, f['header_bytes'])
            if key == 'upper':
                f['valid'] = ratecontrol.valid_points(hist.sum(axis=2), MAP_SIZE)
                assert f['valid'].all()
                # (the bounds of the trial-coding loop, `encode_images_to_budget`)
                f['bounds'] = (ratecontrol.blob_byte_bounds(hist[:, :, 0], bits[:, :, 0], ladder, SHAPE[0], SHAPE[1]) if form == 'whole' else
                               ratecontrol.blob_byte_bounds(hist, bits, ladder, SHAPE[0], SHAPE[1], TILE))
        f['points'] = []
    paths = []
    for k in range(K):
        paths.append(str(cache['directory']/'{0}_{1}.npy'.format(name, k)))
        numpy.save(paths[k], tables[k])
    for i in range(BATCH):
        rows = {'whole': [], 'tiles': []}
        for k in range(K):
            arguments = (images[i:i + 1], encoder, bin_widths_points[k], map_mean, tables[k], exception)
            # the exception map's cost and the dead maps, from bw * r as the reference-shaped functions of `kodak/` take it
            cq = (bin_widths_points[k]*r[k][i:i + 1]).astype(F32)
            path_bits = int(compression.rescale_compress_lossless_maps(cq[0], bin_widths_points[k], paths[k], exception))
            nb_deads = int(numpy.asarray(tls.count_nb_deads(cq)).reshape(-1)[0])
            exception_bits = None
            for (form, more) in (('whole', {}), ('tiles', {'coding_tile': TILE})):
                (blob, info) = container.encode_images(*arguments, rdo_lambda=float(lambdas[k]), **more)
                decoded = container.decode_images(blob, decoder)
                difference = images[i:i + 1].astype(numpy.int64) - decoded.astype(numpy.int64)
                per_map = info['nb_bits'].astype(numpy.int64).copy()
                if exception >= 0:
                    per_map[:, exception] = 0                    # charged by its entropy (compression.py:68-81)
                if form == 'whole':
                    exception_bits = path_bits - int(per_map.sum())
                    assert exception_bits >= 0 and (exception >= 0 or exception_bits == 0)
                rows[form].append({'blob': blob, 'decoded': decoded[0], 'sse': int((difference*difference).sum()),
                                   'coder_bits': int(per_map.sum()), 'exception_bits': exception_bits, 'nb_deads': nb_deads})
        for form in rows:
            out[form]['points'].append(rows[form])
    for form in ('whole', 'tiles'):
        f = out[form]
        f['sizes'] = numpy.array([[len(p['blob']) for p in row] for row in f['points']])
        f['sse'] = numpy.array([[p['sse'] for p in row] for row in f['points']], dtype=numpy.int64)
        print(name, form, 'blob sizes', f['sizes'].tolist(), 'RDO bounds', f['upper'].tolist(), 'nearest-rounding bounds', f['upper_nearest'].tolist())
        assert (f['sizes'] <= f['upper']).all()                  # every RDO blob is within its RDO bound
        assert (f['upper'] < f['upper_nearest']).any()           # and some bound is strictly below the one of nearest rounding
        assert (f['upper'] <= f['upper_nearest']).all()
    assert numpy.array_equal(out['whole']['sse'], out['tiles']['sse'])      # the symbols do not depend on the coding tile
    cache[name] = out
    return out


# ---- budgets ---------------------------------------------------------------------------------------------------------------------------

def budgets_of_step(f, step):
    """Image i of step s aims at point j = (s + i) % 4 -- the fourth being "under the coarsest point's bound": nothing fits. Steps 0-3
    sit AT the RDO bound of the point; steps 4-7 one byte under its NEAREST-ROUNDING bound, which is still within the RDO bound where
    that is strictly smaller (the budget between the two) and under it where the two are equal; step 8 one byte under the RDO bound."""
    (upper, nearest) = (f['upper'], f['upper_nearest'])
    budgets = numpy.zeros(BATCH, dtype=numpy.int64)
    for i in range(BATCH):
        j = (step + i) % 4
        budgets[i] = upper[i].min() - 1 if j == 3 else (upper[i, j], nearest[i, j] - 1, upper[i, j] - 1)[step//4]
    return budgets


def between_the_bounds(f):
    """[(step, image, point)]: the budget lies in [RDO bound, nearest-rounding bound) of the point, the host rule on the RDO bounds
    takes that point, promised, and on the nearest-rounding bounds of the same ladder a later one. Asserted not empty."""
    from autoencoder_based_image_compression_amd import ratecontrol
    found = []
    for step in range(NB_STEPS):
        budgets = budgets_of_step(f, step)
        (point, promised) = ratecontrol.select_by_upper_bound(f['upper'], f['valid'], budgets)
        (point_nearest, _) = ratecontrol.select_by_upper_bound(f['upper_nearest'], f['valid'], budgets)
        for i in range(BATCH):
            j = int(point[i])
            if promised[i] and f['upper'][i, j] <= budgets[i] < f['upper_nearest'][i, j] and point_nearest[i] > j:
                found.append((step, i, j))
    assert found
    return found


def chosen_values(f, point):
    chosen = [f['points'][i][int(point[i])] for i in range(BATCH)]
    blob_bytes = numpy.array([len(p['blob']) for p in chosen], dtype=numpy.int64)
    (coder_bits, exception_bits) = (numpy.array([p[key] for p in chosen], dtype=numpy.int64) for key in ('coder_bits', 'exception_bits'))
    values = {'rate_point': point, 'upper_bound_bytes': f['upper'], 'blob_bytes': blob_bytes, 'nb_bits': coder_bits + exception_bits,
              'coder_bits': coder_bits, 'exception_bits': exception_bits, 'sse': numpy.array([p['sse'] for p in chosen], dtype=numpy.int64),
              'nb_deads': numpy.array([p['nb_deads'] for p in chosen], dtype=numpy.int64), 'container_bytes': blob_bytes - f['header_bytes']}
    return values, [p['blob'] for p in chosen], numpy.stack([p['decoded'] for p in chosen])


def expected_budget_step(f, budgets):
    from autoencoder_based_image_compression_amd import ratecontrol
    (point, promised) = ratecontrol.select_by_upper_bound(f['upper'], f['valid'], budgets)
    (values, blobs, decoded) = chosen_values(f, point)
    values.update({'budget_bytes': budgets, 'promised': promised, 'fits': values['blob_bytes'] <= budgets})
    return values, blobs, decoded


# ---- thresholds ------------------------------------------------------------------------------------------------------------------------

def thresholds_of_step(f, step):
    """Image i of step s: the squared error of point (s + i) % (K + 1) -- the K + 1-th being "under the smallest": nothing meets it --,
    exact, and one under it every other time the index comes round."""
    sse = f['sse']
    thresholds = numpy.zeros(BATCH, dtype=numpy.int64)
    for i in range(BATCH):
        j = (step + i) % (K + 1)
        thresholds[i] = sse[i, j] - ((step + i)//(K + 1)) % 2 if j < K else sse[i].min() - 1
    return thresholds


def expected_quality_step(f, thresholds, budgets=None):
    from autoencoder_based_image_compression_amd import ratecontrol
    budgets = numpy.full(BATCH, NO_BUDGET, dtype=numpy.int64) if budgets is None else numpy.asarray(budgets, dtype=numpy.int64)
    (first, _) = ratecontrol.select_by_upper_bound(f['upper'], f['valid'], budgets)
    (point, met, probe_points, probe_sse) = ratecontrol.select_by_quality(f['sse'], first, thresholds)
    (values, blobs, decoded) = chosen_values(f, point)
    values.update({'first_point': first, 'met': met, 'max_sse': thresholds, 'probe_points': probe_points, 'probe_sse': probe_sse,
                   'budget_bytes': budgets, 'promised': f['upper'][numpy.arange(BATCH), point] <= budgets, 'fits': values['blob_bytes'] <= budgets})
    return values, blobs, decoded


# ---- the codecs ------------------------------------------------------------------------------------------------------------------------

def build(ref, kind, mode, ladder=None, **more):
    from autoencoder_based_image_compression_amd import codec
    cls = {'budget': codec.BudgetCodec, 'tiled_budget': codec.TiledBudgetCodec, 'quality': codec.QualityCodec,
           'tiled_quality': codec.TiledQualityCodec}[kind]
    tile = (TILE,) if FORMS[kind] == 'tiles' else ()
    return cls(ref['variables'], ref['learned'], ref['ladder'] if ladder is None else ladder, BATCH, SHAPE[0], SHAPE[1], *tile, nb_in_flight=2,
               keep_reconstruction=True, container_capacity_bytes=8*BATCH*SHAPE[0]*SHAPE[1], **dict(MODES[mode], **more))


def submit(c, kind, images, budgets, thresholds):
    if kind in ('budget', 'tiled_budget'):
        return c.submit(images, budgets)
    return c.submit(images, max_sse=thresholds, budget_bytes=budgets)


def check_step(ref, kind, ticket, step, budgets=None, thresholds=None, decoder=None):
    f = ref[FORMS[kind]]
    if kind in ('budget', 'tiled_budget'):
        ((values, blobs, decoded), keys) = (expected_budget_step(f, budgets), BUDGET_KEYS)
    else:
        ((values, blobs, decoded), keys) = (expected_quality_step(f, thresholds, budgets), QUALITY_KEYS)
    r = ticket.result()
    for key in keys:
        print(kind, 'step', step, key, numpy.asarray(r[key]).tolist(), 'reference', values[key].tolist())
        assert r[key].dtype == values[key].dtype and numpy.array_equal(r[key], values[key]), (step, key)
    assert not (r['promised'] & ~r['fits']).any()                 # (expected, not proven: the allowance of ratecontrol.py is measured)
    containers = ticket.image_containers()
    assert [bytes(blob) for blob in containers] == blobs, step
    reconstruction = ticket.reconstruction_uint8.cpu().numpy()
    assert numpy.array_equal(reconstruction, decoded), step
    if decoder is not None:
        assert numpy.array_equal(decoder.submit(containers).result(), reconstruction), step
    return r


def run_steps(ref, kind, mode, with_decoder=True, between=None):
    """NB_STEPS steps of one codec against the reference; returns the results."""
    from autoencoder_based_image_compression_amd import codec
    f = ref[FORMS[kind]]
    images = torch.from_numpy(ref['images']).cuda()
    more = {} if f['coding_tile'] is None else {'coding_tile': f['coding_tile']}
    results = []
    reader = (codec.BatchDecoder(ref['variables'], ref['learned'], BATCH, SHAPE[0], SHAPE[1], ref['length'], **more) if with_decoder else
              contextlib.nullcontext())
    with build(ref, kind, mode) as c, reader as decoder:
        assert c.emit_container and c.nb_slots == 4 and NB_STEPS == 2*c.nb_slots + 1
        if between is not None:
            between(c)
        for step in range(NB_STEPS):
            (budgets, thresholds) = (budgets_of_step(f, step), None) if kind.endswith('budget') else (None, thresholds_of_step(f, step))
            ticket = submit(c, kind, images, budgets, thresholds)
            results.append(check_step(ref, kind, ticket, step, budgets, thresholds, decoder if with_decoder and step < 2 else None))
            if between is not None:
                between(c)
    return results


BUDGET_RUNS = [('budget', 'fixed_L10_exception', 'launches'), ('budget', 'fixed_L10_exception', 'graphs'), ('budget', 'fixed_L3', 'graphs'),
               ('budget', 'learned_L10_exception', 'launches'), ('tiled_budget', 'fixed_L10_exception', 'launches'),
               ('tiled_budget', 'fixed_L10_exception', 'graphs'), ('tiled_budget', 'fixed_L3', 'launches'),
               ('tiled_budget', 'learned_L10_exception', 'graphs')]
QUALITY_RUNS = [(kind.replace('budget', 'quality'), name, mode) for (kind, name, mode) in BUDGET_RUNS]


@pytest.mark.parametrize('kind, name, mode', BUDGET_RUNS)
def test_budget_steps_land_where_the_host_rule_puts_them_on_the_rdo_counts(references, kind, name, mode):
    ref = reference(references, name)
    found = between_the_bounds(ref[FORMS[kind]])
    results = run_steps(ref, kind, mode)
    points = [p for r in results for p in r['rate_point'].tolist()]
    promises = [p for r in results for p in r['promised'].tolist()]
    assert set(points) == {0, 1, 2} and not all(promises) and any(promises)
    for (step, i, j) in found:                                    # the budget between the two bounds: the point is taken, promised
        assert results[step]['rate_point'][i] == j and results[step]['promised'][i] and results[step]['fits'][i]


@pytest.mark.parametrize('kind', ['budget', 'tiled_budget'])
def test_the_same_ladder_without_a_price_takes_the_next_point(references, kind):
    """What the feature buys, observed on the codecs themselves: at a budget between the two bounds the ladder with a price lands on
    the point and the ladder without one on a later point."""
    ref = reference(references, 'fixed_L10_exception')
    f = ref[FORMS[kind]]
    images = torch.from_numpy(ref['images']).cuda()
    found = between_the_bounds(f)
    with build(ref, kind, 'launches') as priced, build(ref, kind, 'launches', ladder=ref['plain']) as plain:
        for step in sorted({step for (step, _, _) in found}):
            budgets = budgets_of_step(f, step)
            (r, p) = (priced.submit(images, budgets).result(), plain.submit(images, budgets).result())
            assert numpy.array_equal(p['upper_bound_bytes'], f['upper_nearest'])
            for (s, i, j) in found:
                if s == step:
                    print(kind, 'step', step, 'image', i, 'budget', int(budgets[i]), 'with a price', int(r['rate_point'][i]), 'without',
                          int(p['rate_point'][i]))
                    assert r['rate_point'][i] == j and r['promised'][i] and p['rate_point'][i] > j
                    assert r['blob_bytes'][i] <= budgets[i]


@pytest.mark.parametrize('kind, name, mode', QUALITY_RUNS)
def test_quality_steps_land_where_the_bisection_puts_them_on_the_rdo_errors(references, kind, name, mode):
    ref = reference(references, name)
    results = run_steps(ref, kind, mode)
    mets = {m for r in results for m in r['met'].tolist()}
    assert mets == {True, False}
    f = ref[FORMS[kind]]
    for r in results:                                             # what a round found is the RDO symbols' squared error at the point it probed
        assert numpy.array_equal(r['probe_sse'], f['sse'][numpy.arange(BATCH)[:, None], r['probe_points']])


@pytest.mark.parametrize('kind', ['quality', 'tiled_quality'])
def test_a_floor_and_a_budget(references, kind):
    """Image i gets the RDO bound of point i, and every other step one byte under the nearest-rounding bound of that point: the search
    starts where `BudgetCodec` would land on the RDO counts."""
    ref = reference(references, 'fixed_L10_exception')
    f = ref[FORMS[kind]]
    images = torch.from_numpy(ref['images']).cuda()
    at = f['upper'][numpy.arange(BATCH), numpy.arange(BATCH)]
    under_nearest = f['upper_nearest'][numpy.arange(BATCH), numpy.arange(BATCH)] - 1
    firsts = set()
    with build(ref, kind, 'launches', budget_bytes=at) as c:
        for step in range(NB_STEPS):
            thresholds = thresholds_of_step(f, step)
            given = (None, under_nearest, at - 1)[step % 3]
            ticket = c.submit(images, max_sse=thresholds, budget_bytes=given)
            r = check_step(ref, kind, ticket, step, at if given is None else given, thresholds)
            assert (r['rate_point'] >= r['first_point']).all()
            firsts.update(r['first_point'].tolist())
    assert firsts == {0, 1, 2}


@pytest.mark.parametrize('kind', sorted(FORMS))
def test_a_price_of_zero_gives_the_bytes_and_results_of_no_price(references, kind):
    ref = reference(references, 'fixed_L10_exception')
    f = ref[FORMS[kind]]
    images = torch.from_numpy(ref['images']).cuda()
    assert ref['zero'].rdo_thresholds_points is not None and not ref['zero'].rdo_thresholds_points.any()
    with build(ref, kind, 'graphs', ladder=ref['zero']) as zero, build(ref, kind, 'graphs', ladder=ref['plain']) as plain:
        assert zero._rdo_thresholds_points is not None and plain._rdo_thresholds_points is None      # the RDO path, and today's
        for step in (0, 3, 5):
            budgets = budgets_of_step(dict(f, upper=f['upper_nearest']), step)
            thresholds = thresholds_of_step(f, step)
            (a, b) = (submit(zero, kind, images, budgets, thresholds), submit(plain, kind, images, budgets, thresholds))
            (ra, rb) = (a.result(), b.result())
            assert set(ra) == set(rb)
            for key in ra:
                assert ra[key].dtype == rb[key].dtype and numpy.array_equal(ra[key], rb[key]), (step, key)
            assert numpy.array_equal(ra['upper_bound_bytes'], f['upper_nearest'])
            assert [bytes(x) for x in a.image_containers()] == [bytes(x) for x in b.image_containers()]
            assert numpy.array_equal(a.reconstruction_uint8.cpu().numpy(), b.reconstruction_uint8.cpu().numpy())


# ---- the host loops --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form', ['whole', 'tiles'])
def test_encode_images_to_budget_codes_the_rdo_symbols(references, form):
    """Every budget of the codecs' steps: the bounds are those of the RDO counts, the point is the first in ladder order whose RDO blob
    fits -- the codec's point, or, where trial coding finds that a finer blob fits although its bound does not, a finer one --, and
    the blob is `encode_images(..., rdo_lambda=...)`'s byte for byte."""
    from autoencoder_based_image_compression_amd import container, ratecontrol
    ref = reference(references, 'fixed_L10_exception')
    f = ref[form]
    more = {} if f['coding_tile'] is None else {'coding_tile': f['coding_tile']}
    (same, finer) = (0, 0)
    for step in range(NB_STEPS):
        budgets = budgets_of_step(f, step)
        (blobs, info) = container.encode_images_to_budget(ref['images'], ref['encoder'], ref['ladder'], budgets, **more)
        assert info['upper_bound_misses'] == 0
        assert numpy.array_equal(info['lower_bytes'], f['bounds'][0]) and numpy.array_equal(info['upper_bytes'], f['bounds'][1])
        (codec_point, _) = ratecontrol.select_by_upper_bound(f['upper'], f['valid'], budgets)
        for i in range(BATCH):
            fitting = [k for k in range(K) if f['sizes'][i, k] <= budgets[i]]
            (k, fits) = (fitting[0], True) if fitting else (K - 1, False)
            assert (int(info['rate_point'][i]), bool(info['fits'][i])) == (k, fits), (step, i)
            assert bytes(blobs[i]) == f['points'][i][k]['blob'] and int(info['blob_bytes'][i]) == f['sizes'][i, k]
            assert k <= codec_point[i]
            same += k == codec_point[i]
            finer += k < codec_point[i]
    print(form, 'points equal to the codec\'s', same, 'finer', finer)
    assert same > 0
    decoded = container.decode_images(blobs[0], ref['decoder'])
    assert decoded.shape == (1,) + SHAPE


@pytest.mark.parametrize('form', ['whole', 'tiles'])
def test_encode_images_to_quality_probes_and_codes_the_rdo_symbols(references, form):
    from autoencoder_based_image_compression_amd import container
    ref = reference(references, 'fixed_L10_exception')
    f = ref[form]
    more = {} if f['coding_tile'] is None else {'coding_tile': f['coding_tile']}
    at = f['upper'][numpy.arange(BATCH), numpy.arange(BATCH)]
    for step in range(NB_STEPS):
        thresholds = thresholds_of_step(f, step)
        budgets = (None, at, f['upper_nearest'][numpy.arange(BATCH), numpy.arange(BATCH)] - 1)[step % 3]
        (values, expected_blobs, _) = expected_quality_step(f, thresholds, budgets)
        (blobs, info) = container.encode_images_to_quality(ref['images'], ref['encoder'], ref['decoder'], ref['ladder'], max_sse=thresholds,
                                                           budget_bytes=budgets, **more)
        assert [bytes(blob) for blob in blobs] == expected_blobs, step
        for key in ('rate_point', 'first_point', 'met', 'max_sse', 'probe_points', 'probe_sse', 'blob_bytes', 'upper_bound_bytes'):
            assert info[key].dtype == values[key].dtype and numpy.array_equal(info[key], values[key]), (step, key)


def test_the_keyword_is_still_refused_and_says_where_the_price_goes(references):
    from autoencoder_based_image_compression_amd import codec
    ref = reference(references, 'fixed_L10_exception')
    head = (ref['variables'], False, ref['ladder'], BATCH, SHAPE[0], SHAPE[1])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for make in (lambda **k: codec.BudgetCodec(*head, budget_bytes=1 << 20, **k), lambda **k: codec.TiledBudgetCodec(*head, TILE, budget_bytes=1 << 20, **k),
                 lambda **k: codec.QualityCodec(*head, target_psnr=30., **k), lambda **k: codec.TiledQualityCodec(*head, TILE, target_psnr=30., **k)):
        for value in (0.5, 0.):
            with pytest.raises(ValueError, match='rdo_lambda.*ladder'):
                make(rdo_lambda=value)
    assert torch.cuda.memory_allocated() == before
