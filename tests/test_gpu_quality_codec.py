"""`codec.QualityCodec`: the coarsest rate point per image that keeps a PSNR floor, searched inside the step, on the device (DESIGN.md
section 21), and its host-loop sibling `container.encode_images_to_quality`.

tests/test_gpu_budget_codec.py's inputs: three 176 x 208 images of different entropy (an 11 x 13 latent plane), `trained_like_variables`
with `decoder/weights_6` scaled, the tables of `stats.compute_binary_probabilities_ladder`; ladders of three points (two rounds) and,
once, of nine (four rounds); L = 10 with and without an exception map, L = 3 and the learned-bin-width model once; launch by launch and
replayed as hipGraphs, 2 x nb_slots + 1 steps whose thresholds change every step.

The multipliers. The model is not a trained one: its reconstruction is far from the image at every bin width (6 dB), and up to about
four times the model's bin widths the squared error does not grow with the bin width at all -- at 1, 2 and 4 times it FALLS for all
three images (534587661, 534529041, 533549582 for the noise image), and over the reference's nine multipliers, 1 to 10, it wanders. A
search for the coarsest point that keeps a floor never takes a middle point of such a table, so the reference's choices would not
cover the ladder. From 4 times on the quantiser's error shows (the ramp: 524391048 at 4, 552857277 at 64; every latent is zero from
96 on). The ladders are therefore 16, 32 and 64 times the bin widths, and nine points from 4 to 64 times: the ramp and the nearly flat
image grow strictly along both, the noise image falls over the first five of the nine, which puts a table that is not monotone
through the codec as well. `assert_reference_coverage` holds the reference to it before the codec is consulted.

The reference uses nothing under test: `container.encode_images` + `container.decode_images` of every image at every point for the
squared error, the blob, the bit counts and the reconstruction, the image-by-image functions of `kodak/` for the exception map's cost
and the dead maps, `ratecontrol.upper_bounds_fixed` + `select_by_upper_bound` (the rule of `BudgetCodec`) for the bounds and the first
point, and a bisection WRITTEN HERE over that table for the choice. Every comparison is exact."""
import numpy
import pytest
import torch

import model_cases

pytestmark = pytest.mark.gpu

SHAPE = (176, 208)
MAP_SIZE = 11*13
BATCH = 3
THREE = (16., 32., 64.)
NINE = (4., 6., 8., 10., 16., 24., 32., 48., 64.)                # (the module's docstring: why not the reference's 1 .. 10)
EXCEPTION = 5
NO_BUDGET = 1 << 62
MODES = {'launches': {}, 'graphs': {'use_graphs': True}}
# (model kind, truncated unary length, exception map, multipliers)
CASES = {'fixed_L10_exception': (False, 10, EXCEPTION, THREE), 'fixed_L10': (False, 10, -1, THREE), 'fixed_L3_exception': (False, 3, EXCEPTION, THREE),
         'learned_L10_exception': (True, 10, EXCEPTION, THREE), 'fixed_L10_nine_points': (False, 10, -1, NINE)}
KEYS = ('rate_point', 'first_point', 'met', 'max_sse', 'probe_points', 'probe_sse', 'upper_bound_bytes', 'budget_bytes', 'blob_bytes', 'promised',
        'fits', 'nb_bits', 'coder_bits', 'exception_bits', 'sse', 'nb_deads', 'container_bytes')


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
    return {'directory': tmp_path_factory.mktemp('quality')}


def reference(cache, name):
    """Once per case: the ladder, and for every (image, point) what the existing functions give."""
    if name in cache:
        return cache[name]
    from autoencoder_based_image_compression_amd import container, device as dev, pipeline, ratecontrol
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    from autoencoder_based_image_compression_amd.kodak.lossless import compression, stats as lossless_stats
    from autoencoder_based_image_compression_amd.kodak.tools import tools as tls
    (learned, length, exception, multipliers) = CASES[name]
    k_points = len(multipliers)
    v = model_cases.trained_like_variables(0.05, learned, seed=11 + int(learned))
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    encoder = pipeline.DeviceEncoder(v, learned)
    decoder = pipeline.DeviceDecoder(v, learned)
    images = _images()
    base = v[var.BIN_WIDTHS_NAME] if not learned else numpy.random.RandomState(17).uniform(0.04, 0.06, size=128).astype(numpy.float32)
    bin_widths_points = (numpy.array(multipliers, dtype=numpy.float32)[:, None]*base[None, :]).astype(numpy.float32)
    y_device = encoder(torch.from_numpy(images).cuda())
    y = y_device.cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y)
    tables = lossless_stats.compute_binary_probabilities_ladder(y, bin_widths_points, map_mean, length)
    ladder = ratecontrol.RateLadder(bin_widths_points, tables, map_mean, exception)
    (hist, bypass, _) = dev.ladder_histograms(y_device, torch.from_numpy(bin_widths_points).cuda(), torch.from_numpy(map_mean).cuda(), length)
    (hist, bypass) = (hist.cpu().numpy(), bypass.cpu().numpy())
    out = {'variables': v, 'learned': learned, 'length': length, 'images': images, 'ladder': ladder, 'encoder': encoder, 'decoder': decoder,
           'upper': ratecontrol.upper_bounds_fixed(hist, bypass, ladder, MAP_SIZE), 'valid': ratecontrol.valid_points(hist, MAP_SIZE),
           'header_bytes': ratecontrol.header_bytes(ladder), 'points': [], 'k_points': k_points}
    assert out['valid'].all()
    paths = []
    for k in range(k_points):
        paths.append(str(cache['directory']/'{0}_{1}.npy'.format(name, k)))
        numpy.save(paths[k], tables[k])
    for i in range(BATCH):
        row = []
        for k in range(k_points):
            (blob, info) = container.encode_images(images[i:i + 1], encoder, bin_widths_points[k], map_mean, tables[k], exception)
            decoded = container.decode_images(blob, decoder)
            difference = images[i:i + 1].astype(numpy.int64) - decoded.astype(numpy.int64)
            per_map = info['nb_bits'].astype(numpy.int64).copy()
            if exception >= 0:
                per_map[:, exception] = 0                        # charged by its entropy (compression.py:68-81)
            # bits of the lossless code and dead maps as the reference-shaped functions of `kodak/` give them image by image
            cq = tls.quantize_per_map(y[i:i + 1] - numpy.tile(map_mean, y[i:i + 1].shape[:3] + (1,)), bin_widths_points[k])
            path_bits = int(compression.rescale_compress_lossless_maps(cq[0], bin_widths_points[k], paths[k], exception))
            exception_bits = path_bits - int(per_map.sum())
            assert exception_bits >= 0 and (exception >= 0 or exception_bits == 0)
            row.append({'blob': blob, 'decoded': decoded[0], 'sse': int((difference*difference).sum()), 'coder_bits': int(per_map.sum()),
                        'exception_bits': exception_bits, 'nb_deads': int(numpy.asarray(tls.count_nb_deads(cq)).reshape(-1)[0])})
        out['points'].append(row)
    out['sse'] = numpy.array([[p['sse'] for p in row] for row in out['points']], dtype=numpy.int64)
    print(name, 'squared errors', out['sse'].tolist(), 'upper bounds', out['upper'].tolist())
    cache[name] = out
    return out


def bisect(row, first, max_sse):
    """The search of the issue for one image, over the reference's table -> (point, met, probed points, their squared errors)."""
    k_points = len(row)
    nb_rounds = 0
    while (1 << nb_rounds) < k_points + 1:
        nb_rounds += 1
    (L, R) = (first - 1, k_points)
    (points, values) = ([], [])
    for _ in range(nb_rounds):
        probed = (L + R) >> 1 if R - L > 1 else max(L, first)
        points.append(probed)
        values.append(row[probed])
        if R - L > 1:
            if row[probed] <= max_sse:
                L = probed
            else:
                R = probed
    return (L, True, points, values) if L >= first else (first, False, points, values)


def thresholds_of_step(ref, step):
    """Image i of step s: the squared error of point (s + i) % (K + 1) -- the K + 1-th being "under the smallest": nothing meets it --,
    exact, and one under it every other time the index comes round."""
    (sse, k_points) = (ref['sse'], ref['k_points'])
    thresholds = numpy.zeros(BATCH, dtype=numpy.int64)
    for i in range(BATCH):
        j = (step + i) % (k_points + 1)
        thresholds[i] = sse[i, j] - ((step + i)//(k_points + 1)) % 2 if j < k_points else sse[i].min() - 1
    return thresholds


def expected_of_step(ref, thresholds, budgets=None):
    from autoencoder_based_image_compression_amd import ratecontrol
    budgets = numpy.full(BATCH, NO_BUDGET, dtype=numpy.int64) if budgets is None else numpy.asarray(budgets, dtype=numpy.int64)
    (first, _) = ratecontrol.select_by_upper_bound(ref['upper'], ref['valid'], budgets)
    searched = [bisect(ref['sse'][i].tolist(), int(first[i]), int(thresholds[i])) for i in range(BATCH)]
    point = numpy.array([s[0] for s in searched], dtype=numpy.int64)
    chosen = [ref['points'][i][int(point[i])] for i in range(BATCH)]
    blob_bytes = numpy.array([len(p['blob']) for p in chosen], dtype=numpy.int64)
    (coder_bits, exception_bits) = (numpy.array([p[key] for p in chosen], dtype=numpy.int64) for key in ('coder_bits', 'exception_bits'))
    values = {'rate_point': point, 'first_point': first, 'met': numpy.array([s[1] for s in searched], dtype=bool), 'max_sse': thresholds,
              'probe_points': numpy.array([s[2] for s in searched], dtype=numpy.int64), 'probe_sse': numpy.array([s[3] for s in searched], dtype=numpy.int64),
              'upper_bound_bytes': ref['upper'], 'budget_bytes': budgets, 'blob_bytes': blob_bytes,
              'promised': ref['upper'][numpy.arange(BATCH), point] <= budgets, 'fits': blob_bytes <= budgets,
              'nb_bits': coder_bits + exception_bits, 'coder_bits': coder_bits, 'exception_bits': exception_bits,
              'sse': numpy.array([p['sse'] for p in chosen], dtype=numpy.int64), 'nb_deads': numpy.array([p['nb_deads'] for p in chosen], dtype=numpy.int64),
              'container_bytes': blob_bytes - ref['header_bytes']}
    # (the table is the reference's own: what a round found is the squared error of the point it probed, the published one the chosen point's)
    assert all(values['probe_sse'][i, r] == ref['sse'][i, values['probe_points'][i, r]] for i in range(BATCH) for r in range(values['probe_sse'].shape[1]))
    assert numpy.array_equal(values['sse'], ref['sse'][numpy.arange(BATCH), point])
    return values, [p['blob'] for p in chosen], numpy.stack([p['decoded'] for p in chosen])


def assert_reference_coverage(ref, nb_steps, budgets=None):
    """On the reference alone, before the codec is consulted: over the steps every ladder index is chosen and both values of `met` occur."""
    (points, mets) = (set(), set())
    for step in range(nb_steps):
        (values, _, _) = expected_of_step(ref, thresholds_of_step(ref, step), budgets)
        points.update(values['rate_point'].tolist())
        mets.update(values['met'].tolist())
    if budgets is None:
        assert points == set(range(ref['k_points'])), (points, ref['sse'].tolist())
    assert mets == {True, False}


def build(ref, mode, **more):
    from autoencoder_based_image_compression_amd import codec
    return codec.QualityCodec(ref['variables'], ref['learned'], ref['ladder'], BATCH, SHAPE[0], SHAPE[1], nb_in_flight=2, keep_reconstruction=True,
                              container_capacity_bytes=8*BATCH*SHAPE[0]*SHAPE[1], **dict(MODES[mode], **more))


def check_step(ref, ticket, thresholds, step, budgets=None, decoder=None):
    """The ticket against the reference."""
    (values, blobs, decoded) = expected_of_step(ref, thresholds, budgets)
    r = ticket.result()
    for key in KEYS:
        print('step', step, key, numpy.asarray(r[key]).tolist(), 'reference', values[key].tolist())
        assert r[key].dtype == values[key].dtype and numpy.array_equal(r[key], values[key]), (step, key)
    containers = ticket.image_containers()
    assert [bytes(blob) for blob in containers] == blobs, step
    with pytest.raises(RuntimeError, match='one rate point'):
        ticket.container()
    reconstruction = ticket.reconstruction_uint8.cpu().numpy()
    assert numpy.array_equal(reconstruction, decoded), step
    if decoder is not None:
        assert numpy.array_equal(decoder.submit(containers).result(), reconstruction), step
    return r


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('name', sorted(CASES))
def test_every_step_lands_where_the_bisection_of_the_reference_puts_it(references, name, mode):
    from autoencoder_based_image_compression_amd import codec, ratecontrol
    ref = reference(references, name)
    images = torch.from_numpy(ref['images']).cuda()
    nb_steps = 2*4 + 1
    assert_reference_coverage(ref, nb_steps)
    with build(ref, mode) as c, codec.BatchDecoder(ref['variables'], ref['learned'], BATCH, SHAPE[0], SHAPE[1], ref['length']) as decoder:
        assert c.emit_container and c.nb_slots == 4 and nb_steps == 2*c.nb_slots + 1
        assert c.nb_rounds == ratecontrol.quality_rounds(ref['k_points']) == (2 if ref['k_points'] == 3 else 4)
        for step in range(nb_steps):
            thresholds = thresholds_of_step(ref, step)
            ticket = c.submit(images, max_sse=thresholds if step % 2 else thresholds.tolist())
            check_step(ref, ticket, thresholds, step, decoder=decoder if step < 1 else None)


def test_a_budget_moves_the_finest_point_the_search_may_take(references):
    ref = reference(references, 'fixed_L10_exception')
    images = torch.from_numpy(ref['images']).cuda()
    # image i gets the bound of point i: the search of image 1 starts at point 1 or later, that of image 2 at point 2 (the last one)
    budgets = ref['upper'][numpy.arange(BATCH), numpy.arange(BATCH)]
    (values, _, _) = expected_of_step(ref, thresholds_of_step(ref, 0), budgets)
    assert (values['first_point'] > 0).any() and values['first_point'][0] == 0
    assert_reference_coverage(ref, 9, budgets)
    not_promised = False
    with build(ref, 'launches', budget_bytes=budgets) as c:
        for step in range(9):
            thresholds = thresholds_of_step(ref, step)
            # (every other step names the budgets itself, one byte under the bounds: the point of the bound is then out of reach)
            given = budgets - 1 if step % 2 else None
            r = check_step(ref, c.submit(images, max_sse=thresholds, budget_bytes=given), thresholds, step, budgets if given is None else given)
            assert (r['rate_point'] >= r['first_point']).all()
            assert numpy.array_equal(r['promised'], r['upper_bound_bytes'][numpy.arange(BATCH), r['rate_point']] <= r['budget_bytes'])
            assert numpy.array_equal(r['fits'], r['blob_bytes'] <= r['budget_bytes'])
            assert not (r['promised'] & ~r['fits']).any()         # (expected, not proven: the allowance of ratecontrol.py is measured)
            not_promised = not_promised or not r['promised'].all()
    assert not_promised                                           # image 2 one byte under the last point's bound: nothing is promised


def test_thresholds_as_psnr_defaults_and_scalars(references):
    from autoencoder_based_image_compression_amd import ratecontrol
    from autoencoder_based_image_compression_amd.kodak.tools import tools as tls
    ref = reference(references, 'fixed_L10')
    images = torch.from_numpy(ref['images']).cuda()
    nb_pixels = SHAPE[0]*SHAPE[1]
    # a target that the middle point of image 0 meets exactly: the float64 PSNR of its squared error
    target = float(tls.psnr_from_sse(int(ref['sse'][0, 1]), nb_pixels))
    assert int(ratecontrol.max_sse_for_psnr(target, nb_pixels)) == int(ref['sse'][0, 1])
    targets = numpy.array([target, 20., 60.])
    thresholds = ratecontrol.max_sse_for_psnr(targets, nb_pixels)
    with build(ref, 'launches', target_psnr=targets) as c:
        check_step(ref, c.submit(images), thresholds, 'default')
        check_step(ref, c.submit(images, target_psnr=target), numpy.full(BATCH, ref['sse'][0, 1], dtype=numpy.int64), 'scalar psnr')
        check_step(ref, c.submit(images, max_sse=0), numpy.zeros(BATCH, dtype=numpy.int64), 'scalar max_sse')
        for bad in ({'max_sse': [1, 2]}, {'max_sse': 1.5}, {'target_psnr': [30., 31.]}, {'target_psnr': numpy.nan},
                    {'max_sse': 5, 'budget_bytes': 1.5}):
            with pytest.raises(ValueError):
                c.submit(images, **bad)


def test_the_host_loop_lands_on_the_same_points(references):
    from autoencoder_based_image_compression_amd import container, ratecontrol
    ref = reference(references, 'fixed_L10_exception')
    for (step, budgets) in ((0, None), (1, None), (3, None), (5, ref['upper'][numpy.arange(BATCH), numpy.arange(BATCH)]), (6, int(ref['upper'][:, 1].max()))):
        thresholds = thresholds_of_step(ref, step)
        (values, expected_blobs, _) = expected_of_step(ref, thresholds, None if budgets is None else numpy.broadcast_to(budgets, (BATCH,)))
        (blobs, info) = container.encode_images_to_quality(ref['images'], ref['encoder'], ref['decoder'], ref['ladder'], max_sse=thresholds,
                                                           budget_bytes=budgets)
        assert [bytes(blob) for blob in blobs] == expected_blobs, step
        for key in ('rate_point', 'first_point', 'met', 'max_sse', 'probe_points', 'probe_sse', 'blob_bytes', 'upper_bound_bytes'):
            assert info[key].dtype == values[key].dtype and numpy.array_equal(info[key], values[key]), (step, key)
    # the same through a PSNR, and the two ways to say it wrong
    nb_pixels = SHAPE[0]*SHAPE[1]
    (blobs, info) = container.encode_images_to_quality(ref['images'], ref['encoder'], ref['decoder'], ref['ladder'], target_psnr=25.)
    (values, expected_blobs, _) = expected_of_step(ref, numpy.full(BATCH, ratecontrol.max_sse_for_psnr(25., nb_pixels), dtype=numpy.int64))
    assert [bytes(blob) for blob in blobs] == expected_blobs and numpy.array_equal(info['rate_point'], values['rate_point'])
    for bad in ({}, {'target_psnr': 30., 'max_sse': 5}):
        with pytest.raises(ValueError, match='target_psnr'):
            container.encode_images_to_quality(ref['images'], ref['encoder'], ref['decoder'], ref['ladder'], **bad)


def test_refusals(references):
    from autoencoder_based_image_compression_amd import codec
    ref = reference(references, 'fixed_L10')
    ladder = ref['ladder']
    images = torch.from_numpy(ref['images']).cuda()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match='QualityCodec.*coding_tile'):
        codec.QualityCodec(ref['variables'], False, ladder, BATCH, SHAPE[0], SHAPE[1], max_sse=5, coding_tile=(2, 2))
    with pytest.raises(ValueError, match='not both'):
        codec.QualityCodec(ref['variables'], False, ladder, BATCH, SHAPE[0], SHAPE[1], target_psnr=30., max_sse=5)
    for (options, error) in (({'fuse_latent': True}, ValueError), ({'coder': 'host'}, ValueError), ({'coder_chunks': 2}, ValueError),
                             ({'emit_container': False}, ValueError), ({'max_sse': [1, 2]}, ValueError), ({'budget_bytes': [1, 2]}, ValueError)):
        with pytest.raises(error):
            codec.QualityCodec(ref['variables'], False, ladder, BATCH, SHAPE[0], SHAPE[1], **options)
    assert torch.cuda.memory_allocated() == before
    with build(ref, 'launches') as c:
        with pytest.raises(ValueError, match='neither'):
            c.submit(images)
        with pytest.raises(ValueError, match='not both'):
            c.submit(images, target_psnr=30., max_sse=5)
        # the codec still takes a step
        thresholds = thresholds_of_step(ref, 0)
        check_step(ref, c.submit(images, max_sse=thresholds), thresholds, 'after')
