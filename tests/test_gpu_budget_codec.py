"""`codec.BudgetCodec`: a rate point per image chosen inside the step, on the device, to a byte budget.

Three 176 x 208 images (an 11 x 13 latent plane: 143 symbols per map, tiles of 32 positions straddle the images), a ladder of three
points at 1, 2 and 4 times the model's bin widths with the tables of `stats.compute_binary_probabilities_ladder`, L = 10 and 3, with
and without an exception map, the learned-bin-width model once; launch by launch and replayed as hipGraphs, 2 x nb_slots + 1 steps
whose budgets change every step.

The reference uses nothing under test: `DeviceEncoder` latents and `device.ladder_histograms`, the host rule of ratecontrol.py for
the expected point, bounds and promise, `container.encode_images` of every image at every point for the expected blob, bit counts and
sizes, `container.decode_images` of that blob for the reconstruction and the squared error, the image-by-image functions of `kodak/`
for the exception map's cost and the dead maps. Every comparison is exact."""
import numpy
import pytest
import torch

import budget_slot_buffers
import guarded
import model_cases
import slot_buffers

pytestmark = pytest.mark.gpu

SHAPE = (176, 208)
MAP_SIZE = 11*13
BATCH = 3
MULTIPLIERS = (1., 2., 4.)
EXCEPTION = 5
MODES = {'launches': {}, 'graphs': {'use_graphs': True}}
# (model kind, truncated unary length, exception map)
CASES = {'fixed_L10_exception': (False, 10, EXCEPTION), 'fixed_L10': (False, 10, -1), 'fixed_L3_exception': (False, 3, EXCEPTION),
         'fixed_L3': (False, 3, -1), 'learned_L10_exception': (True, 10, EXCEPTION)}
KEYS = ('rate_point', 'upper_bound_bytes', 'budget_bytes', 'blob_bytes', 'promised', 'fits', 'nb_bits', 'coder_bits', 'exception_bits', 'sse',
        'nb_deads', 'container_bytes')


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
    return {'directory': tmp_path_factory.mktemp('budget')}


def reference(cache, name):
    """Once per case: the ladder, and for every (image, point) what the existing functions give."""
    if name in cache:
        return cache[name]
    from autoencoder_based_image_compression_amd import container, device as dev, pipeline, ratecontrol
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
    y_device = encoder(torch.from_numpy(images).cuda())
    y = y_device.cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y)
    tables = lossless_stats.compute_binary_probabilities_ladder(y, bin_widths_points, map_mean, length)
    ladder = ratecontrol.RateLadder(bin_widths_points, tables, map_mean, exception)
    (hist, bypass, _) = dev.ladder_histograms(y_device, torch.from_numpy(bin_widths_points).cuda(), torch.from_numpy(map_mean).cuda(), length)
    (hist, bypass) = (hist.cpu().numpy(), bypass.cpu().numpy())
    out = {'variables': v, 'learned': learned, 'length': length, 'images': images, 'ladder': ladder,
           'upper': ratecontrol.upper_bounds_fixed(hist, bypass, ladder, MAP_SIZE), 'valid': ratecontrol.valid_points(hist, MAP_SIZE),
           'header_bytes': ratecontrol.header_bytes(ladder), 'points': []}
    assert out['valid'].all()
    paths = []
    for k in range(len(MULTIPLIERS)):
        paths.append(str(cache['directory']/'{0}_{1}.npy'.format(name, k)))
        numpy.save(paths[k], tables[k])
    for i in range(BATCH):
        row = []
        for k in range(len(MULTIPLIERS)):
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
    sizes = numpy.array([[len(p['blob']) for p in row] for row in out['points']])
    print(name, 'blob sizes', sizes.tolist(), 'upper bounds', out['upper'].tolist())
    assert (sizes <= out['upper']).all()
    cache[name] = out
    return out


def budgets_of_step(ref, step):
    """Image i of step s: the bound of point (s + i) % 4 -- the fourth being "under the coarsest point's bound": nothing fits --, at
    the bound in four steps and one byte under it in the next four."""
    upper = ref['upper']
    budgets = numpy.zeros(BATCH, dtype=numpy.int64)
    for i in range(BATCH):
        j = (step + i) % 4
        budgets[i] = (upper[i, j] - (step//4) % 2) if j < 3 else upper[i].min() - 1
    return budgets


def expected_of_step(ref, budgets):
    from autoencoder_based_image_compression_amd import ratecontrol
    (point, promised) = ratecontrol.select_by_upper_bound(ref['upper'], ref['valid'], budgets)
    chosen = [ref['points'][i][int(point[i])] for i in range(BATCH)]
    blob_bytes = numpy.array([len(p['blob']) for p in chosen], dtype=numpy.int64)
    (coder_bits, exception_bits) = (numpy.array([p[key] for p in chosen], dtype=numpy.int64) for key in ('coder_bits', 'exception_bits'))
    values = {'rate_point': point, 'upper_bound_bytes': ref['upper'], 'budget_bytes': budgets, 'blob_bytes': blob_bytes, 'promised': promised,
              'fits': blob_bytes <= budgets, 'nb_bits': coder_bits + exception_bits, 'coder_bits': coder_bits, 'exception_bits': exception_bits,
              'sse': numpy.array([p['sse'] for p in chosen], dtype=numpy.int64), 'nb_deads': numpy.array([p['nb_deads'] for p in chosen], dtype=numpy.int64),
              'container_bytes': blob_bytes - ref['header_bytes']}
    return values, [p['blob'] for p in chosen], numpy.stack([p['decoded'] for p in chosen])


def build(ref, mode, **more):
    from autoencoder_based_image_compression_amd import codec
    return codec.BudgetCodec(ref['variables'], ref['learned'], ref['ladder'], BATCH, SHAPE[0], SHAPE[1], nb_in_flight=2, keep_reconstruction=True,
                             container_capacity_bytes=8*BATCH*SHAPE[0]*SHAPE[1], **dict(MODES[mode], **more))


def check_step(ref, ticket, budgets, step, decoder=None):
    """The ticket against the reference; returns (rate points, promised) of the step."""
    (values, blobs, decoded) = expected_of_step(ref, budgets)
    r = ticket.result()
    for key in KEYS:
        print('step', step, key, numpy.asarray(r[key]).tolist(), 'reference', values[key].tolist())
        assert r[key].dtype == values[key].dtype and numpy.array_equal(r[key], values[key]), (step, key)
    assert not (r['promised'] & ~r['fits']).any()                 # (expected, not proven: the allowance of ratecontrol.py is measured)
    containers = ticket.image_containers()
    assert [bytes(blob) for blob in containers] == blobs, step
    with pytest.raises(RuntimeError, match='one rate point'):
        ticket.container()
    reconstruction = ticket.reconstruction_uint8.cpu().numpy()
    assert numpy.array_equal(reconstruction, decoded), step
    if decoder is not None:
        assert numpy.array_equal(decoder.submit(containers).result(), reconstruction), step
    return r['rate_point'].tolist(), r['promised'].tolist()


def assert_coverage(points, promises):
    assert set(points) == {0, 1, 2} and not all(promises) and any(promises)


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('name', sorted(CASES))
def test_every_step_lands_where_the_host_rule_puts_it(references, name, mode):
    from autoencoder_based_image_compression_amd import codec
    ref = reference(references, name)
    images = torch.from_numpy(ref['images']).cuda()
    (points, promises) = ([], [])
    with build(ref, mode) as c, codec.BatchDecoder(ref['variables'], ref['learned'], BATCH, SHAPE[0], SHAPE[1], ref['length']) as decoder:
        assert c.emit_container and c.nb_slots == 4
        for step in range(2*c.nb_slots + 1):
            budgets = budgets_of_step(ref, step)
            ticket = c.submit(images, budgets if step % 2 else budgets.tolist())
            (p, q) = check_step(ref, ticket, budgets, step, decoder if step < 2 else None)
            points += p
            promises += q
    assert_coverage(points, promises)


def test_the_default_budget_and_a_scalar(references):
    ref = reference(references, 'fixed_L10')
    images = torch.from_numpy(ref['images']).cuda()
    scalar = int(ref['upper'][:, 1].max())
    with build(ref, 'launches', budget_bytes=scalar) as c:
        check_step(ref, c.submit(images), numpy.full(BATCH, scalar, dtype=numpy.int64), 'default')
        check_step(ref, c.submit(images, 0), numpy.zeros(BATCH, dtype=numpy.int64), 'scalar')
        for bad in ([1, 2], 1.5, numpy.zeros((BATCH, 1), dtype=numpy.int64)):
            with pytest.raises(ValueError):
                c.submit(images, bad)
    with build(ref, 'launches') as c:
        with pytest.raises(ValueError, match='budget_bytes'):
            c.submit(images)


def test_refused_options_raise_in_front_of_every_allocation(references):
    from autoencoder_based_image_compression_amd import codec, ratecontrol
    ref = reference(references, 'fixed_L10')
    ladder = ref['ladder']
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for (options, error) in (({'coding_tile': (2, 2)}, ValueError), ({'fuse_latent': True}, ValueError), ({'coder': 'host'}, ValueError),
                             ({'coder': 'none'}, ValueError), ({'coder_chunks': 2}, ValueError), ({'emit_container': False}, ValueError),
                             ({'idx_map_exception': 3}, TypeError)):
        with pytest.raises(error):
            codec.BudgetCodec(ref['variables'], False, ladder, BATCH, SHAPE[0], SHAPE[1], **options)
    with pytest.raises(TypeError):
        codec.BudgetCodec(ref['variables'], False, None, BATCH, SHAPE[0], SHAPE[1])
    with pytest.raises(ValueError, match='budget_bytes'):
        codec.BudgetCodec(ref['variables'], False, ladder, BATCH, SHAPE[0], SHAPE[1], budget_bytes=[1, 2])
    long_ladder = ratecontrol.RateLadder(numpy.tile(ladder.bin_widths_points[:1], (10, 1)), numpy.tile(ladder.binary_probabilities_points[:1], (10, 1, 1)),
                                         ladder.map_mean)
    with pytest.raises(ValueError, match='ladder_max_points'):
        codec.BudgetCodec(ref['variables'], False, long_ladder, BATCH, SHAPE[0], SHAPE[1])
    assert torch.cuda.memory_allocated() == before


def test_an_image_without_a_valid_point_fails_the_range_check(references):
    from autoencoder_based_image_compression_amd import ratecontrol
    ref = reference(references, 'fixed_L10')
    ladder = ref['ladder']
    tiny = ratecontrol.RateLadder(ladder.bin_widths_points*numpy.float32(1e-7), ladder.binary_probabilities_points, ladder.map_mean)
    images = torch.from_numpy(ref['images']).cuda()
    with build(dict(ref, ladder=tiny), 'launches') as c:
        ticket = c.submit(images, 10**9)
        with pytest.raises(AssertionError, match='16-bit signed integers'):
            ticket.result()
    # the codec next to it is unaffected
    with build(ref, 'launches') as c:
        check_step(ref, c.submit(images, budgets_of_step(ref, 0)), budgets_of_step(ref, 0), 'after')


@pytest.mark.parametrize('mode', sorted(MODES))
def test_steps_on_poisoned_slots_between_guard_bands(references, mode):
    """tests/test_gpu_codec_slots.py's procedure on a `BudgetCodec`: every device buffer of its slots between guard bands, the
    bands verified after every step, every SCRATCH buffer of `_Slot` AND of `_BudgetSlot` filled with 0xFF between steps; the
    tickets are those of the runs above."""
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    ref = reference(references, 'fixed_L10_exception')
    images = torch.from_numpy(ref['images']).cuda()
    poison = 0xFF
    (points, promises) = ([], [])

    def between_steps(c, guard):
        c.drain()
        guard.check(keep=True)
        assert slot_buffers.poison_scratch(c, poison) > 0 and budget_slot_buffers.poison_scratch(c, poison) > 0

    with guarded.guarded((device, pipeline, codec), poison) as guard:
        with build(ref, mode) as c:
            for owner in budget_slot_buffers.budget_slots(c):
                assert slot_buffers.check_tiling(owner, budget_slot_buffers.BUDGET_SLOT) == ['accum', 'select', 'table']
            for (owner, table) in slot_buffers.owners(c):
                assert 'block' in slot_buffers.check_tiling(owner, table)
            torch.cuda.synchronize()
            between_steps(c, guard)
            for step in range(2*c.nb_slots + 1):
                budgets = budgets_of_step(ref, step)
                (p, q) = check_step(ref, c.submit(images, budgets), budgets, step)
                points += p
                promises += q
                between_steps(c, guard)
    assert_coverage(points, promises)
