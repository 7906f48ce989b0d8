"""`codec.TiledBudgetCodec`: a rate point per image chosen inside the step, on the device, to a byte budget, for tile-indexed (`EAT1`)
containers, and `container.encode_images_to_budget(coding_tile=...)`, its trial-coding counterpart.

tests/test_gpu_budget_codec.py's scheme and images: three 176 x 208 images of three entropies (an 11 x 13 latent plane), a ladder of
three points at 1, 2 and 4 times the model's bin widths, L = 10 and 3, with and without an exception map, the learned-bin-width model
once; coding tiles of (4, 4) -- twelve tiles of four shape classes, down to 3 x 1 -- and (16, 16), clamped to one tile per plane;
launch by launch and replayed as hipGraphs, 2 x nb_slots + 1 steps whose budgets change every step, at a bound and one byte under it.

The reference: `DeviceEncoder` latents and `device.ladder_histograms_tiles` (held against numpy in
tests/test_gpu_tiled_ladder_kernels.py), the host rule of ratecontrol.py for the expected point, bounds and promise,
`container.encode_images(..., coding_tile=...)` of every image at every point for the expected blob, bit counts and sizes,
`container.decode_images` of that blob for the reconstruction and the squared error, the image-by-image functions of `kodak/` for the
exception map's cost and the dead maps. Every comparison is exact."""
import numpy
import pytest
import torch

import guarded
import model_cases
import slot_buffers
import tiled_budget_slot_buffers
from test_gpu_budget_codec import BATCH, CASES, MODES, MULTIPLIERS, SHAPE, _images, assert_coverage, budgets_of_step, check_step

pytestmark = pytest.mark.gpu

(H_MAP, W_MAP) = (11, 13)
MAP_SIZE = H_MAP*W_MAP
TILED_CASES = [(name, (4, 4)) for name in sorted(CASES)] + [('fixed_L10_exception', (16, 16)), ('fixed_L3', (16, 16))]


@pytest.fixture(scope='module')
def references(tmp_path_factory):
    return {'directory': tmp_path_factory.mktemp('tiled_budget')}


def reference(cache, name, coding_tile):
    """Once per (case, coding tile): the ladder, and for every (image, point) what the existing functions give."""
    key = (name, coding_tile)
    if key in cache:
        return cache[key]
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
    (hist, bypass, _) = dev.ladder_histograms_tiles(y_device.view(BATCH, H_MAP, W_MAP, 128), torch.from_numpy(bin_widths_points).cuda(), coding_tile,
                                                    torch.from_numpy(map_mean).cuda(), length)
    (hist, bypass) = (hist.cpu().numpy().astype(numpy.int64), bypass.cpu().numpy())
    header_bytes = ratecontrol.header_bytes(ladder, SHAPE[0], SHAPE[1], coding_tile)
    out = {'variables': v, 'learned': learned, 'length': length, 'images': images, 'ladder': ladder, 'coding_tile': coding_tile,
           'encoder': encoder, 'decoder': decoder,
           'upper': ratecontrol.upper_bounds_fixed_tiles(hist, bypass, ladder, MAP_SIZE, header_bytes),
           'valid': ratecontrol.valid_points(hist.sum(axis=2), MAP_SIZE), 'header_bytes': header_bytes, 'points': [],
           'bounds': ratecontrol.blob_byte_bounds(hist, bypass, ladder, SHAPE[0], SHAPE[1], coding_tile)}
    assert out['valid'].all()
    paths = []
    for k in range(len(MULTIPLIERS)):
        paths.append(str(cache['directory']/'{0}_{1}_{2}.npy'.format(name, coding_tile[0], k)))
        numpy.save(paths[k], tables[k])
    for i in range(BATCH):
        row = []
        for k in range(len(MULTIPLIERS)):
            (blob, info) = container.encode_images(images[i:i + 1], encoder, bin_widths_points[k], map_mean, tables[k], exception,
                                                   coding_tile=coding_tile)
            assert blob[:4] == b'EAT1' and info['header_bytes'] == header_bytes
            decoded = container.decode_images(blob, decoder)
            difference = images[i:i + 1].astype(numpy.int64) - decoded.astype(numpy.int64)
            per_map = info['nb_bits'].astype(numpy.int64).copy()              # summed over the image's tiles (section 15)
            if exception >= 0:
                per_map[:, exception] = 0                        # charged by its entropy (compression.py:68-81)
            cq = tls.quantize_per_map(y[i:i + 1] - numpy.tile(map_mean, y[i:i + 1].shape[:3] + (1,)), bin_widths_points[k])
            # the exception map's entropy cost does not depend on the tiles: the whole-map coder's bits of the other maps drop out
            whole = container.encode_images(images[i:i + 1], encoder, bin_widths_points[k], map_mean, tables[k], exception)[1]['nb_bits'].astype(numpy.int64)
            if exception >= 0:
                whole[:, exception] = 0
            path_bits = int(compression.rescale_compress_lossless_maps(cq[0], bin_widths_points[k], paths[k], exception))
            exception_bits = path_bits - int(whole.sum())
            assert exception_bits >= 0 and (exception >= 0 or exception_bits == 0)
            row.append({'blob': blob, 'decoded': decoded[0], 'sse': int((difference*difference).sum()), 'coder_bits': int(per_map.sum()),
                        'exception_bits': exception_bits, 'nb_deads': int(numpy.asarray(tls.count_nb_deads(cq)).reshape(-1)[0])})
        out['points'].append(row)
    sizes = numpy.array([[len(p['blob']) for p in row] for row in out['points']])
    print(name, coding_tile, 'blob sizes', sizes.tolist(), 'upper bounds', out['upper'].tolist(), 'float bounds', out['bounds'][0].tolist(),
          out['bounds'][1].tolist())
    # a condition on the inputs: every real blob lies within its bounds (the allowances of ratecontrol.py are measured, not proven)
    assert (sizes <= out['upper']).all() and (out['bounds'][0] <= sizes).all() and (sizes <= out['bounds'][1]).all()
    out['sizes'] = sizes
    cache[key] = out
    return out


def build(ref, mode, **more):
    from autoencoder_based_image_compression_amd import codec
    return codec.TiledBudgetCodec(ref['variables'], ref['learned'], ref['ladder'], BATCH, SHAPE[0], SHAPE[1], ref['coding_tile'], nb_in_flight=2,
                                  keep_reconstruction=True, container_capacity_bytes=8*BATCH*SHAPE[0]*SHAPE[1], **dict(MODES[mode], **more))


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('name, coding_tile', TILED_CASES)
def test_every_step_lands_where_the_host_rule_puts_it(references, name, coding_tile, mode):
    from autoencoder_based_image_compression_amd import codec
    ref = reference(references, name, coding_tile)
    images = torch.from_numpy(ref['images']).cuda()
    (points, promises) = ([], [])
    with build(ref, mode) as c, codec.BatchDecoder(ref['variables'], ref['learned'], BATCH, SHAPE[0], SHAPE[1], ref['length'],
                                                   coding_tile=coding_tile) as decoder:
        assert c.emit_container and c.nb_slots == 4 and c.coding_tile == (min(coding_tile[0], H_MAP), min(coding_tile[1], W_MAP))
        for step in range(2*c.nb_slots + 1):
            budgets = budgets_of_step(ref, step)
            ticket = c.submit(images, budgets if step % 2 else budgets.tolist())
            (p, q) = check_step(ref, ticket, budgets, step, decoder if step < 2 else None)
            points += p
            promises += q
    assert_coverage(points, promises)


def test_the_blobs_give_crops(references):
    """One step's blobs, each at another point, through `container.decode_region`: the crop of `decode_images` of the same blob."""
    from autoencoder_based_image_compression_amd import container
    ref = reference(references, 'fixed_L10_exception', (4, 4))
    images = torch.from_numpy(ref['images']).cuda()
    budgets = numpy.array([ref['upper'][0, 0], ref['upper'][1, 1], ref['upper'][2, 2]])
    with build(ref, 'launches') as c:
        ticket = c.submit(images, budgets)
        assert ticket.result()['rate_point'].tolist() == [0, 1, 2]
        blobs = ticket.image_containers()
    for (i, blob) in enumerate(blobs):
        header = container.read_header(blob)
        assert header['format'] == 'EAT1' and header['coding_tile'] == (4, 4) and header['nb_images'] == 1
        whole = container.decode_images(blob, ref['decoder'])
        assert numpy.array_equal(whole[0], ref['points'][i][i]['decoded'])
        crop = container.decode_region(blob, ref['decoder'], (40, 72, 64, 80))
        assert numpy.array_equal(crop, whole[:, 40:104, 72:152])


def test_refused_options_raise_in_front_of_every_allocation(references):
    from autoencoder_based_image_compression_amd import codec, ratecontrol
    ref = reference(references, 'fixed_L10', (4, 4))
    ladder = ref['ladder']
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for (options, error) in (({'fuse_latent': True}, ValueError), ({'coder': 'host'}, ValueError), ({'coder': 'none'}, ValueError),
                             ({'coder_chunks': 2}, ValueError), ({'emit_container': False}, ValueError), ({'idx_map_exception': 3}, TypeError)):
        with pytest.raises(error):
            codec.TiledBudgetCodec(ref['variables'], False, ladder, BATCH, SHAPE[0], SHAPE[1], (4, 4), **options)
    for bad_tile in ((0, 4), (4,), 4, (70000, 4)):
        with pytest.raises(ValueError):
            codec.TiledBudgetCodec(ref['variables'], False, ladder, BATCH, SHAPE[0], SHAPE[1], bad_tile)
    long_ladder = ratecontrol.RateLadder(numpy.tile(ladder.bin_widths_points[:1], (10, 1)), numpy.tile(ladder.binary_probabilities_points[:1], (10, 1, 1)),
                                         ladder.map_mean)
    with pytest.raises(ValueError, match='ladder_max_points'):
        codec.TiledBudgetCodec(ref['variables'], False, long_ladder, BATCH, SHAPE[0], SHAPE[1], (4, 4))
    with pytest.raises(ValueError, match='65535'):                     # 459 images of 143 tiles each
        codec.TiledBudgetCodec(ref['variables'], False, ladder, 459, SHAPE[0], SHAPE[1], (1, 1))
    # `BudgetCodec` itself goes on refusing the tile
    with pytest.raises(ValueError, match='coding_tile'):
        codec.BudgetCodec(ref['variables'], False, ladder, BATCH, SHAPE[0], SHAPE[1], coding_tile=(4, 4))
    assert torch.cuda.memory_allocated() == before


@pytest.mark.parametrize('mode', sorted(MODES))
def test_steps_on_poisoned_slots_between_guard_bands(references, mode):
    """tests/test_gpu_budget_codec.py's procedure on a `TiledBudgetCodec`: every device buffer of its slots between guard bands, the
    bands verified after every step, every SCRATCH buffer of `_Slot` AND of `_TiledBudgetSlot` filled with 0xFF between steps."""
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    ref = reference(references, 'fixed_L10_exception', (4, 4))
    images = torch.from_numpy(ref['images']).cuda()
    poison = 0xFF
    (points, promises) = ([], [])

    def between_steps(c, guard):
        c.drain()
        guard.check(keep=True)
        assert slot_buffers.poison_scratch(c, poison) > 0 and tiled_budget_slot_buffers.poison_scratch(c, poison) > 0

    with guarded.guarded((device, pipeline, codec), poison) as guard:
        with build(ref, mode) as c:
            for owner in tiled_budget_slot_buffers.budget_slots(c):
                assert slot_buffers.check_tiling(owner, tiled_budget_slot_buffers.TILED_BUDGET_SLOT) == ['accum', 'select', 'table']
                assert tuple(owner.hist.shape) == (BATCH, 3, 12, 128, 11) and owner.prob_row.numel() == BATCH*12*128
                assert sum(rows.numel() for rows in owner.class_rows) == owner.prob_row.numel()
            torch.cuda.synchronize()
            between_steps(c, guard)
            for step in range(2*c.nb_slots + 1):
                budgets = budgets_of_step(ref, step)
                (p, q) = check_step(ref, c.submit(images, budgets), budgets, step)
                points += p
                promises += q
                between_steps(c, guard)
    assert_coverage(points, promises)


@pytest.mark.parametrize('name', ['fixed_L10_exception', 'fixed_L3'])
def test_encode_images_to_budget_in_tiles_against_brute_force(references, name):
    """Every budget at, and one byte under, every blob size: the first point in ladder order whose blob fits, and that blob byte for
    byte; the brute force is the reference's `encode_images(..., coding_tile=(4, 4))` of every image at every point."""
    from autoencoder_based_image_compression_amd import container
    ref = reference(references, name, (4, 4))
    sizes = ref['sizes']
    budgets = [sizes[:, k] - delta for k in range(3) for delta in (0, 1)] + [int(sizes.max()) + 1000, 0]
    for budget in budgets:
        (blobs, info) = container.encode_images_to_budget(ref['images'], ref['encoder'], ref['ladder'], budget, coding_tile=(4, 4))
        print(name, 'budget', numpy.asarray(budget).tolist(), 'rate_point', info['rate_point'].tolist(), 'attempts', info['attempts'].tolist())
        assert numpy.array_equal(info['lower_bytes'], ref['bounds'][0]) and numpy.array_equal(info['upper_bytes'], ref['bounds'][1])
        assert info['upper_bound_misses'] == 0
        per_image = numpy.broadcast_to(numpy.asarray(budget), (BATCH,))
        for i in range(BATCH):
            fitting = [k for k in range(3) if sizes[i, k] <= per_image[i]]
            (k, fits) = (fitting[0], True) if fitting else (2, False)
            assert (int(info['rate_point'][i]), bool(info['fits'][i])) == (k, fits), (i, per_image[i])
            assert blobs[i] == ref['points'][i][k]['blob']
            assert int(info['blob_bytes'][i]) == sizes[i, k] and 1 <= int(info['attempts'][i]) <= 3
    # without the tile the function is what it was: EAE1 blobs
    (plain, _) = container.encode_images_to_budget(ref['images'][:1], ref['encoder'], ref['ladder'], int(sizes.max()) + 1000)
    assert plain[0][:4] == b'EAE1'
