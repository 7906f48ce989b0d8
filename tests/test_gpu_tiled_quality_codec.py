"""`codec.TiledQualityCodec`: the coarsest rate point per image that keeps a PSNR floor, searched inside the step, on the device, for
tile-indexed (`EAT1`) containers, and `container.encode_images_to_quality(coding_tile=...)`, its host loop.

tests/test_gpu_quality_codec.py's images, model, ladders (16, 32, 64 times the bin widths, and nine points from 4 to 64 times: its
docstring says why), threshold schedule and checks, imported from it; coding tiles of (4, 4) -- twelve tiles of four shape classes on
the 11 x 13 latent plane, so that the coder's run order is not the payload order -- and (16, 16), clamped to one tile per plane; launch
by launch and replayed as hipGraphs, nine steps whose thresholds change every step.

The reference uses nothing under test. Per (image, point): `container.encode_images(..., coding_tile=...)` for the blob and the bit
counts, `container.decode_images` of THAT blob for the reconstruction and the squared error -- the table the probes must find --, the
whole-map module's image-by-image figures for the exception map's cost and the dead maps (neither depends on the tiles);
`device.ladder_histograms_tiles` + `ratecontrol.upper_bounds_fixed_tiles` + `select_by_upper_bound` (the rule of `TiledBudgetCodec`) for
the bounds and the first point; the bisection written in tests/test_gpu_quality_codec.py over that table for the choice. Every
comparison is exact."""
import numpy
import pytest
import torch

import test_gpu_quality_codec as whole_maps
from test_gpu_quality_codec import BATCH, CASES, MODES, SHAPE, assert_reference_coverage, check_step, expected_of_step, thresholds_of_step

pytestmark = pytest.mark.gpu

(H_MAP, W_MAP) = (11, 13)
MAP_SIZE = H_MAP*W_MAP
TILED_CASES = [('fixed_L10_exception', (4, 4)), ('fixed_L10_nine_points', (4, 4)), ('learned_L10_exception', (4, 4)),
               ('fixed_L10_exception', (16, 16))]
NB_STEPS = 9


@pytest.fixture(scope='module')
def references(tmp_path_factory):
    return {'directory': tmp_path_factory.mktemp('tiled_quality')}


def reference(cache, name, coding_tile):
    """Once per (case, coding tile): the whole-map module's reference with everything that depends on the container replaced."""
    key = (name, coding_tile)
    if key in cache:
        return cache[key]
    from autoencoder_based_image_compression_amd import container, device as dev, ratecontrol
    base = whole_maps.reference(cache, name)
    (ladder, images, encoder, decoder, exception) = (base['ladder'], base['images'], base['encoder'], base['decoder'], CASES[name][2])
    y = encoder(torch.from_numpy(images).cuda())
    (hist, bypass, _) = dev.ladder_histograms_tiles(y.view(BATCH, H_MAP, W_MAP, 128), torch.from_numpy(ladder.bin_widths_points).cuda(), coding_tile,
                                                    torch.from_numpy(ladder.map_mean).cuda(), base['length'])
    (hist, bypass) = (hist.cpu().numpy().astype(numpy.int64), bypass.cpu().numpy())
    header_bytes = ratecontrol.header_bytes(ladder, SHAPE[0], SHAPE[1], coding_tile)
    out = dict(base, coding_tile=coding_tile, whole=base, header_bytes=header_bytes, points=[], valid=ratecontrol.valid_points(hist.sum(axis=2), MAP_SIZE),
               upper=ratecontrol.upper_bounds_fixed_tiles(hist, bypass, ladder, MAP_SIZE, header_bytes))
    assert out['valid'].all()
    for i in range(BATCH):
        row = []
        for k in range(base['k_points']):
            (blob, info) = container.encode_images(images[i:i + 1], encoder, ladder.bin_widths_points[k], ladder.map_mean,
                                                   ladder.binary_probabilities_points[k], exception, coding_tile=coding_tile)
            assert blob[:4] == b'EAT1' and info['header_bytes'] == header_bytes
            decoded = container.decode_images(blob, decoder)
            difference = images[i:i + 1].astype(numpy.int64) - decoded.astype(numpy.int64)
            per_map = info['nb_bits'].astype(numpy.int64).copy()              # summed over the image's tiles (section 15)
            if exception >= 0:
                per_map[:, exception] = 0                        # charged by its entropy, which does not depend on the tiles
            row.append(dict(base['points'][i][k], blob=blob, decoded=decoded[0], sse=int((difference*difference).sum()), coder_bits=int(per_map.sum())))
        out['points'].append(row)
    out['sse'] = numpy.array([[p['sse'] for p in row] for row in out['points']], dtype=numpy.int64)
    sizes = numpy.array([[len(p['blob']) for p in row] for row in out['points']])
    print(name, coding_tile, 'squared errors', out['sse'].tolist(), 'upper bounds', out['upper'].tolist(), 'blob sizes', sizes.tolist())
    # conditions on the inputs: a point's squared error does not depend on the coding tile (the probes are `QualityCodec`'s); every
    # blob lies within its bound, and the bound of the tiled blob lies above the whole-map one (a budget can fall between the two)
    assert numpy.array_equal(out['sse'], base['sse'])
    assert (sizes <= out['upper']).all() and (out['upper'] > base['upper']).all()
    cache[key] = out
    return out


def build(ref, mode, **more):
    from autoencoder_based_image_compression_amd import codec
    return codec.TiledQualityCodec(ref['variables'], ref['learned'], ref['ladder'], BATCH, SHAPE[0], SHAPE[1], ref['coding_tile'], nb_in_flight=2,
                                   keep_reconstruction=True, container_capacity_bytes=8*BATCH*SHAPE[0]*SHAPE[1], **dict(MODES[mode], **more))


def budget_between_the_bounds(ref):
    """Budgets under which image 1's finest point fits as a whole-map blob and not as a tiled one: one byte under its `EAT1` bound at
    point 0, which is at or above its `EAE1` bound there. The other images have no budget to speak of."""
    budgets = numpy.full(BATCH, int(ref['upper'].max()) + 1000, dtype=numpy.int64)
    budgets[1] = ref['upper'][1, 0] - 1
    assert ref['whole']['upper'][1, 0] <= budgets[1] < ref['upper'][1, 0]
    return budgets


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('name, coding_tile', TILED_CASES)
def test_every_step_lands_where_the_bisection_of_the_reference_puts_it(references, name, coding_tile, mode):
    from autoencoder_based_image_compression_amd import codec, ratecontrol
    ref = reference(references, name, coding_tile)
    images = torch.from_numpy(ref['images']).cuda()
    assert_reference_coverage(ref, NB_STEPS)                      # every ladder point is taken, `met` occurs true and false
    with build(ref, mode) as c, codec.BatchDecoder(ref['variables'], ref['learned'], BATCH, SHAPE[0], SHAPE[1], ref['length'],
                                                   coding_tile=coding_tile) as decoder:
        assert c.emit_container and c.nb_slots == 4 and NB_STEPS == 2*c.nb_slots + 1
        assert c.coding_tile == (min(coding_tile[0], H_MAP), min(coding_tile[1], W_MAP))
        assert c.nb_rounds == ratecontrol.quality_rounds(ref['k_points']) == (2 if ref['k_points'] == 3 else 4)
        for step in range(NB_STEPS):
            thresholds = thresholds_of_step(ref, step)
            ticket = c.submit(images, max_sse=thresholds if step % 2 else thresholds.tolist())
            check_step(ref, ticket, thresholds, step, decoder=decoder if step < 1 else None)
            assert all(bytes(blob[:4]) == b'EAT1' for blob in ticket.image_containers())


def test_without_a_budget_the_search_is_the_whole_map_codecs(references):
    """The same images and thresholds through `QualityCodec`: the squared errors do not depend on the coding tile, so the probes, what
    they found and the choice are the same, step for step."""
    ref = reference(references, 'fixed_L10_exception', (4, 4))
    images = torch.from_numpy(ref['images']).cuda()
    with build(ref, 'launches') as tiled, whole_maps.build(ref['whole'], 'launches') as plain:
        for step in (0, 3, 7):
            thresholds = thresholds_of_step(ref, step)
            (r, s) = (tiled.submit(images, max_sse=thresholds).result(), plain.submit(images, max_sse=thresholds).result())
            for key in ('rate_point', 'first_point', 'met', 'max_sse', 'probe_points', 'probe_sse', 'sse', 'exception_bits', 'nb_deads', 'budget_bytes'):
                assert r[key].dtype == s[key].dtype and numpy.array_equal(r[key], s[key]), (step, key)
            assert (r['upper_bound_bytes'] > s['upper_bound_bytes']).all() and (r['blob_bytes'] > s['blob_bytes']).all()


def test_a_budget_between_the_two_bounds_moves_the_first_point(references):
    """A budget between the `EAE1` and the `EAT1` bound of image 1's point 0: `QualityCodec` may take that point, `TiledQualityCodec`
    may not -- the bound is that of the blob the step writes --, and every step lands where the reference's bisection from the tiled
    first point puts it."""
    ref = reference(references, 'fixed_L10_exception', (4, 4))
    images = torch.from_numpy(ref['images']).cuda()
    budgets = budget_between_the_bounds(ref)
    (values, _, _) = expected_of_step(ref, thresholds_of_step(ref, 0), budgets)
    (plain_values, _, _) = expected_of_step(ref['whole'], thresholds_of_step(ref, 0), budgets)
    assert values['first_point'].tolist() == [0, values['first_point'][1], 0] and values['first_point'][1] > 0
    assert plain_values['first_point'].tolist() == [0, 0, 0]
    assert_reference_coverage(ref, NB_STEPS, budgets)
    with build(ref, 'graphs', budget_bytes=budgets) as c, whole_maps.build(ref['whole'], 'launches', budget_bytes=budgets) as plain:
        for step in range(NB_STEPS):
            thresholds = thresholds_of_step(ref, step)
            # (every other step names the budgets itself)
            r = check_step(ref, c.submit(images, max_sse=thresholds, budget_bytes=budgets if step % 2 else None), thresholds, step, budgets)
            assert (r['rate_point'] >= r['first_point']).all() and r['first_point'][1] > 0
            assert numpy.array_equal(r['promised'], r['upper_bound_bytes'][numpy.arange(BATCH), r['rate_point']] <= r['budget_bytes'])
            assert not (r['promised'] & ~r['fits']).any()         # (expected, not proven: the allowance of ratecontrol.py is measured)
            if step < 2:
                s = plain.submit(images, max_sse=thresholds).result()
                assert s['first_point'].tolist() == [0, 0, 0] and r['first_point'][1] != s['first_point'][1]


def test_the_tiled_readers_take_the_blobs(references):
    """One step's blobs, each at another point, through `container.decode_region` and `container.decode_images`."""
    from autoencoder_based_image_compression_amd import container
    ref = reference(references, 'fixed_L10_exception', (4, 4))
    images = torch.from_numpy(ref['images']).cuda()
    thresholds = ref['sse'][numpy.arange(BATCH), numpy.arange(BATCH)]            # image i: exactly what its point i leaves
    with build(ref, 'launches') as c:
        ticket = c.submit(images, max_sse=thresholds)
        assert ticket.result()['rate_point'].tolist() == [0, 1, 2] and ticket.result()['met'].all()
        blobs = ticket.image_containers()
    for (i, blob) in enumerate(blobs):
        header = container.read_header(blob)
        assert header['format'] == 'EAT1' and header['coding_tile'] == (4, 4) and header['nb_images'] == 1
        whole = container.decode_images(blob, ref['decoder'])
        assert numpy.array_equal(whole[0], ref['points'][i][i]['decoded'])
        crop = container.decode_region(blob, ref['decoder'], (40, 72, 64, 80))
        assert numpy.array_equal(crop, whole[:, 40:104, 72:152])


def test_the_host_loop_lands_on_the_same_points(references):
    from autoencoder_based_image_compression_amd import container
    for (name, coding_tile) in (('fixed_L10_exception', (4, 4)), ('fixed_L10_exception', (16, 16))):
        ref = reference(references, name, coding_tile)
        for (step, budgets) in ((0, None), (1, None), (3, None), (5, budget_between_the_bounds(ref)), (6, int(ref['upper'][:, 1].max()))):
            thresholds = thresholds_of_step(ref, step)
            (values, expected_blobs, _) = expected_of_step(ref, thresholds, None if budgets is None else numpy.broadcast_to(budgets, (BATCH,)))
            (blobs, info) = container.encode_images_to_quality(ref['images'], ref['encoder'], ref['decoder'], ref['ladder'], max_sse=thresholds,
                                                               budget_bytes=budgets, coding_tile=coding_tile)
            assert [bytes(blob) for blob in blobs] == expected_blobs, step
            for key in ('rate_point', 'first_point', 'met', 'max_sse', 'probe_points', 'probe_sse', 'blob_bytes', 'upper_bound_bytes'):
                assert info[key].dtype == values[key].dtype and numpy.array_equal(info[key], values[key]), (step, key)
    # without the tile the function is what it was: EAE1 blobs, the whole-map bounds
    (plain, info) = container.encode_images_to_quality(ref['images'], ref['encoder'], ref['decoder'], ref['ladder'], max_sse=thresholds_of_step(ref, 0))
    assert all(bytes(blob[:4]) == b'EAE1' for blob in plain) and numpy.array_equal(info['upper_bound_bytes'], ref['whole']['upper'])
    for bad_tile in ((0, 4), (4,), 4):            # (a side beyond the plane is clamped to it, as `encode_images` clamps it)
        with pytest.raises(ValueError):
            container.encode_images_to_quality(ref['images'], ref['encoder'], ref['decoder'], ref['ladder'], max_sse=5, coding_tile=bad_tile)


def test_refusals(references):
    from autoencoder_based_image_compression_amd import codec, ratecontrol
    ref = reference(references, 'fixed_L10_exception', (4, 4))
    ladder = ref['ladder']
    images = torch.from_numpy(ref['images']).cuda()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    arguments = (ref['variables'], False, ladder, BATCH, SHAPE[0], SHAPE[1])
    # `QualityCodec`'s and `BudgetCodec`'s
    with pytest.raises(ValueError, match='not both'):
        codec.TiledQualityCodec(*arguments, (4, 4), target_psnr=30., max_sse=5)
    for (options, error) in (({'fuse_latent': True}, ValueError), ({'coder': 'host'}, ValueError), ({'coder': 'none'}, ValueError),
                             ({'coder_chunks': 2}, ValueError), ({'emit_container': False}, ValueError), ({'max_sse': [1, 2]}, ValueError),
                             ({'budget_bytes': [1, 2]}, ValueError), ({'idx_map_exception': 3}, TypeError)):
        with pytest.raises(error):
            codec.TiledQualityCodec(*arguments, (4, 4), **options)
    with pytest.raises(TypeError, match='RateLadder'):
        codec.TiledQualityCodec(ref['variables'], False, None, BATCH, SHAPE[0], SHAPE[1], (4, 4))
    # `TiledBudgetCodec`'s
    for bad_tile in ((0, 4), (4,), 4, (70000, 4)):
        with pytest.raises(ValueError):
            codec.TiledQualityCodec(*arguments, bad_tile, max_sse=5)
    long_ladder = ratecontrol.RateLadder(numpy.tile(ladder.bin_widths_points[:1], (10, 1)), numpy.tile(ladder.binary_probabilities_points[:1], (10, 1, 1)),
                                         ladder.map_mean)
    with pytest.raises(ValueError, match='ladder_max_points'):
        codec.TiledQualityCodec(ref['variables'], False, long_ladder, BATCH, SHAPE[0], SHAPE[1], (4, 4))
    with pytest.raises(ValueError, match='65535'):                     # 459 images of 143 tiles each
        codec.TiledQualityCodec(ref['variables'], False, ladder, 459, SHAPE[0], SHAPE[1], (1, 1))
    # the whole-map codecs go on refusing the tile, in their own words
    with pytest.raises(ValueError, match='`QualityCodec` does not take `coding_tile`.*run order'):
        codec.QualityCodec(*arguments, max_sse=5, coding_tile=(4, 4))
    with pytest.raises(ValueError, match='`BudgetCodec` does not take `coding_tile`'):
        codec.BudgetCodec(*arguments, coding_tile=(4, 4))
    assert torch.cuda.memory_allocated() == before
    with build(ref, 'launches') as c:
        with pytest.raises(ValueError, match='neither'):
            c.submit(images)
        with pytest.raises(ValueError, match='not both'):
            c.submit(images, target_psnr=30., max_sse=5)
        # the codec still takes a step
        thresholds = thresholds_of_step(ref, 0)
        check_step(ref, c.submit(images, max_sse=thresholds), thresholds, 'after')
