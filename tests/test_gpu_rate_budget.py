"""container.encode_images_to_budget against brute force: every image coded at every rate point with `container.encode_images`
(existing code), the first point in ladder order whose blob fits the budget is the one to choose, and the blob returned is that
blob byte for byte. Three 64 x 96 images (24 symbols per map) and one 128 x 192 image on a trained-like model, a ladder of three
multipliers of its bin widths, L = 4 so that symbols reach the Exp-Golomb suffixes, tables from
`stats.compute_binary_probabilities_ladder`."""
import numpy
import pytest
import torch

import model_cases

pytestmark = pytest.mark.gpu

LENGTH = 4
MULTIPLIERS = (1., 2.5, 6.)
EXCEPTION = 5


@pytest.fixture(scope='module')
def case():
    from autoencoder_based_image_compression_amd import container, pipeline, ratecontrol
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats
    v = model_cases.trained_like_variables(0.05, False, seed=11)
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    encoder = pipeline.DeviceEncoder(v, False)
    decoder = pipeline.DeviceDecoder(v, False)
    rng = numpy.random.RandomState(5)
    small = rng.randint(16, 236, size=(3, 64, 96)).astype(numpy.uint8)
    small[2] = (small[2]//8 + 100).astype(numpy.uint8)                      # a flat image: cheaper at every point
    large = rng.randint(16, 236, size=(1, 128, 192)).astype(numpy.uint8)
    bin_widths_points = (numpy.array(MULTIPLIERS, dtype=numpy.float32)[:, None]*v[var.BIN_WIDTHS_NAME][None, :]).astype(numpy.float32)
    y = encoder(torch.from_numpy(small).cuda()).cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y)
    tables = lossless_stats.compute_binary_probabilities_ladder(y, bin_widths_points, map_mean, LENGTH)
    per_point = numpy.stack([lossless_stats.compute_binary_probabilities(y, bin_widths_points[k], map_mean, LENGTH) for k in range(3)])
    out = {'variables': v, 'encoder': encoder, 'decoder': decoder, 'small': small, 'large': large, 'tables': tables, 'per_point': per_point,
           'ladders': {e: ratecontrol.RateLadder(bin_widths_points, tables, map_mean, e) for e in (-1, EXCEPTION)}}

    def brute(images, e):
        return [[container.encode_images(images[i:i + 1], encoder, bin_widths_points[k], map_mean, tables[k], e)[0] for k in range(3)]
                for i in range(images.shape[0])]

    out['brute'] = {('small', -1): brute(small, -1), ('large', -1): brute(large, -1), ('small', EXCEPTION): brute(small, EXCEPTION)}
    return out


def expected_choice(sizes, budget):
    for (k, size) in enumerate(sizes):
        if size <= budget:
            return k, True
    return len(sizes) - 1, False


def test_the_ladder_tables_are_the_tables_of_every_point(case):
    assert case['tables'].shape == (3, 128, LENGTH) and case['tables'].dtype == numpy.float64
    assert numpy.array_equal(case['tables'], case['per_point'])
    assert len({case['tables'][k].tobytes() for k in range(3)}) == 3


@pytest.mark.parametrize('which', ['small', 'large'])
def test_every_budget_gets_the_brute_force_choice(case, which):
    from autoencoder_based_image_compression_amd import container
    images = case[which]
    brute = case['brute'][(which, -1)]
    sizes = numpy.array([[len(b) for b in row] for row in brute])
    print(which, 'sizes', sizes.tolist())
    budgets = [sizes[:, k] - delta for k in range(3) for delta in (0, 1)] + [int(sizes.max()) + 1000, 0]
    for budget in budgets:
        (blobs, info) = container.encode_images_to_budget(images, case['encoder'], case['ladders'][-1], budget)
        print(which, 'budget', numpy.asarray(budget).tolist(), 'rate_point', info['rate_point'].tolist(), 'attempts', info['attempts'].tolist(),
              'lower', info['lower_bytes'].tolist(), 'upper', info['upper_bytes'].tolist())
        assert (info['lower_bytes'] <= sizes).all() and (sizes <= info['upper_bytes']).all()
        assert info['upper_bound_misses'] == 0
        per_image = numpy.broadcast_to(numpy.asarray(budget), (images.shape[0],))
        for i in range(images.shape[0]):
            (k, fits) = expected_choice(sizes[i].tolist(), per_image[i])
            assert (int(info['rate_point'][i]), bool(info['fits'][i])) == (k, fits), (i, per_image[i])
            assert blobs[i] == brute[i][k]
            assert int(info['blob_bytes'][i]) == len(brute[i][k]) and 1 <= int(info['attempts'][i]) <= 3
    # the suffix path ran: at the finest point symbols reach L, and the bypass streams hold more than sign bits
    header = container.read_header(brute[0][0])
    assert int(header['bits'][:, 1].sum()) > 128*(images.shape[1]//16)*(images.shape[2]//16)


def test_the_blobs_decode_like_the_brute_force_blobs(case):
    from autoencoder_based_image_compression_amd import codec, container
    brute = case['brute'][('small', -1)]
    sizes = numpy.array([[len(b) for b in row] for row in brute])
    budget = numpy.array([sizes[0, 0], sizes[1, 1], sizes[2, 2]])            # rate points that differ between the images
    (blobs, info) = container.encode_images_to_budget(case['small'], case['encoder'], case['ladders'][-1], budget)
    assert len(set(info['rate_point'].tolist())) > 1 and info['fits'].all()
    decoded = [container.decode_images(blob, case['decoder']) for blob in blobs]
    for i in range(3):
        assert numpy.array_equal(decoded[i], container.decode_images(brute[i][int(info['rate_point'][i])], case['decoder']))
    # pipelined read-back: one decoder per image size, blobs of mixed rate points in one step
    with codec.BatchDecoder(case['variables'], False, 3, 64, 96, LENGTH) as decoder:
        assert numpy.array_equal(decoder.submit(blobs).result(), numpy.concatenate(decoded))


def test_exception_map_and_tiled_transform_give_the_same_bytes(case):
    from autoencoder_based_image_compression_amd import container
    brute = case['brute'][('small', EXCEPTION)]
    sizes = numpy.array([[len(b) for b in row] for row in brute])
    budget = sizes[:, 1]
    (blobs, info) = container.encode_images_to_budget(case['small'], case['encoder'], case['ladders'][EXCEPTION], budget)
    assert (info['lower_bytes'] <= sizes).all() and (sizes <= info['upper_bytes']).all()
    for i in range(3):
        (k, fits) = expected_choice(sizes[i].tolist(), budget[i])
        assert (int(info['rate_point'][i]), bool(info['fits'][i])) == (k, fits)
        assert blobs[i] == brute[i][k] and container.read_header(blobs[i])['idx_map_exception'] == EXCEPTION
    (tiled, tiled_info) = container.encode_images_to_budget(case['small'], case['encoder'], case['ladders'][EXCEPTION], budget, tile=(2, 2))
    assert tiled == blobs and numpy.array_equal(tiled_info['rate_point'], info['rate_point'])
    plain = case['brute'][('small', -1)]
    (untiled, _) = container.encode_images_to_budget(case['small'], case['encoder'], case['ladders'][-1], int(len(plain[0][1])))
    (tiled, _) = container.encode_images_to_budget(case['small'], case['encoder'], case['ladders'][-1], int(len(plain[0][1])), tile=(2, 2))
    assert tiled == untiled


def test_an_image_no_point_can_hold_raises(case):
    from autoencoder_based_image_compression_amd import container, ratecontrol
    ladder = case['ladders'][-1]
    tiny = ratecontrol.RateLadder(ladder.bin_widths_points*numpy.float32(1e-7), ladder.binary_probabilities_points, ladder.map_mean)
    with pytest.raises(AssertionError, match='16-bit signed integers'):
        container.encode_images_to_budget(case['small'], case['encoder'], tiny, 10**9)
    with pytest.raises(ValueError):
        container.encode_images_to_budget(case['small'], case['encoder'], ladder, [1, 2])
    with pytest.raises(TypeError):
        container.encode_images_to_budget(case['small'], case['encoder'], None, 100)
