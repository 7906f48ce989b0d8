"""`container.encode_colour_images_to_quality`: one PSNR floor per colour picture, every probe over the real
samples.

The configurations of tests/colour_budget_cases.py, three chroma shares. The reference is the table of tests/colour_quality_cases.py
-- `encode_images(plane, ..., pad=True)` -> `decode_images` -> the squared error in numpy, for every plane, picture and point -- and the
numpy rule applied to it; the thresholds come from the table: 0, 2^62, for every k the sum of the three entries at (k, k, k) and that
sum less 1, per picture. On every call the points, 'plane_met', the plane thresholds, the squared errors and 'met' equal the rule's
element for element; every probe's squared error is the table's at the point probed (on 50 x 83 a probe that counted the coded plane
would miss it); every blob is the assembly of the three `encode_images(..., pad=True)` blobs at those points; `decode_colour_images`
reads it. `target_psnr` is `max_sse_for_psnr` over the picture's 4:2:0 sample count. The refusals come last."""
import numpy
import pytest

import colour_budget_cases as cases
import colour_quality_cases as quality
from test_gpu_frame_container import models  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _guarded_buffers():
    """Poisoned buffers between guard bands for everything device.py / pipeline.py / container.py allocate (tests/guarded.py)."""
    import guarded
    from autoencoder_based_image_compression_amd import container, device, pipeline
    with guarded.guarded((device, pipeline, container), 0xFF):
        yield


def _encode(case, share, **thresholds):
    from autoencoder_based_image_compression_amd import container
    return container.encode_colour_images_to_quality(case.rgb, case.encoder, case.decoder, case.ladder, chroma_ladder=case.chroma_ladder,
                                                     chroma_share=share, **thresholds)


def _check(case, blobs, info, expected):
    from autoencoder_based_image_compression_amd import colour, container
    for key in ('rate_point', 'sse', 'probe_points', 'probe_sse'):
        print(key, info[key].tolist(), 'rule', expected[key].tolist())
        assert info[key].dtype == numpy.int64 and numpy.array_equal(info[key], expected[key]), key
    assert (info['first_point'] == 0).all()
    assert numpy.array_equal(info['plane_met'], expected['met']) and numpy.array_equal(info['plane_max_sse'], expected['max_sse'])
    assert numpy.array_equal(info['max_sse'], expected['picture_max_sse']) and numpy.array_equal(info['picture_sse'], expected['picture_sse'])
    assert info['met'].dtype == numpy.bool_ and numpy.array_equal(info['met'], expected['picture_met'])
    # a probe at the point taken found the squared error the picture has
    taken = info['probe_points'] == info['rate_point'][:, :, None]
    assert numpy.array_equal(info['probe_sse'][taken], numpy.broadcast_to(info['sse'][:, :, None], taken.shape)[taken])
    assert len(blobs) == case.count
    for (i, blob) in enumerate(blobs):
        assert bytes(blob) == bytes(case.picture_blob(i, info['rate_point'][i])), i
        assert len(blob) == info['blob_bytes'][i] == cases.HEADER + info['plane_blob_bytes'][i].sum()
        decoded = container.decode_colour_images(blob, case.decoder)
        (_, *plane_blobs) = container.split_colour_blob(blob)
        merged = colour.merge_420_numpy(*(container.decode_images(b, case.decoder) for b in plane_blobs))
        assert decoded.shape == (1,) + case.size + (3,) and numpy.array_equal(decoded, merged), i


@pytest.mark.parametrize('share', quality.SHARES, ids=['quarter', 'third', 'nine_tenths'])
@pytest.mark.parametrize('config', sorted(cases.CONFIGS))
def test_the_sibling_equals_the_rule_on_the_table(models, config, share):
    case = quality.case_of(models, config)
    sets = case.threshold_sets()
    assert len(sets) == 2 + 2*case.nb_points
    outcomes = quality.assert_the_set_tells(case.table, sets, share)
    for (thresholds, expected) in zip(sets, outcomes):
        (blobs, info) = _encode(case, share, max_sse=thresholds)
        _check(case, blobs, info, expected)
    # at (k, k, k)'s own sum the picture is met by some triple, at 2^62 by the coarsest, at 0 by none
    assert outcomes[1]['rate_point'].tolist() == [[case.nb_points - 1]*3]*case.count and not outcomes[0]['picture_met'].any()


def test_a_target_in_decibels_is_over_the_samples_of_the_420_form(models):
    from autoencoder_based_image_compression_amd import ratecontrol
    config = 'fixed_L10_exception_K3_50x83_N3'
    case = quality.case_of(models, config)
    samples = ratecontrol.colour_nb_samples(*case.size)
    assert samples == 50*83 + 2*25*42
    # a target between the pictures' PSNRs at the middle point and at the last, per picture, and one scalar
    from autoencoder_based_image_compression_amd.kodak.tools import tools as tls
    middle = numpy.array([tls.psnr_from_sse(int(s), samples) for s in case.table[:, :, 1].sum(axis=1)])
    for targets in (middle - 0.01, float(middle.min()) - 3., 99.):
        thresholds = ratecontrol.max_sse_for_psnr(numpy.asarray(targets, dtype=numpy.float64), samples)
        (blobs, info) = _encode(case, 1./3., target_psnr=targets)
        _check(case, blobs, info, quality.rule(case.table, thresholds, 1./3.))
        for (i, met) in enumerate(info['met'].tolist()):
            assert met == bool(tls.psnr_from_sse(int(info['picture_sse'][i]), samples) >= numpy.broadcast_to(targets, (case.count,))[i])


def test_what_is_refused(models):
    from autoencoder_based_image_compression_amd import ratecontrol
    case = quality.case_of(models, 'fixed_L10_exception_K3_50x83_N3')
    ladder = case.ladder
    fewer = ratecontrol.RateLadder(ladder.bin_widths_points[:2], ladder.binary_probabilities_points[:2], ladder.map_mean, 67)
    from autoencoder_based_image_compression_amd import container
    for (more, error, match) in (({}, ValueError, 'one of the two'), ({'target_psnr': 30., 'max_sse': 5}, ValueError, 'one of the two'),
                                 ({'max_sse': [1, 2]}, ValueError, 'per picture'), ({'max_sse': 1.5}, ValueError, 'integer'),
                                 ({'max_sse': -1}, ValueError, '2\\^62'), ({'target_psnr': [30., 31.]}, ValueError, 'per picture'),
                                 ({'max_sse': 5, 'chroma_share': 0.}, ValueError, 'chroma_share'), ({'max_sse': 5, 'chroma_share': 1.}, ValueError, 'chroma_share'),
                                 ({'max_sse': 5, 'chroma_ladder': fewer}, ValueError, 'rate points'), ({'max_sse': 5, 'chroma_ladder': 'coarse'}, TypeError, 'RateLadder')):
        with pytest.raises(error, match=match):
            container.encode_colour_images_to_quality(case.rgb, case.encoder, case.decoder, ladder, **more)
    with pytest.raises(TypeError):
        container.encode_colour_images_to_quality(case.rgb.astype(numpy.int32), case.encoder, case.decoder, ladder, max_sse=5)
    with pytest.raises(ValueError):
        container.encode_colour_images_to_quality(case.rgb[..., :2], case.encoder, case.decoder, ladder, max_sse=5)
