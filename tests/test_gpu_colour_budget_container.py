"""`container.encode_colour_images_to_budget`: one byte budget per colour picture, on the bounds alone.

The configurations of tests/colour_budget_cases.py. No budget is fixed in advance: a first call without a budget to speak of (2^62)
gives every plane's bounds at every point, and the budgets of the calls that follow are built from them inside the test:
  * B = 48 + the bounds of a triple of points the rule is consistent with lands exactly on that triple, every plane promised, and
    B - 1 lands the luminance on its next point (or, from the last point, nowhere: not promised);
  * a budget at which the bytes chroma did not use move Y a point finer than the even split would, asserted against the rule.
On every call: `rate_point`, the plane budgets and the promises equal the numpy rule applied to `info['upper_bound_bytes']`; every
plane blob inside every picture's EAC1 equals `encode_images(plane, ..., pad=True)` at `info['rate_point']` byte for byte (with the
ladder's price where it has one); `decode_colour_images` reads every blob and gives the merge of the three decoded planes; `promised`
implies `fits`. The refusals come last."""
import numpy
import pytest

import colour_budget_cases as cases
from test_gpu_frame_container import models  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

NO_BUDGET = 1 << 62


@pytest.fixture(autouse=True)
def _guarded_buffers():
    """Poisoned buffers between guard bands for everything device.py / pipeline.py / container.py allocate (tests/guarded.py)."""
    import guarded
    from autoencoder_based_image_compression_amd import container, device, pipeline
    with guarded.guarded((device, pipeline, container), 0xFF):
        yield


class _Case(object):
    """One configuration: its pictures, planes, ladders, and `encode_images` of every (plane, picture, point) asked for, once."""

    def __init__(self, models, config):
        from autoencoder_based_image_compression_amd import colour
        (self.learned, _, self.nb_points, self.size, self.count, _, _) = cases.CONFIGS[config]
        (self.ladder, self.chroma_ladder) = cases.ladders_of(models, config)
        self.ladders = (self.ladder,) + (self.chroma_ladder or self.ladder,)*2
        (self.encoder, self.decoder) = (models[self.learned]['encoder'], models[self.learned]['decoder'])
        self.rgb = cases.pictures(config)
        self.planes = colour.split_420_numpy(self.rgb)
        self._blobs = {}

    def plane_blob(self, which, i, k):
        from autoencoder_based_image_compression_amd import container
        if (which, i, k) not in self._blobs:
            ladder = self.ladders[which]
            more = {} if ladder.rdo_lambdas is None else {'rdo_lambda': ladder.rdo_lambdas[k]}
            self._blobs[(which, i, k)] = container.encode_images(self.planes[which][i:i + 1], self.encoder, ladder.bin_widths_points[k], ladder.map_mean,
                                                                 ladder.binary_probabilities_points[k], ladder.idx_map_exception, pad=True, **more)[0]
        return self._blobs[(which, i, k)]

    def encode(self, budgets, share):
        from autoencoder_based_image_compression_amd import container
        return container.encode_colour_images_to_budget(self.rgb, self.encoder, self.ladder, budgets, chroma_ladder=self.chroma_ladder, chroma_share=share)

    def check(self, blobs, info, budgets, share):
        """Everything the module's docstring lists for one call."""
        from autoencoder_based_image_compression_amd import colour, container
        (n, k) = (self.count, self.nb_points)
        budgets = numpy.broadcast_to(numpy.asarray(budgets, dtype=numpy.int64), (n,))
        (upper, valid) = (info['upper_bound_bytes'], info['valid_points'])
        assert upper.shape == (n, 3, k) and upper.dtype == numpy.int64 and valid.shape == (n, 3, k) and valid.all()
        (points, plane_budgets, promised) = cases.rule(upper, valid, budgets, share)
        assert info['rate_point'].dtype == numpy.int64 and numpy.array_equal(info['rate_point'], points)
        assert info['plane_budget_bytes'].dtype == numpy.int64 and numpy.array_equal(info['plane_budget_bytes'], plane_budgets)
        assert numpy.array_equal(info['plane_promised'], promised) and numpy.array_equal(info['promised'], promised.all(axis=1))
        assert numpy.array_equal(info['budget_bytes'], budgets) and info['budget_bytes'].dtype == numpy.int64
        assert len(blobs) == n
        for (i, blob) in enumerate(blobs):
            (header, *plane_blobs) = container.split_colour_blob(blob)
            assert (header['nb_images'], header['image_height'], header['image_width']) == (1,) + self.size
            expected = [self.plane_blob(which, i, int(points[i, which])) for which in range(3)]
            assert plane_blobs == expected, i
            assert len(blob) == cases.HEADER + sum(map(len, expected)) == info['blob_bytes'][i]
            assert info['plane_blob_bytes'][i].tolist() == [len(b) for b in expected]
            assert (numpy.array([len(b) for b in expected]) <= upper[i, numpy.arange(3), points[i]]).all()      # the bounds are bounds
            decoded = container.decode_colour_images(blob, self.decoder)
            merged = colour.merge_420_numpy(*(container.decode_images(b, self.decoder) for b in plane_blobs))
            assert decoded.shape == (1,) + self.size + (3,) and numpy.array_equal(decoded, merged), i
        assert numpy.array_equal(info['fits'], info['blob_bytes'] <= budgets)
        assert not (info['promised'] & ~info['fits']).any()
        return points, promised


def _case(models, config):
    key = ('colour_budget_case', config)
    if key not in models:
        models[key] = _Case(models, config)
    return models[key]


@pytest.mark.parametrize('config', sorted(cases.CONFIGS))
def test_budgets_built_from_the_bounds_land_where_the_rule_puts_them(models, config):
    case = _case(models, config)
    (n, k) = (case.count, case.nb_points)
    # the first call: the bounds; with 2^62 every plane takes its finest point
    (blobs, first) = case.encode(NO_BUDGET, 0.25)
    (points, promised) = case.check(blobs, first, NO_BUDGET, 0.25)
    assert (points == 0).all() and promised.all()
    (upper, valid) = (first['upper_bound_bytes'], first['valid_points'])
    assert (numpy.diff(upper, axis=2) < 0).all()                 # coarser points are cheaper: "the next point" below is k + 1
    exact_calls = 0
    for share in cases.SHARES:
        for shift in range(k):
            built = cases.exact_budgets(upper, valid, share, shift)
            if built is None:
                continue
            (budgets, triples) = built
            # B = 48 + the three bounds: exactly there, every plane promised
            (blobs, info) = case.encode(budgets, share)
            assert numpy.array_equal(info['upper_bound_bytes'], upper)
            (points, promised) = case.check(blobs, info, budgets, share)
            assert points.tolist() == [list(t) for t in triples] and promised.all() and info['promised'].all()
            assert (cases.HEADER + upper[numpy.arange(n)[:, None], numpy.arange(3)[None], points].sum(axis=1) == budgets).all()
            # B - 1: the same chroma points, the luminance on its next point, or not promised on its last
            (blobs, info) = case.encode(budgets - 1, share)
            (under, under_promised) = case.check(blobs, info, budgets - 1, share)
            assert numpy.array_equal(under[:, 1:], points[:, 1:])
            for i in range(n):
                if points[i, 0] + 1 < k:
                    assert under[i, 0] == points[i, 0] + 1 and under_promised[i, 0]
                else:
                    assert under[i, 0] == k - 1 and not under_promised[i, 0] and not info['promised'][i]
            exact_calls += 1
            break                                                # one shift per share is enough: the pictures aim at different points
    assert exact_calls >= 1


@pytest.mark.parametrize('config', sorted(cases.CONFIGS))
def test_what_chroma_leaves_moves_the_luminance_a_point_finer(models, config):
    from autoencoder_based_image_compression_amd import ratecontrol
    case = _case(models, config)
    (_, first) = case.encode(NO_BUDGET, 0.25)
    (upper, valid) = (first['upper_bound_bytes'], first['valid_points'])
    found = [(share, cases.spill_budgets(upper, valid, share)) for share in cases.SHARES]
    found = [(share, budgets) for (share, budgets) in found if budgets is not None]
    assert found
    (share, budgets) = found[0]
    (blobs, info) = case.encode(budgets, share)
    (points, _) = case.check(blobs, info, budgets, share)
    c = ratecontrol.colour_chroma_budgets(budgets, share)
    even = numpy.maximum(budgets - cases.HEADER, 0) - 2*c
    (even_point, _) = ratecontrol.select_by_upper_bound(upper[:, 0], valid[:, 0], even)
    assert (info['plane_budget_bytes'][:, 0] > even).all() and (info['rate_point'][:, 0] < even_point).all()


def test_scalar_budgets_and_too_small_ones(models):
    config = 'fixed_L10_exception_K3_50x83_N3'
    case = _case(models, config)
    for budget in (0, 47, 48, 49):
        (blobs, info) = case.encode(budget, 0.25)
        (points, promised) = case.check(blobs, info, budget, 0.25)
        assert (points == case.nb_points - 1).all() and not promised.any() and not info['fits'].any()


def test_what_is_refused(models):
    from autoencoder_based_image_compression_amd import container, ratecontrol
    case = _case(models, 'fixed_L10_exception_K3_50x83_N3')
    other = ratecontrol.RateLadder(case.ladder.bin_widths_points[:2], case.ladder.binary_probabilities_points[:2], case.ladder.map_mean, 67)
    for (arguments, more, error) in (((case.rgb, case.encoder, case.ladder, 1000), {'chroma_ladder': other}, ValueError),      # another K
                                     ((case.rgb, case.encoder, case.ladder, 1000), {'chroma_share': 0.}, ValueError),
                                     ((case.rgb, case.encoder, case.ladder, 1000), {'chroma_share': 1.}, ValueError),
                                     ((case.rgb, case.encoder, case.ladder, [1000, 2000]), {}, ValueError),             # one budget per picture
                                     ((case.rgb, case.encoder, case.ladder, 'many'), {}, ValueError),
                                     ((case.rgb[..., :2], case.encoder, case.ladder, 1000), {}, ValueError),            # not three channels
                                     ((case.rgb[:0], case.encoder, case.ladder, 1000), {}, ValueError),
                                     ((case.rgb.astype(numpy.int32), case.encoder, case.ladder, 1000), {}, TypeError),
                                     ((case.rgb, case.encoder, None, 1000), {}, TypeError),
                                     ((case.rgb, case.encoder, case.ladder, 1000), {'chroma_ladder': 'coarse'}, TypeError)):
        with pytest.raises(error):
            container.encode_colour_images_to_budget(*arguments, **more)
