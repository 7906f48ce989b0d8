"""The rule of `codec.ColourQualityCodec` on the host (ratecontrol.py): `colour_nb_samples`,
`colour_chroma_max_sse` and `colour_luma_max_sse` against Python's big integers, where nothing can overflow, at the values where int64
could: M = 0, 1, 2^17 - 1, 2^17 (where the two halves of the product meet) and 2^62, shares whose 16-bit fraction is 1 and 65535;
the refusals; and `max_sse_for_psnr` over a colour picture's sample count, which must flip exactly where `psnr_from_sse` does."""
import numpy
import pytest

from autoencoder_based_image_compression_amd import ratecontrol
from autoencoder_based_image_compression_amd.kodak.tools import tools as tls

THRESHOLDS = (0, 1, (1 << 17) - 1, 1 << 17, (1 << 17) + 1, 123456789, (1 << 61) + 12345, (1 << 62) - 1, 1 << 62)
SHARES = (1./65536., 65535./65536., 1./3., 0.25, 0.5, 0.999)


def test_nb_samples_at_even_and_odd_sides():
    for (h, w) in ((1, 1), (1, 2), (2, 1), (3, 3), (50, 83), (51, 83), (64, 96), (500, 750), (512, 768), (4095, 4097)):
        (hc, wc) = (-(-h//2), -(-w//2))
        assert ratecontrol.colour_nb_samples(h, w) == h*w + 2*hc*wc
    assert ratecontrol.colour_nb_samples(1, 1) == 3 and ratecontrol.colour_nb_samples(50, 83) == 50*83 + 2*25*42
    assert ratecontrol.colour_nb_samples(64, 96)*2 == 3*64*96                  # even sides: half again as many as the pixels
    from autoencoder_based_image_compression_amd import device
    assert device.chroma_size(51, 83) == (26, 42) and ratecontrol.colour_nb_samples(51, 83) == 51*83 + 2*26*42
    for bad in ((0, 5), (5, 0), (-1, 4)):
        with pytest.raises(ValueError):
            ratecontrol.colour_nb_samples(*bad)


@pytest.mark.parametrize('share', SHARES)
def test_chroma_thresholds_are_the_big_integer_product(share):
    q16 = int(round(share*65536))
    assert 1 <= q16 <= 65535
    expected = [(m*q16) >> 17 for m in THRESHOLDS]
    got = ratecontrol.colour_chroma_max_sse(numpy.array(THRESHOLDS, dtype=numpy.int64), share)
    assert got.dtype == numpy.int64 and got.tolist() == expected
    for (m, a) in zip(THRESHOLDS, expected):                                   # a scalar: one picture
        assert ratecontrol.colour_chroma_max_sse(m, share).tolist() == [a]
        assert 2*a <= m                                                        # both chroma planes together never get more than M


def test_the_share_fractions_at_their_ends():
    assert int(round(SHARES[0]*65536)) == 1 and int(round(SHARES[1]*65536)) == 65535
    assert ratecontrol.colour_chroma_max_sse(1 << 17, SHARES[0]).tolist() == [1]
    assert ratecontrol.colour_chroma_max_sse((1 << 17) - 1, SHARES[0]).tolist() == [0]
    assert ratecontrol.colour_chroma_max_sse(1 << 62, SHARES[1]).tolist() == [((1 << 62)*65535) >> 17]


@pytest.mark.parametrize('share', [0., 1., -0.1, 1.5, float('nan'), float('inf'), True, 'a third', None])
def test_a_share_outside_the_open_interval_is_refused(share):
    with pytest.raises(ValueError):
        ratecontrol.colour_chroma_max_sse(1000, share)


@pytest.mark.parametrize('thresholds', [-1, (1 << 62) + 1, 3.5, numpy.zeros((2, 2), dtype=numpy.int64), [1, -2]])
def test_a_threshold_outside_its_range_is_refused(thresholds):
    with pytest.raises(ValueError):
        ratecontrol.colour_chroma_max_sse(thresholds, 0.25)
    with pytest.raises(ValueError):
        ratecontrol.colour_luma_max_sse(thresholds, numpy.zeros(2, dtype=numpy.int64), numpy.zeros(2, dtype=numpy.int64))


def test_luma_thresholds_are_the_big_integer_difference():
    spent = (0, 1, (1 << 17) - 1, 1 << 17, 1 << 61, (1 << 62) - 1, 1 << 62, (1 << 63) - 1)
    rows = [(m, cb, cr) for m in THRESHOLDS for cb in spent for cr in spent]
    (m, cb, cr) = (numpy.array(column, dtype=numpy.int64) for column in zip(*rows))
    got = ratecontrol.colour_luma_max_sse(m, cb, cr)
    assert got.dtype == numpy.int64 and got.tolist() == [max(a - b - c, 0) for (a, b, c) in rows]
    # a scalar threshold for every picture
    assert ratecontrol.colour_luma_max_sse(1000, numpy.array([0, 400, 1000, 700]), numpy.array([0, 600, 1, 200])).tolist() == [1000, 0, 0, 100]
    assert ratecontrol.colour_luma_max_sse(7, numpy.zeros(0, dtype=numpy.int64), numpy.zeros(0, dtype=numpy.int64)).shape == (0,)


def test_luma_refusals():
    ok = numpy.array([1, 2], dtype=numpy.int64)
    for (cb, cr) in ((ok, ok[:1]), (ok.astype(numpy.float64), ok), (ok.reshape(1, 2), ok.reshape(1, 2)), (numpy.array([-1, 2]), ok),
                     (ok, numpy.array([1, 1 << 63], dtype=numpy.uint64))):
        with pytest.raises(ValueError):
            ratecontrol.colour_luma_max_sse(10, cb, cr)
    with pytest.raises(ValueError):
        ratecontrol.colour_luma_max_sse(numpy.array([1, 2, 3]), ok, ok)


def test_the_picture_rule_in_small():
    """Chroma first, the luminance with the rest: what chroma does not spend goes to Y, and three met planes make a met picture.
    The points are worked out by hand: at M = 120 and a third, a = (120 * 21845) >> 17 = 19, so Cb stops at 5 (20 > 19) and Cr at
    18; Y gets 120 - 23 = 97 and takes 90. At 128 and 129 a = 21 lets Cb take 20. At 12 and a half a = 3, chroma spends 1 + 2 and Y's
    finest point, 10, misses 9; at 13 it meets 10."""
    table = numpy.array([[[10, 40, 90, 200], [1, 5, 20, 60], [2, 6, 18, 50]]], dtype=numpy.int64)        # (N, 3, K), finest first
    first = numpy.zeros(1, dtype=numpy.int64)
    for (threshold, share, points) in ((120, 1./3., (2, 1, 2)), (128, 1./3., (2, 2, 2)), (129, 1./3., (2, 2, 2)), (400, 0.5, (3, 3, 3)),
                                       (12, 0.5, (0, 0, 0)), (13, 0.5, (0, 0, 0)), (0, 0.5, (0, 0, 0))):
        a = ratecontrol.colour_chroma_max_sse(threshold, share)
        (k_cb, met_cb, _, _) = ratecontrol.select_by_quality(table[:, 1], first, a)
        (k_cr, met_cr, _, _) = ratecontrol.select_by_quality(table[:, 2], first, a)
        rest = ratecontrol.colour_luma_max_sse(threshold, table[0, 1, k_cb], table[0, 2, k_cr])
        (k_y, met_y, _, _) = ratecontrol.select_by_quality(table[:, 0], first, rest)
        assert (int(k_y[0]), int(k_cb[0]), int(k_cr[0])) == points, (threshold, share)
        total = int(table[0, 0, k_y[0]] + table[0, 1, k_cb[0]] + table[0, 2, k_cr[0]])
        if met_y[0] and met_cb[0] and met_cr[0]:
            assert total <= threshold


@pytest.mark.parametrize('size', [(50, 83), (64, 96), (1, 1), (500, 750)])
@pytest.mark.parametrize('target', [20., 30.5, 34., 41.25, 60.])
def test_max_sse_for_psnr_flips_with_psnr_from_sse(size, target):
    samples = ratecontrol.colour_nb_samples(*size)
    s = int(ratecontrol.max_sse_for_psnr(target, samples))
    assert 0 <= s < ratecontrol.MAX_SSE_SATURATION
    if s > 0:
        assert tls.psnr_from_sse(s, samples) >= target
    assert not tls.psnr_from_sse(s + 1, samples) >= target
