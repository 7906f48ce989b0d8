"""The window plan of the tiled encode / decode (pipeline.tile_plan) and the argument checks of its two kernels: pure host logic,
no device needed (the C-ABI checks return before anything is launched)."""
import ctypes
import itertools

import numpy
import pytest

from autoencoder_based_image_compression_amd import _native
from autoencoder_based_image_compression_amd import pipeline

HALOS = {'encoder': pipeline.ENCODER_HALO, 'decoder': pipeline.DECODER_HALO}
SIZES = (1, 2, 3, 4, 5, 7, 16, 17, 25, 40)
TILES = (1, 2, 3, 4, 6, 8, 13, 32, 61)


def exact_zone(start, window, size, before, after):
    """Latents of a window [start, start + window) of an axis of `size` latents whose values equal the untiled ones: all but the
    halo on the sides that lie inside the image."""
    return (start + (before if start > 0 else 0), start + window - (after if start + window < size else 0))


def plan_violations(n, h, w, tile, before, after, true_before, true_after):
    """Checks one plan built with (before, after) against the zones of the true halo; returns the list of what is wrong."""
    (plan, (wh, ww)) = pipeline.tile_plan(n, h, w, tile, before, after)
    problems = []
    assert plan.dtype == numpy.int32 and plan.ndim == 2 and plan.shape[1] == 9
    cover = numpy.zeros((n, h, w), dtype=numpy.int64)
    for (img, wr, wc, ir, ic, orow, ocol, er, ec) in plan.tolist():
        if not (0 <= img < n and 0 <= wr and wr + wh <= h and 0 <= wc and wc + ww <= w):
            problems.append(('window outside the image', img, wr, wc))
        if not (0 <= ir and ir + er <= wh and 0 <= ic and ic + ec <= ww and er >= 1 and ec >= 1):
            problems.append(('interior outside its window', ir, ic, er, ec))
        if (orow, ocol) != (wr + ir, wc + ic):
            problems.append(('interior origins disagree', orow, ocol))
        (zr0, zr1) = exact_zone(wr, wh, h, true_before, true_after)
        (zc0, zc1) = exact_zone(wc, ww, w, true_before, true_after)
        if not (zr0 <= orow and orow + er <= zr1 and zc0 <= ocol and ocol + ec <= zc1):
            problems.append(('interior outside the exact zone', orow, ocol, er, ec))
        cover[img, orow:orow + er, ocol:ocol + ec] += 1
    if not (cover == 1).all():
        problems.append(('latents not covered exactly once', int((cover != 1).sum())))
    return problems


@pytest.mark.parametrize('side', sorted(HALOS))
def test_the_plan_covers_every_latent_once_with_exact_interiors(side):
    """Every latent of every image lies in exactly one interior; every window has the same shape min(T + 3, size) and lies inside its
    image; every interior lies inside its window's exact zone. Tiles of 1, tiles larger than the image, remainders."""
    (before, after) = HALOS[side]
    assert before + after == 3
    for (h, w, th, tw) in itertools.product(SIZES, SIZES, TILES, (1, 5, 61)):
        (plan, (wh, ww)) = pipeline.tile_plan(2, h, w, (th, tw), before, after)
        assert (wh, ww) == (min(th + 3, h), min(tw + 3, w))
        assert plan.shape[0] == 2*(-(-h//th))*(-(-w//tw))
        assert plan_violations(2, h, w, (th, tw), before, after, before, after) == [], (h, w, th, tw)


@pytest.mark.parametrize('side', sorted(HALOS))
def test_an_undersized_halo_is_caught(side):
    """A plan built with one latent less of halo on either side still covers the images, but puts interiors where the windows'
    values differ from the untiled ones: the exact-zone check sees it."""
    (before, after) = HALOS[side]
    for (b, a) in ((before - 1, after), (before, after - 1)):
        problems = plan_violations(1, 17, 25, (4, 6), b, a, before, after)
        assert problems and all(p[0] == 'interior outside the exact zone' for p in problems), (b, a)


def test_a_single_window_is_the_whole_image():
    (plan, shape) = pipeline.tile_plan(3, 5, 7, (8, 8), 2, 1)
    assert shape == (5, 7)
    assert plan.tolist() == [[i, 0, 0, 0, 0, 0, 0, 5, 7] for i in range(3)]


@pytest.mark.parametrize('tile, per_launch', [((0, 4), 16), ((4,), 16), (4, 16), ((4, -1), 16), ((4.0, 4), 16), ((True, 4), 16),
                                              ((4, 4), 0), ((4, 4), 1.5), ('ab', 16)])
def test_invalid_tile_arguments_raise_value_error(tile, per_launch):
    with pytest.raises(ValueError):
        pipeline._tile_arguments(tile, per_launch)
    assert pipeline._tile_arguments((3, 2), 1) == ((3, 2), 1)


class _Buffers(object):
    """Host stand-ins for device pointers: the checks must reject the arguments before any launch, so nothing reads them."""

    def __init__(self):
        self.mem = (ctypes.c_uint8*4096)()
        base = ctypes.addressof(self.mem)
        self.aligned = ctypes.c_void_p((base + 15)//16*16)
        self.misaligned = ctypes.c_void_p((base + 15)//16*16 + 4)

    @staticmethod
    def plan(rows):
        plan = numpy.ascontiguousarray(rows, dtype=numpy.int32).reshape(-1, 9)
        return plan, ctypes.c_void_p(plan.ctypes.data)


def test_tile_copy_argument_checks_return_before_any_launch():
    """include/eae_hip.h, eae_hip_tile_copy: NULL -> -1, bad shape / misaligned rows / a plan outside the plane -> -2. A plane of
    16 x 16 latents, windows of 6 x 7."""
    lib = _native.hip()
    b = _Buffers()
    p = b.aligned
    (_, good_p) = b.plan([0, 10, 9, 2, 1, 12, 10, 3, 4])

    def copy(plane=p, n=1, h=16, w=16, windows=p, wh=6, ww=7, unit=1, elem=512, plan=p, host=None, count=1, to_windows=1):
        return lib.eae_hip_tile_copy(plane, n, h, w, windows, wh, ww, unit, elem, plan, good_p if host is None else host, count,
                                     to_windows, None)
    # NULL pointers and non-positive sizes
    assert copy(plane=None) == -1 and copy(windows=None) == -1 and copy(plan=None) == -1
    assert lib.eae_hip_tile_copy(p, 1, 16, 16, p, 6, 7, 1, 512, p, None, 1, 1, None) == -1
    assert copy(n=0) == -1 and copy(h=0) == -1 and copy(wh=-1) == -1 and copy(unit=0) == -1 and copy(elem=0) == -1 and copy(count=-1) == -1
    # rows that are not whole 16-byte chunks, misaligned bases, windows larger than the plane
    assert copy(unit=1, elem=8) == -2 and copy(unit=4, elem=3) == -2
    assert copy(plane=b.misaligned) == -2 and copy(windows=b.misaligned) == -2
    assert copy(wh=17) == -2 and copy(ww=17) == -2
    # plan rows outside the plane / the window, or whose interior origins disagree
    for row in ([1, 10, 9, 2, 1, 12, 10, 3, 4],        # image 1 of 1
                [0, 11, 9, 2, 1, 13, 10, 3, 4],        # window rows 11..16 of 16
                [0, 10, 10, 2, 1, 12, 11, 3, 4],       # window cols 10..16
                [0, -1, 9, 2, 1, 1, 10, 3, 4],
                [0, 10, 9, 4, 1, 14, 10, 3, 4],        # interior rows 4..6 of a 6-row window
                [0, 10, 9, 2, 4, 12, 13, 3, 4],        # interior cols 4..7 of 7
                [0, 10, 9, 2, 1, 12, 10, -1, 4],
                [0, 10, 9, 2, 1, 11, 10, 3, 4]):       # interior at 11 in the image but 10 + 2 = 12 by the window
        (_, bad_p) = b.plan(row)
        assert copy(host=bad_p) == -2, row
        assert copy(host=bad_p, to_windows=0) == -2, row
    # one bad row among good ones
    (_, mixed_p) = b.plan([[0, 10, 9, 2, 1, 12, 10, 3, 4], [0, 0, 0, 0, 0, 0, 0, 7, 1]])
    assert copy(host=mixed_p, count=2) == -2
    # the plane side has no size limit: a 2^31-byte plane passes the checks (nothing is launched: no windows)
    assert copy(h=2048, w=2048, count=0) == 0


def test_tile_stitch_argument_checks_return_before_any_launch():
    lib = _native.hip()
    b = _Buffers()
    p = b.aligned
    (_, good_p) = b.plan([0, 10, 9, 2, 1, 12, 10, 3, 4])

    def stitch(windows=p, wh=6, ww=7, image=p, ref=p, sse=p, n=1, h=16, w=16, plan=p, host=None, count=1):
        return lib.eae_hip_tile_stitch_u8(windows, wh, ww, image, ref, sse, n, h, w, plan, good_p if host is None else host, count, None)
    assert stitch(image=None, ref=None) == -1          # neither output nor reference
    assert stitch(sse=None) == -1                      # a reference without its accumulator
    assert stitch(windows=None) == -1 and stitch(plan=None) == -1 and stitch(n=0) == -1
    assert stitch(image=b.misaligned) == -2 and stitch(ref=b.misaligned) == -2 and stitch(windows=b.misaligned) == -2
    assert stitch(image=None, ref=b.misaligned) == -2
    assert stitch(wh=17) == -2
    (_, bad_p) = b.plan([0, 11, 9, 2, 1, 13, 10, 3, 4])
    assert stitch(host=bad_p) == -2 and stitch(image=None, host=bad_p) == -2
    assert stitch(count=0) == 0
