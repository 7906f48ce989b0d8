"""`device.colour_split_420` and `device.colour_merge_420` (csrc/hip/colour.hip) against `colour.py`, exactly.

Every buffer lies between guard bands and starts out as poison (tests/guarded.py), under the two poisons 0xFF and 0x7F: an element
of an output that is never written keeps the poison and fails the comparison, a store outside an output or into the bands around an
input fails `Guard.check`, and outputs that differ between the two poisons mean a load outside an input reached a result. The
sizes: every (h, w) of 1..5 x 1..7 with three pictures -- one and two rows, one and two columns of the last 2 x 2 block, rows of 3 to
21 bytes at every alignment, pictures that start at odd addresses -- and 50 x 83 with two (the chroma planes of a 99 x 165 or
100 x 166 picture; 2,075 chroma samples an image: nine blocks of 256, the last one ragged). A lane owns one chroma sample whatever
the size, so the grids are not capped -- but for the merge that takes the squared error, which gives an image 64 blocks at most
(csrc/hip/colour.hip: MERGE_SSE_BLOCKS_PER_IMAGE; one atomic per block on the image's word): `test_merge_past_the_blocks_per_image_cap`
runs sizes beyond 64 x 256 samples an image, and asserts first that they are."""
import os

import numpy
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F)
SMALL = [(3, h, w) for h in range(1, 6) for w in range(1, 8)]
SHAPES = SMALL + [(2, 50, 83)]
CODED = ((64, 96), (32, 48))         # the planes a codec keeps for 50 x 83 pictures: luminance, chroma


def _dev():
    from autoencoder_based_image_compression_amd import device
    return device


def _colour():
    from autoencoder_based_image_compression_amd import colour
    return colour


def _pictures(shape, seed=0):
    (n, h, w) = shape
    return numpy.random.RandomState(seed + 131*h + w).randint(0, 256, size=(n, h, w, 3)).astype(numpy.uint8)


def _planes(shape, seed=0):
    (n, h, w) = shape
    rng = numpy.random.RandomState(seed + 17*h + w)
    chroma = _colour().chroma_size(h, w)
    return (rng.randint(0, 256, size=(n, h, w)).astype(numpy.uint8), rng.randint(0, 256, size=(n,) + chroma).astype(numpy.uint8),
            rng.randint(0, 256, size=(n,) + chroma).astype(numpy.uint8))


@pytest.fixture(params=POISONS, ids=['ff', '7f'])
def guard(request):
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


def _shifted_upload(guard, x, shift):
    """`x` on the device between bands, its first byte `shift` bytes behind the interior's (4096-aligned) start; the bytes in front
    of it and behind it, inside the interior, are poison like the bands."""
    flat = guard.full((x.size + 8,), guard.poison, dtype=torch.uint8, device='cuda')
    view = flat[shift:shift + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 4 == shift % 4 and view.is_contiguous()
    return view


def _host(tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_split_equals_numpy_at_every_alignment(guard, shape):
    (dev, colour) = (_dev(), _colour())
    rgb = _pictures(shape)
    expected = colour.split_420_numpy(rgb)
    for shift in (0, 1, 2, 3):
        src = _shifted_upload(guard, rgb, shift)
        got = dev.colour_split_420(src)                 # allocated through the guard: poison until the kernel writes it
        assert [tuple(t.shape) for t in got] == [p.shape for p in expected] and all(t.dtype == torch.uint8 for t in got)
        for (name, a, b) in zip('y cb cr'.split(), _host(got), expected):
            assert numpy.array_equal(a, b), (name, shift)
        assert numpy.array_equal(src.cpu().numpy(), rgb)
        guard.check()


@pytest.mark.parametrize('shape', [(3, 1, 1), (3, 3, 5), (3, 5, 7), (2, 50, 83)], ids=lambda s: 'x'.join(map(str, s)))
def test_split_from_a_pinned_source_and_into_given_planes(guard, shape):
    (dev, colour) = (_dev(), _colour())
    rgb = _pictures(shape, seed=1)
    expected = colour.split_420_numpy(rgb)
    pinned = torch.from_numpy(rgb).pin_memory()
    got = dev.colour_split_420(pinned)
    assert all(t.is_cuda for t in got)
    for (a, b) in zip(_host(got), expected):
        assert numpy.array_equal(a, b)
    out = tuple(guard.empty(p.shape, dtype=torch.uint8, device='cuda') for p in expected)
    again = dev.colour_split_420(pinned, out=out)
    assert all(a is b for (a, b) in zip(again, out))
    for (a, b) in zip(_host(out), expected):
        assert numpy.array_equal(a, b)
    guard.check()


def test_split_of_the_extreme_colours(guard):
    """Black, white and the six corners between them, 2 x 2 blocks of each and of their neighbours in the list: chroma 16 and 240
    come out unclamped."""
    (dev, colour) = (_dev(), _colour())
    corners = numpy.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=numpy.uint8)
    row = numpy.repeat(corners, 2, axis=0)                            # 16 pixels: every corner fills the two columns of a block
    rgb = numpy.stack([numpy.broadcast_to(row[None], (5, 16, 3)), numpy.broadcast_to(numpy.roll(row, 1, axis=0)[None], (5, 16, 3))]).copy()
    expected = colour.split_420_numpy(rgb)
    assert expected[1].max() == 240 and expected[2].max() == 240 and expected[1].min() == 16
    for (a, b) in zip(_host(dev.colour_split_420(guard.upload(rgb))), expected):
        assert numpy.array_equal(a, b)


def _in_coded_planes(guard, planes, filling):
    """The three planes as the top-left of coded planes (64 x 96 and 32 x 48) whose padding holds `filling`."""
    out = []
    for (plane, coded) in zip(planes, (CODED[0], CODED[1], CODED[1])):
        whole = numpy.full((plane.shape[0],) + coded, filling, dtype=numpy.uint8)
        whole[:, :plane.shape[1], :plane.shape[2]] = plane
        out.append(guard.upload(whole))
    return out


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_merge_equals_numpy_in_every_mode(guard, shape):
    (dev, colour) = (_dev(), _colour())
    (n, h, w) = shape
    planes = _planes(shape)
    expected = colour.merge_420_numpy(*planes)
    reference = _pictures(shape, seed=2)
    sse = colour.sse_rgb_numpy(reference, expected)
    start = numpy.arange(1, n + 1, dtype=numpy.int64)*(1 << 40) + 12345
    for source in ('dense', 'coded_0', 'coded_255'):
        if source == 'dense':
            on_device = [guard.upload(p) for p in planes]
        else:
            on_device = _in_coded_planes(guard, planes, int(source.split('_')[1]))
            assert on_device[0].shape[1:] == CODED[0] and on_device[1].shape[1:] == CODED[1]
        # the picture only
        (rgb, none) = dev.colour_merge_420(*on_device, (h, w))
        assert none is None and tuple(rgb.shape) == (n, h, w, 3) and numpy.array_equal(rgb.cpu().numpy(), expected), source
        # the error only, added into words that are not zero
        for shift in (0, 1, 3):
            words = guard.upload(start)
            (none, got) = dev.colour_merge_420(*on_device, (h, w), out=False, reference=_shifted_upload(guard, reference, shift), sse=words)
            assert none is None and got is words and numpy.array_equal(words.cpu().numpy(), start + sse), (source, shift)
        # both, the error into fresh words
        (rgb, got) = dev.colour_merge_420(*on_device, (h, w), reference=guard.upload(reference))
        assert numpy.array_equal(rgb.cpu().numpy(), expected) and got.dtype == torch.int64 and numpy.array_equal(got.cpu().numpy(), sse), source
        # the top-left view a codec hands out as its reconstruction
        if source != 'dense':
            views = [t[:, :p.shape[1], :p.shape[2]] for (t, p) in zip(on_device, planes)]
            assert not views[0].is_contiguous()
            assert numpy.array_equal(dev.colour_merge_420(*views, (h, w))[0].cpu().numpy(), expected)
        guard.check()
    # the largest error there is
    if shape == SHAPES[-1]:
        white = colour.merge_420_numpy(numpy.full((n, h, w), 235, numpy.uint8), *(numpy.full((n,) + planes[1].shape[1:], 128, numpy.uint8),)*2)
        assert (white == 255).all()
        (_, got) = dev.colour_merge_420(guard.upload(numpy.full((n, h, w), 235, numpy.uint8)), guard.upload(numpy.full_like(planes[1], 128)),
                                        guard.upload(numpy.full_like(planes[2], 128)), (h, w), out=False,
                                        reference=guard.upload(numpy.zeros((n, h, w, 3), numpy.uint8)))
        assert got.cpu().tolist() == [65025*3*h*w]*n


MERGE_SSE_BLOCKS_PER_IMAGE = 64      # colour.hip: constexpr int MERGE_SSE_BLOCKS_PER_IMAGE = 64


@pytest.mark.parametrize('shape', [(2, 259, 263), (1, 515, 517)], ids=lambda s: 'x'.join(map(str, s)))
def test_merge_past_the_blocks_per_image_cap(guard, shape):
    """With the squared error an image gets 64 blocks of 256 lanes, which loop: 130 x 132 = 17,160 samples send four blocks of each
    image round a second, ragged time; 258 x 259 = 66,822 send every block round four times and some a fifth."""
    (dev, colour) = (_dev(), _colour())
    source = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'autoencoder_based_image_compression_amd', 'csrc', 'hip',
                          'colour.hip')
    with open(source) as f:
        assert 'constexpr int MERGE_SSE_BLOCKS_PER_IMAGE = {0};'.format(MERGE_SSE_BLOCKS_PER_IMAGE) in f.read()
    (n, h, w) = shape
    (hc, wc) = colour.chroma_size(h, w)
    assert hc*wc > MERGE_SSE_BLOCKS_PER_IMAGE*256                       # beyond the cap
    planes = _planes(shape, seed=5)
    expected = colour.merge_420_numpy(*planes)
    reference = _pictures(shape, seed=6)
    sse = colour.sse_rgb_numpy(reference, expected)
    on_device = [guard.upload(p) for p in planes]
    (rgb, got) = dev.colour_merge_420(*on_device, (h, w), reference=guard.upload(reference))
    assert numpy.array_equal(rgb.cpu().numpy(), expected) and numpy.array_equal(got.cpu().numpy(), sse)
    (none, got) = dev.colour_merge_420(*on_device, (h, w), out=False, reference=guard.upload(reference))
    assert none is None and numpy.array_equal(got.cpu().numpy(), sse)
    # and the grids that are not capped, at the same size
    assert numpy.array_equal(dev.colour_merge_420(*on_device, (h, w))[0].cpu().numpy(), expected)
    for (a, b) in zip(_host(dev.colour_split_420(guard.upload(reference))), colour.split_420_numpy(reference)):
        assert numpy.array_equal(a, b)


def test_merge_into_pinned_memory_and_from_the_split(guard):
    """`merge(split(x))` on the device is numpy's, written straight into pinned memory."""
    (dev, colour) = (_dev(), _colour())
    rgb = _pictures((2, 50, 83), seed=3)
    planes = dev.colour_split_420(guard.upload(rgb))
    pinned = torch.full((2, 50, 83, 3), 0x5A, dtype=torch.uint8).pin_memory()
    (out, sse) = dev.colour_merge_420(*planes, (50, 83), out=pinned, reference=guard.upload(rgb))
    torch.cuda.synchronize()
    expected = colour.merge_420_numpy(*colour.split_420_numpy(rgb))
    assert out is pinned and numpy.array_equal(pinned.numpy(), expected)
    assert numpy.array_equal(sse.cpu().numpy(), colour.sse_rgb_numpy(rgb, expected))


def test_both_kernels_refuse_before_any_launch(guard):
    from autoencoder_based_image_compression_amd import _native
    dev = _dev()
    lib = _native.hip()
    (n, h, w, hc, wc) = (2, 5, 7, 3, 4)
    rgb = guard.full((n, h, w, 3), 3, dtype=torch.uint8, device='cuda')
    y = guard.full((n, h, w), 0x5A, dtype=torch.uint8, device='cuda')
    cb = guard.full((n, hc, wc), 0x5A, dtype=torch.uint8, device='cuda')
    cr = guard.full((n, hc, wc), 0x5A, dtype=torch.uint8, device='cuda')
    out = guard.full((n, h, w, 3), 0x5A, dtype=torch.uint8, device='cuda')
    sse = guard.full((n + 1,), 7, dtype=torch.int64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    (r, a, b, c, o, e) = (t.data_ptr() for t in (rgb, y, cb, cr, out, sse))
    bad = -1                                           # EAE_HIP_BAD_ARGUMENT
    for arguments in ((None, a, b, c, n, h, w), (r, None, b, c, n, h, w), (r, a, None, c, n, h, w), (r, a, b, None, n, h, w),
                      (r, a, b, c, 0, h, w), (r, a, b, c, n, 0, w), (r, a, b, c, n, h, -1),
                      (r, a, b, c, 1, 40000, 40000),               # an image of 2^32 bytes or more
                      (r, a, b, c, 1 << 30, 64, 64)):              # more than 2^31 - 1 blocks
        assert lib.eae_hip_colour_split_420(*arguments, stream) == bad, arguments
    for arguments in ((None, b, c, o, r, e, n, h, w, h, w, hc, wc), (a, None, c, o, r, e, n, h, w, h, w, hc, wc),
                      (a, b, None, o, r, e, n, h, w, h, w, hc, wc),
                      (a, b, c, None, None, None, n, h, w, h, w, hc, wc),      # neither a picture nor an error
                      (a, b, c, o, r, None, n, h, w, h, w, hc, wc),            # a reference without words for its error
                      (a, b, c, o, None, e, n, h, w, h, w, hc, wc),            # words without a reference
                      (a, b, c, o, r, e + 4, n, h, w, h, w, hc, wc),           # words that are not 8-byte aligned
                      (a, b, c, o, r, e, 0, h, w, h, w, hc, wc), (a, b, c, o, r, e, n, 0, w, h, w, hc, wc), (a, b, c, o, r, e, n, h, 0, h, w, hc, wc),
                      (a, b, c, o, r, e, n, h, w, h - 1, w, hc, wc), (a, b, c, o, r, e, n, h, w, h, w - 1, hc, wc),      # planes smaller than the picture
                      (a, b, c, o, r, e, n, h, w, h, w, hc - 1, wc), (a, b, c, o, r, e, n, h, w, h, w, hc, wc - 1),
                      (a, b, c, o, r, e, 1, 40000, 40000, 40000, 40000, 20000, 20000),
                      (a, b, c, o, r, e, 1, 64, 64, 70000, 70000, 32, 32),     # a plane of 2^32 bytes or more
                      (a, b, c, o, r, e, 1 << 30, 64, 64, 64, 64, 32, 32)):
        assert lib.eae_hip_colour_merge_420(*arguments, stream) == bad, arguments
    with pytest.raises(dev.HipError):
        dev.colour_split_420(torch.zeros((n, h, w, 3), dtype=torch.uint8))               # host memory that is not pinned
    with pytest.raises(dev.HipError):
        dev.colour_split_420(rgb.int())
    with pytest.raises(dev.HipError):
        dev.colour_split_420(rgb[..., :2].contiguous())
    with pytest.raises(dev.HipError):
        dev.colour_split_420(rgb, out=(y, cb, cr[:, :, :3].contiguous()))
    with pytest.raises(dev.HipError):
        dev.colour_merge_420(y, cb, cr, (h + 1, w))                                       # planes smaller than the picture
    with pytest.raises(dev.HipError):
        dev.colour_merge_420(y, cb[:, :2].contiguous(), cr[:, :2].contiguous(), (h, w))
    with pytest.raises(dev.HipError):
        dev.colour_merge_420(y, cb, cr[:1], (h, w))
    with pytest.raises(dev.HipError):
        dev.colour_merge_420(y, cb, cr, (h, w), out=False)                                # nothing asked for
    with pytest.raises(dev.HipError):
        dev.colour_merge_420(y, cb, cr, (h, w), sse=sse[:n])                              # words without a reference
    with pytest.raises(dev.HipError):
        dev.colour_merge_420(y, cb, cr, (h, w), reference=rgb, sse=sse)                   # one word too many
    with pytest.raises(dev.HipError):
        dev.colour_merge_420(y, cb, cr, (h, w), out=torch.zeros((n, h, w, 3), dtype=torch.uint8))
    with pytest.raises(dev.HipError):
        dev.colour_merge_420(y.transpose(1, 2), cb, cr, (w, h))                           # no top-left view of contiguous planes
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in (y, cb, cr, out)) and bool((sse == 7).all())      # nothing was launched
