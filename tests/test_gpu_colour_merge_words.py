"""`device.colour_merge_420_words` (csrc/hip/colour.hip) against `colour.merge_420_numpy`, exactly, and against
`device.colour_merge_420` of the same planes.

The expected destination is `numpy.concatenate([colour.merge_420_numpy(y, cb, cr).ravel(), zeros(pad)])`, the pad being what the
last 16-byte word holds behind the pictures; every byte behind that word must still be the poison the buffer started with. Every
buffer lies between guard bands (tests/guarded.py) under the two poisons 0xFF and 0x7F, as in tests/test_gpu_colour_kernels.py. The
sizes: every (h, w) of 1..5 x 1..7 with three pictures (a 1 x 1 picture is 3 bytes: one word then holds all three pictures and 7
zero bytes, and every row end and picture end falls inside a word and inside a lane's 16 pixels); (2, 50, 83), whose pictures are
12,450 bytes, so that the second starts mid-word, rows of 83 pixels take the lanes through both of the kernel's paths, and the 4,669
words make seven blocks, the last one ragged; (2, 3, 16) and (1, 2, 32), whose rows are exactly 3 and 6 words. The grid is one block
per 768 words whatever the size: it is neither capped nor persistent, so no size lies "past a cap"."""
import numpy
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F)
SMALL = [(3, h, w) for h in range(1, 6) for w in range(1, 8)]
SHAPES = SMALL + [(2, 50, 83), (2, 3, 16), (1, 2, 32)]
CODED = ((64, 96), (32, 48))         # the planes a decoder keeps for 50 x 83 pictures: luminance, chroma
BAD = -1                             # EAE_HIP_BAD_ARGUMENT


def _dev():
    from autoencoder_based_image_compression_amd import device
    return device


def _colour():
    from autoencoder_based_image_compression_amd import colour
    return colour


def _planes(shape, seed=0):
    (n, h, w) = shape
    rng = numpy.random.RandomState(seed + 17*h + w)
    chroma = _colour().chroma_size(h, w)
    return (rng.randint(0, 256, size=(n, h, w)).astype(numpy.uint8), rng.randint(0, 256, size=(n,) + chroma).astype(numpy.uint8),
            rng.randint(0, 256, size=(n,) + chroma).astype(numpy.uint8))


_EXPECTED = {}


def _expected(shape, seed=0):
    """(the planes, the flat destination: the pictures and the zero pad of the last word), computed once per shape."""
    if (shape, seed) not in _EXPECTED:
        planes = _planes(shape, seed)
        flat = _colour().merge_420_numpy(*planes).ravel()
        _EXPECTED[(shape, seed)] = (planes, numpy.concatenate([flat, numpy.zeros(-flat.size % 16, dtype=numpy.uint8)]))
    return _EXPECTED[(shape, seed)]


@pytest.fixture(params=POISONS, ids=['ff', '7f'])
def guard(request):
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


def _destination(guard, nbytes, pinned):
    """A flat poisoned destination of `nbytes`: between bands on the device, or in pinned memory."""
    if pinned:
        return torch.full((nbytes,), guard.poison, dtype=torch.uint8).pin_memory()
    return guard.full((nbytes,), guard.poison, dtype=torch.uint8, device='cuda')


def _bytes_of(out):
    torch.cuda.synchronize()
    return (out.cpu() if out.is_cuda else out).numpy().reshape(-1)


@pytest.mark.parametrize('pinned', [False, True], ids=['device', 'pinned'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_words_equal_numpy_and_the_old_kernel(guard, shape, pinned):
    """The exact destination, 48 bytes longer than needed: the words behind the last one keep the poison. The planes are not changed,
    and `device.colour_merge_420` gives the same pictures."""
    dev = _dev()
    (n, h, w) = shape
    (planes, expected) = _expected(shape)
    assert expected.size == dev.colour_words_bytes(n, h, w) and expected.size % 16 == 0 and 0 <= expected.size - n*h*w*3 < 16
    on_device = [guard.upload(p) for p in planes]
    out = _destination(guard, expected.size + 48, pinned)
    assert out.data_ptr() % 16 == 0
    assert dev.colour_merge_420_words(*on_device, (h, w), out) is out
    got = _bytes_of(out)
    assert numpy.array_equal(got[:expected.size], expected), numpy.flatnonzero(got[:expected.size] != expected)[:8]
    assert (got[expected.size:] == guard.poison).all()
    (old, _) = dev.colour_merge_420(*on_device, (h, w))
    assert numpy.array_equal(old.cpu().numpy().ravel(), expected[:n*h*w*3])
    for (t, p) in zip(on_device, planes):
        assert numpy.array_equal(t.cpu().numpy(), p)
    guard.check()


@pytest.mark.parametrize('pinned', [False, True], ids=['device', 'pinned'])
def test_the_top_left_of_coded_planes_whatever_their_padding_holds(guard, pinned):
    """50 x 83 pictures as the top-left of coded planes 64 x 96 and 32 x 48, contiguous and as the view a decoder hands out: two
    different fillings of the padding give the same bytes, numpy's."""
    dev = _dev()
    shape = (2, 50, 83)
    (n, h, w) = shape
    (planes, expected) = _expected(shape)
    seen = []
    for filling in (0, 255):
        whole = []
        for (plane, coded) in zip(planes, (CODED[0], CODED[1], CODED[1])):
            padded = numpy.full((n,) + coded, filling, dtype=numpy.uint8)
            padded[:, :plane.shape[1], :plane.shape[2]] = plane
            whole.append(guard.upload(padded))
        views = [t[:, :p.shape[1], :p.shape[2]] for (t, p) in zip(whole, planes)]
        assert not views[0].is_contiguous()
        for given in (whole, views):
            out = _destination(guard, expected.size, pinned)
            dev.colour_merge_420_words(*given, (h, w), out)
            seen.append(_bytes_of(out).copy())
            assert numpy.array_equal(seen[-1], expected)
        assert numpy.array_equal(dev.colour_merge_420(*views, (h, w))[0].cpu().numpy().ravel(), expected[:n*h*w*3])
    assert all(numpy.array_equal(seen[0], other) for other in seen[1:])
    guard.check()


@pytest.mark.parametrize('pinned', [False, True], ids=['device', 'pinned'])
@pytest.mark.parametrize('shape', [(3, 1, 1), (3, 3, 5), (3, 5, 7), (3, 50, 83)], ids=lambda s: 'x'.join(map(str, s)))
def test_two_pictures_into_a_buffer_for_three(guard, shape, pinned):
    """What a decoder's partial step does: n = 2 launched into the [3, h, w, 3] buffer, rounded up to 16 bytes. The two pictures and the
    pad of their last word are written, everything behind that word is still poison."""
    dev = _dev()
    (_, h, w) = shape
    (planes, expected) = _expected((2, h, w), seed=7)
    room = dev.colour_words_bytes(3, h, w)
    out = _destination(guard, room, pinned)
    dev.colour_merge_420_words(*[guard.upload(p) for p in planes], (h, w), out)
    got = _bytes_of(out)
    assert numpy.array_equal(got[:expected.size], expected) and (got[expected.size:] == guard.poison).all()
    guard.check()


def test_a_shaped_destination_over_a_longer_buffer(guard):
    """`out` as [N, h, w, 3] over a buffer that holds the pad of the last word behind it."""
    dev = _dev()
    shape = (3, 5, 7)
    (n, h, w) = shape
    (planes, expected) = _expected(shape)
    for pinned in (False, True):
        flat = _destination(guard, expected.size + 16, pinned)
        shaped = flat[:n*h*w*3].view(n, h, w, 3)
        assert dev.colour_merge_420_words(*[guard.upload(p) for p in planes], (h, w), shaped) is shaped
        got = _bytes_of(flat)
        assert numpy.array_equal(got[:expected.size], expected) and (got[expected.size:] == guard.poison).all()
    guard.check()


def test_refused_before_any_launch(guard):
    from autoencoder_based_image_compression_amd import _native
    dev = _dev()
    lib = _native.hip()
    (n, h, w, hc, wc) = (2, 5, 7, 3, 4)
    y = guard.full((n, h, w), 0x5A, dtype=torch.uint8, device='cuda')
    cb = guard.full((n, hc, wc), 0x5A, dtype=torch.uint8, device='cuda')
    cr = guard.full((n, hc, wc), 0x5A, dtype=torch.uint8, device='cuda')
    need = dev.colour_words_bytes(n, h, w)
    assert need == 224 and n*h*w*3 == 210
    out = guard.full((need + 32,), 0x5A, dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    (a, b, c, o) = (t.data_ptr() for t in (y, cb, cr, out))
    for arguments in ((None, b, c, o, need, n, h, w, h, w, hc, wc), (a, None, c, o, need, n, h, w, h, w, hc, wc),
                      (a, b, None, o, need, n, h, w, h, w, hc, wc), (a, b, c, None, need, n, h, w, h, w, hc, wc),
                      (a, b, c, o + 1, need, n, h, w, h, w, hc, wc), (a, b, c, o + 4, need, n, h, w, h, w, hc, wc),      # misaligned
                      (a, b, c, o + 8, need, n, h, w, h, w, hc, wc),
                      (a, b, c, o, need + 8, n, h, w, h, w, hc, wc), (a, b, c, o, n*h*w*3, n, h, w, h, w, hc, wc),       # no multiple of 16
                      (a, b, c, o, need - 16, n, h, w, h, w, hc, wc), (a, b, c, o, 0, n, h, w, h, w, hc, wc),            # short
                      (a, b, c, o, need, 0, h, w, h, w, hc, wc), (a, b, c, o, need, n, 0, w, h, w, hc, wc), (a, b, c, o, need, n, h, 0, h, w, hc, wc),
                      (a, b, c, o, need, n, h, w, h - 1, w, hc, wc), (a, b, c, o, need, n, h, w, h, w - 1, hc, wc),      # planes smaller than the picture
                      (a, b, c, o, need, n, h, w, h, w, hc - 1, wc), (a, b, c, o, need, n, h, w, h, w, hc, wc - 1),
                      (a, b, c, o, 1 << 40, 1, 40000, 40000, 40000, 40000, 20000, 20000),                                # a picture of 2^32 bytes or more
                      (a, b, c, o, 1 << 40, 1, 64, 64, 70000, 70000, 32, 32),                                            # a plane of 2^32 bytes or more
                      (a, b, c, o, 1 << 40, 1 << 30, 64, 64, 64, 64, 32, 32)):                                           # colour_shape's block count
        assert lib.eae_hip_colour_merge_420_words(*arguments, stream) == BAD, arguments
    assert lib.eae_hip_colour_merge_420_words(a, b, c, o, need + 32, n, h, w, h, w, hc, wc, stream) == 0          # and what is accepted
    torch.cuda.synchronize()
    assert bool((out[need:] == 0x5A).all()) and not bool((out[:need] == 0x5A).all())
    out.fill_(0x5A)
    for bad in (lambda: dev.colour_merge_420_words(y, cb, cr, (h + 1, w), out),                              # planes smaller than the picture
                lambda: dev.colour_merge_420_words(y, cb, cr[:1], (h, w), out),
                lambda: dev.colour_merge_420_words(y.transpose(1, 2), cb, cr, (w, h), out),                  # no top-left view
                lambda: dev.colour_merge_420_words(y, cb, cr, (h, w), out[:need - 16]),                      # short
                lambda: dev.colour_merge_420_words(y, cb, cr, (h, w), out[:need + 8]),                       # no multiple of 16
                lambda: dev.colour_merge_420_words(y, cb, cr, (h, w), out[8:need + 8]),                      # misaligned
                lambda: dev.colour_merge_420_words(y, cb, cr, (h, w), out[:n*h*w*3].view(n, h, w, 3)[:, :, :, :2]),
                lambda: dev.colour_merge_420_words(y, cb, cr, (h, w), out[:n*h*w*3].view(n*h, w, 3)),        # neither flat nor [N, h, w, 3]
                lambda: dev.colour_merge_420_words(y, cb, cr, (h, w), out.int()),
                lambda: dev.colour_merge_420_words(y, cb, cr, (h, w), torch.zeros(need, dtype=torch.uint8))):  # host memory that is not pinned
        with pytest.raises(dev.HipError):
            bad()
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in (y, cb, cr, out))                                            # nothing was launched
