"""`device.colour_merge_420_crops` (csrc/hip/colour.hip) against `colour.merge_420_region_numpy`, exactly.

Crops are cut on the host out of random full planes -- the luminance at the crop's pixel origin, the chroma at the rectangle
`colour.chroma_region` names --, the kernel gets the dense crops and the pixel origins only and derives every chroma origin itself:
with random planes a kernel that placed a chroma crop one sample off, took a weight's parity from the crop instead of the picture, or
clamped a neighbour at the crop's edge instead of the plane's, gives other bytes. The expected destination is the crops, flat, and
the zero pad of the last 16-byte word; every byte behind that word must still be the poison the buffer started with. Every buffer lies
between guard bands (tests/guarded.py) under the two poisons 0xFF and 0x7F, for a device and for a pinned destination; the origins are
read from device and from pinned memory.

Pictures 37 x 53 (odd both ways: chroma 19 x 27), 2 x 2 and 64 x 96; regions 1 x 1 (every row end and crop end inside a lane's 16
pixels), 5 x 16 (a row is exactly one lane), 16 x 17 and 24 x 33 (both of the kernel's paths in every row), 35 x 50 of 37 x 53 (the
chroma rectangle is the whole plane) and the whole picture, whose result must be `colour.merge_420_numpy` outright; origins at
(0, 0), odd / odd, odd / even, even / odd and flush against the bottom and right edges, where the neighbours clamp at the real chroma
size; one to three crops, every crop at an origin of its own. Three crops of 40 x 48 are 1080 words, two blocks. The grid is one
block per 768 words whatever the size: neither capped nor persistent."""
import numpy
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F)
BAD = -1                             # EAE_HIP_BAD_ARGUMENT
REGIONS = {(37, 53): [(1, 1), (5, 16), (16, 17), (24, 33), (35, 50), (37, 53)],
           (2, 2): [(1, 1), (1, 2), (2, 1), (2, 2)],
           (64, 96): [(1, 1), (5, 16), (16, 17), (24, 33), (40, 48), (64, 96)]}
CASES = [(size, region, n) for size in sorted(REGIONS) for region in REGIONS[size] for n in (1, 2, 3)]


def _dev():
    from autoencoder_based_image_compression_amd import device
    return device


def _colour():
    from autoencoder_based_image_compression_amd import colour
    return colour


def _origins(size, region, n):
    """One crop: flush against the bottom and right edges. Two: (0, 0) and odd / odd. Three: odd / even, even / odd and flush against
    both edges again. Where the picture leaves less room the origins that fit take their places, in order."""
    ((h, w), (rh, rw)) = (size, region)
    (last_y, last_x) = (h - rh, w - rw)
    flush = (last_y, last_x)
    wanted = [(0, 0), (min(5, last_y) | 1, min(7, last_x) | 1), (min(3, last_y) | 1, min(10, last_x) & ~1), (min(8, last_y) & ~1, min(9, last_x) | 1)]
    fitting = []
    for (y0, x0) in wanted + [(last_y, 0), (0, last_x)]:
        if 0 <= y0 <= last_y and 0 <= x0 <= last_x and (y0, x0) not in fitting:
            fitting.append((y0, x0))
    picked = {1: [flush], 2: [fitting[0], fitting[1 % len(fitting)]], 3: [fitting[2 % len(fitting)], fitting[3 % len(fitting)], flush]}[n]
    return numpy.array(picked, dtype=numpy.int32)


_EXPECTED = {}


def _expected(size, region, n):
    """(the crops of the three planes, the origins, the flat destination: the crops and the zero pad of the last word), once a case."""
    key = (size, region, n)
    if key not in _EXPECTED:
        colour = _colour()
        (h, w) = size
        rng = numpy.random.RandomState(1000*h + 10*region[0] + region[1] + n)
        chroma = colour.chroma_size(h, w)
        (y, cb, cr) = (rng.randint(0, 256, size=(n,) + size).astype(numpy.uint8), rng.randint(0, 256, size=(n,) + chroma).astype(numpy.uint8),
                       rng.randint(0, 256, size=(n,) + chroma).astype(numpy.uint8))
        origins = _origins(size, region, n)
        cuts = ([], [], [])
        for (k, (y0, x0)) in enumerate(origins):
            ((rch, rcw), (cy0, cx0)) = colour.chroma_region(h, w, region, int(y0), int(x0))
            cuts[0].append(y[k, y0:y0 + region[0], x0:x0 + region[1]])
            cuts[1].append(cb[k, cy0:cy0 + rch, cx0:cx0 + rcw])
            cuts[2].append(cr[k, cy0:cy0 + rch, cx0:cx0 + rcw])
        crops = tuple(numpy.ascontiguousarray(numpy.stack(cut)) for cut in cuts)
        merged = colour.merge_420_region_numpy(*crops, size, origins)
        full = colour.merge_420_numpy(y, cb, cr)
        for (k, (y0, x0)) in enumerate(origins):
            assert numpy.array_equal(merged[k], full[k, y0:y0 + region[0], x0:x0 + region[1]])
        if region == size:
            assert numpy.array_equal(merged, full)       # the whole picture: `merge_420_numpy` outright
        flat = merged.ravel()
        _EXPECTED[key] = (crops, origins, numpy.concatenate([flat, numpy.zeros(-flat.size % 16, dtype=numpy.uint8)]))
    return _EXPECTED[key]


@pytest.fixture(params=POISONS, ids=['ff', '7f'])
def guard(request):
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


def _destination(guard, nbytes, pinned):
    if pinned:
        return torch.full((nbytes,), guard.poison, dtype=torch.uint8).pin_memory()
    return guard.full((nbytes,), guard.poison, dtype=torch.uint8, device='cuda')


def _origins_tensor(guard, origins, pinned):
    return torch.from_numpy(origins.copy()).pin_memory() if pinned else guard.upload(origins)


def _bytes_of(out):
    torch.cuda.synchronize()
    return (out.cpu() if out.is_cuda else out).numpy().reshape(-1)


def test_the_cases_cover_what_they_claim():
    colour = _colour()
    dev = _dev()
    assert colour.chroma_size(37, 53) == (19, 27)
    assert dev.chroma_region_size((37, 53), (35, 50)) == (19, 27) and dev.chroma_region_size((37, 53), (24, 33)) == (15, 19)
    assert dev.chroma_region_size((2, 2), (1, 1)) == (1, 1) and dev.chroma_region_size((64, 96), (5, 16)) == (5, 11)
    for (size, region, n) in CASES:
        origins = _origins(size, region, n)
        assert origins.shape == (n, 2) and (origins >= 0).all() and (origins + region <= size).all()
        assert n == 2 or (origins[-1] == (size[0] - region[0], size[1] - region[1])).all()          # flush against both edges
        for (y0, x0) in origins:
            assert colour.chroma_region(size[0], size[1], region, int(y0), int(x0))[0] == dev.chroma_region_size(size, region)
    seen = numpy.concatenate([_origins((37, 53), (16, 17), n) for n in (1, 2, 3)])
    assert {(int(y) & 1, int(x) & 1) for (y, x) in seen} == {(0, 0), (1, 1), (1, 0), (0, 1)}
    assert len({tuple(o) for o in _origins((64, 96), (24, 33), 3)}) == 3                            # an origin of its own per crop
    assert -(-3*3*40*48//16) == 1080 > 768                                                         # two blocks
    assert any((3*n*region[0]*region[1]) % 16 for (_, region, n) in CASES)                         # a last word with a pad


@pytest.mark.parametrize('pinned', [False, True], ids=['device', 'pinned'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: '{0}x{1}_{2}x{3}_n{4}'.format(*(c[0] + c[1] + (c[2],))))
def test_crops_equal_numpy(guard, case, pinned):
    """The exact destination, 48 bytes longer than needed: the words behind the last one keep the poison. Neither the planes nor
    the origins are changed. A pinned destination comes with pinned origins."""
    dev = _dev()
    (size, region, n) = case
    (crops, origins, expected) = _expected(size, region, n)
    assert expected.size == dev.colour_words_bytes(n, *region) and 0 <= expected.size - 3*n*region[0]*region[1] < 16
    on_device = [guard.upload(p) for p in crops]
    where = _origins_tensor(guard, origins, pinned)
    out = _destination(guard, expected.size + 48, pinned)
    assert out.data_ptr() % 16 == 0
    assert dev.colour_merge_420_crops(*on_device, size, where, out) is out
    got = _bytes_of(out)
    assert numpy.array_equal(got[:expected.size], expected), numpy.flatnonzero(got[:expected.size] != expected)[:8]
    assert (got[expected.size:] == guard.poison).all()
    for (t, p) in zip(on_device + [where], crops + (origins,)):
        assert numpy.array_equal(t.cpu().numpy(), p)
    guard.check()


def test_the_whole_picture_at_the_origin_is_the_words_kernel(guard):
    """Region = picture: the sibling kernel on the same planes writes the same bytes."""
    dev = _dev()
    for size in ((37, 53), (2, 2)):
        (crops, origins, expected) = _expected(size, size, 3)
        assert not origins.any()
        on_device = [guard.upload(p) for p in crops]
        (out, old) = (_destination(guard, expected.size, False), _destination(guard, expected.size, False))
        dev.colour_merge_420_crops(*on_device, size, guard.upload(origins), out)
        dev.colour_merge_420_words(*on_device, size, old)
        assert numpy.array_equal(_bytes_of(out), expected) and numpy.array_equal(_bytes_of(old), expected)
    guard.check()


@pytest.mark.parametrize('pinned', [False, True], ids=['device', 'pinned'])
def test_two_crops_into_a_buffer_for_three_and_a_shaped_destination(guard, pinned):
    """What a decoder's partial step does: n = 2 launched into the buffer of three, with the first two rows of an origins block of
    three. The two crops and the pad of their last word are written, everything behind is still poison. Then `out` as
    [N, rh, rw, 3] over a buffer that holds the pad of the last word behind it."""
    dev = _dev()
    (size, region) = ((37, 53), (35, 50))
    (crops, origins, expected) = _expected(size, region, 2)
    block = numpy.full((3, 2), 10**6, dtype=numpy.int32)          # the third row is not the kernel's to read
    block[:2] = origins
    where = _origins_tensor(guard, block, pinned)
    out = _destination(guard, dev.colour_words_bytes(3, *region), pinned)
    dev.colour_merge_420_crops(*[guard.upload(p) for p in crops], size, where[:2], out)
    got = _bytes_of(out)
    assert expected.size % 16 == 0 and 2*3*region[0]*region[1] % 16 != 0
    assert numpy.array_equal(got[:expected.size], expected) and (got[expected.size:] == guard.poison).all()
    flat = _destination(guard, expected.size + 16, pinned)
    shaped = flat[:2*region[0]*region[1]*3].view(2, region[0], region[1], 3)
    assert dev.colour_merge_420_crops(*[guard.upload(p) for p in crops], size, where[:2], shaped) is shaped
    got = _bytes_of(flat)
    assert numpy.array_equal(got[:expected.size], expected) and (got[expected.size:] == guard.poison).all()
    guard.check()


def test_refused_before_any_launch(guard):
    from autoencoder_based_image_compression_amd import _native
    dev = _dev()
    lib = _native.hip()
    (n, h, w, rh, rw) = (2, 37, 53, 5, 16)
    (rch, rcw) = dev.chroma_region_size((h, w), (rh, rw))
    assert (rch, rcw) == (5, 11)
    y = guard.full((n, rh, rw), 0x5A, dtype=torch.uint8, device='cuda')
    cb = guard.full((n, rch, rcw), 0x5A, dtype=torch.uint8, device='cuda')
    cr = guard.full((n, rch, rcw), 0x5A, dtype=torch.uint8, device='cuda')
    origins = guard.zeros((n, 2), dtype=torch.int32, device='cuda')
    need = dev.colour_words_bytes(n, rh, rw)
    assert need == 480
    out = guard.full((need + 32,), 0x5A, dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    (a, b, c, g, o) = (t.data_ptr() for t in (y, cb, cr, origins, out))
    good = (a, b, c, g, o, need, n, h, w, rh, rw, rch, rcw)

    def but(**changed):
        names = ('y', 'cb', 'cr', 'origins', 'dst', 'dst_bytes', 'n', 'h', 'w', 'rh', 'rw', 'rch', 'rcw')
        return tuple(changed.get(name, value) for (name, value) in zip(names, good))

    for arguments in (but(y=None), but(cb=None), but(cr=None), but(origins=None), but(dst=None),                  # null pointers
                      but(dst=o + 1), but(dst=o + 4), but(dst=o + 8), but(origins=g + 2),                         # misaligned
                      but(dst_bytes=need + 8), but(dst_bytes=n*rh*rw*3 + 1), but(dst_bytes=need - 16), but(dst_bytes=0),      # ragged, short
                      but(n=0), but(h=0), but(w=0), but(rh=0), but(rw=0), but(n=-1),
                      but(rh=h + 1, rch=19), but(rw=w + 1, rcw=27), but(h=4, rch=2), but(w=15, rcw=8),            # a region larger than the picture
                      but(rch=rch - 1), but(rch=rch + 1), but(rcw=rcw - 1), but(rcw=rcw + 1), but(rch=0), but(rch=19, rcw=27),      # not chroma_region's
                      but(h=6, rch=5), but(w=18, rcw=11),                                                         # (3 and 9 are: the plane is smaller)
                      but(h=40000, w=40000),                                                                      # a picture of 2^32 bytes or more
                      but(dst_bytes=1 << 62, n=1 << 30, h=1 << 14, w=1 << 14, rh=1 << 14, rw=1 << 14, rch=(1 << 13), rcw=(1 << 13))):      # blocks
        assert lib.eae_hip_colour_merge_420_crops(*arguments, stream) == BAD, arguments
    assert lib.eae_hip_colour_merge_420_crops(*but(dst_bytes=need + 32), stream) == 0                             # and what is accepted
    torch.cuda.synchronize()
    assert bool((out[need:] == 0x5A).all()) and not bool((out[:need] == 0x5A).all())
    out.fill_(0x5A)
    for bad in (lambda: dev.colour_merge_420_crops(y, cb, cr, (rh - 1, w), origins, out),                  # crops larger than the picture
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, rw - 1), origins, out),
                lambda: dev.colour_merge_420_crops(y, cb[:, :4], cr[:, :4], (h, w), origins, out),          # not chroma_region's size
                lambda: dev.colour_merge_420_crops(y, cb, cr[:1], (h, w), origins, out),
                lambda: dev.colour_merge_420_crops(y.transpose(1, 2), cb, cr, (h, w), origins, out),        # not dense
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, w), origins[:1], out),                    # an origin per crop
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, w), origins.long(), out),
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, w), origins.t(), out),
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, w), torch.zeros((n, 2), dtype=torch.int32), out),      # host memory that is not pinned
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, w), origins, out[:need - 16]),            # short
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, w), origins, out[:need + 8]),             # no multiple of 16
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, w), origins, out[8:need + 8]),            # misaligned
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, w), origins, out[:n*rh*rw*3].view(n*rh, rw, 3)),
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, w), origins, out.int()),
                lambda: dev.colour_merge_420_crops(y, cb, cr, (h, w), origins, torch.zeros(need, dtype=torch.uint8))):
        with pytest.raises(dev.HipError):
            bad()
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in (y, cb, cr, out)) and not bool(origins.any())              # nothing was launched
