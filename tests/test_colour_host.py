"""The rules of colour pictures in numpy (`colour.py`) and the `EAC1` wrapper (`container.py`), on the CPU.

`split_420_numpy` per pixel is the reference's `rgb_to_ycbcr`, held to the committed result of that function
(tests/golden/tools_golden.npz, the fixture tests/test_gpu_surface.py runs the device kernel against); its box mean and the
edge rule of odd sizes, and `merge_420_numpy`, are held to a second statement written as loops over single pixels, on every size
from 1 x 1 to 5 x 7. The header round-trips with stand-in plane blobs made by `assemble_blob`, and every refusal is reached."""
import os
import struct

import numpy
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tools_golden.npz')
SIZES = [(h, w) for h in range(1, 6) for w in range(1, 8)]


@pytest.fixture(scope='module')
def gold():
    with numpy.load(GOLD) as data:
        return {k: data[k] for k in ('rgb_in', 'rgb_out')}


def _colour():
    from autoencoder_based_image_compression_amd import colour
    return colour


def _pictures(n, h, w, seed=0):
    return numpy.random.RandomState(seed + 97*h + w).randint(0, 256, size=(n, h, w, 3)).astype(numpy.uint8)


# ---- the second statement: one pixel at a time -------------------------------------------------------------------------------------

def _split_by_loops(rgb, ycbcr_of):
    (n, h, w, _) = rgb.shape
    (hc, wc) = ((h + 1)//2, (w + 1)//2)
    full = ycbcr_of(rgb)
    (y, cb, cr) = (numpy.zeros((n, h, w), numpy.uint8), numpy.zeros((n, hc, wc), numpy.uint8), numpy.zeros((n, hc, wc), numpy.uint8))
    for k in range(n):
        for r in range(h):
            for c in range(w):
                y[k, r, c] = full[k, r, c, 0]
        for i in range(hc):
            for j in range(wc):
                for (plane, channel) in ((cb, 1), (cr, 2)):
                    total = 0
                    for dy in (0, 1):
                        for dx in (0, 1):
                            total += int(full[k, min(2*i + dy, h - 1), min(2*j + dx, w - 1), channel])
                    plane[k, i, j] = (total + 2)//4
    return (y, cb, cr)


def _merge_by_loops(y, cb, cr):
    (n, h, w) = y.shape
    (hc, wc) = cb.shape[1:]
    out = numpy.zeros((n, h, w, 3), numpy.uint8)

    def clip(x, low, high):
        return max(low, min(high, x))

    for k in range(n):
        for r in range(h):
            for c in range(w):
                (i, j) = (r//2, c//2)
                i2 = clip(i + (1 if r % 2 else -1), 0, hc - 1)
                j2 = clip(j + (1 if c % 2 else -1), 0, wc - 1)
                chroma = []
                for plane in (cb, cr):
                    p = plane[k].astype(int)
                    chroma.append((9*p[i, j] + 3*p[i, j2] + 3*p[i2, j] + p[i2, j2] + 8)//16)
                scaled = 298*(int(y[k, r, c]) - 16)
                (u, v) = (int(chroma[0]) - 128, int(chroma[1]) - 128)
                # Python's // is a floor on negative sums, as the arithmetic shift is
                out[k, r, c] = (clip((scaled + 409*v + 128)//256, 0, 255), clip((scaled - 100*u - 208*v + 128)//256, 0, 255),
                                clip((scaled + 516*u + 128)//256, 0, 255))
    return out


# ---- the rules ---------------------------------------------------------------------------------------------------------------------

def test_the_forward_transform_per_pixel_is_the_reference_function(gold):
    colour = _colour()
    (rgb, expected) = (gold['rgb_in'], gold['rgb_out'])
    assert rgb.dtype == numpy.uint8 and rgb.ndim == 3 and expected.shape == rgb.shape
    assert numpy.array_equal(colour.ycbcr_numpy(rgb), expected)
    (y, cb, cr) = colour.split_420_numpy(rgb[None])
    assert numpy.array_equal(y[0], expected[:, :, 0])
    # every pixel as its own 2 x 2 block: the box mean of four equal values is the value, so the chroma planes are the reference's
    doubled = numpy.repeat(numpy.repeat(rgb, 2, axis=0), 2, axis=1)
    (y2, cb2, cr2) = colour.split_420_numpy(doubled[None])
    assert numpy.array_equal(cb2[0], expected[:, :, 1]) and numpy.array_equal(cr2[0], expected[:, :, 2])
    assert numpy.array_equal(y2[0, ::2, ::2], expected[:, :, 0])
    # the corners of the cube: chroma reaches 16 and 240 and is not clamped to the cast's 235
    blue_and_red = numpy.zeros((2, 2, 2, 3), dtype=numpy.uint8)
    blue_and_red[0, :, :, 2] = 255
    blue_and_red[1, :, :, 0] = 255
    (_, cb_c, cr_c) = colour.split_420_numpy(blue_and_red)
    assert cb_c[0, 0, 0] == 240 and cr_c[1, 0, 0] == 240 and cb_c.min() >= 16 and cr_c.min() >= 16


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '{0}x{1}'.format(*s))
def test_split_and_merge_equal_the_loops(size):
    colour = _colour()
    (h, w) = size
    rgb = _pictures(2, h, w)
    got = colour.split_420_numpy(rgb)
    expected = _split_by_loops(rgb, colour.ycbcr_numpy)
    assert [p.shape for p in got] == [(2, h, w), (2, (h + 1)//2, (w + 1)//2), (2, (h + 1)//2, (w + 1)//2)]
    assert all(p.dtype == numpy.uint8 and p.flags['C_CONTIGUOUS'] for p in got)
    for (a, b) in zip(got, expected):
        assert numpy.array_equal(a, b)
    # the inverse on planes of its own: every value, not only those a forward transform produces
    rng = numpy.random.RandomState(h*11 + w)
    planes = (rng.randint(0, 256, size=(2, h, w)).astype(numpy.uint8),) + tuple(
        rng.randint(0, 256, size=(2,) + colour.chroma_size(h, w)).astype(numpy.uint8) for _ in range(2))
    merged = colour.merge_420_numpy(*planes)
    assert merged.dtype == numpy.uint8 and merged.shape == (2, h, w, 3)
    assert numpy.array_equal(merged, _merge_by_loops(*planes))
    assert numpy.array_equal(colour.merge_420_numpy(*got), _merge_by_loops(*got))


def test_greys_round_trip_within_one_level():
    colour = _colour()
    levels = numpy.arange(256, dtype=numpy.uint8)
    grey = numpy.broadcast_to(levels[None, :, None, None], (1, 256, 7, 3)).copy()
    (y, cb, cr) = colour.split_420_numpy(grey)
    assert (cb == 128).all() and (cr == 128).all()
    back = colour.merge_420_numpy(y, cb, cr)
    assert int(numpy.abs(back.astype(int) - grey.astype(int)).max()) <= 1
    assert (back[..., 0] == back[..., 1]).all() and (back[..., 1] == back[..., 2]).all()


def test_errors_and_psnr():
    colour = _colour()
    rgb = _pictures(3, 4, 5)
    rec = _pictures(3, 4, 5, seed=1)
    sse = colour.sse_rgb_numpy(rgb, rec)
    assert sse.dtype == numpy.int64 and sse.shape == (3,)
    assert sse.tolist() == [sum((int(a) - int(b))**2 for (a, b) in zip(rgb[k].ravel(), rec[k].ravel())) for k in range(3)]
    assert colour.sse_rgb_numpy(rgb, rgb).tolist() == [0, 0, 0]
    psnr = colour.psnr_from_sse(numpy.array([60, 0]), 60)
    assert psnr.dtype == numpy.float64 and psnr[0] == 10.*numpy.log10(255.**2) and numpy.isinf(psnr[1])
    with pytest.raises(TypeError):
        colour.split_420_numpy(rgb.astype(numpy.float32))
    for bad in (rgb[0], rgb[..., :2], rgb[:, :0]):
        with pytest.raises(ValueError):
            colour.split_420_numpy(bad)
    (y, cb, cr) = colour.split_420_numpy(rgb)
    with pytest.raises(ValueError):
        colour.merge_420_numpy(y, cb[:, :1], cr)
    with pytest.raises(ValueError):
        colour.merge_420_numpy(y, cb, cr[:2])
    with pytest.raises(TypeError):
        colour.merge_420_numpy(y.astype(numpy.int32), cb, cr)
    with pytest.raises(ValueError):
        colour.sse_rgb_numpy(rgb, rec[:2])


# ---- EAC1 --------------------------------------------------------------------------------------------------------------------------

def _stand_in(nb_images, image_size, seed, coding_tile=None):
    """An EAE1 / EAT1 blob with the header of `nb_images` planes of `image_size` and streams of made-up bits (nobody decodes them)."""
    from autoencoder_based_image_compression_amd import container
    rng = numpy.random.RandomState(seed)
    (height, width) = container.coded_size(*image_size)
    nb_tiles = 1
    if coding_tile is not None:
        nb_tiles = len(container.coding_tile_grid(height//16, width//16, coding_tile)[0])
    bits = rng.randint(0, 25, size=(nb_images*nb_tiles*128, 2)).astype(numpy.uint32)
    payload = rng.randint(0, 256, size=int(((bits.astype(numpy.int64) + 7)//8).sum())).astype(numpy.uint8).tobytes()
    return container.assemble_blob(False, nb_images, height, width, -1, rng.rand(128).astype(numpy.float32), rng.rand(128).astype(numpy.float32),
                                   rng.uniform(0.1, 0.9, size=(128, 4)), numpy.zeros((0, 4)), bits, payload, coding_tile=coding_tile,
                                   image_size=image_size)[0]


def test_the_header_round_trips():
    from autoencoder_based_image_compression_amd import container
    for (size, coding_tile) in (((99, 165), None), ((100, 166), (2, 3)), ((1, 1), None), ((128, 192), None)):
        chroma = ((size[0] + 1)//2, (size[1] + 1)//2)
        blobs = (_stand_in(3, size, 0, coding_tile), _stand_in(3, chroma, 1, coding_tile), _stand_in(3, chroma, 2))
        blob = container.assemble_colour_blob(size, *blobs)
        assert blob[:4] == b'EAC1' and len(blob) == 48 + sum(map(len, blobs))
        assert struct.unpack_from('<4sHHIIIB3s3Q', blob) == (b'EAC1', 1, 0, 3, size[0], size[1], 1, b'\0\0\0') + tuple(map(len, blobs))
        header = container.read_colour_header(blob)
        assert header == {'nb_images': 3, 'image_height': size[0], 'image_width': size[1], 'subsampling': 1,
                          'plane_bytes': tuple(map(len, blobs)),
                          'plane_offsets': (48, 48 + len(blobs[0]), 48 + len(blobs[0]) + len(blobs[1]))}
        assert container.split_colour_blob(blob) == (header,) + blobs
        assert container.split_colour_blob(bytearray(blob))[1:] == blobs
        # every plane is an ordinary blob with its own crop byte
        for (plane, plane_size) in zip(blobs, (size, chroma, chroma)):
            plane_header = container.read_header(plane)
            assert (plane_header['image_height'], plane_header['image_width']) == plane_size
        # the other readers treat it as any unknown magic
        with pytest.raises(ValueError, match='magic'):
            container.read_header(blob)


def _patched(blob, offset, fmt, value):
    out = bytearray(blob)
    struct.pack_into(fmt, out, offset, value)
    return bytes(out)


def test_every_refusal():
    from autoencoder_based_image_compression_amd import container
    size = (99, 165)
    chroma = (50, 83)
    (y, cb, cr) = (_stand_in(3, size, 0), _stand_in(3, chroma, 1), _stand_in(3, chroma, 2))
    blob = container.assemble_colour_blob(size, y, cb, cr)
    container.split_colour_blob(blob)
    refused = {
        'bad magic': b'EAC2' + blob[4:],
        'a plane magic in front': y,
        'bad version': _patched(blob, 4, '<H', 2),
        'flags': _patched(blob, 6, '<H', 1),
        'no image': _patched(blob, 8, '<I', 0),
        'no row': _patched(blob, 12, '<I', 0),
        'subsampling 0 (4:4:4, reserved)': _patched(blob, 20, '<B', 0),
        'subsampling 2 (4:2:2, reserved)': _patched(blob, 20, '<B', 2),
        'reserved byte': _patched(blob, 22, '<B', 1),
        'a length that overruns': _patched(blob, 24, '<Q', len(y) + 1),
        'a length that overruns by 2^63': _patched(blob, 40, '<Q', 1 << 63),
        'an empty plane': _patched(blob, 32, '<Q', 0),
        'truncated': blob[:-1],
        'trailing bytes': blob + b'\0',
        'truncated header': blob[:47],
        'empty': b'',
    }
    for (what, bad) in refused.items():
        with pytest.raises(ValueError):
            container.read_colour_header(bad)
        with pytest.raises(ValueError):
            container.split_colour_blob(bad)
    # well-formed headers whose planes do not belong together
    inconsistent = {
        'the height of another picture': _patched(blob, 12, '<I', 100),               # chroma 50 x 83 fits, the luminance plane does not
        'the width of another picture': _patched(blob, 16, '<I', 164),
        'another image count': _patched(blob, 8, '<I', 2),
        'lengths that cut the planes elsewhere': _patched(_patched(blob, 24, '<Q', len(y) - 8), 32, '<Q', len(cb) + 8),
    }
    for (what, bad) in inconsistent.items():
        container.read_colour_header(bad)
        with pytest.raises(ValueError):
            container.split_colour_blob(bad)
    for planes in ((y, cb, _stand_in(2, chroma, 2)),            # image counts that differ
                   (_stand_in(2, size, 0), cb, cr),
                   (y, _stand_in(3, (50, 82), 1), cr),            # plane sizes that do not match (h, w)
                   (y, cb, _stand_in(3, (49, 83), 2)),
                   (cb, cb, cr),
                   (y, cb, cr[:-1] + b'')[:2] + (b'EAE1',)):      # not a blob at all
        with pytest.raises(ValueError):
            container.assemble_colour_blob(size, *planes)
    with pytest.raises(ValueError):
        container.assemble_colour_blob((100, 165), y, cb, cr)
    with pytest.raises(ValueError):
        container.assemble_colour_blob((0, 165), y, cb, cr)
    # the plane decoders go on refusing the wrapper
    with pytest.raises(ValueError, match='magic'):
        container.decode_images(blob, type('NoDecoder', (), {'device': 'cpu'})())       # the header is read first
    with pytest.raises(ValueError):
        container.encode_colour_images(numpy.zeros((1, 4, 4), numpy.uint8), None, None, None, None)
    with pytest.raises(TypeError):
        container.encode_colour_images(numpy.zeros((1, 4, 4, 3), numpy.float32), None, None, None, None)
