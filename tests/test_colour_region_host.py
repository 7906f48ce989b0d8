"""The host side of colour crops, numpy only: `colour.chroma_region` contains every chroma sample
`colour.merge_420_numpy` reads for a crop, exhaustively for pictures up to 9 x 9; `colour.merge_420_region_numpy` of crops cut out of
full planes is `merge_420_numpy` of the planes, cut; `codec.ColourRegionSource` on a blob and on a file whose reads are counted; what
`codec.RegionSource(pad=...)` and `codec.plan_region_step(image_size=...)` refuse. The plane blobs are headers packed by
`container._pack_header` from random bit counts in front of random payload bytes (tests/test_region_decoder_host.py)."""
import io

import numpy
import pytest

from autoencoder_based_image_compression_amd import codec, colour, container

(NB_MAPS, LENGTH) = (128, 10)


def _touched(origin, count, size):
    """The chroma indices `merge_420_numpy` reads along one axis for the pixels origin .. origin + count - 1: i and the clamped i2."""
    r = origin + numpy.arange(count)
    i = r >> 1
    i2 = numpy.clip(i + numpy.where(r & 1, 1, -1), 0, size - 1)
    return min(int(i.min()), int(i2.min())), max(int(i.max()), int(i2.max()))


def test_the_chroma_rectangle_contains_every_sample_the_merge_touches():
    """Every h, w in 1..9, every region, every legal origin: the rectangle lies inside the chroma plane, has the size the region and
    the picture alone give, and holds i, the clamped i2, j and the clamped j2 of every pixel of the crop."""
    checked = 0
    for h in range(1, 10):
        for w in range(1, 10):
            (hc, wc) = colour.chroma_size(h, w)
            for rh in range(1, h + 1):
                for rw in range(1, w + 1):
                    size = (min(hc, rh//2 + 3), min(wc, rw//2 + 3))
                    for y0 in range(h - rh + 1):
                        (low_i, high_i) = _touched(y0, rh, hc)
                        for x0 in range(w - rw + 1):
                            ((rch, rcw), (cy0, cx0)) = colour.chroma_region(h, w, (rh, rw), y0, x0)
                            assert (rch, rcw) == size
                            assert cy0 == min(max((y0 >> 1) - 1, 0), hc - rch) and cx0 == min(max((x0 >> 1) - 1, 0), wc - rcw)
                            assert 0 <= cy0 and cy0 + rch <= hc and 0 <= cx0 and cx0 + rcw <= wc
                            (low_j, high_j) = _touched(x0, rw, wc)
                            assert cy0 <= low_i and high_i < cy0 + rch, (h, w, rh, rw, y0, x0)
                            assert cx0 <= low_j and high_j < cx0 + rcw, (h, w, rh, rw, y0, x0)
                            checked += 1
    assert checked > 10000
    for bad in ((0, 1, 0, 0), (1, 0, 0, 0), (3, 3, -1, 0), (3, 3, 0, -1), (3, 3, 7, 0), (3, 3, 0, 7), (10, 3, 0, 0)):
        with pytest.raises(ValueError):
            colour.chroma_region(9, 9, bad[:2], bad[2], bad[3])


def _cut(planes, size, region, origins):
    (h, w) = size
    (y, cb, cr) = planes
    cuts = ([], [], [])
    for (k, (y0, x0)) in enumerate(origins):
        ((rch, rcw), (cy0, cx0)) = colour.chroma_region(h, w, region, y0, x0)
        cuts[0].append(y[k, y0:y0 + region[0], x0:x0 + region[1]])
        cuts[1].append(cb[k, cy0:cy0 + rch, cx0:cx0 + rcw])
        cuts[2].append(cr[k, cy0:cy0 + rch, cx0:cx0 + rcw])
    return tuple(numpy.ascontiguousarray(numpy.stack(cut)) for cut in cuts)


@pytest.mark.parametrize('size', [(1, 1), (2, 2), (5, 7), (8, 6), (37, 53)], ids=lambda s: 'x'.join(map(str, s)))
def test_the_region_merge_is_the_merge_cut(size):
    """Every region and origin of the small pictures, a sample of them for 37 x 53: three crops at three origins at a time."""
    (h, w) = size
    rng = numpy.random.RandomState(h*100 + w)
    (hc, wc) = colour.chroma_size(h, w)
    planes = (rng.randint(0, 256, size=(3, h, w)).astype(numpy.uint8), rng.randint(0, 256, size=(3, hc, wc)).astype(numpy.uint8),
              rng.randint(0, 256, size=(3, hc, wc)).astype(numpy.uint8))
    full = colour.merge_420_numpy(*planes)
    if h*w <= 64:
        regions = [(rh, rw) for rh in range(1, h + 1) for rw in range(1, w + 1)]
    else:
        regions = [(1, 1), (5, 16), (16, 17), (24, 33), (36, 52), (37, 53)]
    for (rh, rw) in regions:
        places = [(y0, x0) for y0 in range(h - rh + 1) for x0 in range(w - rw + 1)]
        if len(places) > 12:
            places = [places[0], places[-1], (h - rh, 0), (0, w - rw)] + [places[k] for k in rng.choice(len(places), 8, replace=False)]
        places += [places[0]]*((-len(places)) % 3)
        for first in range(0, len(places), 3):
            origins = numpy.array(places[first:first + 3], dtype=numpy.int32)
            got = colour.merge_420_region_numpy(*_cut(planes, size, (rh, rw), origins), size, origins)
            assert got.dtype == numpy.uint8 and got.shape == (3, rh, rw, 3)
            for (k, (y0, x0)) in enumerate(origins):
                assert numpy.array_equal(got[k], full[k, y0:y0 + rh, x0:x0 + rw]), (rh, rw, y0, x0)
    (y, cb, cr) = _cut(planes, size, (1, 1), [(0, 0)]*3)
    with pytest.raises(TypeError):
        colour.merge_420_region_numpy(y.astype(numpy.int32), cb, cr, size, [(0, 0)]*3)
    with pytest.raises(ValueError):
        colour.merge_420_region_numpy(y, cb, cr, size, [(0, 0)]*2)
    if hc > 1:
        with pytest.raises(ValueError):
            colour.merge_420_region_numpy(y, cb[:, :-1], cr[:, :-1], size, [(0, 0)]*3)


# ---- sources ---------------------------------------------------------------------------------------------------------------------------

def _plane_blob(seed, nb_images, size, tile, length=LENGTH, eae1=False):
    """A stand-in plane blob of `nb_images` images of the real `size`, coded at its coded size in `tile`: random header arrays, random
    bit counts of a few bytes, random payload bytes."""
    rng = numpy.random.RandomState(seed)
    (height, width) = container.coded_size(*size)
    (h, w) = (height//16, width//16)
    (tiles, _) = container.coding_tile_grid(h, w, (h, w) if eae1 else tile)
    bits = rng.randint(0, 33, size=(nb_images, len(tiles), NB_MAPS, 2)).astype(numpy.uint32)
    payload = rng.randint(0, 256, size=int(((bits.astype(numpy.int64) + 7)//8).sum())).astype(numpy.uint8).tobytes()
    fields = container._fields(False, nb_images, height, width, -1, rng.uniform(0.05, 2., size=NB_MAPS).astype(numpy.float32),
                               rng.normal(size=NB_MAPS).astype(numpy.float32), rng.uniform(0.01, 0.99, size=(NB_MAPS, length)),
                               numpy.zeros((0, length)), None if eae1 else tile, image_size=size)
    return container._pack_header(fields, bits) + payload


def _colour_blob(seed, nb_images, size, tile):
    chroma = colour.chroma_size(*size)
    planes = [_plane_blob(seed + k, nb_images, plane_size, tile) for (k, plane_size) in enumerate((size, chroma, chroma))]
    return container.assemble_colour_blob(size, *planes), planes


class _Counting(io.BytesIO):
    def __init__(self, data):
        super(_Counting, self).__init__(data)
        self.reads = []

    def read(self, count=-1):
        data = super(_Counting, self).read(count)
        self.reads.append((self.tell() - len(data), len(data)))
        return data


SIZE = (70, 100)          # coded 80 x 112, chroma 35 x 50 coded 48 x 64: every plane padded
TILE = (2, 3)


def test_a_colour_source_on_a_blob_and_on_a_file_whose_reads_are_counted():
    (blob, planes) = _colour_blob(5, 2, SIZE, TILE)
    colour_header = container.read_colour_header(blob)
    memory = codec.ColourRegionSource(blob)
    stream = _Counting(blob)
    source = codec.ColourRegionSource(stream)
    # the 48 bytes, then of every plane its fixed header and the rest of its header: nothing of a payload
    expected = [(0, 48)]
    for (offset, plane) in zip(colour_header['plane_offsets'], planes):
        payload_offset = container.read_header(plane)['payload_offset']
        expected += [(offset, container._TILE_HEADER.size), (offset + container._TILE_HEADER.size, payload_offset - container._TILE_HEADER.size)]
    assert stream.reads == expected
    for made in (memory, source):
        assert (made.nb_images, made.image_height, made.image_width) == (2,) + SIZE and made.header == colour_header
        assert len(made.planes) == 3 and all(isinstance(plane, codec.RegionSource) and plane.pad for plane in made.planes)
        assert [(plane.image_height, plane.image_width) for plane in made.planes] == [SIZE, (35, 50), (35, 50)]
        assert [(plane.header['height'], plane.header['width']) for plane in made.planes] == [(80, 112), (48, 64), (48, 64)]
        assert [plane.coding_tile for plane in made.planes] == [TILE]*3
    # a plane's entries come out of its own byte range of the file: adjacent ones in one read, at the plane's offset in the file
    del stream.reads[:]
    entries = [(1, 1), (0, 2), (1, 0)]
    for (k, (offset, plane)) in enumerate(zip(colour_header['plane_offsets'], planes)):
        (in_file, in_memory, alone) = (source.planes[k], memory.planes[k], codec.RegionSource(plane, pad=True))
        assert numpy.array_equal(in_file.starts, alone.starts) and numpy.array_equal(in_file.sizes, alone.sizes)
        chunks = [bytes(chunk) for chunk in in_file.read(entries)]
        assert chunks == [bytes(chunk) for chunk in in_memory.read(entries)] == [bytes(chunk) for chunk in alone.read(entries)]
        assert stream.reads == [(offset + int(alone.starts[0, 2]), int(alone.sizes[0, 2])),
                                (offset + int(alone.starts[1, 0]), int(alone.sizes[1, 0] + alone.sizes[1, 1]))]
        del stream.reads[:]
    # a read never leaves the plane's range
    view = container._FileRange(io.BytesIO(blob), colour_header['plane_offsets'][1], colour_header['plane_bytes'][1])
    assert view.seek(0, 2) == len(planes[1]) == view.tell() and view.read(10) == b''
    assert view.seek(-4, 2) == len(planes[1]) - 4 and view.read(100) == planes[1][-4:] and view.seek(0) == 0 and view.read() == planes[1]
    with pytest.raises(ValueError):
        view.seek(-1)


def test_what_a_colour_source_refuses():
    (blob, planes) = _colour_blob(9, 2, SIZE, TILE)
    for bad in (blob[:-1], blob[:47], b'', planes[0], blob + b'\0'):
        with pytest.raises(ValueError):
            codec.ColourRegionSource(bad)
        with pytest.raises(ValueError):
            codec.ColourRegionSource(io.BytesIO(bad))
    # planes that do not belong to the header: another image count, a chroma plane of the luminance size
    head = container._COLOUR_HEADER
    def assembled(y, cb, cr):
        return head.pack(container.COLOUR_MAGIC, container.COLOUR_VERSION, 0, 2, SIZE[0], SIZE[1], container.SUBSAMPLING_420, b'\0\0\0',
                         len(y), len(cb), len(cr)) + y + cb + cr
    assert codec.ColourRegionSource(assembled(*planes)).nb_images == 2
    with pytest.raises(ValueError, match='images'):
        codec.ColourRegionSource(assembled(planes[0], _plane_blob(20, 1, (35, 50), TILE), planes[2]))
    with pytest.raises(ValueError, match='plane'):
        codec.ColourRegionSource(io.BytesIO(assembled(planes[0], planes[1], planes[0])))


def test_region_source_takes_a_padded_container_only_with_pad():
    padded = _plane_blob(30, 1, SIZE, TILE)
    with pytest.raises(ValueError, match='do not crop to a real size'):          # the refusal and its message stay
        codec.RegionSource(padded)
    with pytest.raises(ValueError, match='do not crop to a real size'):
        codec.RegionSource(padded, pad=False)
    source = codec.RegionSource(padded, pad=True)
    assert source.pad and (source.image_height, source.image_width) == SIZE and (source.h_map, source.w_map) == (5, 7)
    plain = codec.RegionSource(_plane_blob(31, 1, (80, 112), TILE))
    assert not plain.pad and (plain.image_height, plain.image_width) == (80, 112)
    assert codec.RegionSource(_plane_blob(31, 1, (80, 112), TILE), pad=True).pad


def test_plan_region_step_with_a_real_size():
    region = (24, 40)
    (Rs, Cs) = codec.region_window(5, 7, region)
    layout = codec.region_layout(2, 5, 7, TILE, Rs, Cs)
    (_, head_bytes) = codec.region_head_layout(2, layout['n_slots'], LENGTH)

    def plan(requests, image_size):
        (head, payload) = (numpy.full(head_bytes, 0xA5, dtype=numpy.uint8), numpy.full(1 << 16, 0xA5, dtype=numpy.uint8))
        try:
            return codec.plan_region_step(requests, layout, head, payload, payload.size, region, LENGTH, False, image_size=image_size)
        except ValueError:
            assert (head == 0xA5).all() and (payload == 0xA5).all()          # refused before touching any buffer
            raise

    padded = codec.RegionSource(_plane_blob(40, 2, SIZE, TILE), pad=True)
    other = codec.RegionSource(_plane_blob(41, 1, (71, 100), TILE), pad=True)          # the same coded size, another real size
    whole = codec.RegionSource(_plane_blob(42, 1, (80, 112), TILE))
    # the real image is the top-left of the coded plane: the plan of a padded source is that of the same container without its `crop`
    corner = (SIZE[0] - region[0], SIZE[1] - region[1])
    (n, nbytes, slots) = plan([(padded, 1, 0, 0), (padded, 0) + corner], SIZE)
    (_, placed) = codec.place_region(layout, *corner)
    assert n == 2 and len(slots[1]) == len(placed) and nbytes > 0
    with pytest.raises(ValueError, match='leaves the 70 x 100 image'):                 # inside the coded plane, outside the real image
        plan([(padded, 0, corner[0] + 1, 0)], SIZE)
    with pytest.raises(ValueError, match='leaves'):
        plan([(padded, 0, 0, corner[1] + 1)], SIZE)
    with pytest.raises(ValueError, match='71 x 100 pixels, the decoder was built for 70 x 100'):
        plan([(padded, 0, 0, 0), (other, 0, 0, 0)], SIZE)
    with pytest.raises(ValueError, match='80 x 112 pixels, the decoder was built for 70 x 100'):
        plan([(whole, 0, 0, 0)], SIZE)
    # without a real size a padded source is refused, whatever the region, and an unpadded one goes on working to its last pixel
    with pytest.raises(ValueError, match='without `pad`'):
        plan([(padded, 0, 0, 0)], None)
    assert plan([(whole, 0, 80 - region[0], 112 - region[1])], None)[0] == 1
    assert plan([(whole, 0, 80 - region[0], 112 - region[1])], (80, 112))[0] == 1
