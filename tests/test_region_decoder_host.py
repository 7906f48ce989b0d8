"""The host side of `codec.RegionDecoder`, numpy only: `region_window` / `region_origin` / `region_layout` /
`place_region` against `container.region_plan` at EVERY position of a crop; `plan_region_step`'s head and payload against the
sources' own headers; every step it refuses, with the buffers untouched; and `RegionSource` on a file object, whose reads are
counted. The `EAT1` blobs are headers packed by `container._pack_header` from random bit counts in front of random payload bytes
(tests/test_batch_decoder_tiles_host.py)."""
import io

import numpy
import pytest

from autoencoder_based_image_compression_amd import codec, container

(NB_MAPS, LENGTH, BATCH) = (128, 10, 3)
REGION = (32, 48)
# (image shape, coding tile, shape classes): latent planes 11 x 13 in tiles of (4, 4): four classes, 12 slots a crop; the same in one
# tile per map; 4 x 6 in tiles of (2, 4), where the window is the plane
CASES = [((176, 208), (4, 4), 4), ((176, 208), (16, 16), 1), ((64, 96), (2, 4), 2)]


def _blob(seed, nb_images, idx_map_exception, shape, tile, learned=False, length=LENGTH, eae1=False):
    """-> (blob, its parts): random header arrays, per tile random bit counts of a few bytes (a tenth of them zero), random
    payload bytes. eae1: the same with whole maps behind an `EAE1` header."""
    rng = numpy.random.RandomState(seed)
    (h, w) = (shape[0]//16, shape[1]//16)
    (tiles, _) = container.coding_tile_grid(h, w, (h, w) if eae1 else tile)
    bits = rng.randint(0, 33, size=(nb_images, len(tiles), NB_MAPS, 2)).astype(numpy.uint32)
    bits[rng.rand(*bits.shape) < 0.1] = 0
    parts = {'bin_widths': rng.uniform(0.05, 2., size=NB_MAPS).astype(numpy.float32), 'map_mean': rng.normal(size=NB_MAPS).astype(numpy.float32),
             'probabilities': rng.uniform(0.01, 0.99, size=(NB_MAPS, length)),
             'exception_rows': rng.uniform(0.01, 0.99, size=(nb_images if idx_map_exception >= 0 else 0, length)), 'bits': bits,
             'payload': rng.randint(0, 256, size=int(((bits.astype(numpy.int64) + 7)//8).sum())).astype(numpy.uint8).tobytes(),
             'nb_images': nb_images, 'idx_map_exception': idx_map_exception}
    fields = container._fields(learned, nb_images, shape[0], shape[1], idx_map_exception, parts['bin_widths'], parts['map_mean'],
                               parts['probabilities'], parts['exception_rows'], None if eae1 else tile)
    blob = container._pack_header(fields, bits) + parts['payload']
    header = container.read_header(blob)
    assert header.get('format') == (None if eae1 else 'EAT1') and len(blob) == header['payload_offset'] + len(parts['payload'])
    return blob, parts


def _layout(shape, tile, batch=BATCH):
    (h, w) = (shape[0]//16, shape[1]//16)
    (Rs, Cs) = codec.region_window(h, w, REGION)
    return codec.region_layout(batch, h, w, tile, Rs, Cs)


def _buffers(layout, capacity, fill=0xA5):
    (_, head_bytes) = codec.region_head_layout(layout['batch_size'], layout['n_slots'], LENGTH)
    return numpy.full(head_bytes, fill, dtype=numpy.uint8), numpy.full(capacity, fill, dtype=numpy.uint8)


def _plan(requests, layout, head, payload, capacity=None, learned=False, length=LENGTH):
    return codec.plan_region_step(requests, layout, head, payload, payload.size if capacity is None else capacity, REGION, length, learned)


def test_the_example_of_the_design():
    """11 x 13 latents, tiles of (4, 4), a window of 6 x 7: rows (2 full, 1 last), columns (3 full, 1 last): 12 slots a crop."""
    assert codec.region_window(11, 13, REGION) == (6, 7) and codec.region_window(4, 6, REGION) == (4, 6)
    layout = codec.region_layout(BATCH, 11, 13, (4, 4), 6, 7)
    assert layout['classes'] == [(4, 4), (3, 4), (4, 1), (3, 1)] and layout['class_slots'] == [6, 3, 2, 1]
    assert layout['slots_per_crop'] == 12 and layout['n_slots'] == 36 and layout['n_streams'] == 36*NB_MAPS
    # run order is class -> crop -> slot; class runs start on 128-element boundaries; the static half of the placed plan
    assert layout['class_first'] == [0, 18, 27, 33]
    assert [run[:3] for run in layout['runs']] == [((4, 4), 18, 0), ((3, 4), 9, 18*NB_MAPS), ((4, 1), 6, 27*NB_MAPS), ((3, 1), 3, 33*NB_MAPS)]
    assert all(run[3] % 128 == 0 for run in layout['runs'])
    slots = layout['slots']
    assert slots.shape == (36, 3) and slots.dtype == numpy.int64
    for ((rows, cols), count, first_stream, first_element) in layout['runs']:
        first = first_stream//NB_MAPS
        assert (slots[first:first + count, :2] == (rows, cols)).all()
        assert numpy.array_equal(slots[first:first + count, 2], first_element + numpy.arange(count)*NB_MAPS*rows*cols)
    assert layout['elements'] >= int(slots[-1, 2]) + NB_MAPS*3*1
    # one tile per map: one class, one slot a crop; the window that is the plane: every tile of the grid
    assert codec.region_layout(BATCH, 11, 13, (16, 16), 6, 7)['class_slots'] == [1]
    assert codec.region_layout(BATCH, 4, 6, (2, 4), 4, 6)['class_slots'] == [2, 2]
    for bad in ((0, 4), (4,), 4, (4.0, 4)):
        with pytest.raises(ValueError):
            codec.region_layout(BATCH, 11, 13, bad, 6, 7)
    with pytest.raises(ValueError):
        codec.region_layout(BATCH, 11, 13, (4, 4), 12, 7)


@pytest.mark.parametrize('batch,n_slots', [(1, 1), (1, 12), (2, 24), (3, 36), (3, 3), (4, 7), (5, 65)])
def test_head_layout_at_every_length(batch, n_slots):
    """`region_head_layout` at every truncated unary length the decoder accepts: the fields do not overlap, each starts on a multiple
    of 8, the block is a multiple of 16, and the views write where the layout says (`_check_layout` of tests/test_batch_decoder_host.py)."""
    from tests.test_batch_decoder_host import _check_layout
    for length in range(1, 256):
        (fields, nbytes) = codec.region_head_layout(batch, n_slots, length)
        assert fields['bits'][2] == (n_slots*NB_MAPS, 2) and fields['prob_row'][2] == (n_slots*NB_MAPS,) and fields['placement'][2] == (n_slots, 4)
        assert fields['crop_origin'][2] == (batch, 2) and fields['table'][2] == (batch, NB_MAPS + 1, length)
        assert fields['payload_bytes'][0] == fields['table'][0] + 8*batch*(NB_MAPS + 1)*length
        head = numpy.zeros(nbytes, dtype=numpy.uint8)
        _check_layout(fields, nbytes, codec.region_head_views(head, batch, n_slots, length), head)
        with pytest.raises(ValueError):
            codec.region_head_views(head[:-1], batch, n_slots, length)


@pytest.mark.parametrize('shape,tile,nb_classes', CASES)
def test_geometry_at_every_position(shape, tile, nb_classes):
    (h, w) = (shape[0]//16, shape[1]//16)
    layout = _layout(shape, tile)
    (Rs, Cs) = layout['window']
    assert len(layout['classes']) == nb_classes
    (blob, _) = _blob(1, 1, 67, shape, tile)
    header = container.read_header(blob)
    (tiles, (th, tw)) = (layout['tiles'], layout['coding_tile'])
    most = [0]*nb_classes
    scattered = {}
    for y0 in range(shape[0] - REGION[0] + 1):
        for x0 in range(shape[1] - REGION[1] + 1):
            plan = container.region_plan(header, (y0, x0) + REGION, images=[0])
            ((r0, c0), placed) = codec.place_region(layout, y0, x0)
            assert (r0, c0) == codec.region_origin(h, w, Rs, Cs, y0, x0) and 0 <= r0 <= h - Rs and 0 <= c0 <= w - Cs
            # the window contains region_plan's minimal sub-plane, and its shifted edges are the plane's
            (p0, p1, q0, q1) = plan['sub_plane']
            assert r0 <= p0 and p1 <= r0 + Rs and c0 <= q0 and q1 <= c0 + Cs, (y0, x0)
            assert (r0 == p0 or r0 + Rs == h) and (c0 == q0 or c0 + Cs == w), (y0, x0)
            # where the crop lies in the window's reconstruction: region_plan's crop, moved by the difference of the two origins
            assert (y0 - 16*r0, x0 - 16*c0) == (plan['crop'][0] + 16*(p0 - r0), plan['crop'][1] + 16*(q0 - c0))
            assert 0 <= y0 - 16*r0 <= 16*Rs - REGION[0] and 0 <= x0 - 16*c0 <= 16*Cs - REGION[1]
            if (r0, c0) in scattered:
                assert placed == scattered[(r0, c0)]
                continue
            scattered[(r0, c0)] = placed
            # the placed tiles are exactly the grid tiles that meet the window (so they hold region_plan's), in row-major order
            meeting = [t for t in range(len(tiles)) if tiles[t, 0] < r0 + Rs and tiles[t, 0] + tiles[t, 2] > r0
                       and tiles[t, 1] < c0 + Cs and tiles[t, 1] + tiles[t, 3] > c0]
            assert [t for (t, _, _, _) in placed] == meeting and set(plan['tiles']) <= set(meeting)
            # they fit the layout's slots: every (class, index) once, no class overflows
            used = [slot for (_, slot, _, _) in placed]
            assert len(set(used)) == len(used)
            for (t, (cls, index), row, col) in placed:
                assert cls == tiles[t, 4] and 0 <= index < layout['class_slots'][cls]
                assert (row, col) == (tiles[t, 0] - r0, tiles[t, 1] - c0)
                most[cls] = max(most[cls], index + 1)
            # a numpy model of the placed scatter writes every latent of the window exactly once
            written = numpy.zeros((Rs, Cs), dtype=numpy.int64)
            for (t, _, row, col) in placed:
                (rows, cols) = (int(tiles[t, 2]), int(tiles[t, 3]))
                (a0, a1, b0, b1) = (max(row, 0), min(row + rows, Rs), max(col, 0), min(col + cols, Cs))
                written[a0:a1, b0:b1] += 1
            assert (written == 1).all(), (r0, c0)
    assert len(scattered) == (h - Rs + 1)*(w - Cs + 1)
    assert most == layout['class_slots']          # and no slot of the layout is one too many


def _check_step(head, payload, layout, requests, made):
    """The head and the payload against the sources' own headers. made: {id(source): parts}."""
    (batch, n_slots) = (layout['batch_size'], layout['n_slots'])
    views = codec.region_head_views(head, batch, n_slots, LENGTH)
    bits = views['bits'].reshape(n_slots, NB_MAPS, 2)
    rows = views['prob_row'].reshape(n_slots, NB_MAPS)
    present = {}
    for (k, (source, image, y0, x0)) in enumerate(requests):
        parts = made[id(source)]
        ((r0, c0), placed) = codec.place_region(layout, y0, x0)
        for (t, (cls, index), row, col) in placed:
            run = layout['class_first'][cls] + k*layout['class_slots'][cls] + index
            assert run not in present
            present[run] = (source, image, t)
            assert numpy.array_equal(bits[run], parts['bits'][image, t]) and numpy.array_equal(bits[run], source.header['bits'][image, t])
            expected = k*(NB_MAPS + 1) + numpy.arange(NB_MAPS)
            if parts['idx_map_exception'] >= 0:
                expected[parts['idx_map_exception']] = k*(NB_MAPS + 1) + NB_MAPS
            assert numpy.array_equal(rows[run], expected)
            assert views['placement'][run].tolist() == [k, row, col, 0]
        assert views['crop_origin'][k].tolist() == [y0 - 16*r0, x0 - 16*c0]
        assert numpy.array_equal(views['bin_widths'][k], parts['bin_widths']) and numpy.array_equal(views['map_mean'][k], parts['map_mean'])
        assert numpy.array_equal(views['table'][k, :NB_MAPS], parts['probabilities'])
        if parts['idx_map_exception'] >= 0:
            assert numpy.array_equal(views['table'][k, NB_MAPS], parts['exception_rows'][image])
    # absent slots and absent crops
    absent = numpy.array([run for run in range(n_slots) if run not in present], dtype=numpy.int64)
    assert (rows[absent] == -1).all() and (bits[absent] == 0).all() and (views['placement'][absent] == (-1, 0, 0, 0)).all()
    n = len(requests)
    assert (views['crop_origin'][n:] == 0).all() and (views['bin_widths'][n:] == 0).all() and (views['map_mean'][n:] == 0).all()
    assert numpy.isfinite(views['table']).all() and (views['table'][n:] == 0.5).all()
    # the payload: the entries' byte ranges in run (slot) order, one behind the other
    expected = b''
    for run in sorted(present):
        (source, image, t) = present[run]
        header = source.header
        blob = made[id(source)]['blob']
        sizes = ((header['bits'].astype(numpy.int64) + 7)//8).sum(axis=(2, 3)).reshape(-1)
        start = header['payload_offset'] + int(sizes[:image*header['bits'].shape[1] + t].sum())
        expected += blob[start:start + int(sizes[image*header['bits'].shape[1] + t])]
    assert payload[:len(expected)].tobytes() == expected and int(views['payload_bytes'][0]) == len(expected)
    return len(expected)


def _sources(shape, tile, specs, files=False):
    """[RegionSource], {id: parts + blob} for (seed, images, exception map) specs."""
    (sources, made) = ([], {})
    for (seed, nb_images, idx) in specs:
        (blob, parts) = _blob(seed, nb_images, idx, shape, tile)
        source = codec.RegionSource(io.BytesIO(blob) if files else blob)
        made[id(source)] = dict(parts, blob=blob)
        sources.append(source)
    return sources, made


@pytest.mark.parametrize('files', [False, True])
@pytest.mark.parametrize('shape,tile,nb_classes', CASES)
def test_head_and_payload_of_full_mixed_and_partial_steps(shape, tile, nb_classes, files):
    layout = _layout(shape, tile)
    ((a, b, c), made) = _sources(shape, tile, [(10, 2, 67), (11, 1, -1), (12, 3, 0)], files)
    corner = (shape[0] - REGION[0], shape[1] - REGION[1])
    (head, payload) = _buffers(layout, 1 << 16, fill=0xFF)          # a poison that reads as NaN and as -1
    steps = [[(a, 1, 0, 0), (b, 0, 5, 7), (c, 2) + corner],                                  # three sources
             [(c, 0, corner[0]//2, corner[1]//3), (c, 0, corner[0]//2, corner[1]//3)],      # the same crop twice: a partial step
             [(a, 0) + corner],
             [(b, 0, 0, corner[1]), (a, 1, corner[0], 0), (a, 1, 17, 33)]]
    for requests in steps:
        (n, nbytes, crop_slots) = _plan(requests, layout, head, payload)
        assert n == len(requests) and len(crop_slots) == n
        assert nbytes == _check_step(head, payload, layout, requests, made)
        assert (payload[nbytes:] == 0xFF).all()                     # nothing behind the payload is written
        for (k, (source, image, y0, x0)) in enumerate(requests):    # the worker's map: a crop's slots in tile row-major order
            (_, placed) = codec.place_region(layout, y0, x0)
            assert crop_slots[k] == [layout['class_first'][cls] + k*layout['class_slots'][cls] + index for (_, (cls, index), _, _) in placed]
        payload[:] = 0xFF


def _refused(requests, layout, match=None, capacity=None, learned=False, length=LENGTH):
    (head, payload) = _buffers(layout, 1 << 16)
    with pytest.raises(ValueError, match=match):
        _plan(requests, layout, head, payload, capacity=capacity, learned=learned, length=length)
    assert (head == 0xA5).all() and (payload == 0xA5).all()         # refused before touching any buffer


@pytest.mark.parametrize('shape,tile,nb_classes', CASES[:1] + CASES[2:])
def test_refusals_leave_the_buffers_alone(shape, tile, nb_classes):
    layout = _layout(shape, tile)
    ((good,), _) = _sources(shape, tile, [(30, 2, 67)])
    ok = (good, 1, 0, 0)
    (head, payload) = _buffers(layout, 1 << 16)
    (_, nbytes, _) = _plan([ok, ok], layout, head, payload)
    other = lambda seed, **more: codec.RegionSource(_blob(seed, 1, 67, more.pop('shape', shape), more.pop('tile', tile), **more)[0])
    _refused([ok, (other(31, shape=(shape[0] + 16, shape[1])), 0, 0, 0)], layout, 'images')             # another height, the SECOND request
    _refused([(other(32, shape=(shape[0], shape[1] - 16)), 0, 0, 0)], layout, 'images')                 # another width
    _refused([(other(33, tile=(tile[0], tile[1] - 1)), 0, 0, 0)], layout, 'coding_tile')                # another tile
    _refused([(other(34, tile=(1, 1)), 0, 0, 0)], layout, 'coding_tile')
    _refused([(other(35, length=LENGTH + 1), 0, 0, 0)], layout, 'truncated unary length')               # another L
    _refused([ok], layout, 'truncated unary length', length=LENGTH - 1)
    _refused([(other(36, learned=True), 0, 0, 0)], layout, 'other kind of model')                       # the other model kind
    _refused([ok], layout, 'other kind of model', learned=True)
    _refused([(other(37, eae1=True), 0, 0, 0)], layout, 'EAE1')                                          # an EAE1 source
    for image in (2, -1, 100):                                                                           # an image the source does not hold
        _refused([ok, (good, image, 0, 0)], layout, 'no image')
    for (y0, x0) in ((-1, 0), (0, -1), (shape[0] - REGION[0] + 1, 0), (0, shape[1] - REGION[1] + 1), (shape[0], shape[1])):
        _refused([(good, 0, y0, x0)], layout, 'leaves')                                                  # a region that leaves the image
    _refused([ok]*(BATCH + 1), layout, 'at most')                                                        # more than batch_size requests
    _refused([ok, ok], layout, 'payload', capacity=nbytes - 1)                                           # a payload above capacity
    _refused([], layout, 'at least one')
    for bad in ((good, 0, 0), (good.header, 0, 0, 0), (good, 0.0, 0, 0), (good, 0, True, 0), 'abcd'):
        _refused([bad], layout, 'request')
    # a file that has lost its tail since the source was opened: the reads fail before anything is written
    (blob, _) = _blob(38, 1, 67, shape, tile)
    stream = io.BytesIO(blob)
    lost = codec.RegionSource(stream)
    stream.truncate(len(blob) - 1)
    _refused([(lost,) + (0, shape[0] - REGION[0], shape[1] - REGION[1])], layout, 'truncated')


class _Counting(io.BytesIO):
    def __init__(self, data):
        super(_Counting, self).__init__(data)
        self.reads = []

    def read(self, count=-1):
        data = super(_Counting, self).read(count)
        self.reads.append((self.tell() - len(data), len(data)))
        return data


def test_a_file_source_reads_the_header_once_and_merged_ranges():
    (shape, tile) = CASES[0][:2]
    (blob, parts) = _blob(40, 2, 67, shape, tile)
    header = container.read_header(blob)
    stream = _Counting(blob)
    source = codec.RegionSource(stream)
    # the fixed header, then the rest of the header: nothing of the payload
    assert stream.reads == [(0, container._TILE_HEADER.size), (container._TILE_HEADER.size, header['payload_offset'] - container._TILE_HEADER.size)]
    assert source.header['bits'].shape == (2, 12, NB_MAPS, 2) and source.starts.dtype == numpy.int64 and source.sizes.dtype == numpy.int64
    assert source.starts.shape == source.sizes.shape == (2, 12)
    assert int(source.starts[0, 0]) == header['payload_offset'] and int(source.starts[1, 11] + source.sizes[1, 11]) == len(blob)
    del stream.reads[:]
    # tiles 1, 2 (adjacent), 5, 6 (adjacent; 4 tiles a row) of image 1, asked for out of order: two reads, of exactly those bytes
    entries = [(1, 5), (1, 1), (1, 6), (1, 2)]
    chunks = source.read(entries)
    assert [bytes(chunk) for chunk in chunks] == [blob[int(source.starts[e]):int(source.starts[e] + source.sizes[e])] for e in entries]
    assert stream.reads == [(int(source.starts[1, 1]), int(source.sizes[1, 1] + source.sizes[1, 2])),
                            (int(source.starts[1, 5]), int(source.sizes[1, 5] + source.sizes[1, 6]))]
    # what fetch_region reads for the same tiles is the same: one reader serves both
    del stream.reads[:]
    layout = _layout(shape, tile)
    (head, payload) = _buffers(layout, 1 << 16)
    (_, nbytes, _) = _plan([(source, 0, 40, 60)], layout, head, payload)
    (_, placed) = codec.place_region(layout, 40, 60)
    assert sum(count for (_, count) in stream.reads) == nbytes == int(sum(source.sizes[0, t] for (t, _, _, _) in placed))
    assert len(stream.reads) == len({t//4 for (t, _, _, _) in placed})          # one read per tile row the window meets
    # an in-memory source reads nothing: slices; an EAE1 source parses (submit refuses it, not the constructor)
    memory = codec.RegionSource(bytearray(blob))
    assert [bytes(chunk) for chunk in memory.read(entries)] == [bytes(chunk) for chunk in chunks]
    assert codec.RegionSource(_blob(41, 1, -1, shape, tile, eae1=True)[0]).coding_tile == (11, 13)
    for bad in (blob[:-1], blob[:30], b''):
        with pytest.raises(ValueError):
            codec.RegionSource(bad)


def test_fetch_region_keeps_its_reads():
    """`container.fetch_region` on a file: the fixed header, the rest of the header, then the plan's ranges, adjacent ones merged."""
    (shape, tile) = CASES[0][:2]
    (blob, _) = _blob(42, 2, 67, shape, tile)
    stream = _Counting(blob)
    (header, plan, chunks) = container.fetch_region(stream, (40, 60) + REGION, images=[1])
    assert [bytes(chunk) for chunk in chunks] == [blob[a:b] for (a, b) in plan['ranges']]
    assert stream.reads[:2] == [(0, container._TILE_HEADER.size), (container._TILE_HEADER.size, header['payload_offset'] - container._TILE_HEADER.size)]
    assert sum(count for (_, count) in stream.reads[2:]) == sum(b - a for (a, b) in plan['ranges'])
    assert len(stream.reads) - 2 == len({t//4 for t in plan['tiles']})
    (again, _, memory) = container.fetch_region(blob, (40, 60) + REGION, images=[1])
    assert [bytes(chunk) for chunk in memory] == [bytes(chunk) for chunk in chunks] and again['payload_offset'] == header['payload_offset']
