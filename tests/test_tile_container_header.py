"""The tile-indexed container EAT1 on the host (container.py): the coding-tile grid, the region planner and
the untrusted header, which gets every check EAE1 has, per coding tile. No GPU needed: all of it is pure host code."""
import io

import numpy
import pytest

from autoencoder_based_image_compression_amd import container, pipeline


def build_tile_blob(nb_images=2, height=80, width=112, length=10, idx_map_exception=67, coding_tile=(2, 3), bits=None,
                    version=container.TILE_VERSION, payload_extra=0, seed=0):
    """A synthetic EAT1 blob: random bit counts within each tile's capacity (bits=None), payload bytes numbered so that every
    byte's position can be recognised."""
    (h, w) = (height//16, width//16)
    nb_tiles = container._nb_tiles(max(h, 1), max(w, 1), (max(coding_tile[0], 1), max(coding_tile[1], 1)))
    head = container._TILE_HEADER.pack(container.TILE_MAGIC, version, 0, nb_images, height, width, 128, length, 0, idx_map_exception,
                                       coding_tile[0], coding_tile[1])
    nb_rows = nb_images if idx_map_exception >= 0 else 0
    if bits is None:
        bits = numpy.random.RandomState(seed).randint(0, 33, size=(nb_images, nb_tiles, 128, 2)).astype(numpy.uint32)
    payload = int(((bits.astype(numpy.int64) + 7)//8).sum()) + payload_extra
    return b''.join([head, numpy.ones(128, numpy.float32).tobytes(), numpy.zeros(128, numpy.float32).tobytes(),
                     numpy.full((128, length), 0.5).tobytes(), numpy.full((nb_rows, length), 0.5).tobytes(),
                     bits.astype(numpy.uint32).tobytes(), (numpy.arange(max(payload, 0)) % 251).astype(numpy.uint8).tobytes()])


@pytest.mark.parametrize('h, w, tile', [(5, 7, (2, 3)), (1, 1, (1, 1)), (17, 25, (4, 6)), (8, 8, (8, 8)), (8, 8, (100, 3)),
                                        (64, 48, (16, 16)), (13, 1, (5, 1)), (3, 30, (1, 7))])
def test_the_grid_covers_every_latent_once(h, w, tile):
    (tiles, classes) = container.coding_tile_grid(h, w, tile)
    cover = numpy.zeros((h, w), dtype=numpy.int64)
    for (r0, c0, rows, cols, cls) in tiles.tolist():
        assert classes[cls] == (rows, cols)
        assert 1 <= rows <= tile[0] and 1 <= cols <= tile[1]
        cover[r0:r0 + rows, c0:c0 + cols] += 1
    assert (cover == 1).all()
    assert 1 <= len(classes) <= 4 and len(set(classes)) == len(classes)
    assert len(tiles) == -(-h//tile[0])*(-(-w//tile[1]))
    # row-major, ragged only on the last row and column
    assert [tuple(t[:2]) for t in tiles.tolist()] == [(r, c) for r in range(0, h, tile[0]) for c in range(0, w, tile[1])]
    assert classes[0] == (min(tile[0], h), min(tile[1], w))


def test_the_grid_has_four_classes_when_both_edges_are_ragged():
    (_, classes) = container.coding_tile_grid(5, 7, (2, 3))
    assert classes == [(2, 3), (1, 3), (2, 1), (1, 1)]
    assert container.coding_tile_grid(4, 6, (2, 3))[1] == [(2, 3)]
    for bad in ((0, 3), (2, 0), (2,), 3, (2.5, 3), (True, 3)):
        with pytest.raises(ValueError):
            container.coding_tile_grid(5, 7, bad)


def test_well_formed_tile_header_is_accepted():
    blob = build_tile_blob()
    header = container.read_header(blob)
    assert header['format'] == 'EAT1' and header['coding_tile'] == (2, 3)
    assert (header['nb_images'], header['height'], header['width']) == (2, 80, 112)
    assert header['bits'].shape == (2, 9, 128, 2) and header['exception_probabilities'].shape == (2, 10)
    assert header['payload_offset'] + int(((header['bits'].astype(numpy.int64) + 7)//8).sum()) == len(blob)
    assert container.read_header(build_tile_blob(idx_map_exception=-1))['exception_probabilities'].shape == (0, 10)


@pytest.mark.parametrize('idx_map_exception', [67, -1])
@pytest.mark.parametrize('length', [1, 2, 3, 31, 32, 33, 255])
def test_written_tile_headers_read_back_at_every_length(length, idx_map_exception):
    """`assemble_blob(coding_tile=...)` -> `read_header` at the lengths of tests/unary_length_cases.py, with and without the exception
    row: tiles of (4, 4) on 11 x 13 latents (four shape classes, each with its own stream capacity at that length), and one tile per
    map, whose header is the EAE1 header `ratecontrol.header_bytes` sizes plus the two sides of the coding tile."""
    from autoencoder_based_image_compression_amd import ratecontrol
    from tests.test_container_header import check_round_trip, random_parts
    for (nb_images, height, width, tile, learned) in ((2, 176, 208, (4, 4), False), (1, 64, 96, (4, 6), True)):
        (tiles, _) = container.coding_tile_grid(height//16, width//16, tile)
        sizes = [int(r*c) for (r, c) in tiles[:, 2:4].tolist()]
        parts = random_parts(length, nb_images, height, width, length, idx_map_exception, len(tiles), sizes)
        (blob, header_bytes) = container.assemble_blob(learned, nb_images, height, width, idx_map_exception, parts['bin_widths'], parts['map_mean'],
                                                       parts['probabilities'], parts['exception_rows'], parts['bits'].reshape(-1, 2),
                                                       parts['payload'], coding_tile=tile)
        header = container.read_header(blob)
        check_round_trip(header, parts, nb_images, height, width, length, idx_map_exception, learned)
        assert header['format'] == 'EAT1' and header['coding_tile'] == tile
        assert header['bits'].shape == parts['bits'].shape and numpy.array_equal(header['bits'], parts['bits'])
        assert header['payload_offset'] == header_bytes == len(blob) - len(parts['payload']) and blob[header_bytes:] == parts['payload']
        if len(tiles) == 1:
            ladder = ratecontrol.RateLadder(parts['bin_widths'][None], parts['probabilities'][None], parts['map_mean'], idx_map_exception)
            assert header_bytes == ratecontrol.header_bytes(ladder) + container._TILE_HEADER.size - container._HEADER.size
        # a count one bit above the capacity of the smallest tile's streams at this length, with a payload to match: refused
        smallest = int(numpy.argmin(sizes))
        bits = parts['bits'].copy()
        bits[0, smallest, 5, 1] = container.stream_capacity_bits(sizes[smallest], length) + 1
        payload = bytes(int(((bits.astype(numpy.int64) + 7)//8).sum()))
        (bad, _) = container.assemble_blob(learned, nb_images, height, width, idx_map_exception, parts['bin_widths'], parts['map_mean'],
                                           parts['probabilities'], parts['exception_rows'], bits.reshape(-1, 2), payload, coding_tile=tile)
        with pytest.raises(ValueError, match='capacity'):
            container.read_header(bad)
        for bad in (blob[:-1], blob + b'\x00'):
            with pytest.raises(ValueError):
                container.read_header(bad)


@pytest.mark.parametrize('kwargs', [
    dict(coding_tile=(0, 3)), dict(coding_tile=(2, 0)), dict(coding_tile=(0, 0)), dict(payload_extra=1), dict(payload_extra=-1),
    dict(version=container.TILE_VERSION + 1), dict(length=0), dict(height=40, width=0), dict(height=72), dict(nb_images=0),
    dict(idx_map_exception=128), dict(idx_map_exception=-2),
])
def test_bad_tile_headers_are_rejected(kwargs):
    with pytest.raises(ValueError):
        container.read_header(build_tile_blob(**kwargs))


@pytest.mark.parametrize('which', [(0, 0, 0, 0), (1, 8, 127, 1), (0, 2, 67, 0), (1, 6, 5, 1), (0, 4, 100, 1)])
def test_a_count_above_the_tile_capacity_is_rejected(which):
    """The capacity is per tile: 6 symbols for the interior tiles of 5 x 7 latents at (2, 3), 3, 2 and 1 on the edges. Exactly the
    capacity is legal; one bit more is not, with a payload sized to match."""
    (tiles, _) = container.coding_tile_grid(5, 7, (2, 3))
    capacity = container.stream_capacity_bits(int(tiles[which[1], 2]*tiles[which[1], 3]), 10)
    bits = numpy.full((2, 9, 128, 2), 9, dtype=numpy.uint32)
    bits[which] = capacity
    container.read_header(build_tile_blob(bits=bits))
    bits[which] += 1
    with pytest.raises(ValueError):
        container.read_header(build_tile_blob(bits=bits))


def test_a_truncated_index_is_rejected_before_it_is_read():
    blob = build_tile_blob()
    header = container.read_header(blob)
    index_start = header['payload_offset'] - header['bits'].nbytes
    for cut in (index_start, index_start + 1, header['payload_offset'] - 1, container._TILE_HEADER.size - 1, 3):
        with pytest.raises(ValueError):
            container.read_header(blob[:cut])
    # a header announcing a huge index: refused from the fixed fields and the length alone
    huge = container._TILE_HEADER.pack(container.TILE_MAGIC, 1, 0, 0xFFFFFFFF, 16*4096, 16*4096, 128, 10, 0, -1, 1, 1)
    with pytest.raises(ValueError):
        container.read_header(huge + bytes(4096))


def test_eae1_version_2_is_still_rejected():
    from tests.test_container_header import build_blob
    with pytest.raises(ValueError):
        container.read_header(build_blob(version=2))
    assert 'format' not in container.read_header(build_blob())


def _random_region(rng, height, width):
    y0 = int(rng.randint(0, height))
    x0 = int(rng.randint(0, width))
    return (y0, x0, int(rng.randint(1, height - y0 + 1)), int(rng.randint(1, width - x0 + 1)))


@pytest.mark.parametrize('shape, tile', [((2, 80, 112), (2, 3)), ((1, 80, 112), (1, 1)), ((3, 272, 400), (4, 6)),
                                         ((1, 512, 768), (16, 16)), ((1, 512, 768), (64, 64)), ((2, 160, 32), (3, 2))])
def test_region_plan(shape, tile):
    (n, height, width) = shape
    (h, w) = (height//16, width//16)
    header = container.read_header(build_tile_blob(nb_images=n, height=height, width=width, coding_tile=tile, seed=height))
    (tiles, _) = container.coding_tile_grid(h, w, tile)
    (before, after) = pipeline.DECODER_HALO
    rng = numpy.random.RandomState(width)
    regions = [(0, 0, 1, 1), (height - 1, width - 1, 1, 1), (0, 0, height, width), (5, 7, 1, 1), (17, 3, 9, 30)]
    regions += [_random_region(rng, height, width) for _ in range(40)]
    for region in regions:
        (y0, x0, rh, rw) = region
        if y0 + rh > height or x0 + rw > width:
            continue
        plan = container.region_plan(header, region)
        (r0, r1, c0, c1) = plan['sub_plane']
        # region +- halo, clamped
        assert r0 == max(y0//16 - before, 0) and r1 == min(-(-(y0 + rh)//16) + after, h)
        assert c0 == max(x0//16 - before, 0) and c1 == min(-(-(x0 + rw)//16) + after, w)
        (cy, cx, ch, cw) = plan['crop']
        assert (cy + 16*r0, cx + 16*c0, ch, cw) == region and cy + ch <= 16*(r1 - r0) and cx + cw <= 16*(c1 - c0)
        # exactly the tiles that meet the sub-plane
        meets = [t for t in range(len(tiles)) if tiles[t, 0] < r1 and tiles[t, 0] + tiles[t, 2] > r0 and tiles[t, 1] < c1 and
                 tiles[t, 1] + tiles[t, 3] > c0]
        assert plan['tiles'] == meets
        assert plan['entries'] == [(i, t) for i in range(n) for t in meets]
        # byte ranges: disjoint, inside the payload, each the entry's streams
        spans = sorted(plan['ranges'])
        assert all(a < b or a == b for (a, b) in spans)
        assert all(spans[k][1] <= spans[k + 1][0] for k in range(len(spans) - 1))
        assert spans[0][0] >= header['payload_offset'] and spans[-1][1] <= header['payload_offset'] + \
            int(((header['bits'].astype(numpy.int64) + 7)//8).sum())
        for ((i, t), (a, b)) in zip(plan['entries'], plan['ranges']):
            assert b - a == int(((header['bits'][i, t].astype(numpy.int64) + 7)//8).sum())
    plan = container.region_plan(header, (0, 0, height, width), images=[n - 1])
    assert plan['entries'] == [(n - 1, t) for t in range(len(tiles))] and plan['sub_plane'] == (0, h, 0, w)


def test_the_ranges_tile_the_payload_in_order():
    blob = build_tile_blob(nb_images=3, coding_tile=(2, 2))
    header = container.read_header(blob)
    plan = container.region_plan(header, (0, 0, 80, 112))
    assert plan['ranges'][0][0] == header['payload_offset'] and plan['ranges'][-1][1] == len(blob)
    assert all(plan['ranges'][k][1] == plan['ranges'][k + 1][0] for k in range(len(plan['ranges']) - 1))


@pytest.mark.parametrize('region', [(0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 4, 4), (0, -1, 4, 4), (79, 0, 2, 1), (0, 111, 1, 2),
                                    (80, 0, 1, 1), (0, 112, 1, 1), (0, 0, 81, 112), (0, 0, 1), (0.5, 0, 1, 1), 'abc'])
def test_out_of_image_or_empty_regions_are_rejected(region):
    header = container.read_header(build_tile_blob())
    with pytest.raises(ValueError):
        container.region_plan(header, region)


def test_bad_image_selections_are_rejected():
    header = container.read_header(build_tile_blob())
    for images in ([], [2], [-1], [0, 0]):
        with pytest.raises(ValueError):
            container.region_plan(header, (0, 0, 16, 16), images=images)


def test_an_eae1_header_plans_whole_maps():
    from tests.test_container_header import build_blob
    bits = numpy.random.RandomState(5).randint(0, 100, size=(3*128, 2)).astype(numpy.uint32)
    blob = build_blob(nb_images=3, height=32, width=48, bits=bits)
    header = container.read_header(blob)
    plan = container.region_plan(header, (17, 20, 3, 3), images=[2, 0])
    assert plan['tiles'] == [0] and plan['entries'] == [(2, 0), (0, 0)] and plan['sub_plane'] == (0, 2, 0, 3)
    per_image = ((bits.astype(numpy.int64) + 7)//8).reshape(3, -1).sum(axis=1)
    start = header['payload_offset']
    assert plan['ranges'] == [(start + int(per_image[:2].sum()), start + int(per_image.sum())), (start, start + int(per_image[0]))]


class CountingFile(io.BytesIO):
    """A seekable file that records every byte range read from it."""

    def __init__(self, data):
        super().__init__(data)
        self.reads = []

    def read(self, size=-1):
        start = self.tell()
        data = super().read(size)
        self.reads.append((start, start + len(data)))
        return data


@pytest.mark.parametrize('region, images', [((0, 0, 1, 1), None), ((40, 50, 20, 30), [1]), ((0, 0, 80, 112), None),
                                            ((79, 111, 1, 1), [0, 1]), ((33, 0, 2, 112), [1, 0])])
def test_the_file_reader_reads_the_header_and_the_listed_ranges_only(region, images):
    blob = build_tile_blob(nb_images=2, coding_tile=(1, 2), seed=11)
    f = CountingFile(blob)
    (header, plan, chunks) = container.fetch_region(f, region, images)
    assert plan == container.region_plan(container.read_header(blob), region, images)
    read = numpy.zeros(len(blob), dtype=numpy.int64)
    for (a, b) in f.reads:
        read[a:b] += 1
    expected = numpy.zeros(len(blob), dtype=numpy.int64)
    expected[:header['payload_offset']] = 1
    for (a, b) in plan['ranges']:
        expected[a:b] += 1
    assert numpy.array_equal(read, expected)                # every byte once, nothing else
    assert sum(b - a for (a, b) in f.reads) == header['payload_offset'] + sum(b - a for (a, b) in plan['ranges'])
    for ((a, b), chunk) in zip(plan['ranges'], chunks):
        assert bytes(chunk) == blob[a:b]
    # the blob as bytes gives the same plan and chunks
    (_, plan_bytes, chunks_bytes) = container.fetch_region(blob, region, images)
    assert plan_bytes == plan and [bytes(c) for c in chunks_bytes] == [bytes(c) for c in chunks]


def test_the_file_reader_refuses_a_truncated_file_before_reading_the_payload():
    blob = build_tile_blob()
    header = container.read_header(blob)
    f = CountingFile(blob[:header['payload_offset'] - 5])
    with pytest.raises(ValueError):
        container.fetch_region(f, (0, 0, 16, 16))
    assert all(b <= container._TILE_HEADER.size for (_, b) in f.reads)
    f = CountingFile(blob[:-1])
    with pytest.raises(ValueError):
        container.fetch_region(f, (0, 0, 16, 16))
    assert sum(b - a for (a, b) in f.reads) == header['payload_offset']
