"""The host side of `codec.BatchCodec(coding_tile=...)`, without a GPU: `codec.coding_tile_layout` (where the entries, the symbols,
the streams and the results of a step in tiles lie) against `container._group_layout` / `_prob_rows` / `_symbols_plan` on the full
list of entries, and `container.assemble_blob` / `assemble_image_blobs` with a coding tile against `container.read_header`."""
import numpy
import pytest

from autoencoder_based_image_compression_amd import codec, container

NB_MAPS = 128
# (batch, h, w, coding tile) -> (clamped tile, tiles per image, the classes' (rows, cols) in run order)
CASES = {(2, 4, 6, (2, 3)): ((2, 3), 4, [(2, 3)]),
         (2, 4, 6, (3, 4)): ((3, 4), 4, [(3, 4), (1, 4), (3, 2), (1, 2)]),
         (3, 3, 5, (2, 2)): ((2, 2), 6, [(2, 2), (1, 2), (2, 1), (1, 1)]),
         (1, 3, 2, (1, 1)): ((1, 1), 6, [(1, 1)]),
         (2, 4, 6, (100, 100)): ((4, 6), 1, [(4, 6)])}


@pytest.mark.parametrize('idx_map_exception', [-1, 67])
@pytest.mark.parametrize('case', sorted(CASES))
def test_layout_is_the_group_layout_of_every_entry_of_the_step(case, idx_map_exception):
    (batch, h, w, tile) = case
    (clamped, nb_tiles, shapes) = CASES[case]
    layout = codec.coding_tile_layout(batch, h, w, tile, idx_map_exception)
    assert layout['coding_tile'] == clamped and layout['nb_tiles'] == nb_tiles
    assert [run[0] for run in layout['runs']] == shapes
    n_entries = batch*nb_tiles
    assert layout['n_streams'] == n_entries*NB_MAPS
    assert layout['entries'] == [(i, t) for i in range(batch) for t in range(nb_tiles)]

    (tiles, classes) = container.coding_tile_grid(h, w, clamped)
    assert numpy.array_equal(layout['tiles'], tiles) and layout['classes'] == classes
    (runs, offsets, elements) = container._group_layout(layout['entries'], tiles, classes)
    assert layout['elements'] == elements
    assert numpy.array_equal(layout['offsets'], offsets) and layout['offsets'].dtype == numpy.int64
    plan = container._symbols_plan(layout['entries'], tiles, offsets)
    assert numpy.array_equal(layout['plan'], plan) and layout['plan'].dtype == numpy.int64 and layout['plan'].flags.c_contiguous
    # the runs: class after class, the entries of a class in payload order, streams and symbols counted on from run to run
    assert len(layout['runs']) == len(runs)
    first_entry = 0
    prob_rows = []
    for ((shape, count, first_stream, first_element), (cls, ks, start)) in zip(layout['runs'], runs):
        assert shape == tuple(classes[cls]) and count == len(ks)
        assert first_stream == first_entry*NB_MAPS and first_element == start and first_element % 128 == 0
        # run-order entry r of this class is the payload-order entry ks[r - first_entry], and the other way round
        assert layout['payload_entry'][first_entry:first_entry + count].tolist() == list(ks)
        assert layout['run_entry'][ks].tolist() == list(range(first_entry, first_entry + count))
        # the symbols of the class's entries lie side by side from the run's first element on
        size = shape[0]*shape[1]
        assert layout['offsets'][ks].tolist() == [first_element + k*NB_MAPS*size for k in range(count)]
        prob_rows.append(container._prob_rows(layout['entries'], ks, idx_map_exception))
        first_entry += count
    assert first_entry == n_entries
    expected_rows = numpy.concatenate(prob_rows)
    assert layout['prob_row'].dtype == numpy.int32 and numpy.array_equal(layout['prob_row'], expected_rows)
    if idx_map_exception >= 0:
        # the exception map of every tile of image i is coded with row 128 + i
        images = numpy.array([layout['entries'][k][0] for k in layout['payload_entry']])
        assert numpy.array_equal(layout['prob_row'][idx_map_exception::NB_MAPS], NB_MAPS + images)

    # the permutation is a bijection, for entries and for streams
    assert sorted(layout['run_entry'].tolist()) == list(range(n_entries))
    assert numpy.array_equal(layout['run_entry'][layout['payload_entry']], numpy.arange(n_entries))
    assert sorted(layout['payload_order'].tolist()) == list(range(layout['n_streams']))
    assert numpy.array_equal(layout['payload_order'].reshape(n_entries, NB_MAPS),
                             layout['run_entry'][:, None]*NB_MAPS + numpy.arange(NB_MAPS)[None, :])

    # no two entries' symbols overlap, and every one lies inside the buffer
    used = numpy.zeros(layout['elements'], dtype=numpy.int32)
    for (k, (_, t)) in enumerate(layout['entries']):
        (start, count) = (int(layout['offsets'][k]), NB_MAPS*int(tiles[t, 2]*tiles[t, 3]))
        assert 0 <= start and start + count <= layout['elements']
        used[start:start + count] += 1
    assert used.max() == 1 and int(used.sum()) == batch*NB_MAPS*h*w


def test_layout_refuses_what_is_no_coding_tile():
    for bad in ((0, 2), (2,), (2, 3, 4), (1.5, 2), 'ab', None, (True, 2)):
        with pytest.raises(ValueError):
            codec.coding_tile_layout(1, 4, 6, bad)
    with pytest.raises(ValueError):
        codec.coding_tile_layout(0, 4, 6, (2, 2))


def _parts(nb_images, height, width, idx_map_exception, entries_per_image, seed):
    """Synthetic parts of a blob: bit counts (some zero, some whole bytes) for `entries_per_image` x 128 maps per image, a payload of
    the size they announce. The counts stay within the smallest tile's capacity (32 bits per symbol, one symbol)."""
    rng = numpy.random.RandomState(seed)
    length = 10
    bits = rng.randint(0, 33, size=(nb_images*entries_per_image*NB_MAPS, 2)).astype(numpy.uint32)
    bits[rng.rand(*bits.shape) < 0.2] = 0
    nbytes = int(((bits.astype(numpy.int64) + 7)//8).sum())
    payload = rng.randint(0, 256, size=nbytes).astype(numpy.uint8).tobytes()
    rows = rng.uniform(0.05, 0.95, size=(nb_images if idx_map_exception >= 0 else 0, length))
    head = (False, nb_images, height, width, idx_map_exception, rng.uniform(0.5, 2., size=NB_MAPS).astype(numpy.float32),
            rng.normal(size=NB_MAPS).astype(numpy.float32), rng.uniform(0.05, 0.95, size=(NB_MAPS, length)))
    return head, rows, bits, payload


@pytest.mark.parametrize('idx_map_exception', [-1, 67])
@pytest.mark.parametrize('tile,clamped,nb_tiles', [((2, 3), (2, 3), 4), ((3, 4), (3, 4), 4), ((100, 100), (4, 6), 1)])
def test_assembled_tile_blobs_parse(tile, clamped, nb_tiles, idx_map_exception):
    """`assemble_blob(..., coding_tile=...)` is an `EAT1` blob `read_header` takes apart into the parts it was made of; its split by
    `assemble_image_blobs` parses image by image, every image holding its slice of the bit counts, the rows and the payload."""
    (nb_images, height, width) = (3, 64, 96)
    (head, rows, bits, payload) = _parts(nb_images, height, width, idx_map_exception, nb_tiles, 7)
    (blob, header_bytes) = container.assemble_blob(*(head + (rows, bits, payload)), coding_tile=tile)
    assert blob[:4] == b'EAT1'
    header = container.read_header(blob)
    assert header['format'] == 'EAT1' and header['coding_tile'] == clamped
    assert header['payload_offset'] == header_bytes and blob[header_bytes:] == payload
    assert (header['nb_images'], header['height'], header['width'], header['idx_map_exception']) == (nb_images, height, width, idx_map_exception)
    assert header['bits'].shape == (nb_images, nb_tiles, NB_MAPS, 2)
    assert numpy.array_equal(header['bits'].reshape(-1, 2), bits)
    assert numpy.array_equal(header['exception_probabilities'], rows)
    assert numpy.array_equal(header['bin_widths'], head[5]) and numpy.array_equal(header['map_mean'], head[6])
    assert numpy.array_equal(header['binary_probabilities'], head[7])

    blobs = container.assemble_image_blobs(*(head + (rows, bits, payload)), coding_tile=tile)
    assert len(blobs) == nb_images
    per_image = nb_tiles*NB_MAPS
    pos = 0
    for (i, image_blob) in enumerate(blobs):
        h = container.read_header(image_blob)
        assert h['format'] == 'EAT1' and h['coding_tile'] == clamped and h['nb_images'] == 1
        assert numpy.array_equal(h['bits'].reshape(-1, 2), bits[i*per_image:(i + 1)*per_image])
        assert numpy.array_equal(h['exception_probabilities'], rows[i:i + 1] if idx_map_exception >= 0 else rows)
        size = len(image_blob) - h['payload_offset']
        assert image_blob[h['payload_offset']:] == payload[pos:pos + size]
        pos += size
    assert pos == len(payload)
    # the shape of the bit counts is checked against the tiles the header announces
    with pytest.raises(ValueError):
        container.assemble_blob(*(head + (rows, bits[:-1], payload)), coding_tile=tile)
    with pytest.raises(ValueError):
        container.assemble_blob(*(head + (rows, bits, payload)), coding_tile=(0, 1))
    if nb_tiles > 1:
        with pytest.raises(ValueError):
            container.assemble_blob(*(head + (rows, bits, payload)))


@pytest.mark.parametrize('idx_map_exception', [-1, 67])
def test_without_a_coding_tile_the_bytes_are_unchanged(idx_map_exception):
    """The EAE1 blob, spelt out here byte by byte from the module's documented layout: what `assemble_blob` and `assemble_image_blobs`
    wrote before they knew coding tiles."""
    import struct
    (nb_images, height, width) = (2, 64, 96)
    (head, rows, bits, payload) = _parts(nb_images, height, width, idx_map_exception, 1, 11)

    def expected(n, rows_, bits_, payload_):
        fixed = struct.pack('<4sHHIIIHBBi', b'EAE1', 1, 0, n, height, width, NB_MAPS, 10, 0, idx_map_exception)
        return b''.join([fixed, head[5].tobytes(), head[6].tobytes(), head[7].tobytes(), rows_.tobytes(), bits_.tobytes(), payload_])

    (blob, header_bytes) = container.assemble_blob(*(head + (rows, bits, payload)))
    assert blob == expected(nb_images, rows, bits, payload) and header_bytes == len(blob) - len(payload)
    image_bytes = ((bits.astype(numpy.int64) + 7)//8).reshape(nb_images, -1).sum(axis=1)
    blobs = container.assemble_image_blobs(*(head + (rows, bits, payload)))
    pos = 0
    for i in range(nb_images):
        rows_i = rows[i:i + 1] if idx_map_exception >= 0 else rows
        assert blobs[i] == expected(1, rows_i, bits[i*NB_MAPS:(i + 1)*NB_MAPS], payload[pos:pos + int(image_bytes[i])])
        pos += int(image_bytes[i])
    assert container.read_header(blob)['bits'].shape == (nb_images*NB_MAPS, 2)
