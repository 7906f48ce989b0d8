"""`codec.plan_decode_step`: the host side of a `codec.BatchDecoder` step, numpy only. Blobs assembled by
`container.assemble_blob` from random bit counts and payload bytes go in; the step head must come out as `decode_head_layout`
says, the payloads one behind the other, and every step the decoder cannot take is refused before a byte of either buffer
changes."""
import struct

import numpy
import pytest

from autoencoder_based_image_compression_amd import codec, container

(NB_MAPS, LENGTH, HEIGHT, WIDTH, BATCH) = (128, 10, 32, 48, 4)
MAP_SIZE = (HEIGHT//16)*(WIDTH//16)


def _blob(seed, nb_images, idx_map_exception, learned=False, height=HEIGHT, width=WIDTH, length=LENGTH):
    """-> (blob, its parts): random header arrays, random bit counts up to a stream's capacity (a tenth of them zero), random bytes."""
    rng = numpy.random.RandomState(seed)
    most = container.stream_capacity_bits((height//16)*(width//16), length)
    bits = rng.randint(0, most + 1, size=(nb_images*NB_MAPS, 2)).astype(numpy.uint32)
    bits[rng.rand(*bits.shape) < 0.1] = 0
    bits[0, 0] = most
    parts = {'bin_widths': rng.uniform(0.05, 2., size=NB_MAPS).astype(numpy.float32), 'map_mean': rng.normal(size=NB_MAPS).astype(numpy.float32),
             'probabilities': rng.uniform(0.01, 0.99, size=(NB_MAPS, length)),
             'exception_rows': rng.uniform(0.01, 0.99, size=(nb_images if idx_map_exception >= 0 else 0, length)), 'bits': bits,
             'payload': rng.randint(0, 256, size=int(((bits.astype(numpy.int64) + 7)//8).sum())).astype(numpy.uint8).tobytes(),
             'nb_images': nb_images, 'idx_map_exception': idx_map_exception}
    (blob, header_bytes) = container.assemble_blob(learned, nb_images, height, width, idx_map_exception, parts['bin_widths'], parts['map_mean'],
                                                   parts['probabilities'], parts['exception_rows'], bits, parts['payload'])
    assert len(blob) == header_bytes + len(parts['payload'])
    return blob, parts


def _buffers(capacity, batch=BATCH, fill=0xA5):
    (_, head_bytes) = codec.decode_head_layout(batch, NB_MAPS, LENGTH)
    return numpy.full(head_bytes, fill, dtype=numpy.uint8), numpy.full(capacity, fill, dtype=numpy.uint8)


def _plan(blobs, head, payload, capacity=None, batch=BATCH, learned=False):
    return codec.plan_decode_step(blobs, batch, HEIGHT, WIDTH, LENGTH, learned, payload.size if capacity is None else capacity, head, payload)


def _check_head(head, payload, all_parts, batch=BATCH):
    views = codec.decode_head_views(head, batch, NB_MAPS, LENGTH)
    (image, position) = (0, 0)
    for parts in all_parts:
        for k in range(parts['nb_images']):
            maps = slice(image*NB_MAPS, (image + 1)*NB_MAPS)
            assert numpy.array_equal(views['bits'][maps], parts['bits'][k*NB_MAPS:(k + 1)*NB_MAPS])
            rows = image*(NB_MAPS + 1) + numpy.arange(NB_MAPS)
            if parts['idx_map_exception'] >= 0:
                rows[parts['idx_map_exception']] = image*(NB_MAPS + 1) + NB_MAPS
                assert numpy.array_equal(views['table'][image, NB_MAPS], parts['exception_rows'][k])
            assert numpy.array_equal(views['prob_row'][maps], rows)
            assert numpy.array_equal(views['bin_widths'][image], parts['bin_widths'])
            assert numpy.array_equal(views['map_mean'][image], parts['map_mean'])
            assert numpy.array_equal(views['table'][image, :NB_MAPS], parts['probabilities'])
            image += 1
        assert payload[position:position + len(parts['payload'])].tobytes() == parts['payload']
        position += len(parts['payload'])
    # absent images: not coded, nothing to place, finite rows
    assert (views['prob_row'][image*NB_MAPS:] == -1).all() and (views['bits'][image*NB_MAPS:] == 0).all()
    assert numpy.isfinite(views['bin_widths']).all() and numpy.isfinite(views['map_mean']).all() and numpy.isfinite(views['table']).all()
    assert int(views['payload_bytes'][0]) == position
    return image, position


def test_layout_is_the_documented_one():
    (fields, nbytes) = codec.decode_head_layout(BATCH, NB_MAPS, LENGTH)
    n_maps = BATCH*NB_MAPS
    assert [(name, fields[name][0]) for name in ('bits', 'prob_row', 'bin_widths', 'map_mean', 'table', 'payload_bytes')] == [
        ('bits', 0), ('prob_row', 8*n_maps), ('bin_widths', 12*n_maps), ('map_mean', 16*n_maps), ('table', 20*n_maps),
        ('payload_bytes', 20*n_maps + 8*BATCH*(NB_MAPS + 1)*LENGTH)]
    assert fields['bits'][1:] == (numpy.dtype(numpy.uint32), (n_maps, 2)) and fields['prob_row'][1:] == (numpy.dtype(numpy.int32), (n_maps,))
    assert fields['table'][1:] == (numpy.dtype(numpy.float64), (BATCH, NB_MAPS + 1, LENGTH)) and fields['payload_bytes'][1] == numpy.dtype(numpy.uint64)
    assert nbytes % 16 == 0 and 0 <= nbytes - (fields['payload_bytes'][0] + 8) < 16
    # odd sizes keep every field on its own alignment
    (odd, _) = codec.decode_head_layout(3, NB_MAPS, 7)
    assert all(pos % dtype.itemsize == 0 for (pos, dtype, _) in odd.values())


def _check_layout(fields, nbytes, views, head):
    """A step head's fields do not overlap, each starts on a multiple of 8, the block is a multiple of 16 bytes that the last field
    ends in, and the views write where the layout says: a value put into the last element of every field is read back from the
    bytes [end - itemsize, end) of that field, and from nowhere else."""
    spans = sorted((pos, pos + dtype.itemsize*int(numpy.prod(shape)), name) for (name, (pos, dtype, shape)) in fields.items())
    assert spans[0][0] == 0
    for ((_, end, name), (start, _, following)) in zip(spans, spans[1:]):
        assert end <= start < end + 8, (name, following)
    assert all(start % 8 == 0 and stop > start for (start, stop, _) in spans)
    assert nbytes % 16 == 0 and 0 <= nbytes - spans[-1][1] < 16 and head.size == nbytes
    assert sorted(views) == sorted(fields)
    head[:] = 0
    for (k, (start, stop, name)) in enumerate(spans):
        (_, dtype, shape) = fields[name]
        assert views[name].shape == shape and views[name].dtype == dtype
        views[name].reshape(-1)[-1] = 3 + k
    for (k, (start, stop, name)) in enumerate(spans):
        dtype = fields[name][1]
        assert head[stop - dtype.itemsize:stop].view(dtype)[0] == 3 + k, name
        assert views[name].reshape(-1)[-1] == 3 + k, name
    written = numpy.zeros(nbytes, dtype=bool)
    for (start, stop, name) in spans:
        written[stop - fields[name][1].itemsize:stop] = True
    assert not head[~written].any()


@pytest.mark.parametrize('batch,n_streams', [(1, None), (2, None), (3, None), (4, None), (3, 3*12*NB_MAPS), (2, 2*7*NB_MAPS), (1, 5*NB_MAPS)])
def test_layout_at_every_length(batch, n_streams):
    """Every truncated unary length the decoder accepts moves 'payload_bytes' behind the table, by 8*batch*129 bytes a column."""
    for length in range(1, 256):
        (fields, nbytes) = codec.decode_head_layout(batch, NB_MAPS, length, n_streams)
        n = batch*NB_MAPS if n_streams is None else n_streams
        assert fields['bits'][2] == (n, 2) and fields['prob_row'][2] == (n,) and fields['table'][2] == (batch, NB_MAPS + 1, length)
        assert fields['payload_bytes'][0] == fields['table'][0] + 8*batch*(NB_MAPS + 1)*length
        head = numpy.zeros(nbytes, dtype=numpy.uint8)
        _check_layout(fields, nbytes, codec.decode_head_views(head, batch, NB_MAPS, length, n_streams), head)
        with pytest.raises(ValueError):
            codec.decode_head_views(head[:-1], batch, NB_MAPS, length, n_streams)


@pytest.mark.parametrize('idx_map_exception', [-1, 0, 127])
def test_one_multi_image_blob(idx_map_exception):
    (blob, parts) = _blob(1 + idx_map_exception, BATCH, idx_map_exception)
    (head, payload) = _buffers(len(parts['payload']) + 16)
    assert _plan(blob, head, payload) == (BATCH, len(parts['payload']))
    assert _check_head(head, payload, [parts]) == (BATCH, len(parts['payload']))
    assert (payload[len(parts['payload']):] == 0xA5).all()          # nothing behind the payload is written


def test_single_image_blobs_with_different_tables_and_exception_maps():
    made = [_blob(10 + k, 1, idx) for (k, idx) in enumerate((-1, 0, 127, 67))]
    total = sum(len(parts['payload']) for (_, parts) in made)
    (head, payload) = _buffers(total)
    for blobs in ([b for (b, _) in made], tuple(bytearray(b) for (b, _) in made), [memoryview(b) for (b, _) in made]):
        head[:] = 0xA5
        payload[:] = 0xA5
        assert _plan(blobs, head, payload) == (4, total)
        _check_head(head, payload, [parts for (_, parts) in made])
    views = codec.decode_head_views(head, BATCH, NB_MAPS, LENGTH)
    assert [int(views['prob_row'][i*NB_MAPS + idx]) for (i, idx) in ((1, 0), (2, 127), (3, 67))] == [1*129 + 128, 2*129 + 128, 3*129 + 128]
    assert int(views['prob_row'][0]) == 0 and int(views['prob_row'][NB_MAPS - 1]) == NB_MAPS - 1      # image 0 has no exception map


def test_partial_step_and_mixed_blob_sizes():
    made = [_blob(20, 2, 5), _blob(21, 1, -1)]
    total = sum(len(parts['payload']) for (_, parts) in made)
    (head, payload) = _buffers(total + 64, fill=0xFF)                 # poison that reads as NaN and as -1
    assert _plan([b for (b, _) in made], head, payload) == (3, total)
    assert _check_head(head, payload, [parts for (_, parts) in made]) == (3, total)
    # a step that follows a fuller one in the same buffers leaves nothing of it behind
    (blob, parts) = _blob(22, 1, 127)
    assert _plan(blob, head, payload) == (1, len(parts['payload']))
    _check_head(head, payload, [parts])


def _refused(blobs, match=None, capacity=None, learned=False, batch=BATCH):
    (head, payload) = _buffers(1 << 16, batch=batch)
    with pytest.raises(ValueError, match=match):
        _plan(blobs, head, payload, capacity=capacity, batch=batch, learned=learned)
    assert (head == 0xA5).all() and (payload == 0xA5).all()         # refused before touching any buffer


def test_refusals_leave_the_buffers_alone():
    (good, parts) = _blob(30, 1, 67)
    _refused([good, _blob(31, 1, 67, height=HEIGHT + 16)[0]], 'images')                     # the wrong height, in the SECOND blob
    _refused(_blob(32, 1, 67, width=WIDTH - 16)[0], 'images')                               # the wrong width
    _refused(_blob(33, 1, 67, length=LENGTH + 1)[0], 'truncated unary length')              # the wrong L
    _refused(_blob(34, 1, 67, learned=True)[0], 'other kind of model')                      # the wrong model kind
    _refused(good, 'other kind of model', learned=True)
    _refused([good]*(BATCH + 1), 'images')                                                  # too many images: five blobs of one
    _refused([_blob(35, BATCH, -1)[0], good], 'images')                                     # ... and a full blob plus one
    _refused(_blob(36, 3, -1)[0], 'images', batch=2)
    _refused([good, good], 'payload', capacity=2*len(parts['payload']) - 1)                 # a payload beyond capacity
    _refused(good[:-1])                                                                     # a truncated blob
    _refused(good[:40])
    _refused([])
    # EAT1 magic: named with the function that reads such files
    tiled = container._pack_header(dict(container._fields(False, 1, HEIGHT, WIDTH, -1, parts['bin_widths'], parts['map_mean'],
                                                          parts['probabilities'], parts['exception_rows'][:0], (1, 1))),
                                   numpy.zeros((1, MAP_SIZE, NB_MAPS, 2), dtype=numpy.uint32))
    assert tiled[:4] == container.TILE_MAGIC and container.read_header(tiled)['format'] == 'EAT1'
    _refused(tiled, 'decode_region')
    # a bit count beyond the capacity of a stream (the payload resized to match, so only that check can refuse it)
    header = container.read_header(good)
    position = header['payload_offset'] - 8*NB_MAPS + 8*3
    most = container.stream_capacity_bits(MAP_SIZE, LENGTH)
    old = struct.unpack_from('<I', good, position)[0]
    grown = bytearray(good)
    struct.pack_into('<I', grown, position, most + 8)
    grown += bytes((most + 8 + 7)//8 - (old + 7)//8)
    _refused(bytes(grown), 'capacity of a stream')
    # the same edit at the capacity itself is a legal header
    struct.pack_into('<I', grown, position, most)
    legal = bytes(grown[:len(good) + (most + 7)//8 - (old + 7)//8])
    (head, payload) = _buffers(1 << 16)
    assert _plan(legal, head, payload)[0] == 1
