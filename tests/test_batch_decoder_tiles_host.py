"""`codec.plan_decode_step(coding_tile=...)`: the host side of a step of `codec.BatchDecoder(coding_tile=...)`, numpy only
(DESIGN.md section 16). `EAT1` headers packed by `container._pack_header` / `_fields` from random bit counts, in front of random
payload bytes, go in; 'bits' and 'prob_row' of the step head must come out in run order -- the payload-order values permuted by
`coding_tile_layout(...)['payload_order']` --, the payloads one behind the other, and every step the decoder cannot take is refused
before a byte of either buffer changes. Without `coding_tile` the head and the refusal of `EAT1` are the untiled decoder's."""
import numpy
import pytest

from autoencoder_based_image_compression_amd import codec, container

(NB_MAPS, LENGTH, BATCH) = (128, 10, 3)
# latent planes 3 x 5 with tiles of (2, 2): four shape classes; 4 x 6 with tiles of (2, 4): two
CASES = [((48, 80), (2, 2), 4), ((64, 96), (2, 4), 2)]


def _blob(seed, nb_images, idx_map_exception, shape, tile, learned=False, length=LENGTH, eae1=False):
    """-> (blob, its parts): random header arrays, per tile random bit counts up to the capacity of a stream of that tile (a tenth
    of them zero), random payload bytes. eae1: the same with whole maps behind an `EAE1` header."""
    rng = numpy.random.RandomState(seed)
    (h, w) = (shape[0]//16, shape[1]//16)
    (tiles, _) = container.coding_tile_grid(h, w, (h, w) if eae1 else tile)
    bits = numpy.zeros((nb_images, len(tiles), NB_MAPS, 2), dtype=numpy.uint32)
    for (t, (_, _, rows, cols, _)) in enumerate(tiles.tolist()):
        most = container.stream_capacity_bits(rows*cols, length)
        bits[:, t] = rng.randint(0, most + 1, size=(nb_images, NB_MAPS, 2))
        bits[0, t, 0, 0] = most
    bits[rng.rand(*bits.shape) < 0.1] = 0
    parts = {'bin_widths': rng.uniform(0.05, 2., size=NB_MAPS).astype(numpy.float32), 'map_mean': rng.normal(size=NB_MAPS).astype(numpy.float32),
             'probabilities': rng.uniform(0.01, 0.99, size=(NB_MAPS, length)),
             'exception_rows': rng.uniform(0.01, 0.99, size=(nb_images if idx_map_exception >= 0 else 0, length)), 'bits': bits,
             'payload': rng.randint(0, 256, size=int(((bits.astype(numpy.int64) + 7)//8).sum())).astype(numpy.uint8).tobytes(),
             'nb_images': nb_images, 'idx_map_exception': idx_map_exception}
    fields = container._fields(learned, nb_images, shape[0], shape[1], idx_map_exception, parts['bin_widths'], parts['map_mean'],
                               parts['probabilities'], parts['exception_rows'], None if eae1 else tile)
    blob = container._pack_header(fields, bits) + parts['payload']
    header = container.read_header(blob)                                  # a legal blob of the format asked for
    assert header.get('format') == (None if eae1 else 'EAT1') and len(blob) == header['payload_offset'] + len(parts['payload'])
    return blob, parts


def _buffers(shape, tile, capacity, batch=BATCH, fill=0xA5, length=LENGTH):
    layout = codec.coding_tile_layout(batch, shape[0]//16, shape[1]//16, tile)
    (_, head_bytes) = codec.decode_head_layout(batch, NB_MAPS, length, layout['n_streams'])
    return numpy.full(head_bytes, fill, dtype=numpy.uint8), numpy.full(capacity, fill, dtype=numpy.uint8), layout


def _plan(blobs, shape, tile, head, payload, capacity=None, batch=BATCH, learned=False, layout=None):
    return codec.plan_decode_step(blobs, batch, shape[0], shape[1], LENGTH, learned, payload.size if capacity is None else capacity, head,
                                  payload, coding_tile=tile, layout=layout)


def _check_head(head, payload, all_parts, layout, batch=BATCH):
    """The head against the blobs' parts: what the step holds in PAYLOAD order (image -> tile -> map), written out from the parts,
    must be the head's run-order arrays taken through `payload_order`."""
    nb_tiles = layout['nb_tiles']
    views = codec.decode_head_views(head, batch, NB_MAPS, LENGTH, layout['n_streams'])
    assert views['bits'].shape == (batch*nb_tiles*NB_MAPS, 2) and views['prob_row'].shape == (batch*nb_tiles*NB_MAPS,)
    bits = numpy.zeros((batch, nb_tiles, NB_MAPS, 2), dtype=numpy.uint32)
    rows = numpy.full((batch, nb_tiles, NB_MAPS), -1, dtype=numpy.int32)
    (image, position) = (0, 0)
    for parts in all_parts:
        for k in range(parts['nb_images']):
            bits[image] = parts['bits'][k]
            rows[image] = image*(NB_MAPS + 1) + numpy.arange(NB_MAPS)
            if parts['idx_map_exception'] >= 0:
                rows[image, :, parts['idx_map_exception']] = image*(NB_MAPS + 1) + NB_MAPS       # in every tile
                assert numpy.array_equal(views['table'][image, NB_MAPS], parts['exception_rows'][k])
            assert numpy.array_equal(views['bin_widths'][image], parts['bin_widths'])
            assert numpy.array_equal(views['map_mean'][image], parts['map_mean'])
            assert numpy.array_equal(views['table'][image, :NB_MAPS], parts['probabilities'])
            image += 1
        assert payload[position:position + len(parts['payload'])].tobytes() == parts['payload']
        position += len(parts['payload'])
    order = layout['payload_order']
    assert numpy.array_equal(numpy.sort(order), numpy.arange(order.size))                           # a permutation of the streams
    assert numpy.array_equal(views['bits'].take(order, axis=0), bits.reshape(-1, 2))
    assert numpy.array_equal(views['prob_row'].take(order), rows.reshape(-1))
    # absent images: -1 and zero bits for every stream of theirs, finite rows
    absent = order[image*nb_tiles*NB_MAPS:]
    assert (views['prob_row'][absent] == -1).all() and (views['bits'][absent] == 0).all()
    assert int((views['prob_row'] == -1).sum()) == (batch - image)*nb_tiles*NB_MAPS
    assert numpy.isfinite(views['bin_widths']).all() and numpy.isfinite(views['map_mean']).all() and numpy.isfinite(views['table']).all()
    assert int(views['payload_bytes'][0]) == position
    return image, position


def test_head_layout_defaults_are_the_untiled_ones_and_stream_counts_grow_it():
    (batch, length) = (3, 10)
    n_maps = batch*NB_MAPS
    (fields, nbytes) = codec.decode_head_layout(batch, NB_MAPS, length)
    # the untiled decoder's block, written out: fields, offsets, byte count
    assert fields == {'bits': (0, numpy.dtype(numpy.uint32), (n_maps, 2)), 'prob_row': (8*n_maps, numpy.dtype(numpy.int32), (n_maps,)),
                      'bin_widths': (12*n_maps, numpy.dtype(numpy.float32), (batch, NB_MAPS)),
                      'map_mean': (16*n_maps, numpy.dtype(numpy.float32), (batch, NB_MAPS)),
                      'table': (20*n_maps, numpy.dtype(numpy.float64), (batch, NB_MAPS + 1, length)),
                      'payload_bytes': (20*n_maps + 8*batch*(NB_MAPS + 1)*length, numpy.dtype(numpy.uint64), (1,))}
    assert nbytes == -(-(20*n_maps + 8*batch*(NB_MAPS + 1)*length + 8)//16)*16
    assert codec.decode_head_layout(batch, NB_MAPS, length, None) == (fields, nbytes)
    assert codec.decode_head_layout(batch, NB_MAPS, length, n_maps) == (fields, nbytes)
    head = numpy.zeros(nbytes, dtype=numpy.uint8)
    views = codec.decode_head_views(head, batch, NB_MAPS, length)
    assert {name: view.shape for (name, view) in views.items()} == {name: shape for (name, (_, _, shape)) in fields.items()}
    # with a stream count: 'bits' and 'prob_row' hold that many entries, the rest keeps its shape and moves behind them
    n_streams = codec.coding_tile_layout(batch, 3, 5, (2, 2))['n_streams']
    assert n_streams == batch*6*NB_MAPS
    (tiled, tiled_bytes) = codec.decode_head_layout(batch, NB_MAPS, length, n_streams)
    assert tiled['bits'] == (0, numpy.dtype(numpy.uint32), (n_streams, 2)) and tiled['prob_row'] == (8*n_streams, numpy.dtype(numpy.int32), (n_streams,))
    for name in ('bin_widths', 'map_mean', 'table', 'payload_bytes'):
        assert tiled[name][1:] == fields[name][1:] and tiled[name][0] == fields[name][0] + 12*(n_streams - n_maps)
    assert tiled_bytes == nbytes + 12*(n_streams - n_maps) and tiled_bytes % 16 == 0
    views = codec.decode_head_views(numpy.zeros(tiled_bytes, dtype=numpy.uint8), batch, NB_MAPS, length, n_streams)
    assert views['bits'].shape == (n_streams, 2) and views['prob_row'].shape == (n_streams,) and views['table'].shape == (batch, NB_MAPS + 1, length)
    with pytest.raises(ValueError):
        codec.decode_head_views(head, batch, NB_MAPS, length, n_streams)          # the untiled block is too small for it


@pytest.mark.parametrize('shape,tile,nb_classes', CASES)
def test_one_multi_image_blob_lands_in_run_order(shape, tile, nb_classes):
    (blob, parts) = _blob(1, BATCH, 67, shape, tile)
    (head, payload, layout) = _buffers(shape, tile, len(parts['payload']) + 16)
    assert len(layout['classes']) == nb_classes and len(layout['runs']) == nb_classes
    assert not numpy.array_equal(layout['payload_order'], numpy.arange(layout['n_streams']))       # run order is not payload order here
    assert _plan(blob, shape, tile, head, payload, layout=layout) == (BATCH, len(parts['payload']))
    assert _check_head(head, payload, [parts], layout) == (BATCH, len(parts['payload']))
    assert (payload[len(parts['payload']):] == 0xA5).all()          # nothing behind the payload is written
    # the layout is a convenience: without it the function computes the same one
    again = numpy.full_like(head, 0x5A)
    assert _plan(blob, shape, tile, again, payload) == (BATCH, len(parts['payload']))
    assert _check_head(again, payload, [parts], layout) == (BATCH, len(parts['payload']))


@pytest.mark.parametrize('shape,tile,nb_classes', CASES)
def test_blobs_with_different_exception_maps_and_without_one(shape, tile, nb_classes):
    made = [_blob(10 + k, 1, idx, shape, tile) for (k, idx) in enumerate((0, -1, 127))]
    total = sum(len(parts['payload']) for (_, parts) in made)
    (head, payload, layout) = _buffers(shape, tile, total)
    for blobs in ([b for (b, _) in made], tuple(bytearray(b) for (b, _) in made), [memoryview(b) for (b, _) in made]):
        head[:] = 0xA5
        payload[:] = 0xA5
        assert _plan(blobs, shape, tile, head, payload, layout=layout) == (3, total)
        _check_head(head, payload, [parts for (_, parts) in made], layout)
    # written out for one stream each: image 0's map 0 and image 2's map 127 take their images' exception rows in EVERY tile,
    # image 1 has no exception map
    views = codec.decode_head_views(head, BATCH, NB_MAPS, LENGTH, layout['n_streams'])
    rows = views['prob_row'].take(layout['payload_order']).reshape(BATCH, layout['nb_tiles'], NB_MAPS)
    assert (rows[0, :, 0] == 128).all() and (rows[0, :, 1] == 1).all()
    assert (rows[1] == 129 + numpy.arange(NB_MAPS)[None, :]).all()
    assert (rows[2, :, 127] == 2*129 + 128).all() and (rows[2, :, 126] == 2*129 + 126).all()


@pytest.mark.parametrize('shape,tile,nb_classes', CASES)
def test_partial_steps_and_mixed_blob_sizes(shape, tile, nb_classes):
    made = [_blob(20, 1, 5, shape, tile), _blob(21, 1, -1, shape, tile)]
    total = sum(len(parts['payload']) for (_, parts) in made)
    (head, payload, layout) = _buffers(shape, tile, total + 64, fill=0xFF)          # poison that reads as NaN and as -1
    assert _plan([b for (b, _) in made], shape, tile, head, payload, layout=layout) == (2, total)
    assert _check_head(head, payload, [parts for (_, parts) in made], layout) == (2, total)
    # a blob of two images and nothing else; then one image: a step that follows a fuller one leaves nothing of it behind
    (pair, pair_parts) = _blob(22, 2, 127, shape, tile)
    (head2, payload2, _) = _buffers(shape, tile, len(pair_parts['payload']), fill=0xFF)
    assert _plan(pair, shape, tile, head2, payload2, layout=layout) == (2, len(pair_parts['payload']))
    _check_head(head2, payload2, [pair_parts], layout)
    (blob, parts) = _blob(23, 1, 127, shape, tile)
    assert _plan(blob, shape, tile, head, payload, layout=layout) == (1, len(parts['payload']))
    _check_head(head, payload, [parts], layout)


def test_a_tile_beyond_the_plane_is_the_clamped_one():
    """(16, 16) on a 3 x 5 plane is one tile per map: run order is payload order, and a blob that says (3, 5) is that decoder's."""
    (shape, tile) = ((48, 80), (16, 16))
    (blob, parts) = _blob(40, 2, 67, shape, (3, 5))
    (head, payload, layout) = _buffers(shape, tile, len(parts['payload']))
    assert layout['coding_tile'] == (3, 5) and layout['nb_tiles'] == 1
    assert _plan(blob, shape, tile, head, payload, layout=layout) == (2, len(parts['payload']))
    _check_head(head, payload, [parts], layout)


def _refused(blobs, shape, tile, match=None, capacity=None, learned=False, batch=BATCH):
    (head, payload, layout) = _buffers(shape, tile, 1 << 17, batch=batch)
    with pytest.raises(ValueError, match=match):
        _plan(blobs, shape, tile, head, payload, capacity=capacity, batch=batch, learned=learned, layout=layout)
    assert (head == 0xA5).all() and (payload == 0xA5).all()         # refused before touching any buffer


@pytest.mark.parametrize('shape,tile,nb_classes', CASES)
def test_refusals_leave_the_buffers_alone(shape, tile, nb_classes):
    (good, parts) = _blob(30, 1, 67, shape, tile)
    _refused([good, _blob(31, 1, 67, shape, tile, eae1=True)[0]], shape, tile, 'coding_tile')        # an EAE1 blob, the SECOND of the step
    _refused(_blob(32, 1, 67, shape, (tile[0], tile[1] - 1))[0], shape, tile, 'coding_tile')          # another tile
    _refused(_blob(33, 1, 67, shape, (1, 1))[0], shape, tile, 'coding_tile')
    _refused([good, _blob(34, 1, 67, (shape[0] + 16, shape[1]), tile)[0]], shape, tile, 'images')    # the wrong height
    _refused(_blob(35, 1, 67, (shape[0], shape[1] - 16), tile)[0], shape, tile, 'images')            # the wrong width
    _refused(_blob(36, 1, 67, shape, tile, length=LENGTH + 1)[0], shape, tile, 'truncated unary length')
    _refused(_blob(37, 1, 67, shape, tile, learned=True)[0], shape, tile, 'other kind of model')
    _refused([good]*(BATCH + 1), shape, tile, 'images')                                              # too many images
    _refused(_blob(38, 3, -1, shape, tile)[0], shape, tile, 'images', batch=2)
    _refused([good, good], shape, tile, 'payload', capacity=2*len(parts['payload']) - 1)             # a payload beyond capacity
    _refused(good[:-1], shape, tile)                                                                 # a truncated blob
    _refused(good[:40], shape, tile)
    _refused([], shape, tile)
    (head, payload, layout) = _buffers(shape, tile, 1 << 17)
    with pytest.raises(ValueError, match='coding_tile'):
        _plan(good, shape, (0, 2), head, payload)                                                    # no tile at all
    assert (head == 0xA5).all() and (payload == 0xA5).all()


@pytest.mark.parametrize('shape,tile,nb_classes', CASES)
def test_without_coding_tile_an_eat1_blob_is_still_refused(shape, tile, nb_classes):
    (tiled, _) = _blob(50, 1, 67, shape, tile)
    (_, head_bytes) = codec.decode_head_layout(BATCH, NB_MAPS, LENGTH)
    (head, payload) = (numpy.full(head_bytes, 0xA5, dtype=numpy.uint8), numpy.full(1 << 17, 0xA5, dtype=numpy.uint8))
    for arguments in ({}, {'coding_tile': None}):
        with pytest.raises(ValueError, match='decode_region'):
            codec.plan_decode_step(tiled, BATCH, shape[0], shape[1], LENGTH, False, payload.size, head, payload, **arguments)
        assert (head == 0xA5).all() and (payload == 0xA5).all()
    # and an EAE1 blob fills the untiled head whether or not the keyword is spelt out
    (plain, parts) = _blob(51, 2, 67, shape, tile, eae1=True)
    assert codec.plan_decode_step(plain, BATCH, shape[0], shape[1], LENGTH, False, payload.size, head, payload, coding_tile=None) == (2, len(parts['payload']))
    views = codec.decode_head_views(head, BATCH, NB_MAPS, LENGTH)
    assert numpy.array_equal(views['bits'][:2*NB_MAPS], parts['bits'].reshape(-1, 2)) and (views['prob_row'][2*NB_MAPS:] == -1).all()
