"""`codec.BatchCodec(emit_container=True, coding_tile=...)`: the pipelined codec codes every (image, tile, map) as its own pair of
streams and hands out the tile-indexed `EAT1` containers of its steps, byte-identical to `container.encode_images(..., coding_tile=...)`
on the same images. The index kernel first (`device.coder_index_tiles`, csrc/hip/codec_container.hip) against a numpy cumsum in payload
order, then the codec end to end in its three launch modes, the overflow of the payload buffer, and the refused arguments.
(`BatchCodec.submit` takes whole batches only, so there is no partial last step to handle.)"""
import ctypes
import os

import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _guarded_buffers():
    """Every test of this module runs on poisoned buffers between guard bands: what device.py / pipeline.py allocate holds 0xFF bytes
    (NaN, -1) until a kernel writes it, and a byte written outside a tensor fails the test (tests/guarded.py). The kernel tests
    upload their inputs through the guard as well."""
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), 0xFF) as guard:
        yield guard


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coder_golden.npz')


# ---- the index kernel -------------------------------------------------------------------------------------------------------------

def _tiles_reference(bac, bypass, table, maps_per_entry, entries_per_image, capacity):
    """bac / bypass uint32 [n_streams] in run order, table int64 [entries, 2] (run-order entry, half stride) in payload order ->
    (offsets uint64 [2 n_streams] in run order, index uint64 [2 + images], total): a cumsum in payload order of the clamped lengths."""
    entries = table.shape[0]
    bits = numpy.stack([bac, bypass], axis=1).astype(numpy.uint64).reshape(entries, 2*maps_per_entry)          # [run-order entry, piece]
    lengths = numpy.minimum((bits[table[:, 0]] + numpy.uint64(7)) >> numpy.uint64(3), table[:, 1].astype(numpy.uint64)[:, None])
    flat = lengths.reshape(-1)                                                                                  # payload order
    starts = numpy.cumsum(flat, dtype=numpy.uint64) - flat
    offsets = numpy.empty((entries, 2*maps_per_entry), dtype=numpy.uint64)
    offsets[table[:, 0]] = starts.reshape(entries, -1)
    total = int(flat.sum(dtype=numpy.uint64))
    per_image = lengths.reshape(entries//entries_per_image, -1).sum(axis=1, dtype=numpy.uint64)
    index = numpy.concatenate([numpy.array([total, 1 if total > capacity else 0], dtype=numpy.uint64), per_image])
    return offsets.reshape(-1), index, total


def _check_tiles(guard, bac, bypass, table, maps_per_entry, entries_per_image):
    """At capacity = total and total - 1: offsets and index words equal the reference, on poisoned outputs between guard bands."""
    from autoencoder_based_image_compression_amd import device as dev
    (bac_d, bypass_d) = (guard.upload(bac.view(numpy.int32)), guard.upload(bypass.view(numpy.int32)))
    table_d = guard.upload(table)
    (_, _, total) = _tiles_reference(bac, bypass, table, maps_per_entry, entries_per_image, 0)
    for capacity in (total, total - 1):
        if capacity < 0:
            continue
        (offsets_ref, index_ref, _) = _tiles_reference(bac, bypass, table, maps_per_entry, entries_per_image, capacity)
        (offsets, index) = dev.coder_index_tiles(bac_d, bypass_d, table_d, maps_per_entry, entries_per_image, capacity)
        assert offsets.shape == (len(bac), 2) and index.shape == (2 + table.shape[0]//entries_per_image,)
        assert numpy.array_equal(offsets.cpu().numpy().view(numpy.uint64).reshape(-1), offsets_ref), (table.shape[0], capacity)
        assert numpy.array_equal(index.cpu().numpy().view(numpy.uint64), index_ref), (table.shape[0], capacity)
        assert int(index_ref[1]) == (0 if capacity == total else 1)
        assert int(index_ref[2:].sum(dtype=numpy.uint64)) == total
    return total


def _counts(rng, half_strides, maps_per_entry):
    """Bit counts for entries whose half strides are `half_strides` (run order): a fifth zero, a fifth whole bytes, a tenth beyond
    the clamp of their own entry."""
    entries = len(half_strides)
    most = numpy.repeat(8*numpy.asarray(half_strides, dtype=numpy.int64), maps_per_entry)
    counts = (1 + rng.randint(0, 2**31 - 1, size=(2, entries*maps_per_entry)) % most[None, :]).astype(numpy.uint32)
    kind = rng.rand(2, entries*maps_per_entry)
    counts[kind < 0.2] = 0
    whole = (kind >= 0.2) & (kind < 0.4)
    counts[whole] = counts[whole]//8*8
    beyond = kind > 0.9
    counts[beyond] = (numpy.broadcast_to(most, counts.shape)[beyond] + 1 + rng.randint(0, 1000, size=int(beyond.sum()))).astype(numpy.uint32)
    return counts


@pytest.mark.parametrize('entries,entries_per_image,maps_per_entry', [(1, 1, 128), (2, 2, 128), (7, 1, 128), (7, 7, 128), (8, 4, 128), (9, 3, 128),
                                                                      (65, 5, 128), (600, 6, 128), (5, 1, 1), (6, 2, 300), (1030, 2, 2)])
def test_index_tiles_equals_numpy(_guarded_buffers, entries, entries_per_image, maps_per_entry):
    """The seams of the two-level scan: one block of 256 threads per entry (128 maps are exactly its 256 pieces; 300 maps take three
    rounds with a carry, one map leaves most of a wavefront idle), one block of 1,024 threads over the entries (7 / 8 / 9 around a
    wavefront's and 1,030 around the block's chunk). The entries are shuffled between payload and run order, and every entry
    draws one of four half strides of its own."""
    rng = numpy.random.RandomState(1000*entries + maps_per_entry)
    run_entry = rng.permutation(entries).astype(numpy.int64)
    if entries > 2:
        assert not numpy.array_equal(run_entry, numpy.arange(entries))
    half = numpy.array([24, 40, 136, 1032], dtype=numpy.int64)[rng.randint(0, 4, size=entries)]                # of payload-order entries
    table = numpy.stack([run_entry, half], axis=1)
    half_run = numpy.empty(entries, dtype=numpy.int64)
    half_run[run_entry] = half
    counts = _counts(rng, half_run, maps_per_entry)
    if entries*maps_per_entry >= 128:
        assert (counts == 0).any() and (counts.astype(numpy.int64) > 8*numpy.repeat(half_run, maps_per_entry)[None, :]).any()
    _check_tiles(_guarded_buffers, counts[0], counts[1], table, maps_per_entry, entries_per_image)


def test_index_tiles_with_the_table_of_a_step_of_four_classes(_guarded_buffers):
    """Three images of a 2 x 2 grid of tiles of four shapes: the table `BatchCodec` builds (run order from `coding_tile_layout`, half
    strides from the coder's own stream regions), which is no identity; bytes per image are the sums over the image's four tiles."""
    from autoencoder_based_image_compression_amd import codec
    from autoencoder_based_image_compression_amd import device as dev
    layout = codec.coding_tile_layout(3, 8, 12, (6, 8))
    assert len(layout['runs']) == 4 and layout['nb_tiles'] == 4 and layout['run_entry'].tolist() != list(range(12))
    sizes = [int(layout['tiles'][t, 2]*layout['tiles'][t, 3]) for (_, t) in layout['entries']]
    half = numpy.array([dev.coder_stream_stride_bytes(size, 10)//2 for size in sizes], dtype=numpy.int64)
    assert len(set(half.tolist())) == 4
    table = numpy.stack([layout['run_entry'], half], axis=1)
    half_run = numpy.empty(12, dtype=numpy.int64)
    half_run[layout['run_entry']] = half
    counts = _counts(numpy.random.RandomState(3), half_run, 128)
    _check_tiles(_guarded_buffers, counts[0], counts[1], table, 128, 4)


def test_index_tiles_totals_beyond_32_bits_zeros_and_the_identity(_guarded_buffers):
    from autoencoder_based_image_compression_amd import device as dev
    guard = _guarded_buffers
    # pieces of 2^29 bytes under half strides of 2^31 and 2^29 - 5: the offsets pass 2^32 inside one entry and between entries;
    # nothing is packed, so no memory is needed
    rng = numpy.random.RandomState(0)
    near = (numpy.uint64(2**32 - 1) - rng.randint(0, 7, size=(2, 3*128)).astype(numpy.uint64)).astype(numpy.uint32)
    table = numpy.array([[2, 2**31], [0, 2**29 - 5], [1, 2**31]], dtype=numpy.int64)
    total = _check_tiles(guard, near[0], near[1], table, 128, 1)
    assert total == 2*256*2**29 + 256*(2**29 - 5) and total > 2**32
    # all empty (total 0: capacity = total - 1 does not exist); all clamped
    zeros = numpy.zeros(2*128, dtype=numpy.uint32)
    assert _check_tiles(guard, zeros, zeros, numpy.array([[1, 32], [0, 32]], dtype=numpy.int64), 128, 2) == 0
    full = numpy.full(2*128, 10**6, dtype=numpy.uint32)
    assert _check_tiles(guard, full, full, numpy.array([[1, 32], [0, 48]], dtype=numpy.int64), 128, 1) == 256*(32 + 48)
    # one entry per image, the identity table and one stride: `coder_index_streams`, word for word
    import types
    for n_images in (1, 5, 24):
        stride = 96
        counts = _counts(rng, numpy.full(n_images, stride//2, dtype=numpy.int64), 128)
        (bac_d, bypass_d) = (guard.upload(counts[0].view(numpy.int32)), guard.upload(counts[1].view(numpy.int32)))
        streams = types.SimpleNamespace(n_maps=128*n_images, stride=stride, bac_bits=bac_d, bypass_bits=bypass_d, streams=None)
        table_d = guard.upload(numpy.stack([numpy.arange(n_images, dtype=numpy.int64), numpy.full(n_images, stride//2, dtype=numpy.int64)], axis=1))
        (_, _, total) = _tiles_reference(counts[0], counts[1], numpy.stack([numpy.arange(n_images), numpy.full(n_images, stride//2)], axis=1), 128, 1, 0)
        for capacity in (total, total - 1):
            (offsets_s, index_s) = dev.coder_index_streams(streams, 128, capacity)
            (offsets_t, index_t) = dev.coder_index_tiles(bac_d, bypass_d, table_d, 128, 1, capacity)
            assert torch.equal(offsets_s, offsets_t) and torch.equal(index_s, index_t), (n_images, capacity)
            assert int(index_t[1].item()) == (0 if capacity == total else 1)


def test_index_tiles_refuses_its_arguments_before_any_launch():
    """The codes come from the entry point's own checks: the pointers are host memory no kernel could take."""
    from autoencoder_based_image_compression_amd import _native
    from autoencoder_based_image_compression_amd import device as dev
    lib = _native.hip()
    buffer = (ctypes.c_uint64*64)()
    p = ctypes.cast(buffer, ctypes.c_void_p)
    (bad_argument, bad_shape) = (-1, -2)
    for k in range(5):                                              # every pointer in turn
        pointers = [p]*5
        pointers[k] = None
        assert lib.eae_hip_coder_index_tiles(256, 128, 2, pointers[0], pointers[1], pointers[2], 0, pointers[3], pointers[4], None) == bad_argument
    assert lib.eae_hip_coder_index_tiles(0, 128, 1, p, p, p, 0, p, p, None) == bad_argument
    assert lib.eae_hip_coder_index_tiles(256, 0, 1, p, p, p, 0, p, p, None) == bad_argument
    assert lib.eae_hip_coder_index_tiles(256, 128, 0, p, p, p, 0, p, p, None) == bad_argument
    assert lib.eae_hip_coder_index_tiles(200, 128, 1, p, p, p, 0, p, p, None) == bad_shape          # no whole entry
    assert lib.eae_hip_coder_index_tiles(384, 128, 2, p, p, p, 0, p, p, None) == bad_shape          # three entries, two per image
    # the wrapper says the same in front of the library
    counts = torch.zeros(384, dtype=torch.int32, device='cuda')
    table = torch.zeros((3, 2), dtype=torch.int64, device='cuda')
    with pytest.raises(dev.HipError):
        dev.coder_index_tiles(counts, counts, table, 128, 2, 0)
    with pytest.raises(dev.HipError):
        dev.coder_index_tiles(counts, counts, table[:2], 128, 1, 0)
    with pytest.raises(dev.HipError):
        dev.coder_index_tiles(counts, counts, table, 128, 1, 0, offsets=torch.zeros(5, dtype=torch.int64, device='cuda'))


# ---- end to end ---------------------------------------------------------------------------------------------------------------

KEYS = ('nb_bits', 'coder_bits', 'exception_bits', 'sse', 'nb_deads')
MODES = {'launches': {}, 'graphs': {'use_graphs': True, 'nb_transform_streams': 2},
         'one_stream': {'use_graphs': True, 'one_stream_steps': True}}
CASES = [((2, 64, 96), 0.5, (2, 3)), ((2, 64, 96), 0.5, (3, 4)), ((2, 64, 96), 0.5, (100, 100)), ((3, 48, 80), 0.05, (2, 2))]
REGION = (17, 30, 40, 50)          # (y0, x0, height, width): the crop `decode_region` takes out of the (3, 4) case


@pytest.fixture(scope='module')
def model():
    from autoencoder_based_image_compression_amd import pipeline
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    v = var.random_variables(1., False, seed=4, bias_std=0.01)
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    with numpy.load(GOLD) as g:
        probabilities = g['real_probabilities_1']
    return {'variables': v, 'encoder': pipeline.DeviceEncoder(v, False), 'decoder': pipeline.DeviceDecoder(v, False),
            'probabilities': probabilities, 'references': {}}


def _batches(shape):
    """Four batches of different entropy: a constant image, uniform noise, a ramp with a little noise, and a mix of the three."""
    rng = numpy.random.RandomState(shape[1])
    (n, h, w) = shape
    constant = numpy.full(shape, 128, dtype=numpy.uint8)
    noise = rng.randint(16, 236, size=shape).astype(numpy.uint8)
    ramp = numpy.broadcast_to((16 + 219*numpy.arange(w)/(w - 1))[None, None, :], shape)
    ramp = numpy.clip(ramp + rng.randint(-4, 5, size=shape), 16, 235).astype(numpy.uint8)
    mixed = numpy.stack([(constant, noise, ramp)[i % 3][i] for i in range(n)])
    return [constant, noise, ramp, mixed]


def _capacity(shape):
    """Payload bytes a step of the tests may take: 8 bytes per pixel. (Every stream of every tile pays its own termination and byte
    padding, and these random weights code the small bin width at more than 8 bits per pixel as whole maps already.)"""
    return 8*shape[0]*shape[1]*shape[2]


def _references(model, shape, scale, idx_map_exception, tile):
    """Once per (shape, bin width, exception map, coding tile), shared by the three launch modes: per batch, the blobs of
    `container.encode_images(..., coding_tile=tile)` (the batch's and every image's) and its `info`, `decode_images` of the batch's
    blob (and one `decode_region` crop of the (3, 4) case), and the results of a twin codec with `emit_container` but no coding tile."""
    from autoencoder_based_image_compression_amd import codec, container
    key = (shape, scale, idx_map_exception, tile)
    if key in model['references']:
        return model['references'][key]
    bin_widths = numpy.full(128, scale, dtype=numpy.float32)
    map_mean = numpy.random.RandomState(shape[2]).normal(scale=0.1, size=128).astype(numpy.float32)
    arguments = (model['encoder'], bin_widths, map_mean, model['probabilities'], idx_map_exception)
    twin = codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], idx_map_exception, *shape,
                            emit_container=True, container_capacity_bytes=_capacity(shape))
    out = []
    for images in _batches(shape):
        (blob, info) = container.encode_images(images, *arguments, coding_tile=tile)
        assert blob[:4] == b'EAT1'
        tile_bits = info['tile_bits'].astype(numpy.int64)                      # [N, nb_tiles, 128, 2]
        coded = tile_bits.sum(axis=3)
        if idx_map_exception >= 0:
            coded[:, :, idx_map_exception] = 0
        reference = {'images': torch.from_numpy(images).cuda(), 'blob': blob, 'payload_bytes': info['payload_bytes'],
                     'image_blobs': [container.encode_images(images[i:i + 1], *arguments, coding_tile=tile)[0] for i in range(shape[0])],
                     'decoded': container.decode_images(blob, model['decoder']),
                     'coder_bits': coded.sum(axis=(1, 2)), 'container_bytes': ((tile_bits + 7)//8).sum(axis=(1, 2, 3)),
                     'twin': twin.submit(torch.from_numpy(images).cuda()).result()}
        if tile == (3, 4):
            reference['region'] = container.decode_region(blob, model['decoder'], REGION)
        out.append(reference)
    twin.close()
    sizes = [r['payload_bytes'] for r in out]
    print('payload bytes of the four batches:', sizes, 'capacity', _capacity(shape))
    assert len(set(sizes)) == 4 and max(sizes) <= _capacity(shape)      # every step of a run has another payload size than the one before
    model['references'][key] = (bin_widths, map_mean, out)
    return model['references'][key]


def _check_step(ticket, reference, with_container=True):
    r = ticket.result()
    assert set(r) == set(KEYS) | {'container_bytes'}
    for key in ('sse', 'nb_deads', 'exception_bits'):                          # those of the same codec without a coding tile
        assert numpy.array_equal(r[key], reference['twin'][key]), key
    assert r['coder_bits'].dtype == numpy.int64 and numpy.array_equal(r['coder_bits'], reference['coder_bits'])
    assert numpy.array_equal(r['nb_bits'], reference['coder_bits'] + reference['twin']['exception_bits'])
    assert r['container_bytes'].dtype == numpy.int64 and numpy.array_equal(r['container_bytes'], reference['container_bytes'])
    assert int(r['container_bytes'].sum()) == reference['payload_bytes']
    if with_container:
        assert ticket.container() == reference['blob']
        assert ticket.image_containers() == reference['image_blobs']
        reconstruction = ticket.reconstruction_uint8.cpu().numpy()
        assert numpy.array_equal(reconstruction, reference['decoded'])
        if 'region' in reference:
            (y0, x0, height, width) = REGION
            assert numpy.array_equal(reference['region'], reconstruction[:, y0:y0 + height, x0:x0 + width])


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('idx_map_exception', [67, -1])
@pytest.mark.parametrize('shape,scale,tile', CASES)
def test_tickets_hold_the_containers_encode_images_writes(model, shape, scale, tile, idx_map_exception, mode):
    """More steps than slots, three in flight, payload sizes that change from step to step: every slot is reused and (in the graph
    modes) every graph replayed with another payload size. One class of tiles, all four classes (with a 1 x 1 tile at the corner of
    the 3 x 5 plane), and a tile clamped to the plane (EAE1's payload behind EAT1's header). Per step: the batch's blob and every
    image's equal `container.encode_images(..., coding_tile=tile)`'s byte for byte, `decode_images` of it is the ticket's
    reconstruction, the bit counts are the sums of `info['tile_bits']`, everything else is the twin's."""
    from autoencoder_based_image_compression_amd import codec
    (bin_widths, map_mean, references) = _references(model, shape, scale, idx_map_exception, tile)
    c = codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], idx_map_exception, *shape,
                         keep_reconstruction=True, emit_container=True, coding_tile=tile, container_capacity_bytes=_capacity(shape),
                         **MODES[mode])
    try:
        assert c.coding_tile == (min(tile[0], shape[1]//16), min(tile[1], shape[2]//16))
        steps = [(0, 1, 2, 3, 1, 0, 3, 2, 2, 1, 0)[k % 11] for k in range(c.nb_slots + 3)]
        window = []
        for (k, which) in enumerate(steps):
            window.append((c.submit(references[which]['images']), which))
            if len(window) == 3 or k == len(steps) - 1:
                # a ticket's reconstruction is its step's until the slot comes up again, nb_slots >= 3 submits later
                while window:
                    (ticket, done) = window.pop(0)
                    if k % 2:
                        assert ticket.container() == references[done]['blob']          # container() in front of result()
                    _check_step(ticket, references[done])
    finally:
        c.close()


def test_launch_hook_sees_the_coder_once_per_class(model):
    from autoencoder_based_image_compression_amd import codec
    shape = (2, 64, 96)
    (bin_widths, map_mean, references) = _references(model, shape, 0.5, 67, (3, 4))
    seen = []

    def hook(name, fn):
        seen.append(name)
        return fn()

    c = codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], 67, *shape, keep_reconstruction=True,
                         emit_container=True, coding_tile=(3, 4), container_capacity_bytes=_capacity(shape), launch_hook=hook)
    try:
        _check_step(c.submit(references[1]['images']), references[1])
    finally:
        c.close()
    assert [name for name in seen if name.startswith('coder')] == ['coder_encode', 'coder_decode']*4


def test_payload_beyond_the_capacity(model):
    """A capacity the smallest batch's payload just fits: it comes through between overflowing steps, on slots those have used; a
    step whose payload does not fit keeps its results and says so from `container()` only."""
    from autoencoder_based_image_compression_amd import codec
    (shape, tile) = ((2, 64, 96), (3, 4))
    (bin_widths, map_mean, references) = _references(model, shape, 0.5, 67, tile)
    by_size = sorted(range(4), key=lambda which: references[which]['payload_bytes'])
    (fits, large, larger) = (by_size[0], by_size[2], by_size[3])
    small = references[fits]['payload_bytes']
    assert -(-small//16)*16 < references[large]['payload_bytes']
    c = codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], 67, *shape, emit_container=True,
                         coding_tile=tile, container_capacity_bytes=small)
    try:
        tickets = [(c.submit(references[which]['images']), which) for which in [larger, fits, large, fits]*(c.nb_slots//2 + 1)]
        for (ticket, which) in tickets:
            if which == fits:
                assert ticket.container() == references[fits]['blob'] and ticket.image_containers() == references[fits]['image_blobs']
            else:
                with pytest.raises(codec.ContainerOverflow):
                    ticket.container()
                with pytest.raises(codec.ContainerOverflow):
                    ticket.image_containers()
            _check_step(ticket, references[which], with_container=False)
    finally:
        c.close()


def test_refused_arguments(model):
    """Every refusal is a ValueError in front of the first allocation: nothing of the codec exists behind it."""
    from autoencoder_based_image_compression_amd import codec
    ones = numpy.ones(128, dtype=numpy.float32)
    arguments = (model['variables'], False, ones, 0*ones, model['probabilities'], 67)
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match='emit_container'):
        codec.BatchCodec(*arguments, 1, 64, 96, coding_tile=(2, 3))
    for coder in ('host', 'none'):
        with pytest.raises(ValueError):
            codec.BatchCodec(*arguments, 1, 64, 96, coder=coder, emit_container=True, coding_tile=(2, 3))
    with pytest.raises(ValueError, match='coder_chunks'):
        codec.BatchCodec(*arguments, 1, 64, 96, emit_container=True, coding_tile=(2, 3), coder_chunks=2)
    for bad in ((0, 3), (2, -1), (2,), (2, 3, 4), (2.0, 3), 4, 'ab', (True, 2), (65536, 2), (2, 70000)):
        with pytest.raises(ValueError, match='coding_tile'):
            codec.BatchCodec(*arguments, 1, 64, 96, emit_container=True, coding_tile=bad)
    # 256 x 256 tiles of one latent are one (image, tile) pair too many for a step; so are two images of half as many
    with pytest.raises(ValueError, match='65535'):
        codec.BatchCodec(*arguments, 1, 4096, 4096, emit_container=True, coding_tile=(1, 1))
    with pytest.raises(ValueError, match='65535'):
        codec.BatchCodec(*arguments, 2, 4096, 4096, emit_container=True, coding_tile=(1, 2))
    assert torch.cuda.memory_allocated() == before
    # the largest side the header holds is taken (and clamped to the plane)
    c = codec.BatchCodec(*arguments, 1, 64, 96, emit_container=True, coding_tile=(65535, 65535))
    try:
        assert c.coding_tile == (4, 6)
        ticket = c.submit(torch.full((1, 64, 96), 100, dtype=torch.uint8, device='cuda'))
        assert len(ticket.image_containers()) == 1 and ticket.image_containers()[0] == ticket.container()
        assert ticket.container()[:4] == b'EAT1'
    finally:
        c.close()
