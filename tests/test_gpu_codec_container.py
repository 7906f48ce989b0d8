"""`codec.BatchCodec(emit_container=True)`: the pipelined codec hands out the `EAE1` containers of its steps, byte-identical to
`container.encode_images` on the same images, with the offsets, the packing and the exception maps' probability rows formed on the
device (csrc/hip/codec_container.hip). The four kernels first, each against numpy, then the codec end to end in its three launch
modes, the overflow of the payload buffer, and the refused arguments."""
import os
import types

import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _guarded_buffers():
    """Every test of this module runs on poisoned buffers between guard bands: what device.py / pipeline.py allocate holds 0xFF bytes
    (NaN, -1) until a kernel writes it, and a byte written outside a tensor fails the test (tests/guarded.py)."""
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), 0xFF):
        yield


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coder_golden.npz')


def _bits_tensor(bits_uint32):
    return torch.from_numpy(numpy.ascontiguousarray(bits_uint32, dtype=numpy.uint32).view(numpy.int32)).cuda()


def _fake_streams(bac, bypass, stride, regions=None):
    """What the index / pack wrappers read of a device.CoderStreams."""
    return types.SimpleNamespace(n_maps=len(bac), stride=stride, bac_bits=_bits_tensor(bac), bypass_bits=_bits_tensor(bypass), streams=regions)


def _piece_lengths(bac, bypass, stride):
    bits = numpy.stack([bac, bypass], axis=1).astype(numpy.uint64).reshape(-1)
    return numpy.minimum((bits + numpy.uint64(7)) >> numpy.uint64(3), numpy.uint64(stride//2))


def _index_reference(bac, bypass, stride, maps_per_image, capacity):
    lengths = _piece_lengths(bac, bypass, stride)
    offsets = numpy.cumsum(lengths, dtype=numpy.uint64) - lengths
    total = int(lengths.sum(dtype=numpy.uint64))
    per_image = lengths.reshape(-1, 2*maps_per_image).sum(axis=1, dtype=numpy.uint64)
    index = numpy.concatenate([numpy.array([total, 1 if total > capacity else 0], dtype=numpy.uint64), per_image])
    return offsets, index, total


def _check_index(bac, bypass, stride, maps_per_image):
    from autoencoder_based_image_compression_amd import device as dev
    streams = _fake_streams(bac, bypass, stride)
    (_, _, total) = _index_reference(bac, bypass, stride, maps_per_image, 0)
    for capacity in (total, total - 1):
        if capacity < 0:
            continue
        (offsets_ref, index_ref, _) = _index_reference(bac, bypass, stride, maps_per_image, capacity)
        (offsets, index) = dev.coder_index_streams(streams, maps_per_image, capacity)
        assert offsets.shape == (len(bac), 2) and index.shape == (2 + len(bac)//maps_per_image,)
        assert numpy.array_equal(offsets.cpu().numpy().view(numpy.uint64).reshape(-1), offsets_ref), (len(bac), capacity)
        assert numpy.array_equal(index.cpu().numpy().view(numpy.uint64), index_ref), (len(bac), capacity)
        assert int(index_ref[1]) == (0 if capacity == total else 1)
    return total


@pytest.mark.parametrize('n_maps', [1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 3072, 20000])
def test_index_streams_equals_numpy(n_maps):
    """Every chunk boundary of the one-block scan (1,024 entries = 512 maps per chunk, 32 maps per wavefront), more than one chunk,
    one map per image and 128; a fifth of the counts zero, a fifth whole bytes, some beyond the clamp."""
    rng = numpy.random.RandomState(n_maps)
    stride = 96
    counts = rng.randint(1, 8*stride//2 + 1, size=(2, n_maps)).astype(numpy.uint32)
    kind = rng.rand(2, n_maps)
    counts[kind < 0.2] = 0
    whole = (kind >= 0.2) & (kind < 0.4)
    counts[whole] = counts[whole]//8*8
    beyond = kind > 0.9
    counts[beyond] = 4*stride + rng.randint(0, 1000, size=int(beyond.sum())).astype(numpy.uint32)
    assert (counts > 8*(stride//2)).any() or n_maps < 8
    maps_per_image = 128 if n_maps % 128 == 0 else 1
    _check_index(counts[0], counts[1], stride, maps_per_image)


def test_index_streams_clamp_zeros_and_totals_beyond_32_bits():
    from autoencoder_based_image_compression_amd import device as dev
    # all clamped; all empty (total 0: capacity = total - 1 does not exist)
    assert _check_index(numpy.full(70, 10**6, dtype=numpy.uint32), numpy.full(70, 4*64 + 1, dtype=numpy.uint32), 64, 1) == 140*32
    assert _check_index(numpy.zeros(128, dtype=numpy.uint32), numpy.zeros(128, dtype=numpy.uint32), 64, 128) == 0
    # 128 pieces of 2^29 bytes: the offsets pass 2^32 inside one wavefront's scan; nothing is copied, so no memory is needed
    rng = numpy.random.RandomState(0)
    near = (numpy.uint64(2**32 - 1) - rng.randint(0, 7, size=(2, 64)).astype(numpy.uint64)).astype(numpy.uint32)
    total = _check_index(near[0], near[1], 2**32, 1)
    assert total == 128*2**29 and total > 2**32
    # refusals: before anything is launched
    streams = _fake_streams(near[0], near[1], 64)
    with pytest.raises(dev.HipError):
        dev.coder_index_streams(streams, 3, 0)                      # 64 % 3
    with pytest.raises(dev.HipError):
        dev.coder_index_streams(streams, 1, 0, offsets=torch.zeros(5, dtype=torch.int64, device='cuda'))


def _pieces_summing_to(rng, total, pieces, most):
    lengths = numpy.zeros(pieces, dtype=numpy.int64)
    left = total
    for e in rng.permutation(pieces):
        lengths[e] = min(left, int(rng.randint(0, most + 1)))
        left -= lengths[e]
    for e in range(pieces):                       # whatever the draws left over
        take = min(left, most - lengths[e])
        lengths[e] += take
        left -= take
    assert left == 0 and lengths.max(initial=0) <= most
    return lengths


@pytest.mark.parametrize('total', [0, 1, 15, 16, 17, 3001])
def test_pack_indexed_and_publish_prefix(total):
    """index -> pack -> publish, as a step of the codec chains them: the pinned destination holds the numpy-assembled payload, and
    nothing from the rounded-up length on; with the overflow flag set the payload buffer is untouched."""
    from autoencoder_based_image_compression_amd import device as dev
    rng = numpy.random.RandomState(total)
    (n_maps, stride, capacity) = (130, 64, 130*64)
    lengths = _pieces_summing_to(rng, total, 2*n_maps, stride//2)
    bits = numpy.where(lengths > 0, 8*lengths - rng.randint(0, 8, size=lengths.shape), 0).astype(numpy.uint32).reshape(n_maps, 2)
    regions = rng.randint(0, 256, size=(n_maps, stride)).astype(numpy.uint8)
    expected = b''.join(regions[m, piece*(stride//2):piece*(stride//2) + lengths[2*m + piece]].tobytes()
                        for m in range(n_maps) for piece in range(2))
    assert len(expected) == total
    streams = _fake_streams(bits[:, 0], bits[:, 1], stride, torch.from_numpy(regions).cuda())
    payload = torch.full((capacity,), 0x5A, dtype=torch.uint8, device='cuda')
    pinned = torch.full((capacity,), 0xA5, dtype=torch.uint8).pin_memory()
    (offsets, index) = dev.coder_index_streams(streams, 1, capacity)
    dev.coder_pack_indexed(streams, offsets, index, payload)
    dev.publish_prefix(payload, pinned, index[0:1])
    torch.cuda.synchronize()
    host = pinned.numpy()
    rounded = -(-total//16)*16
    assert int(index[0].item()) == total and int(index[1].item()) == 0
    assert host[:total].tobytes() == expected
    assert (host[rounded:] == 0xA5).all()
    assert (payload.cpu().numpy()[total:] == 0x5A).all()
    if total == 0:
        return
    # overflow: the flag is set and nothing is packed; what the publication then copies (the length's prefix of the buffer, cut at the
    # capacity the buffers have) holds no byte of the streams, and stops where it has to
    payload.fill_(0x5A)
    pinned.fill_(0xA5)
    (offsets, index) = dev.coder_index_streams(streams, 1, total - 1)
    dev.coder_pack_indexed(streams, offsets, index, payload)
    dev.publish_prefix(payload, pinned, index[0:1])
    torch.cuda.synchronize()
    assert int(index[0].item()) == total and int(index[1].item()) == 1
    assert (payload.cpu().numpy() == 0x5A).all()
    assert (pinned.numpy()[:rounded] == 0x5A).all() and (pinned.numpy()[rounded:] == 0xA5).all()


def test_publish_prefix_stops_at_the_capacity_and_checks_its_arguments():
    from autoencoder_based_image_compression_amd import device as dev
    source = torch.arange(256, dtype=torch.uint8, device='cuda').repeat(4)                  # 1,024 bytes
    pinned = torch.full((1024,), 0xA5, dtype=torch.uint8).pin_memory()
    dev.publish_prefix(source, pinned, torch.tensor([10**12], dtype=torch.int64, device='cuda'))      # a length beyond the buffers
    torch.cuda.synchronize()
    assert numpy.array_equal(pinned.numpy(), source.cpu().numpy())
    with pytest.raises(dev.HipError):
        dev.publish_prefix(source[:1000], pinned[:1000], torch.zeros(1, dtype=torch.int64, device='cuda'))      # 1000 % 16
    with pytest.raises(dev.HipError):
        dev.publish_prefix(source, torch.zeros(1024, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64, device='cuda'))
    with pytest.raises(dev.HipError):
        dev.publish_prefix(source[16:], pinned[8:1016], torch.zeros(1, dtype=torch.int64, device='cuda'))     # destination off by 8


def _rows_reference(hist, overflow, map_size, length):
    """container._exception_rows' arithmetic on a histogram over [-R, R] plus the count of the symbols beyond it."""
    from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats
    radius = (hist.shape[1] - 1)//2
    rows = numpy.zeros((hist.shape[0], length), dtype=numpy.float64)
    for i in range(hist.shape[0]):
        hist_abs = numpy.concatenate([hist[i, radius:].astype(numpy.int64), [int(overflow[i])]])
        hist_abs[1:radius + 1] += hist[i, :radius][::-1]
        (zeros, ones) = lossless_stats._decisions_from_hist(hist_abs, length)
        assert int(zeros[0] + ones[0]) == map_size
        with numpy.errstate(invalid='ignore', divide='ignore'):
            p = zeros.astype(numpy.float64)/(zeros + ones).astype(numpy.float64)
        p[numpy.isnan(p)] = 0.5
        p[p == 0.] = 0.01
        p[p == 1.] = 0.99
        rows[i] = p
    return rows


@pytest.mark.parametrize('length', [1, 10, 32, 255])
def test_exception_rows_equal_the_host_rows(length):
    """Real histograms (`dev.symbol_histograms` of synthetic maps, at radius 2047 and at radius L) against
    `container._exception_rows` on the same symbols, and synthetic histograms against the same arithmetic in numpy, as int64 views."""
    from autoencoder_based_image_compression_amd import container
    from autoencoder_based_image_compression_amd import device as dev
    rng = numpy.random.RandomState(length)
    map_size = 1536
    maps = numpy.zeros((7, 1, map_size), dtype=numpy.int16)
    maps[1] = rng.randint(-3, 4, size=map_size)                                   # small magnitudes
    maps[2] = rng.randint(-300, 301, size=map_size)                               # every position of a long prefix
    maps[3] = numpy.where(rng.rand(map_size) < 0.5, 1, -1)*rng.randint(length, length + 40, size=map_size)      # every |s| >= L
    maps[4] = rng.randint(-3000, 3001, size=map_size)                             # beyond the radius of 2047
    maps[5] = numpy.round(rng.laplace(scale=2., size=map_size))
    maps[6, 0, :7] = (length - 1, -(length - 1), length, -length, 32767, -32767, 0)      # the last position, and the far ends
    symbols = torch.from_numpy(maps).cuda()
    expected = container._exception_rows(symbols, 0, length)
    assert numpy.array_equal(expected[0], numpy.r_[0.99, numpy.full(length - 1, 0.5)])          # an all-zero map
    assert (expected[3] == 0.01).all()
    for radius in (2047, length):
        (hist, overflow) = dev.symbol_histograms(symbols, radius)
        assert int(overflow.sum().item()) > 0
        rows = dev.exception_rows(hist, overflow, map_size, length)
        assert rows.shape == (7, length) and rows.dtype == torch.float64
        assert numpy.array_equal(rows.cpu().numpy().view(numpy.int64), expected.view(numpy.int64)), radius
    # synthetic histograms: counts that no map of this size is needed for, at the smallest radius allowed
    hist = rng.randint(0, 50, size=(5, 2*length + 1)).astype(numpy.int32)
    hist[0] = 0
    hist[1, length] = 0                                                           # no zero symbol: p[0] = 0 -> 0.01
    overflow = rng.randint(0, 1000, size=5).astype(numpy.int32)
    overflow[2] = 0
    big = int(hist.sum(axis=1).max() + overflow.max())
    hist[:, 0] += (big - hist.sum(axis=1) - overflow).astype(numpy.int32)         # the same map size for all five
    out = torch.full((5, length), -1., dtype=torch.float64, device='cuda')
    rows = dev.exception_rows(torch.from_numpy(hist).cuda(), torch.from_numpy(overflow).cuda(), big, length, out=out)
    assert rows is out
    assert numpy.array_equal(rows.cpu().numpy().view(numpy.int64), _rows_reference(hist, overflow, big, length).view(numpy.int64))
    with pytest.raises(dev.HipError):                                             # radius L - 1
        dev.exception_rows(torch.zeros((1, 2*length - 1), dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'),
                           map_size, length)


# ---- end to end ---------------------------------------------------------------------------------------------------------------

KEYS = ('nb_bits', 'coder_bits', 'exception_bits', 'sse', 'nb_deads')
MODES = {'launches': {}, 'graphs': {'use_graphs': True, 'nb_transform_streams': 2},
         'one_stream': {'use_graphs': True, 'one_stream_steps': True}}


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


def _references(model, shape, scale, idx_map_exception):
    """Once per (shape, bin width, exception map), shared by the three launch modes: per batch, the blobs of
    `container.encode_images` (the batch's and every image's), `decode_images` of the batch's blob, and the results of a twin codec
    built without `emit_container`."""
    from autoencoder_based_image_compression_amd import codec, container
    key = (shape, scale, idx_map_exception)
    if key in model['references']:
        return model['references'][key]
    bin_widths = numpy.full(128, scale, dtype=numpy.float32)
    map_mean = numpy.random.RandomState(shape[2]).normal(scale=0.1, size=128).astype(numpy.float32)
    arguments = (model['encoder'], bin_widths, map_mean, model['probabilities'], idx_map_exception)
    twin = codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], idx_map_exception, *shape)
    out = []
    for images in _batches(shape):
        (blob, info) = container.encode_images(images, *arguments)
        out.append({'images': torch.from_numpy(images).cuda(), 'blob': blob, 'payload_bytes': info['payload_bytes'],
                    'image_blobs': [container.encode_images(images[i:i + 1], *arguments)[0] for i in range(shape[0])],
                    'decoded': container.decode_images(blob, model['decoder']),
                    'twin': twin.submit(torch.from_numpy(images).cuda()).result()})
    twin.close()
    sizes = [r['payload_bytes'] for r in out]
    print('payload bytes of the four batches:', sizes)
    assert len(set(sizes)) == 4                          # every step of a run has another payload size than the one before
    model['references'][key] = (bin_widths, map_mean, out)
    return model['references'][key]


def _check_step(ticket, reference, with_container=True):
    r = ticket.result()
    for key in KEYS:
        assert numpy.array_equal(r[key], reference['twin'][key]), key
    assert set(r) == set(KEYS) | {'container_bytes'}
    assert r['container_bytes'].dtype == numpy.int64 and int(r['container_bytes'].sum()) == reference['payload_bytes']
    if with_container:
        assert ticket.container() == reference['blob']
        assert ticket.image_containers() == reference['image_blobs']
        assert numpy.array_equal(ticket.reconstruction_uint8.cpu().numpy(), reference['decoded'])


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('idx_map_exception', [67, -1])
@pytest.mark.parametrize('shape,scale', [((2, 64, 96), 0.5), ((3, 48, 80), 0.05)])
def test_tickets_hold_the_containers_encode_images_writes(model, shape, scale, idx_map_exception, mode):
    """More steps than slots, three in flight, payload sizes that change from step to step: every slot is reused and (in the graph
    modes) every graph replayed with another payload size. Per step: the batch's blob and every image's equal
    `container.encode_images`' byte for byte, `decode_images` of it is the ticket's reconstruction, the results are the twin's."""
    from autoencoder_based_image_compression_amd import codec
    (bin_widths, map_mean, references) = _references(model, shape, scale, idx_map_exception)
    # (these random weights code the small bin width at more than the default capacity's 8 bits per pixel)
    pixels = shape[0]*shape[1]*shape[2]
    capacity = {} if scale == 0.5 else {'container_capacity_bytes': 4*pixels - 3}
    c = codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], idx_map_exception, *shape,
                         keep_reconstruction=True, emit_container=True, **capacity, **MODES[mode])
    try:
        assert c.container_capacity_bytes == (-(-pixels//16)*16 if scale == 0.5 else -(-(4*pixels - 3)//16)*16)
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


def test_payload_beyond_the_capacity(model):
    """A step whose payload does not fit keeps its results and says so from `container()`; the steps around it, on the same slots,
    are not disturbed, and `close()` returns."""
    from autoencoder_based_image_compression_amd import codec
    shape = (2, 64, 96)
    (bin_widths, map_mean, references) = _references(model, shape, 0.5, 67)
    c = codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], 67, *shape, emit_container=True,
                         container_capacity_bytes=16)
    assert c.container_capacity_bytes == 16
    for which in (1, 0, 1):
        ticket = c.submit(references[which]['images'])
        with pytest.raises(codec.ContainerOverflow):
            ticket.container()
        with pytest.raises(codec.ContainerOverflow):
            ticket.image_containers()
        _check_step(ticket, references[which], with_container=False)
    c.close()
    # a capacity the smallest batch's payload just fits: it comes through between overflowing steps, on slots those have used
    by_size = sorted(range(4), key=lambda which: references[which]['payload_bytes'])
    (fits, large, larger) = (by_size[0], by_size[2], by_size[3])
    small = references[fits]['payload_bytes']
    assert -(-small//16)*16 < references[large]['payload_bytes']
    c = codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], 67, *shape, emit_container=True,
                         container_capacity_bytes=small)
    tickets = [(c.submit(references[which]['images']), which) for which in [larger, fits, large, fits]*(c.nb_slots//2 + 1)]
    for (ticket, which) in tickets:
        if which == fits:
            assert ticket.container() == references[fits]['blob'] and ticket.image_containers() == references[fits]['image_blobs']
        else:
            with pytest.raises(codec.ContainerOverflow):
                ticket.container()
        _check_step(ticket, references[which], with_container=False)
    c.close()
    # without `emit_container` a ticket has no container to give
    plain = codec.BatchCodec(model['variables'], False, bin_widths, map_mean, model['probabilities'], 67, *shape)
    ticket = plain.submit(references[0]['images'])
    assert 'container_bytes' not in ticket.result()
    with pytest.raises(RuntimeError):
        ticket.container()
    plain.close()


def test_refused_arguments(model):
    from autoencoder_based_image_compression_amd import codec
    ones = numpy.ones(128, dtype=numpy.float32)
    probabilities = model['probabilities']
    length = probabilities.shape[1]
    arguments = (model['variables'], False, ones, 0*ones, probabilities)
    for coder in ('host', 'none'):
        with pytest.raises(ValueError, match='emit_container'):
            codec.BatchCodec(*arguments, 67, 1, 64, 96, coder=coder, emit_container=True)
    with pytest.raises(ValueError, match='hist_radius'):
        codec.BatchCodec(*arguments, 67, 1, 64, 96, hist_radius=length - 1, emit_container=True)
    # the histogram is the exception map's: without one, and at radius L exactly, the codec is built
    for (idx_map_exception, radius) in ((-1, length - 1), (67, length)):
        c = codec.BatchCodec(*arguments, idx_map_exception, 1, 64, 96, hist_radius=radius, emit_container=True)
        ticket = c.submit(torch.full((1, 64, 96), 100, dtype=torch.uint8, device='cuda'))
        assert len(ticket.image_containers()) == 1 and ticket.image_containers()[0] == ticket.container()
        c.close()
