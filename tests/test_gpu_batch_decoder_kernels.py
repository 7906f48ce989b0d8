"""The two launches of csrc/hip/codec_decode.hip, each alone, on poisoned buffers between guard bands (tests/guarded.py):
`eae_hip_fetch_prefix` against the bytes it was given, `eae_hip_dequantize_maps_rows` against `eae_hip_dequantize_maps` called image
by image, bit for bit."""
import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=[0xFF, 0x7F])
def guard(request):
    """Every test runs twice, on buffers poisoned with 0xFF (NaN, -1) and with 0x7F (3.4e38, 32639): what device.py allocates and
    what the tests allocate through the guard keeps the poison until a kernel writes it, and a byte written outside a tensor fails
    the test."""
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


@pytest.mark.parametrize('capacity', [64, 4096])
def test_fetch_prefix_copies_the_prefix_and_nothing_else(guard, capacity):
    from autoencoder_based_image_compression_amd import device as dev
    rng = numpy.random.RandomState(capacity)
    source = torch.from_numpy(rng.randint(0, 256, size=capacity).astype(numpy.uint8)).pin_memory()
    for nbytes in (0, 1, 15, 16, 17, capacity - 1, capacity, capacity + 5):
        destination = guard.full((capacity,), 0x5A, dtype=torch.uint8, device='cuda')
        length = guard.upload(numpy.array([nbytes], dtype=numpy.int64))
        dev.fetch_prefix(source, destination, length)
        torch.cuda.synchronize()
        got = destination.cpu().numpy()
        copied = min(nbytes, capacity)
        rounded = -(-copied//16)*16
        assert numpy.array_equal(got[:copied], source.numpy()[:copied]), nbytes
        assert numpy.array_equal(got[copied:rounded], source.numpy()[copied:rounded]), nbytes      # whole 16-byte words
        assert (got[rounded:] == 0x5A).all(), nbytes
        guard.check()


def test_fetch_prefix_refuses_misaligned_buffers_and_odd_capacities(guard):
    from autoencoder_based_image_compression_amd import _native
    from autoencoder_based_image_compression_amd import device as dev
    lib = _native.hip()
    source = torch.zeros(96, dtype=torch.uint8).pin_memory()
    destination = guard.full((96,), 0x5A, dtype=torch.uint8, device='cuda')
    length = guard.upload(numpy.array([64, 64], dtype=numpy.int64))
    stream = torch.cuda.current_stream().cuda_stream
    (src, dst, word) = (source.data_ptr(), destination.data_ptr(), length.data_ptr())
    assert src % 16 == 0 and dst % 16 == 0 and word % 8 == 0
    assert lib.eae_hip_fetch_prefix(src, dst, 64, word, stream) == 0
    for arguments in ((src + 4, dst, 64, word), (src, dst + 8, 64, word), (src, dst, 64, word + 4), (src, dst, 72, word), (src, dst, 15, word),
                      (None, dst, 64, word), (src, None, 64, word), (src, dst, 64, None)):
        assert lib.eae_hip_fetch_prefix(*arguments, stream) == -1, arguments            # EAE_HIP_BAD_ARGUMENT, nothing launched
    assert lib.eae_hip_fetch_prefix(src, dst, 0, word, stream) == 0                         # nothing to copy
    with pytest.raises(dev.HipError):
        dev.fetch_prefix(source[:72], destination[:72], length[:1])                         # not a multiple of 16
    with pytest.raises(dev.HipError):
        dev.fetch_prefix(source[:64], destination[:80], length[:1])                         # two sizes
    with pytest.raises(dev.HipError):
        dev.fetch_prefix(torch.zeros(64, dtype=torch.uint8), destination[:64], length[:1])  # not pinned
    with pytest.raises(dev.HipError):
        dev.fetch_prefix(source[:64], destination[1:65], length[:1])                        # misaligned
    torch.cuda.synchronize()
    got = destination.cpu().numpy()
    assert (got[:64] == 0).all() and (got[64:] == 0x5A).all()


@pytest.mark.parametrize('outputs', ['cq', 'shifted', 'both'])
@pytest.mark.parametrize('hw', [15, 24, 64, 65, 130])
def test_dequantize_maps_rows_equals_dequantize_maps_image_by_image(guard, hw, outputs):
    """Three images with three different rows, map sizes on both sides of the 64-pixel chunk edge, symbols that include +-32767 and
    0: every output equals `dequantize_maps` of that image with its row, as int32 patterns; an output that was not asked for is
    not made."""
    from autoencoder_based_image_compression_amd import device as dev
    rng = numpy.random.RandomState(hw)
    n = 3
    symbols = rng.randint(-300, 301, size=(n, 128, hw)).astype(numpy.int16)
    symbols[rng.rand(n, 128, hw) < 0.3] = 0
    symbols[:, ::7, 0] = 32767
    symbols[:, 3::7, hw - 1] = -32767
    symbols[1, :, hw//2] = rng.randint(-32767, 32768, size=128)
    bin_widths = numpy.stack([numpy.full(128, 1.0), numpy.full(128, 0.05), rng.uniform(0.01, 3., size=128)]).astype(numpy.float32)
    map_mean = rng.normal(scale=2., size=(n, 128)).astype(numpy.float32)
    map_mean[0, :5] = (0., -0., 1e-30, -1e30, 3.)
    (want_cq, want_shifted) = (outputs != 'shifted', outputs != 'cq')
    device_symbols = guard.upload(symbols)
    got = dev.dequantize_maps_rows(device_symbols, guard.upload(bin_widths), guard.upload(map_mean), want_cq=want_cq, want_shifted=want_shifted)
    assert (got['cq'] is not None) == want_cq and (got['shifted'] is not None) == want_shifted
    for i in range(n):
        reference = dev.dequantize_maps(device_symbols[i:i + 1], guard.upload(bin_widths[i]), guard.upload(map_mean[i]), want_cq=want_cq,
                                        want_shifted=want_shifted)
        for key in ('cq', 'shifted'):
            if got[key] is not None:
                assert got[key].shape == (n, hw, 128)
                assert numpy.array_equal(got[key][i].cpu().numpy().view(numpy.int32), reference[key][0].cpu().numpy().view(numpy.int32)), (key, i)
    # without means the shifted output is cq + 0, as `dequantize_maps` forms it
    plain = dev.dequantize_maps_rows(device_symbols, guard.upload(bin_widths), None, want_cq=True, want_shifted=True)
    for i in range(n):
        reference = dev.dequantize_maps(device_symbols[i:i + 1], guard.upload(bin_widths[i]), None, want_cq=True, want_shifted=True)
        for key in ('cq', 'shifted'):
            assert numpy.array_equal(plain[key][i].cpu().numpy().view(numpy.int32), reference[key][0].cpu().numpy().view(numpy.int32)), (key, i)


def test_dequantize_maps_rows_refuses_what_it_cannot_do(guard):
    from autoencoder_based_image_compression_amd import _native
    from autoencoder_based_image_compression_amd import device as dev
    lib = _native.hip()
    symbols = guard.upload(numpy.zeros((2, 128, 16), dtype=numpy.int16))
    rows = guard.upload(numpy.ones((2, 128), dtype=numpy.float32))
    out = guard.full((2*16*128 + 4,), 7., dtype=torch.float32, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    (s, r, o) = (symbols.data_ptr(), rows.data_ptr(), out.data_ptr())
    assert lib.eae_hip_dequantize_maps_rows(s, r, r, None, None, 2, 16, 128, stream) == -1         # no output
    assert lib.eae_hip_dequantize_maps_rows(None, r, r, o, None, 2, 16, 128, stream) == -1
    assert lib.eae_hip_dequantize_maps_rows(s, None, r, o, None, 2, 16, 128, stream) == -1
    assert lib.eae_hip_dequantize_maps_rows(s, r, r, o, None, 0, 16, 128, stream) == -1
    assert lib.eae_hip_dequantize_maps_rows(s, r, r, o, None, 2, 0, 128, stream) == -1
    assert lib.eae_hip_dequantize_maps_rows(s, r, r, o, None, 2, 16, 64, stream) == -2             # EAE_HIP_BAD_SHAPE: not 128 maps
    assert lib.eae_hip_dequantize_maps_rows(s, r, r, o + 4, None, 2, 16, 128, stream) == -2        # 16-byte stores
    assert lib.eae_hip_dequantize_maps_rows(s, r, r, None, o + 8, 2, 16, 128, stream) == -2
    assert lib.eae_hip_dequantize_maps_rows(s, r, r, o, None, 65536, 16, 128, stream) == -2
    with pytest.raises(dev.HipError):
        dev.dequantize_maps_rows(symbols, rows[:1])                                                 # one row for two images
    with pytest.raises(dev.HipError):
        dev.dequantize_maps_rows(symbols, rows, out_shifted=out[:100])
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.).all()                                                          # nothing was launched
