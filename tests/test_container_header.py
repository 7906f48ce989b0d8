"""The container header is untrusted input: every field that sizes a device buffer or a copy is checked on the host before
anything reaches the GPU (an inflated per-map bit count with a payload sized to match made the unpacking
kernel write past the map's stream region). No GPU needed: `read_header` is pure host code."""
import numpy
import pytest

from autoencoder_based_image_compression_amd import container


def build_blob(nb_images=1, height=32, width=48, nb_maps=128, length=10, idx_map_exception=67, bits=None, version=container.VERSION,
               payload_extra=0):
    head = container._HEADER.pack(container.MAGIC, version, 0, nb_images, height, width, nb_maps, length, 0, idx_map_exception)
    nb_rows = nb_images if idx_map_exception >= 0 else 0
    if bits is None:
        bits = numpy.full((nb_images*nb_maps, 2), 9, dtype=numpy.uint32)
    payload = int(((bits.astype(numpy.int64) + 7)//8).sum()) + payload_extra
    return b''.join([head, numpy.ones(nb_maps, numpy.float32).tobytes(), numpy.zeros(nb_maps, numpy.float32).tobytes(),
                     numpy.full((nb_maps, length), 0.5).tobytes(), numpy.full((nb_rows, length), 0.5).tobytes(),
                     bits.astype(numpy.uint32).tobytes(), bytes(payload)])


def test_well_formed_header_is_accepted():
    header = container.read_header(build_blob())
    assert (header['nb_images'], header['height'], header['width'], header['nb_maps']) == (1, 32, 48, 128)
    assert header['bits'].shape == (128, 2) and header['exception_probabilities'].shape == (1, 10)
    assert container.read_header(build_blob(idx_map_exception=-1))['exception_probabilities'].shape == (0, 10)


def test_capacity_matches_the_coder_library():
    """The pure-Python capacity equals the host library's (the reference's compression.cpp:24 rule)."""
    from autoencoder_based_image_compression_amd import _native
    lib = _native.coder()
    for (map_size, length) in ((6, 10), (1536, 10), (16384, 10), (7, 40), (1, 1), (1536, 255)):
        assert container.stream_capacity_bits(map_size, length) == 8*int(lib.eae_coder_stream_capacity_bytes(map_size, length))


@pytest.mark.parametrize('kwargs', [
    dict(nb_maps=64), dict(nb_maps=129), dict(length=0), dict(height=0), dict(width=0), dict(nb_images=0), dict(height=40),
    dict(width=50), dict(idx_map_exception=128), dict(idx_map_exception=-2), dict(version=container.VERSION + 1), dict(payload_extra=1),
])
def test_bad_sizes_are_rejected(kwargs):
    with pytest.raises(ValueError):
        container.read_header(build_blob(**kwargs))


@pytest.mark.parametrize('which', [(0, 0), (127, 1), (60, 0)])
def test_inflated_bit_count_with_matching_payload_is_rejected(which):
    """One count above the capacity of a stream (6 symbols * 32 bits = 192 bits for a 32x48 image), payload sized to match."""
    bits = numpy.full((128, 2), 9, dtype=numpy.uint32)
    bits[which] = container.stream_capacity_bits(6, 10)
    container.read_header(build_blob(bits=bits))              # exactly the capacity: legal
    bits[which] += 1
    with pytest.raises(ValueError):
        container.read_header(build_blob(bits=bits))
    bits[which] = 0xFFFFFFF0
    with pytest.raises(ValueError):
        container.read_header(build_blob(bits=bits)[:4096])   # and no 500 MB payload is needed to find out


LENGTHS = (1, 2, 3, 31, 32, 33, 255)          # tests/unary_length_cases.py: the lengths the containers and codecs are run at on the GPU


def random_parts(seed, nb_images, height, width, length, idx_map_exception, nb_tiles=1, tile_sizes=None):
    """Random header arrays and payload for a blob of `nb_images` images: bit counts up to the capacity of each tile's streams."""
    rng = numpy.random.RandomState(seed)
    sizes = [(height//16)*(width//16)] if tile_sizes is None else tile_sizes
    most = numpy.array([container.stream_capacity_bits(size, length) for size in sizes], dtype=numpy.int64)
    bits = (rng.rand(nb_images, nb_tiles, 128, 2)*(most[None, :, None, None] + 1)).astype(numpy.uint32)
    bits[rng.rand(*bits.shape) < 0.1] = 0
    bits[0, 0, 0, 0] = most[0]
    return {'bin_widths': rng.uniform(0.05, 2., size=128).astype(numpy.float32), 'map_mean': rng.normal(size=128).astype(numpy.float32),
            'probabilities': rng.uniform(0.01, 0.99, size=(128, length)),
            'exception_rows': rng.uniform(0.01, 0.99, size=(nb_images if idx_map_exception >= 0 else 0, length)), 'bits': bits,
            'payload': rng.randint(0, 256, size=int(((bits.astype(numpy.int64) + 7)//8).sum())).astype(numpy.uint8).tobytes()}


def check_round_trip(header, parts, nb_images, height, width, length, idx_map_exception, learned):
    """Every field `read_header` gives is the one that was written, bit for bit."""
    assert (header['nb_images'], header['height'], header['width'], header['nb_maps']) == (nb_images, height, width, 128)
    assert header['truncated_unary_length'] == length and header['idx_map_exception'] == idx_map_exception
    assert header['are_bin_widths_learned'] is learned
    for (key, written) in (('bin_widths', 'bin_widths'), ('map_mean', 'map_mean'), ('binary_probabilities', 'probabilities'),
                           ('exception_probabilities', 'exception_rows')):
        assert header[key].dtype == parts[written].dtype and header[key].shape == parts[written].shape, key
        assert header[key].tobytes() == parts[written].tobytes(), key
    assert header['exception_probabilities'].shape == (nb_images if idx_map_exception >= 0 else 0, length)
    assert header['bits'].dtype == numpy.uint32


@pytest.mark.parametrize('idx_map_exception', [67, 0, 127, -1])
@pytest.mark.parametrize('length', LENGTHS)
def test_written_headers_read_back_at_every_length(length, idx_map_exception):
    """`assemble_blob` -> `read_header` at the lengths on both sides of every parity and of the coder's 32 / 33 boundary, with and
    without the exception row, for one image and for three; `ratecontrol.header_bytes` is the single-image header's size."""
    from autoencoder_based_image_compression_amd import ratecontrol
    for (nb_images, learned) in ((1, False), (3, True)):
        parts = random_parts(length + nb_images, nb_images, 64, 96, length, idx_map_exception)
        bits = parts['bits'].reshape(-1, 2)
        (blob, header_bytes) = container.assemble_blob(learned, nb_images, 64, 96, idx_map_exception, parts['bin_widths'], parts['map_mean'],
                                                       parts['probabilities'], parts['exception_rows'], bits, parts['payload'])
        header = container.read_header(blob)
        check_round_trip(header, parts, nb_images, 64, 96, length, idx_map_exception, learned)
        assert header['bits'].shape == bits.shape and numpy.array_equal(header['bits'], bits) and 'format' not in header
        assert header['payload_offset'] == header_bytes == len(blob) - len(parts['payload'])
        assert blob[header_bytes:] == parts['payload']
        if nb_images == 1:
            ladder = ratecontrol.RateLadder(parts['bin_widths'][None], parts['probabilities'][None], parts['map_mean'], idx_map_exception)
            assert ratecontrol.header_bytes(ladder) == header_bytes
        # one byte less, one byte more, and a length that is not the table's: refused
        for bad in (blob[:-1], blob + b'\x00'):
            with pytest.raises(ValueError):
                container.read_header(bad)
        other = bytearray(blob)
        other[container._HEADER.size - 6] = length + 1 if length < 255 else length - 1          # the header's L byte
        assert container._HEADER.unpack_from(bytes(other), 0)[7] != length
        with pytest.raises(ValueError):
            container.read_header(bytes(other))
