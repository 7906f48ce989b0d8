"""The host half of the codec's containers: `container.assemble_blob` (what `encode_images` and `codec.Ticket.container()` both end
with) and `container.assemble_image_blobs` (`Ticket.image_containers()`), against `container.read_header`. No GPU."""
import numpy
import pytest

from autoencoder_based_image_compression_amd import container

NB_MAPS = 128


def _parts(nb_images, length, idx_map_exception, seed, height=32, width=48):
    """Synthetic parts of a blob: bit counts below the capacity of a stream, some zero, some multiples of 8."""
    rng = numpy.random.RandomState(seed)
    map_size = (height//16)*(width//16)
    capacity = container.stream_capacity_bits(map_size, length)
    bits = rng.randint(0, capacity + 1, size=(nb_images*NB_MAPS, 2)).astype(numpy.uint32)
    bits[rng.rand(*bits.shape) < 0.2] = 0
    bits[::7] = bits[::7]//8*8
    nb_rows = nb_images if idx_map_exception >= 0 else 0
    payload_bytes = int(((bits.astype(numpy.int64) + 7)//8).sum())
    return {'learned': bool(seed & 1), 'nb_images': nb_images, 'height': height, 'width': width, 'idx': idx_map_exception,
            'bin_widths': rng.rand(NB_MAPS).astype(numpy.float32) + numpy.float32(0.1),
            'map_mean': rng.randn(NB_MAPS).astype(numpy.float32),
            'probabilities': numpy.clip(rng.rand(NB_MAPS, length), 0.01, 0.99),
            'rows': numpy.clip(rng.rand(nb_rows, length), 0.01, 0.99),
            'bits': bits, 'payload': rng.randint(0, 256, size=payload_bytes).astype(numpy.uint8).tobytes()}


def _arguments(p):
    return (p['learned'], p['nb_images'], p['height'], p['width'], p['idx'], p['bin_widths'], p['map_mean'], p['probabilities'], p['rows'],
            p['bits'], p['payload'])


@pytest.mark.parametrize('nb_images, length, idx_map_exception', [(1, 10, -1), (3, 10, 67), (2, 1, 0), (2, 255, 127)])
def test_assembled_blob_reads_back(nb_images, length, idx_map_exception):
    p = _parts(nb_images, length, idx_map_exception, seed=nb_images + length)
    (blob, header_bytes) = container.assemble_blob(*_arguments(p))
    header = container.read_header(blob)
    assert header['payload_offset'] == header_bytes and blob[header_bytes:] == p['payload']
    assert (header['nb_images'], header['height'], header['width'], header['nb_maps']) == (nb_images, p['height'], p['width'], NB_MAPS)
    assert header['truncated_unary_length'] == length and header['idx_map_exception'] == idx_map_exception
    assert header['are_bin_widths_learned'] == p['learned']
    for (key, name) in (('bin_widths', 'bin_widths'), ('map_mean', 'map_mean'), ('binary_probabilities', 'probabilities'),
                        ('exception_probabilities', 'rows'), ('bits', 'bits')):
        assert header[key].dtype == p[name].dtype and numpy.array_equal(header[key], p[name]), key
    assert header['exception_probabilities'].shape == ((nb_images if idx_map_exception >= 0 else 0), length)


def test_assemble_refuses_parts_that_do_not_fit_each_other():
    p = _parts(2, 10, 67, seed=5)
    with pytest.raises(ValueError, match='payload size'):
        container.assemble_blob(*(_arguments(p)[:-1] + (p['payload'] + b'\0',)))
    with pytest.raises(ValueError, match='shape'):
        container.assemble_blob(*(_arguments(p)[:8] + (p['rows'][:1], p['bits'], p['payload'])))
    with pytest.raises(ValueError, match='float64'):
        container.assemble_blob(*(_arguments(p)[:9] + (p['bits'].astype(numpy.int64), p['payload'])))


@pytest.mark.parametrize('idx_map_exception', [67, -1])
def test_image_blobs_are_the_slices_of_the_batch(idx_map_exception):
    p = _parts(3, 10, idx_map_exception, seed=9)
    p['bits'][NB_MAPS:2*NB_MAPS] = 0            # an image without a payload byte
    p['payload'] = p['payload'][:int(((p['bits'].astype(numpy.int64) + 7)//8).sum())]
    blobs = container.assemble_image_blobs(*_arguments(p))
    assert len(blobs) == 3
    payloads = []
    for (i, blob) in enumerate(blobs):
        header = container.read_header(blob)
        assert header['nb_images'] == 1 and header['idx_map_exception'] == idx_map_exception
        assert numpy.array_equal(header['bits'], p['bits'][i*NB_MAPS:(i + 1)*NB_MAPS])
        if idx_map_exception >= 0:
            assert numpy.array_equal(header['exception_probabilities'], p['rows'][i:i + 1])
        else:
            assert header['exception_probabilities'].shape == (0, 10)
        assert numpy.array_equal(header['binary_probabilities'], p['probabilities'])
        payloads.append(blob[header['payload_offset']:])
    assert len(payloads[1]) == 0
    assert b''.join(payloads) == p['payload']
    # a batch of one image is its own single blob
    one = _parts(1, 10, idx_map_exception, seed=11)
    assert container.assemble_image_blobs(*_arguments(one)) == [container.assemble_blob(*_arguments(one))[0]]
