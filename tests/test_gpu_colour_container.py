"""`container.encode_colour_images` / `decode_colour_images` and the `EAC1` blob on the device.

Pictures of 99 x 165, 100 x 166, 97 x 192 and 128 x 192: luminance planes coded as 112 x 176, 112 x 176, 112 x 192 and 128 x 192,
chroma planes of 50 x 83, 50 x 83, 49 x 96 and 64 x 96, all coded as 64 x 96 (the sizes tests/test_gpu_frame_container.py runs). With
the trained-like models of that module, fixed and learned bin widths, a truncated unary length of 10 with exception map 67 and of 3
without, as EAE1 and in coding tiles of (2, 3), with chroma at doubled bin widths, and with `rdo_lambda`:
  * the three plane blobs inside the EAC1 are `encode_images(plane_k, ..., pad=True, ...)` of `colour.split_420_numpy`'s planes, the
    infos are theirs, and the wrapper around them is the 48 bytes of the format;
  * `decode_colour_images` is `colour.merge_420_numpy` of the three `decode_images` results;
  * at 128 x 192 every `crop` byte is 0."""
import numpy
import pytest

from test_gpu_frame_container import arguments_of, images_of, models  # noqa: F401 (`models` is a fixture)

pytestmark = pytest.mark.gpu

N = 2
SIZES = ((99, 165), (100, 166), (97, 192), (128, 192))
CHROMA_SIZES = ((50, 83), (50, 83), (49, 96), (64, 96))
CROP_BYTE = 23
# name: (learned bin widths, rate, keyword arguments, chroma at doubled bin widths)
CONFIGS = {
    'fixed_L10_exception_EAE1': (False, 'L10_exception_67', {}, False),
    'learned_L3_EAE1': (True, 'L3_no_exception', {}, False),
    'fixed_L10_tiles_2x3': (False, 'L10_exception_67', {'coding_tile': (2, 3)}, False),
    'learned_L10_chroma_doubled': (True, 'L10_exception_67', {}, True),
    'fixed_L10_rdo': (False, 'L10_exception_67', {'rdo_lambda': 0.02}, False),
}


@pytest.fixture(autouse=True)
def _guarded_buffers():
    """Poisoned buffers between guard bands for everything device.py / pipeline.py / container.py allocate (tests/guarded.py)."""
    import guarded
    from autoencoder_based_image_compression_amd import container, device, pipeline
    with guarded.guarded((device, pipeline, container), 0xFF):
        yield


def pictures_of(size, seed=0, count=N):
    """Smoothed noise in every channel (tests/test_gpu_frame_container.py: `images_of`), the channels unrelated: busy chroma."""
    return numpy.stack([images_of(size, seed + 1000*channel, count) for channel in range(3)], axis=3)


def points_of(models, learned, rate, doubled):
    """(encoder, the luminance rate point, the chroma rate point or None)."""
    (encoder, bin_widths, map_mean, probabilities, idx_map_exception) = arguments_of(models, learned, rate)
    luma = (bin_widths, map_mean, probabilities, idx_map_exception)
    chroma = (bin_widths*numpy.float32(2.), map_mean, probabilities, idx_map_exception) if doubled else None
    return (encoder, luma, chroma)


@pytest.mark.parametrize('config', sorted(CONFIGS))
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '{0}x{1}'.format(*s))
def test_colour_blobs_are_three_plane_blobs_and_decode_to_their_merge(models, size, config):
    from autoencoder_based_image_compression_amd import colour, container
    (learned, rate, more, doubled) = CONFIGS[config]
    (encoder, luma, chroma) = points_of(models, learned, rate, doubled)
    decoder = models[learned]['decoder']
    rgb = pictures_of(size)
    planes = colour.split_420_numpy(rgb)
    assert planes[1].shape[1:] == CHROMA_SIZES[SIZES.index(size)]
    (blob, info) = container.encode_colour_images(rgb, encoder, *luma, chroma=chroma, **more)
    expected = [container.encode_images(plane, encoder, *point, pad=True, **more)
                for (plane, point) in zip(planes, (luma, chroma or luma, chroma or luma))]
    (header, *plane_blobs) = container.split_colour_blob(blob)
    assert plane_blobs == [b for (b, _) in expected]
    assert blob == container.assemble_colour_blob(size, *plane_blobs) and blob[:4] == b'EAC1' and len(blob) == 48 + sum(map(len, plane_blobs))
    assert (header['nb_images'], header['image_height'], header['image_width'], header['subsampling']) == (N,) + size + (1,)
    assert info['plane_bytes'] == header['plane_bytes'] == tuple(map(len, plane_blobs))
    for (name, (_, plane_info)) in zip(('y', 'cb', 'cr'), expected):
        assert sorted(info[name]) == sorted(plane_info) and all(numpy.array_equal(info[name][key], plane_info[key]) for key in plane_info)
    assert all(b[:4] == (b'EAT1' if 'coding_tile' in more else b'EAE1') for b in plane_blobs)
    if doubled:
        assert numpy.array_equal(container.read_header(plane_blobs[1])['bin_widths'], luma[0]*numpy.float32(2.))
        assert numpy.array_equal(container.read_header(plane_blobs[0])['bin_widths'], luma[0])
        assert len(plane_blobs[1]) < len(container.encode_images(planes[1], encoder, *luma, pad=True)[0])      # the coarser point is cheaper
    # every existing decoder reads a plane of a colour file unchanged; the picture is the merge of the three
    decoded = [container.decode_images(b, decoder) for b in plane_blobs]
    assert [d.shape for d in decoded] == [p.shape for p in planes]
    got = container.decode_colour_images(blob, decoder)
    assert got.dtype == numpy.uint8 and got.shape == rgb.shape
    assert numpy.array_equal(got, colour.merge_420_numpy(*decoded))
    crops = [b[CROP_BYTE] for b in plane_blobs]
    if size == (128, 192):
        assert crops == [0, 0, 0]
    else:
        luma_coded = container.coded_size(*size)
        chroma_size = planes[1].shape[1:]
        assert crops == [(luma_coded[0] - size[0]) << 4 | (luma_coded[1] - size[1])] + [(64 - chroma_size[0]) << 4 | (96 - chroma_size[1])]*2


def test_refusals_on_the_device_paths(models):
    from autoencoder_based_image_compression_amd import container
    (encoder, luma, _) = points_of(models, False, 'L10_exception_67', False)
    rgb = pictures_of((99, 165))
    with pytest.raises(ValueError):
        container.encode_colour_images(rgb, encoder, *luma, chroma=luma[:3])
    with pytest.raises(ValueError):
        container.encode_colour_images(rgb[..., 0], encoder, *luma)
    (blob, _) = container.encode_colour_images(rgb[:1], encoder, *luma)
    decoder = models[False]['decoder']
    for bad in (blob[:-1], b'EAC2' + blob[4:], blob[:20] + b'\x02' + blob[21:]):
        with pytest.raises(ValueError):
            container.decode_colour_images(bad, decoder)
    with pytest.raises(ValueError, match='magic'):
        container.decode_images(blob, decoder)
    with pytest.raises(ValueError):
        container.decode_colour_images(blob, models[True]['decoder'])          # the other kind of model, as for any plane
