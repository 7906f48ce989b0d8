"""The `crop` byte of both container headers (container.py, module docstring): byte 23, which was reserved
and written as 0, holds (H - h) << 4 | (W - w) for an h x w image coded at H x W. Host code only: what `assemble_blob` /
`assemble_image_blobs` write, what `read_header` gives back, and where `region_plan` draws the image's edge."""
import numpy
import pytest

from autoencoder_based_image_compression_amd import container

CROP_BYTE = 23
LENGTH = 10


def _parts(nb_images, height, width, coding_tile=None, idx_map_exception=67, seed=0):
    """The arguments of `assemble_blob` for images of `height` x `width` (coded size) whose streams hold a few bytes each."""
    rng = numpy.random.RandomState(seed)
    (h, w) = (height//16, width//16)
    nb_tiles = 1 if coding_tile is None else container._nb_tiles(h, w, (min(coding_tile[0], h), min(coding_tile[1], w)))
    bits = rng.randint(0, 30, size=(nb_images*nb_tiles*128, 2)).astype(numpy.uint32)
    payload = rng.randint(0, 256, size=int(((bits.astype(numpy.int64) + 7)//8).sum())).astype(numpy.uint8).tobytes()
    rows = rng.uniform(0.1, 0.9, size=(nb_images if idx_map_exception >= 0 else 0, LENGTH))
    return (False, nb_images, height, width, idx_map_exception, rng.uniform(0.5, 2., size=128).astype(numpy.float32),
            rng.normal(size=128).astype(numpy.float32), rng.uniform(0.1, 0.9, size=(128, LENGTH)), rows, bits, payload)


@pytest.mark.parametrize('coding_tile', [None, (2, 3)])
def test_a_real_size_changes_byte_23_and_nothing_else(coding_tile):
    parts = _parts(2, 64, 96, coding_tile)
    (plain, header_bytes) = container.assemble_blob(*parts, coding_tile=coding_tile)
    assert container._HEADER.size > CROP_BYTE and plain[CROP_BYTE] == 0
    for (h, w) in ((50, 83), (49, 96), (64, 81), (64, 96)):
        (blob, length) = container.assemble_blob(*parts, coding_tile=coding_tile, image_size=(h, w))
        crop = (64 - h) << 4 | (96 - w)
        assert length == header_bytes and blob[CROP_BYTE] == crop
        assert blob[:CROP_BYTE] == plain[:CROP_BYTE] and blob[CROP_BYTE + 1:] == plain[CROP_BYTE + 1:]
        assert (blob == plain) == (crop == 0)
        header = container.read_header(blob)
        assert (header['height'], header['width'], header['image_height'], header['image_width']) == (64, 96, h, w)
        reference = container.read_header(plain)
        assert header['payload_offset'] == reference['payload_offset'] and numpy.array_equal(header['bits'], reference['bits'])
    # a real size of another coded size is refused, and so is one that is no size
    for image_size in ((48, 96), (64, 97), (65, 96), (64, 80), (0, 96), (64, -1), (64.0, 96), (64,)):
        with pytest.raises(ValueError):
            container.assemble_blob(*parts, coding_tile=coding_tile, image_size=image_size)


def test_all_256_crops_round_trip_at_16_x_16():
    parts = _parts(1, 16, 16)
    (plain, _) = container.assemble_blob(*parts)
    seen = set()
    for h in range(1, 17):
        for w in range(1, 17):
            (blob, _) = container.assemble_blob(*parts, image_size=(h, w))
            header = container.read_header(blob)
            assert (header['image_height'], header['image_width'], header['height'], header['width']) == (h, w, 16, 16)
            seen.add(blob[CROP_BYTE])
            # and the byte alone decides: the plain blob with that byte set parses to the same real size
            patched = bytearray(plain)
            patched[CROP_BYTE] = (16 - h) << 4 | (16 - w)
            assert bytes(patched) == blob
    assert seen == set(range(256))


@pytest.mark.parametrize('coding_tile', [None, (2, 2)])
def test_a_blob_without_a_crop_parses_to_equal_sizes(coding_tile):
    (blob, _) = container.assemble_blob(*_parts(3, 48, 80, coding_tile), coding_tile=coding_tile)
    assert blob[CROP_BYTE] == 0
    header = container.read_header(blob)
    assert (header['image_height'], header['image_width']) == (header['height'], header['width']) == (48, 80)
    # the fixed part alone says so too (what `fetch_region` reads first of a file)
    (fields, _, _) = container._fixed_header(blob[:container._TILE_HEADER.size], len(blob))
    assert (fields['image_height'], fields['image_width']) == (48, 80)


@pytest.mark.parametrize('coding_tile', [None, (2, 3)])
def test_every_image_blob_carries_the_crop(coding_tile):
    parts = _parts(3, 64, 96, coding_tile)
    plain = container.assemble_image_blobs(*parts, coding_tile=coding_tile)
    blobs = container.assemble_image_blobs(*parts, coding_tile=coding_tile, image_size=(50, 83))
    assert len(blobs) == len(plain) == 3
    for (blob, reference) in zip(blobs, plain):
        assert blob[CROP_BYTE] == (14 << 4 | 13) and reference[CROP_BYTE] == 0
        assert blob[:CROP_BYTE] == reference[:CROP_BYTE] and blob[CROP_BYTE + 1:] == reference[CROP_BYTE + 1:]
        header = container.read_header(blob)
        assert (header['nb_images'], header['image_height'], header['image_width']) == (1, 50, 83)


@pytest.mark.parametrize('coding_tile', [None, (2, 3)])
def test_region_plan_draws_the_edge_at_the_real_size(coding_tile):
    parts = _parts(2, 64, 96, coding_tile)
    header = container.read_header(container.assemble_blob(*parts, coding_tile=coding_tile, image_size=(50, 83))[0])
    coded = container.read_header(container.assemble_blob(*parts, coding_tile=coding_tile)[0])
    # a region that ends at the real corner is the coded blob's plan for the same rectangle
    for region in ((0, 0, 50, 83), (40, 70, 10, 13), (49, 82, 1, 1)):
        assert container.region_plan(header, region) == container.region_plan(coded, region)
    # one pixel further, either way, leaves the image -- where the coded blob still has pixels
    for region in ((40, 70, 11, 13), (40, 70, 10, 14), (50, 0, 1, 1), (0, 83, 1, 1), (0, 0, 64, 96)):
        with pytest.raises(ValueError, match='leaves the 50 x 83 image'):
            container.region_plan(header, region)
        container.region_plan(coded, region)
    # the whole real image needs every coding tile: `decode_images` goes through this plan
    plan = container.region_plan(header, (0, 0, 50, 83))
    assert plan['sub_plane'] == (0, 4, 0, 6) and len(plan['entries']) == 2*header['bits'].reshape(2, -1, 128, 2).shape[1]
    (entries, chunks) = container._all_entries(header, container.assemble_blob(*parts, coding_tile=coding_tile, image_size=(50, 83))[0])
    assert entries == plan['entries'] and len(chunks) == len(entries)
