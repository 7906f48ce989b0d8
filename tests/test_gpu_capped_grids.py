"""Every kernel with a capped or persistent grid, at a size where a block (or a lane) takes more than one unit of work, against
numpy / the CPU oracle, exactly (the rule).

At the small shapes of the other kernel-level modules every block of such a grid does exactly one unit: the grid-stride increment,
the persistent `for (k = slot; k < cnt; k += S)` walk, the prefetch of the next tile and the re-basing of a buffer resource on the
next image are then never compared with anything. Here each launch goes beyond its cap, each test first asserts that it does (a
cap that moves turns the test red, not hollow; `test_the_caps_are_the_ones_in_the_sources` holds the constants below against the
source lines they mirror), and everything is compared bit for bit: `numpy.array_equal`, integer equality for the sums; there is no
tolerance in this module. Every buffer lies between guard bands and starts out as poison (tests/guarded.py), under the two poisons
0xFF and 0x7F.

One thread of a 256-thread block takes one unit (a 16-byte word, a dword, an element, a run of four pixels) per trip of its loop;
tconv3's unit is a tile of 8 x 16 input sites per block. "CUs" is `device.device_info()['compute_units']`, read at run time.

  kernel (file)                        | one unit per block up to                 | smallest size beyond, here          | test
  -------------------------------------+------------------------------------------+-------------------------------------+-----------------------------------------------
  tconv3_kernel (tconv3.hip)           | grid = ceil8(min(tiles, 3 CUs)) tiles,   | grid + 1 tiles; 2 grid + 2 tiles;   | test_tconv3_when_a_block_takes_several_tiles
    persistent, eight XCD shares       |   768 on 256 CUs                         |   ragged shares, images changing    |   [one_more, ragged, three, sites]
  frame_pad_kernel (frame.hip)         | PAD_BLOCKS = 1024: 262,144 words, 4 MiB  | 3 x 1216 x 1216 = 277,248 words     | test_frame_pad_past_the_block_cap
  frame_sse_kernel (frame.hip)         | SSE_BLOCKS_PER_IMAGE = 64: 65,536 runs   | 1201 x 301 = 361,501 runs an image  | test_frame_sse_past_the_blocks_per_image_cap
  publish_crops_kernel                 | CROP_BLOCKS = 256: 65,536 words, 1 MiB   | 5 x 500 x 421 = 65,782 words        | test_publish_crops_past_the_block_cap
    (codec_decode.hip)                 |                                          |                                     |
  fetch_prefix_kernel                  | FETCH_BLOCKS = 64: 16,384 words, 256 KiB | 262,145 bytes ... capacity + 5      | test_fetch_prefix_past_one_pass
    (codec_decode.hip)                 |                                          |                                     |
  publish_prefix_kernel                | PREFIX_BLOCKS = 64: 256 KiB              | 262,145 bytes ... capacity + 5      | test_publish_prefix_past_one_pass
    (codec_container.hip)              |                                          |                                     |
  publish_kernel behind                | 64 blocks: 16,384 dwords, 64 KiB         | 16,385 dwords ... 32,768 + 1,041    | test_publish_to_host_past_one_pass
    publish_to_host (misc.hip)         |                                          |                                     |
  publish_step_kernel (misc.hip)       | 65,536 words                             |                                     | test_gpu_codec.py::
                                       |                                          |                                     |   test_publish_step_copies_clears_and_counts
  cast_bt601_kernel (quantize.hip)     | 4096 blocks: 1,048,576 elements          | 4096*256 + 9000 elements            | test_cast_bt601_past_the_block_cap
  sse_kernel (quantize.hip)            | 64 blocks an image of 4096 pixels each:  | 513 x 515 = 264,195 pixels (odd)    | test_sse_u8_past_the_blocks_per_image_cap
                                       |   262,144 pixels an image                |                                     |
  rgb_to_ycbcr_kernel (quantize.hip)   | grid_for: 8192 blocks, 2,097,152 pixels  | 2^24 pixels                         | test_gpu_surface.py::
                                       |                                          |                                     |   test_rgb_to_ycbcr_all_colours
  quantize_generic, nonzero_flags,     | grid_for: 8192 blocks; map_minmax and    |                                     | test_gpu_quantize_helpers.py (GRID_CAP,
    cast_int16, map_minmax, floor_hist |   floor_hist 1024 blocks                 |                                     |   "past the 1024-block cap")
  svhn.hip's element-wise kernels      | grid_for: 4096 blocks                    |                                     | test_gpu_svhn_kernels.py (GRID_CAP)
  ladder per-tile histograms           | 2 CUs blocks                             |                                     | test_gpu_tiled_ladder_kernels.py::test_histograms_
    (ladder.hip)                       |                                          |                                     |   per_tile_when_a_block_takes_several_whole_tiles
  tile_stitch_u8_kernel with a         | blocks = ceil(window chunks / 4096); one | windows of 17,952 chunks: 5 blocks, | test_tile_stitch_with_a_reference_when_lanes_loop
    reference (tile.hip)               |   trip of a lane's loop covers 1024      |   an interior of 14,880 chunks      |
                                       |   blocks chunks of the interior          |   takes three trips                 |

The test modules named without a test are neighbours that carry their own guard. A new kernel with a cap gets a row here, a constant
below with its source line, and a test that asserts its precondition first."""
import functools
import os
import re

import numpy
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F)
THREADS = 256                        # threads per block of every kernel below
# the caps, each with the source line it mirrors (csrc/hip/); test_the_caps_are_the_ones_in_the_sources reads those lines
T3_BLOCKS_PER_CU = 3                 # tconv3.hip: BLOCKS_PER_CU = (PASSES == 2 ? 4 : 6) * 2 / WAVES with PASSES = WAVES = 4
(T3_TILE_H, T3_TILE_W) = (8, 16)     # tconv3.hip: TH = 2 * WAVES, TW = 16: input sites per tile
PAD_BLOCKS = 1024                    # frame.hip: constexpr int PAD_BLOCKS = 1024
FRAME_SSE_BLOCKS_PER_IMAGE = 64      # frame.hip: constexpr int SSE_BLOCKS_PER_IMAGE = 64
FRAME_SSE_RUNS_PER_BLOCK = 1024      # frame.hip: bpi = (runs + 1023) / 1024
CROP_BLOCKS = 256                    # codec_decode.hip: constexpr int CROP_BLOCKS = 256
FETCH_BLOCKS = 64                    # codec_decode.hip: constexpr int FETCH_BLOCKS = 64
PREFIX_BLOCKS = 64                   # codec_container.hip: constexpr int PREFIX_BLOCKS = 64
PUBLISH_BLOCKS = 64                  # misc.hip, eae_hip_publish_to_host: (words + 255) / 256 > 64 ? 64
CAST_BLOCKS = 4096                   # quantize.hip, eae_hip_cast_bt601: blocks > 4096 ? 4096
SSE_BLOCKS_PER_IMAGE = 64            # quantize.hip, eae_hip_sse_u8: if (bpi > 64) bpi = 64
SSE_PIXELS_PER_BLOCK = 4096          # quantize.hip, eae_hip_sse_u8: bpi = (pixels_per_image + 4095) / 4096
(TILE_UNROLL, STITCH_CHUNKS_PER_LANE) = (4, 16)      # tile.hip: TILE_UNROLL = 4, STITCH_CHUNKS_PER_LANE = 4 * TILE_UNROLL

SOURCE_LINES = {
    'tconv3.hip': ('#define EAE_T3_WAVES 4', '#define EAE_T3_PASSES 4', 'constexpr int TH = 2 * WAVES, TW = 16;',
                   'constexpr int BLOCKS_PER_CU = (PASSES == 2 ? 4 : 6) * 2 / WAVES;', 'long grid = (long)cus * BLOCKS_PER_CU;',
                   'grid = (grid + 7) / 8 * 8;'),
    'frame.hip': ('constexpr int PAD_BLOCKS = 1024;', 'constexpr int SSE_BLOCKS_PER_IMAGE = 64;', 'uint64_t bpi = (runs + 1023) / 1024;'),
    'codec_decode.hip': ('constexpr int CROP_BLOCKS = 256;', 'constexpr int FETCH_BLOCKS = 64;'),
    'codec_container.hip': ('constexpr int PREFIX_BLOCKS = 64;',),
    'misc.hip': ('const unsigned blocks = (unsigned)((words + 255) / 256 > 64 ? 64 : (words + 255) / 256);',),
    'quantize.hip': ('dim3((unsigned)(blocks > 4096 ? 4096 : blocks))', 'long bpi = (pixels_per_image + 4095) / 4096;', 'if (bpi > 64) bpi = 64;'),
    'tile.hip': ('constexpr int TILE_THREADS = 256;', 'constexpr int TILE_UNROLL = 4;', 'constexpr int STITCH_CHUNKS_PER_LANE = 4 * TILE_UNROLL;'),
}


def _dev():
    from autoencoder_based_image_compression_amd import device
    return device


@pytest.fixture(params=POISONS, ids=['ff', '7f'])
def guard(request):
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


def _shifted_upload(guard, x, shift):
    """`x` on the device between bands, its first byte `shift` bytes behind the interior's (4096-aligned) start; the bytes in
    front of it and behind it, inside the interior, are poison like the bands."""
    flat = guard.full((x.size + 8,), guard.poison, dtype=torch.uint8, device='cuda')
    view = flat[shift:shift + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 4 == shift % 4 and view.is_contiguous()
    return view


def test_the_caps_are_the_ones_in_the_sources():
    """The constants of this module mirror lines of the launchers. A launcher whose line is gone has another cap: the sizes below
    and the table above are then to be worked out again."""
    import autoencoder_based_image_compression_amd as package
    folder = os.path.join(os.path.dirname(os.path.abspath(package.__file__)), 'csrc', 'hip')
    for (name, lines) in sorted(SOURCE_LINES.items()):
        with open(os.path.join(folder, name)) as file:
            text = re.sub(r'\s+', ' ', file.read())
        for line in lines:
            assert line in text, (name, line)


# ---- tconv3_kernel: persistent blocks, eight XCD shares ----------------------------------------------------------------------------

def _t3_grid():
    """The launch's grid for a tile count beyond it: 3 blocks per compute unit, rounded up to the eight XCD shares."""
    return -(-T3_BLOCKS_PER_CU*_dev().device_info()['compute_units']//8)*8


def _t3_tiles(shape):
    (n, h, w) = shape
    return n*(-(-h//T3_TILE_H))*(-(-w//T3_TILE_W))


def _t3_shape(case, grid):
    """(n, h, w) in input sites for a grid of `grid` blocks, S = grid/8 slots per XCD share."""
    if case == 'one_more':         # grid + 1 tiles in one row: XCD 0's share has one tile more, one block takes two tiles, the rest one
        return (1, 1, T3_TILE_W*(grid + 1))
    if case == 'ragged':           # images of 2 x 3 tiles, the second tile row one site high, the last tile column 3 sites wide; more
        n = grid//6 + 1            # tiles than blocks, no multiple of 8; a block's next tile, S tiles on, lies in another image
        while (6*n) % 8 == 0:
            n += 1
        return (n, T3_TILE_H + 1, 2*T3_TILE_W + 3)
    if case == 'three':            # 2 grid + 2 tiles, the last one 5 sites wide: r8 = 2, slot 0 of XCD 0 and 1 takes three tiles
        return (1, 1, T3_TILE_W*(2*grid + 1) + 5)
    if case == 'sites':            # grid + 9 images of one site: every step of every walk changes image, 127 sites of 128 outside
        return (grid + 9, 1, 1)
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def _t3_reference(case, grid):
    """Inputs and the oracle's outputs of one case, computed once and shared by the two poisons; the test leaves them unchanged."""
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables
    from oracle import transforms
    shape = _t3_shape(case, grid)
    (n, h, w) = shape
    v = variables.random_variables(1., False, seed=7, bias_std=0.01)
    rng = numpy.random.RandomState(len(case))
    # positive weights and inputs so that the reconstruction spans the BT.601 range instead of sitting on the clip floor; a pixel of
    # an image one site high or wide has a third of the 3 x 3 neighbours in the image, and the weights make up for that
    gain = 8.*9./(min(h, 3)*min(w, 3))
    w6 = (numpy.absolute(v['decoder/weights_6'])*numpy.float32(gain)).astype(numpy.float32)
    x = (rng.standard_normal(size=shape + (128,)) + 1.5).astype(numpy.float32)
    f32 = transforms.conv2d_transpose_same(x, w6, 4, None)[..., 0]
    u8 = numpy.round(f32.clip(min=16., max=235.)).astype(numpy.uint8)
    target = rng.randint(16, 236, size=(n, 4*h, 4*w)).astype(numpy.uint8)
    sse = ((target.astype(numpy.int64) - u8.astype(numpy.int64))**2).reshape(n, -1).sum(axis=1)
    return {'shape': shape, 'w6': w6, 'x': x, 'f32': f32, 'u8': u8, 'target': target, 'sse': sse}


@pytest.mark.parametrize('case', ['one_more', 'ragged', 'three', 'sites'])
def test_tconv3_when_a_block_takes_several_tiles(guard, case):
    dev = _dev()
    grid = _t3_grid()
    stride = grid//8
    shape = _t3_shape(case, grid)
    (n, h, w) = shape
    n_tiles = _t3_tiles(shape)
    per_image = n_tiles//n
    assert n_tiles > grid                                   # a block takes a second tile: the walk this test is about
    if case == 'one_more':
        assert n_tiles == grid + 1 and n_tiles % 8 == 1     # one XCD share with one tile more, one block with two tiles
    elif case == 'ragged':
        assert n_tiles % 8 != 0                             # unequal shares (xcd < r8) together with a second tile
        assert n > 1 and h % T3_TILE_H == 1 and w % T3_TILE_W != 0 and per_image == 6
        assert per_image < stride                           # the next tile of a block, `stride` tiles on, lies in another image
    elif case == 'three':
        assert n_tiles > 2*grid and n_tiles % 8 != 0 and w % T3_TILE_W != 0      # some blocks take three tiles
    else:
        assert per_image == 1 and n_tiles % 8 != 0          # every step of every walk changes image
    r = _t3_reference(case, grid)
    assert len(numpy.unique(r['u8'])) > 4                   # the data exercises the cast, not only the clip floor
    wph = dev.pack_tconv9x9s4_weights(guard.upload(r['w6']))
    x = guard.upload(r['x'])
    (f32, u8, sse) = dev.tconv9x9s4_luma(x, wph, want_f32=True, want_u8=True, ref_u8=guard.upload(r['target']))
    assert numpy.array_equal(f32.cpu().numpy(), r['f32'])
    assert numpy.array_equal(u8.cpu().numpy(), r['u8'])
    assert numpy.array_equal(sse.cpu().numpy(), r['sse'])
    # the same walk with ref == nullptr and no uint8 output
    (f32, u8, sse) = dev.tconv9x9s4_luma(x, wph, want_f32=True, want_u8=False)
    assert u8 is None and sse is None and numpy.array_equal(f32.cpu().numpy(), r['f32'])
    assert numpy.array_equal(x.cpu().numpy(), r['x'])
    guard.check()


# ---- frame_pad_kernel, frame_sse_kernel ---------------------------------------------------------------------------------------------

FRAME_SHAPE = (3, 1201, 1203)        # odd h, w and h*w: images 1 and 2 start at odd addresses; coded 1216 x 1216


def _coded(h, w):
    return (-(-h//16)*16, -(-w//16)*16)


@functools.lru_cache(maxsize=None)
def _frame_images():
    x = numpy.random.RandomState(1201).randint(0, 256, size=FRAME_SHAPE).astype(numpy.uint8)
    (H, W) = _coded(*FRAME_SHAPE[1:])
    padded = numpy.pad(x, ((0, 0), (0, H - x.shape[1]), (0, W - x.shape[2])), mode='edge')
    rec = numpy.random.RandomState(1203).randint(0, 256, size=padded.shape).astype(numpy.uint8)
    return (x, padded, rec)


def test_frame_pad_past_the_block_cap(guard):
    dev = _dev()
    (x, expected, _) = _frame_images()
    (n, h, w) = x.shape
    assert expected.size > 16*THREADS*PAD_BLOCKS            # more 16-byte words than lanes: the grid-stride loop runs
    assert n > 1 and (h*w) % 2 == 1                         # ... and its later trips cross into images at odd addresses
    for shift in (0, 1):
        src = _shifted_upload(guard, x, shift)
        out = dev.frame_pad_u8(src)
        assert tuple(out.shape) == expected.shape and numpy.array_equal(out.cpu().numpy(), expected), shift
        assert numpy.array_equal(src.cpu().numpy(), x)
        guard.check()
    out = dev.frame_pad_u8(torch.from_numpy(x.copy()).pin_memory())
    assert out.is_cuda and numpy.array_equal(out.cpu().numpy(), expected)
    guard.check()


def test_frame_sse_past_the_blocks_per_image_cap(guard):
    dev = _dev()
    (ref, _, rec) = _frame_images()
    (n, h, w) = ref.shape
    (H, W) = _coded(h, w)
    runs = h*(-(-w//4))
    assert runs > FRAME_SSE_RUNS_PER_BLOCK*FRAME_SSE_BLOCKS_PER_IMAGE        # the 64-block cap is taken
    assert runs > 4*THREADS*FRAME_SSE_BLOCKS_PER_IMAGE                       # ... and a lane makes more trips than at any smaller size
    for outside in (0, 255):
        filled = rec.copy()
        filled[:, h:, :] = outside
        filled[:, :, w:] = outside
        expected = ((ref.astype(numpy.int64) - filled[:, :h, :w].astype(numpy.int64))**2).sum(axis=(1, 2))
        for shift in (0, 1):
            got = dev.frame_sse_u8(guard.upload(filled), _shifted_upload(guard, ref, shift))
            assert got.dtype == torch.int64 and numpy.array_equal(got.cpu().numpy(), expected), (outside, shift)
        guard.check()
    # the largest error there is: 65025 h w per image
    got = dev.frame_sse_u8(guard.upload(numpy.full((n, H, W), 255, dtype=numpy.uint8)), guard.upload(numpy.zeros((n, h, w), dtype=numpy.uint8)))
    assert got.cpu().tolist() == [65025*h*w]*n
    guard.check()


# ---- publish_crops_kernel ------------------------------------------------------------------------------------------------------------

CROP_PLANES = (5, 512, 448)
CROP = (500, 421)                    # odd width: 16-byte words straddle crop rows and crops
CROP_ORIGINS = [(0, 0), (12, 27), (-3, 500), (5, 7), (11, 26)]      # the first corner, the last, one out of range (clamped), odd ones


@pytest.mark.parametrize('pinned', [False, True], ids=['device', 'pinned'])
def test_publish_crops_past_the_block_cap(guard, pinned):
    dev = _dev()
    (n, H, W) = CROP_PLANES
    (ch, cw) = CROP
    nbytes = n*ch*cw
    words = -(-nbytes//16)*16
    assert nbytes > 16*THREADS*CROP_BLOCKS                  # more 16-byte words than lanes: the grid-stride loop runs
    assert cw % 2 == 1 and nbytes % 16 != 0
    assert CROP_ORIGINS[1] == (H - ch, W - cw)
    planes = numpy.random.RandomState(ch + cw).randint(0, 256, size=CROP_PLANES).astype(numpy.uint8)
    expected = []
    for (plane, (y, x)) in zip(planes, CROP_ORIGINS):
        (y, x) = (min(max(y, 0), H - ch), min(max(x, 0), W - cw))
        expected.append(plane[y:y + ch, x:x + cw])
    planes_d = guard.upload(planes)
    origins_d = guard.upload(numpy.array(CROP_ORIGINS, dtype=numpy.int32))
    whole = torch.full((words + 16,), 0x5A, dtype=torch.uint8).pin_memory() if pinned else guard.full((words + 16,), 0x5A, dtype=torch.uint8, device='cuda')
    dev.publish_crops(planes_d, origins_d, whole[:words], ch, cw)
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert numpy.array_equal(got[:nbytes].reshape(n, ch, cw), numpy.stack(expected))
    assert (got[nbytes:words] == 0).all()                   # the pad of the last word
    assert (got[words:] == 0x5A).all()                      # the word behind it
    assert numpy.array_equal(planes_d.cpu().numpy(), planes)
    guard.check()


# ---- fetch_prefix_kernel, publish_prefix_kernel, publish_kernel ----------------------------------------------------------------------

def _prefix_lengths(one_pass, capacity):
    """Just below, at and above one pass of the grid, beyond two passes, the capacity and beyond it."""
    return (one_pass - 1, one_pass, one_pass + 1, 2*one_pass + 17, capacity, capacity + 5)


def _assert_prefix(got, source, nbytes, capacity, fill):
    copied = min(nbytes, capacity)
    rounded = -(-copied//16)*16
    assert numpy.array_equal(got[:copied], source[:copied]), nbytes
    assert numpy.array_equal(got[copied:rounded], source[copied:rounded]), nbytes      # whole 16-byte words
    assert (got[rounded:] == fill).all(), nbytes


def test_fetch_prefix_past_one_pass(guard):
    dev = _dev()
    one_pass = 16*THREADS*FETCH_BLOCKS
    capacity = 2*one_pass + 4096
    assert capacity % 16 == 0 and capacity > 2*one_pass + 17
    data = numpy.random.RandomState(capacity % 9973).randint(0, 256, size=capacity).astype(numpy.uint8)
    source = torch.from_numpy(data.copy()).pin_memory()
    for nbytes in _prefix_lengths(one_pass, capacity):
        destination = guard.full((capacity,), 0x5A, dtype=torch.uint8, device='cuda')
        dev.fetch_prefix(source, destination, guard.upload(numpy.array([nbytes], dtype=numpy.int64)))
        torch.cuda.synchronize()
        _assert_prefix(destination.cpu().numpy(), data, nbytes, capacity, 0x5A)
        guard.check()
    assert numpy.array_equal(source.numpy(), data)


def test_publish_prefix_past_one_pass(guard):
    dev = _dev()
    one_pass = 16*THREADS*PREFIX_BLOCKS
    capacity = 2*one_pass + 4096
    assert capacity % 16 == 0 and capacity > 2*one_pass + 17
    data = numpy.random.RandomState(capacity % 9967).randint(0, 256, size=capacity).astype(numpy.uint8)
    source = guard.upload(data)
    for nbytes in _prefix_lengths(one_pass, capacity):
        pinned = torch.full((capacity,), 0xA5, dtype=torch.uint8).pin_memory()
        dev.publish_prefix(source, pinned, guard.upload(numpy.array([nbytes], dtype=numpy.int64)))
        torch.cuda.synchronize()
        _assert_prefix(pinned.numpy(), data, nbytes, capacity, 0xA5)
    assert numpy.array_equal(source.cpu().numpy(), data)
    guard.check()


def test_publish_to_host_past_one_pass(guard):
    """The launch copies all of a tensor, so the lengths are tensor sizes: slices of one source into slices of one pinned buffer,
    whose rest keeps its fill."""
    dev = _dev()
    one_pass = THREADS*PUBLISH_BLOCKS                       # dwords
    capacity = 2*one_pass + 1024 + 17
    data = numpy.random.RandomState(one_pass).randint(-2**31, 2**31, size=capacity + 8, dtype=numpy.int64).astype(numpy.int32)
    source = guard.upload(data)
    for words in (one_pass - 1, one_pass, one_pass + 1, 2*one_pass + 17, capacity):
        pinned = torch.full((capacity + 8,), 0x5A5A5A5A, dtype=torch.int32).pin_memory()
        dev.publish_to_host(source[:words], pinned[:words])
        torch.cuda.synchronize()
        got = pinned.numpy()
        assert numpy.array_equal(got[:words], data[:words]), words
        assert (got[words:] == 0x5A5A5A5A).all(), words
    assert numpy.array_equal(source.cpu().numpy(), data)
    guard.check()


# ---- cast_bt601_kernel, sse_kernel ---------------------------------------------------------------------------------------------------

def test_cast_bt601_past_the_block_cap(guard):
    dev = _dev()
    count = THREADS*CAST_BLOCKS + 9000
    assert count > THREADS*CAST_BLOCKS                      # more elements than lanes: the grid-stride loop runs
    rng = numpy.random.RandomState(601)
    x = rng.uniform(0., 260., size=count).astype(numpy.float32)
    ties = numpy.arange(14.5, 238., 1., dtype=numpy.float32)                 # every half between two levels, and beyond both clips
    for at in (0, THREADS*CAST_BLOCKS - 100, count - ties.size):             # in the first trip, across the cap, at the very end
        x[at:at + ties.size] = ties
    expected = numpy.round(x.clip(min=16., max=235.)).astype(numpy.uint8)
    got = dev.cast_bt601(guard.upload(x))
    assert got.dtype == torch.uint8 and numpy.array_equal(got.cpu().numpy(), expected)
    guard.check()


def test_sse_u8_past_the_blocks_per_image_cap(guard):
    dev = _dev()
    (n, h, w) = (2, 513, 515)
    assert h*w > SSE_PIXELS_PER_BLOCK*SSE_BLOCKS_PER_IMAGE and (h*w) % 2 == 1         # the 64-block cap is taken; image 1 starts at an odd address
    rng = numpy.random.RandomState(h + w)
    a = rng.randint(0, 256, size=(n, h, w)).astype(numpy.uint8)
    b = rng.randint(0, 256, size=(n, h, w)).astype(numpy.uint8)
    b[1, -1, -1] = 255 - a[1, -1, -1]//128*255                                          # the last pixel counts, and plenty
    expected = ((a.astype(numpy.int64) - b.astype(numpy.int64))**2).sum(axis=(1, 2))
    got = dev.sse_u8(guard.upload(a), guard.upload(b))
    assert got.dtype == torch.int64 and numpy.array_equal(got.cpu().numpy(), expected)
    full = numpy.full((n, h, w), 255, dtype=numpy.uint8)
    assert dev.sse_u8(guard.upload(full), guard.upload(numpy.zeros_like(full))).cpu().tolist() == [65025*h*w]*n
    guard.check()


# ---- tile_stitch_u8_kernel with a reference --------------------------------------------------------------------------------------------

def test_tile_stitch_with_a_reference_when_lanes_loop(guard):
    from autoencoder_based_image_compression_amd import pipeline
    dev = _dev()
    (n, h, w) = (2, 37, 35)                                 # latents: planes of 592 x 560 pixels
    (plan, (wh, ww)) = pipeline.tile_plan(n, h, w, (30, 31), 2, 1)
    window_chunks = 16*wh*ww
    blocks = -(-window_chunks//(THREADS*STITCH_CHUNKS_PER_LANE))
    assert window_chunks > THREADS*STITCH_CHUNKS_PER_LANE and blocks > 1            # several blocks per window ...
    interiors = 16*plan[:, 7]*plan[:, 8]
    assert interiors.max() > 2*blocks*THREADS*TILE_UNROLL                            # ... whose lanes take a third trip,
    assert len(set((interiors > blocks*THREADS*TILE_UNROLL).tolist())) == 2          # next to windows done in one
    rng = numpy.random.RandomState(wh*ww)
    plane = rng.randint(0, 256, size=(n, 16*h, 16*w)).astype(numpy.uint8)
    windows = rng.randint(0, 256, size=(len(plan), 16*wh, 16*ww)).astype(numpy.uint8)
    expected = numpy.zeros_like(plane)
    for (g, (img, wr, wc, ir, ic, orow, ocol, er, ec)) in enumerate(plan.tolist()):
        expected[img, 16*orow:16*(orow + er), 16*ocol:16*(ocol + ec)] = windows[g, 16*ir:16*(ir + er), 16*ic:16*(ic + ec)]
    d = expected.astype(numpy.int64) - plane.astype(numpy.int64)
    (plane_d, plan_d, windows_d) = (guard.upload(plane), guard.upload(plan), guard.upload(windows))
    image = guard.empty(plane.shape, dtype=torch.uint8, device='cuda')               # the interiors cover the plane: every element is written
    sse = dev.tile_stitch_u8(windows_d, plan_d, plan, image=image, ref_u8=plane_d)
    assert numpy.array_equal(image.cpu().numpy(), expected)
    assert numpy.array_equal(sse.cpu().numpy(), (d*d).sum(axis=(1, 2)))
    assert numpy.array_equal(dev.tile_stitch_u8(windows_d, plan_d, plan, ref_u8=plane_d).cpu().numpy(), (d*d).sum(axis=(1, 2)))
    guard.check()
