"""`device.tconv9x9s4_luma_frame` (`eae_hip_tconv9x9s4_luma_frame`, csrc/hip/tconv3.hip): transpose_conv_3 whose
squared error is over the real pixels of a padded plane, out of the kernel's own epilogue.

Equality is exact, on integers. The reference is the EXISTING entry point: `device.tconv9x9s4_luma(want_u8=True)`'s plane, with the
squared error summed in numpy over `[:real_h, :real_w]` against the reference frame. Inputs of 16 x 24 sites (coded 64 x 96: two tile
rows, a partial second tile column), 8 x 12 sites (coded 32 x 48) and 4 x 4 sites (coded 16 x 16), three planes each; real sizes that cut
a four-pixel group at every position (83 = 4*20 + 3, 81 = 4*20 + 1, 42 = 4*10 + 2, 13, 1), that end on a group (64, 32, 16), that lie
in the first tile column only (33 x 65 leaves one pixel in the second), one short of the coded plane (63 x 95) and the coded plane
itself, where the sum is what `eae_hip_tconv9x9s4_luma` adds. The reference frame's bytes outside the real rectangle are random, not
replicated, and a second frame that differs from the first exactly there gives the same sums. The accumulators start non-zero. The
planes, where requested, are the existing entry point's bit for bit over the whole coded plane; every buffer lies between guard bands
(tests/guarded.py) under two poisons. One case runs past the persistent grid's cap, as tests/test_gpu_capped_grids.py does for the
existing kernel."""
import functools

import numpy
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F)
BAD = -1                             # EAE_HIP_BAD_ARGUMENT
NB_PLANES = 3
SITES = ((16, 24), (8, 12), (4, 4))
REAL_SIZES = ((64, 96), (50, 83), (63, 95), (49, 81), (33, 65), (32, 64), (25, 42), (16, 13), (1, 1))
CASES = [(sites, real) for sites in SITES for real in REAL_SIZES if real[0] <= 4*sites[0] and real[1] <= 4*sites[1]]
INITIAL = (5, 0, 1 << 40)            # what the accumulators hold before the launch
T3_BLOCKS_PER_CU = 3                 # tconv3.hip: BLOCKS_PER_CU (tests/test_gpu_capped_grids.py checks the line)
(T3_TILE_H, T3_TILE_W) = (8, 16)     # tconv3.hip: TH, TW: input sites per tile


def _dev():
    from autoencoder_based_image_compression_amd import device
    return device


@pytest.fixture(params=POISONS, ids=['ff', '7f'])
def guard(request):
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


def _inputs(shape, seed):
    """(x, w6, frame): positive weights and inputs, so that the reconstruction spans the BT.601 range, and a random reference frame."""
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables
    (n, h, w) = shape
    v = variables.random_variables(1., False, seed=7, bias_std=0.01)
    rng = numpy.random.RandomState(seed)
    gain = 8.*9./(min(h, 3)*min(w, 3))
    w6 = (numpy.absolute(v['decoder/weights_6'])*numpy.float32(gain)).astype(numpy.float32)
    x = (rng.standard_normal(size=shape + (128,)) + 1.5).astype(numpy.float32)
    frame = rng.randint(0, 256, size=(n, 4*h, 4*w)).astype(numpy.uint8)
    return x, w6, frame


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """The inputs of one shape and what the EXISTING entry point makes of them, computed once and left unchanged: its float32 and
    uint8 planes and the squared error it adds against the whole frame."""
    dev = _dev()
    (x, w6, frame) = _inputs(shape, seed=shape[1]*100 + shape[2])
    wph = dev.pack_tconv9x9s4_weights(torch.from_numpy(w6).cuda())
    (f32, u8, sse) = dev.tconv9x9s4_luma(torch.from_numpy(x).cuda(), wph, want_f32=True, want_u8=True, ref_u8=torch.from_numpy(frame).cuda())
    torch.cuda.synchronize()
    return {'x': x, 'w6': w6, 'frame': frame, 'f32': f32.cpu().numpy(), 'u8': u8.cpu().numpy(), 'sse_whole': sse.cpu().numpy()}


def _sse(u8, frame, real):
    difference = frame[:, :real[0], :real[1]].astype(numpy.int64) - u8[:, :real[0], :real[1]].astype(numpy.int64)
    return (difference*difference).reshape(u8.shape[0], -1).sum(axis=1)


def _initial(n):
    return numpy.array([INITIAL[i % len(INITIAL)] for i in range(n)], dtype=numpy.int64)


def test_the_cases_cover_what_they_claim():
    assert len(CASES) == 9 + 3 + 2 and ((4, 4), (16, 13)) in CASES and ((8, 12), (25, 42)) in CASES and ((8, 12), (33, 65)) not in CASES
    assert {real[1] % 4 for (_, real) in CASES} == {0, 1, 2, 3}            # a group cut behind its first, second and third pixel, and none
    assert -(-16//T3_TILE_H) == 2 and -(-24//T3_TILE_W) == 2 and 24 % T3_TILE_W != 0


@pytest.mark.parametrize('sites,real', CASES, ids=['{0}x{1}_real_{2}x{3}'.format(*(s + r)) for (s, r) in CASES])
def test_the_error_is_over_the_real_pixels(guard, sites, real):
    dev = _dev()
    shape = (NB_PLANES,) + sites
    r = _reference(shape)
    assert len(numpy.unique(r['u8'])) > 4                   # the data exercises the cast, not only the clip floor
    expected = _sse(r['u8'], r['frame'], real)
    whole = (4*sites[0], 4*sites[1])
    if real != whole:
        assert (expected < r['sse_whole']).all()            # the pixels left out carry error: a sum over the coded plane differs
    wph = dev.pack_tconv9x9s4_weights(guard.upload(r['w6']))
    x = guard.upload(r['x'])
    frame = guard.upload(r['frame'])
    # both planes and the error
    sse = guard.upload(_initial(NB_PLANES))
    (f32, u8, got) = dev.tconv9x9s4_luma_frame(x, wph, real, want_f32=True, want_u8=True, ref_u8=frame, sse=sse)
    assert got is sse
    assert numpy.array_equal(f32.cpu().numpy().view(numpy.uint32), r['f32'].view(numpy.uint32))
    assert numpy.array_equal(u8.cpu().numpy(), r['u8'])
    assert numpy.array_equal(sse.cpu().numpy(), _initial(NB_PLANES) + expected)
    # the probe's form: the error alone, into accumulators the wrapper makes
    (f32, u8, got) = dev.tconv9x9s4_luma_frame(x, wph, real, want_f32=False, want_u8=False, ref_u8=frame)
    assert f32 is None and u8 is None and numpy.array_equal(got.cpu().numpy(), expected)
    # another frame outside the real rectangle, the same inside: the same sums
    other = numpy.random.RandomState(5).randint(0, 256, size=r['frame'].shape).astype(numpy.uint8)
    other[other == r['frame']] ^= 0xFF
    other[:, :real[0], :real[1]] = r['frame'][:, :real[0], :real[1]]
    (_, _, got) = dev.tconv9x9s4_luma_frame(x, wph, real, want_f32=False, want_u8=False, ref_u8=guard.upload(other))
    assert numpy.array_equal(got.cpu().numpy(), expected)
    assert numpy.array_equal(x.cpu().numpy(), r['x']) and numpy.array_equal(frame.cpu().numpy(), r['frame'])
    guard.check()


@pytest.mark.parametrize('sites', SITES, ids=['{0}x{1}'.format(*s) for s in SITES])
def test_at_the_coded_size_it_adds_what_the_existing_entry_point_adds(guard, sites):
    dev = _dev()
    r = _reference((NB_PLANES,) + sites)
    wph = dev.pack_tconv9x9s4_weights(guard.upload(r['w6']))
    (x, frame) = (guard.upload(r['x']), guard.upload(r['frame']))
    (sse_frame, sse_whole) = (guard.upload(_initial(NB_PLANES)), guard.upload(_initial(NB_PLANES)))
    (_, u8_frame, _) = dev.tconv9x9s4_luma_frame(x, wph, (4*sites[0], 4*sites[1]), want_u8=True, ref_u8=frame, sse=sse_frame)
    (_, u8_whole, _) = dev.tconv9x9s4_luma(x, wph, want_u8=True, ref_u8=frame, sse=sse_whole)
    assert numpy.array_equal(sse_frame.cpu().numpy(), sse_whole.cpu().numpy())
    assert numpy.array_equal(sse_whole.cpu().numpy(), _initial(NB_PLANES) + r['sse_whole'])
    assert numpy.array_equal(u8_frame.cpu().numpy(), u8_whole.cpu().numpy())
    guard.check()


def test_planes_without_a_reference(guard):
    dev = _dev()
    r = _reference((NB_PLANES, 8, 12))
    wph = dev.pack_tconv9x9s4_weights(guard.upload(r['w6']))
    (f32, u8, sse) = dev.tconv9x9s4_luma_frame(guard.upload(r['x']), wph, (25, 42), want_f32=True, want_u8=True)
    assert sse is None and numpy.array_equal(u8.cpu().numpy(), r['u8'])
    assert numpy.array_equal(f32.cpu().numpy().view(numpy.uint32), r['f32'].view(numpy.uint32))
    guard.check()


def test_a_real_size_outside_the_coded_plane_is_refused(guard):
    from autoencoder_based_image_compression_amd import _native
    dev = _dev()
    lib = _native.hip()
    (n, h, w) = (NB_PLANES, 4, 4)
    r = _reference((n, h, w))
    wph = dev.pack_tconv9x9s4_weights(guard.upload(r['w6']))
    (x, frame) = (guard.upload(r['x']), guard.upload(r['frame']))
    sse = guard.full((n,), 0x5A5A, dtype=torch.int64, device='cuda')
    u8 = guard.full((n, 4*h, 4*w), 0x5A, dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    front = (x.data_ptr(), wph.data_ptr(), None, u8.data_ptr(), frame.data_ptr(), sse.data_ptr(), n, h, w)
    for real in ((0, 16), (16, 0), (-1, 16), (16, -1), (17, 16), (16, 17), (0, 0), (1 << 30, 1), (1, 1 << 30)):
        assert lib.eae_hip_tconv9x9s4_luma_frame(*front, real[0], real[1], stream) == BAD, real
        with pytest.raises(dev.HipError):
            dev.tconv9x9s4_luma_frame(x, wph, real, want_u8=False, ref_u8=frame, sse=sse)
    # what the existing entry point refuses: nothing asked for, a reference without accumulators
    assert lib.eae_hip_tconv9x9s4_luma_frame(x.data_ptr(), wph.data_ptr(), None, None, None, None, n, h, w, 16, 16, stream) == BAD
    assert lib.eae_hip_tconv9x9s4_luma_frame(x.data_ptr(), wph.data_ptr(), None, u8.data_ptr(), frame.data_ptr(), None, n, h, w, 16, 16, stream) == BAD
    with pytest.raises(dev.HipError):                        # a reference that is not the coded frame
        dev.tconv9x9s4_luma_frame(x, wph, (13, 13), want_u8=False, ref_u8=frame[:, :13, :13].contiguous(), sse=sse)
    torch.cuda.synchronize()
    assert bool((sse == 0x5A5A).all()) and bool((u8 == 0x5A).all())          # nothing was launched
    assert lib.eae_hip_tconv9x9s4_luma_frame(*front, 16, 16, stream) == 0     # and what is accepted
    torch.cuda.synchronize()
    assert numpy.array_equal(sse.cpu().numpy(), 0x5A5A + r['sse_whole']) and numpy.array_equal(u8.cpu().numpy(), r['u8'])
    guard.check()


def test_past_the_persistent_grids_cap(guard):
    """grid + 1 tiles, the fewest a launch needs for one block to take a second tile: one plane, one tile row, grid + 1 tile columns.
    The real rectangle ends inside the last tile, 37 pixels short of the coded width, so the tile a block takes second is masked by
    its own origin."""
    dev = _dev()
    grid = -(-T3_BLOCKS_PER_CU*dev.device_info()['compute_units']//8)*8
    shape = (1, 1, T3_TILE_W*(grid + 1))
    n_tiles = shape[0]*(-(-shape[1]//T3_TILE_H))*(-(-shape[2]//T3_TILE_W))
    assert n_tiles > T3_BLOCKS_PER_CU*dev.device_info()['compute_units'] and n_tiles == grid + 1
    real = (3, 4*shape[2] - 37)
    assert real[1] > 4*T3_TILE_W*grid and real[1] % 4 == 3
    r = _reference(shape)
    expected = _sse(r['u8'], r['frame'], real)
    assert expected[0] < r['sse_whole'][0]
    wph = dev.pack_tconv9x9s4_weights(guard.upload(r['w6']))
    sse = guard.upload(_initial(1))
    (_, u8, _) = dev.tconv9x9s4_luma_frame(guard.upload(r['x']), wph, real, want_u8=True, ref_u8=guard.upload(r['frame']), sse=sse)
    assert numpy.array_equal(u8.cpu().numpy(), r['u8'])
    assert numpy.array_equal(sse.cpu().numpy(), _initial(1) + expected)
    guard.check()
