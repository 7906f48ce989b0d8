"""`device.colour_quality_rest` (`eae_hip_colour_quality_rest`, csrc/hip/colour.hip) against the numpy rule
`ratecontrol.colour_luma_max_sse`, exactly.

Every buffer lies between guard bands (tests/guarded.py) under the two poisons 0xFF and 0x7F; the output starts as poison, so a picture
no lane wrote keeps it. N = 1, 3 and 65 pictures (a lane owns one picture, so 65 pictures need a second wave), and 257 once, for the
second block. The thresholds run from 0 to 2^62; the chroma errors from 0 to more than any threshold; pictures sit at the clamp
(sse_cb + sse_cr = M, M + 1, M - 1, sse_cb alone = M and M + 1) and near 2^62, where M - sse_cb - sse_cr must not leave int64 on
the way. Each operand is read from, and the output written to, pinned host memory once. The refusals of the entry point and of the
wrapper come last: nothing is launched by any of them."""
import numpy
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F)
BAD = -1                             # EAE_HIP_BAD_ARGUMENT
COUNTS = (1, 3, 65)
TOP = 1 << 62
NAMES = ('max_sse', 'sse_cb', 'sse_cr')
# (M, sse_cb, sse_cr) at 0, at the clamp and near 2^62
EDGES = ((0, 0, 0), (TOP, 0, 0), (TOP, TOP, 0), (TOP, TOP - 1, 1), (TOP, TOP - 1, 2), (TOP, 1, TOP - 2), (TOP, TOP, TOP),
         (TOP, (1 << 63) - 1, (1 << 63) - 1), (1000, 400, 600), (1000, 400, 601), (1000, 400, 599), (1000, 1000, 0), (1000, 1001, 0),
         (0, 5, 0), (1, 0, 0), (TOP - 1, TOP >> 1, TOP >> 1))


def _dev():
    from autoencoder_based_image_compression_amd import device
    return device


@pytest.fixture(params=POISONS, ids=['ff', '7f'])
def guard(request):
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


def _case(n, first_edge=0):
    """(max_sse, sse_cb, sse_cr) as numpy, the edges from `first_edge` on in front, and what the host rule gives for them."""
    from autoencoder_based_image_compression_amd import ratecontrol
    rng = numpy.random.RandomState(77*n + first_edge)
    arrays = [rng.randint(0, 3000000, size=n, dtype=numpy.int64), rng.randint(0, 1500000, size=n, dtype=numpy.int64),
              rng.randint(0, 1500000, size=n, dtype=numpy.int64)]
    edges = (EDGES[first_edge:] + EDGES[:first_edge])[:n]
    for (i, edge) in enumerate(edges):
        for (array, value) in zip(arrays, edge):
            array[n - 1 - i if n > len(EDGES) else i] = value           # in a long batch: at its end, in the last wave
    return tuple(arrays), ratecontrol.colour_luma_max_sse(*arrays)


def _big(m, cb, cr):
    return max(int(m) - int(cb) - int(cr), 0)


def _run(guard, arguments, pinned=()):
    tensors = [torch.from_numpy(a.copy()).pin_memory() if name in pinned else guard.upload(a) for (name, a) in zip(NAMES, arguments)]
    n = arguments[0].shape[0]
    if 'out' in pinned:
        out = torch.full((n,), -1 if guard.poison == 0xFF else 0x7F7F7F7F7F7F7F7F, dtype=torch.int64).pin_memory()
    else:
        out = guard.empty((n,), dtype=torch.int64, device='cuda')               # poison: -1 or 0x7F7F...
    assert _dev().colour_quality_rest(*tensors, out) is out
    torch.cuda.synchronize()
    return (out.cpu() if out.is_cuda else out).numpy().copy()


def test_the_host_rule_is_big_integer_arithmetic_on_these_cases():
    for n in COUNTS + (257,):
        for first_edge in range(0, len(EDGES), 3):
            ((m, cb, cr), expected) = _case(n, first_edge)
            assert expected.tolist() == [_big(*row) for row in zip(m.tolist(), cb.tolist(), cr.tolist())]
    ((m, cb, cr), expected) = _case(65)
    assert (expected == 0).any() and (expected > 0).any() and TOP in expected.tolist() and m.max() == TOP


@pytest.mark.parametrize('first_edge', range(0, len(EDGES), 3))
@pytest.mark.parametrize('n', COUNTS)
def test_the_kernel_equals_the_host_rule(guard, n, first_edge):
    (arguments, expected) = _case(n, first_edge)
    got = _run(guard, arguments)
    assert got.dtype == numpy.int64 and numpy.array_equal(got, expected)
    guard.check()


def test_a_second_block(guard):
    (arguments, expected) = _case(257)
    got = _run(guard, arguments)
    assert numpy.array_equal(got, expected) and got[256] == expected[256] == _big(*EDGES[0])
    guard.check()


@pytest.mark.parametrize('pinned', [('max_sse', 'out'), ('sse_cb',), ('sse_cr',), ('max_sse', 'sse_cb', 'sse_cr', 'out')],
                         ids=['thresholds_and_out', 'cb', 'cr', 'all'])
def test_pinned_host_memory_on_either_side(guard, pinned):
    (arguments, expected) = _case(65, 3)
    assert numpy.array_equal(_run(guard, arguments, pinned), expected)
    guard.check()


def test_a_slice_of_a_pinned_block_is_an_operand(guard):
    """What `codec.ColourQualityCodec` passes: the first N words of a chroma slot's pinned block of N + 1."""
    ((m, cb, cr), expected) = _case(3, 6)
    blocks = [torch.from_numpy(numpy.concatenate([a, [-7]])).pin_memory() for a in (cb, cr)]
    out = guard.empty((3,), dtype=torch.int64, device='cuda')
    _dev().colour_quality_rest(guard.upload(m), blocks[0][:3], blocks[1][:3], out)
    torch.cuda.synchronize()
    assert numpy.array_equal(out.cpu().numpy(), expected)
    guard.check()


def test_refused_before_any_launch(guard):
    from autoencoder_based_image_compression_amd import _native
    dev = _dev()
    lib = _native.hip()
    n = 5
    (arguments, expected) = _case(n)
    tensors = [guard.upload(a) for a in arguments]
    out = guard.full((n + 1,), 0x5A5A, dtype=torch.int64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    good = tuple(t.data_ptr() for t in tensors) + (out.data_ptr(), n)
    names = NAMES + ('out', 'n')

    def but(**changed):
        return tuple(changed.get(name, value) for (name, value) in zip(names, good))

    refused = [but(**{name: None}) for name in names[:4]]                                                    # null pointers
    refused += [but(**{name: good[names.index(name)] + 4}) for name in names[:4]]                            # 64-bit words off by 4
    refused += [but(n=0), but(n=-1)]                                                                         # not positive
    for arguments in refused:
        assert lib.eae_hip_colour_quality_rest(*arguments, stream) == BAD, arguments
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())                                                                       # nothing was launched
    assert lib.eae_hip_colour_quality_rest(*good, stream) == 0                                               # and what is accepted
    torch.cuda.synchronize()
    assert out[:n].cpu().tolist() == expected.tolist() and int(out[n]) == 0x5A5A
    out.fill_(0x5A5A)
    (m, cb, cr) = tensors
    for bad in (lambda: dev.colour_quality_rest(m.int(), cb, cr, out[:n]),                                   # dtypes
                lambda: dev.colour_quality_rest(m, cb.int(), cr, out[:n]),
                lambda: dev.colour_quality_rest(m, cb, cr, out[:n].int()),
                lambda: dev.colour_quality_rest(m, cb[:n - 1], cr, out[:n]),                                 # one per picture
                lambda: dev.colour_quality_rest(m, cb, cr, out),
                lambda: dev.colour_quality_rest(m[::2], cb[::2], cr[::2], out[:n][::2]),                     # not contiguous
                lambda: dev.colour_quality_rest(m.view(n, 1), cb.view(n, 1), cr.view(n, 1), out[:n].view(n, 1)),      # not [N]
                lambda: dev.colour_quality_rest(m[:0], cb[:0], cr[:0], out[:0]),                             # no picture
                lambda: dev.colour_quality_rest(torch.zeros(n, dtype=torch.int64), cb, cr, out[:n])):        # host memory that is not pinned
        with pytest.raises(dev.HipError):
            bad()
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())
