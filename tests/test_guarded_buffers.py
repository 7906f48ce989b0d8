"""tests/guarded.py has teeth: each kind of miss -- an element never written, a byte written in front of or behind a tensor, a read
outside an input -- is detected, on host tensors with small fake "kernels" written with torch indexing. CPU only."""
import types

import numpy
import pytest
import torch

import guarded

POISONS = (0xFF, 0x7F)
DTYPES = (torch.float32, torch.float64, torch.uint8, torch.int16, torch.int32)


def _reference(dtype):
    return (torch.arange(12, dtype=torch.float64).reshape(4, 3)*7 + 1).to(dtype)


def _kernel(out, rows):
    """Writes the first `rows` rows of the reference into `out`."""
    out[:rows] = _reference(out.dtype)[:rows]


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_an_unwritten_last_row_fails_the_bit_exact_comparison(poison, dtype):
    guard = guarded.Guard(poison, cpu=True)
    ref = _reference(dtype).numpy()
    whole = guard.empty((4, 3), dtype=dtype)
    _kernel(whole, 4)
    assert numpy.array_equal(whole.numpy(), ref)
    short = guard.empty_like(whole)
    _kernel(short, 3)
    assert numpy.array_equal(short.numpy()[:3], ref[:3])
    assert not numpy.array_equal(short.numpy(), ref)
    assert not numpy.any(short.numpy()[3] == ref[3])          # every element of the unwritten row differs, not only one
    guard.check()


def test_the_poison_bytes_read_as_documented():
    ff = guarded.Guard(0xFF, cpu=True)
    assert torch.isnan(ff.empty(5, dtype=torch.float32)).all() and torch.isnan(ff.empty(5, dtype=torch.float64)).all()
    assert ff.empty(5, dtype=torch.uint8).tolist() == [255]*5
    assert ff.empty(5, dtype=torch.int16).tolist() == [-1]*5 and ff.empty(5, dtype=torch.int32).tolist() == [-1]*5
    sf = guarded.Guard(0x7F, cpu=True)
    f32 = sf.empty(5, dtype=torch.float32)
    f64 = sf.empty(5, dtype=torch.float64)
    assert (f32 > 3.3e38).all() and torch.isfinite(f32).all() and (f64 > 1.3e306).all() and torch.isfinite(f64).all()
    assert sf.empty(5, dtype=torch.uint8).tolist() == [127]*5 and sf.empty(5, dtype=torch.int16).tolist() == [32639]*5


def _raw_of(guard, index=-1):
    a = guard._live[index]
    return a.raw, a.start, a.nbytes


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('where', ['under', 'over'])
def test_one_byte_outside_the_interior_fails_the_check_with_its_offset(poison, where):
    guard = guarded.Guard(poison, cpu=True)

    def allocating_function():
        return guard.empty((3, 5), dtype=torch.int16)
    guard.zeros(7, dtype=torch.float32)                  # an untouched neighbour: not named in the failure
    t = allocating_function()
    (raw, start, nbytes) = _raw_of(guard)
    assert nbytes == 30 and raw[start:].data_ptr() == t.data_ptr()
    offset = -1 if where == 'under' else nbytes
    raw[start + offset] = 0
    with pytest.raises(AssertionError) as failure:
        guard.check()
    message = str(failure.value)
    assert 'offset {} of the interior'.format(offset) in message
    assert '(3, 5)' in message and 'torch.int16' in message and 'allocating_function' in message
    assert '(7,)' not in message
    guard.check()                                          # the references were dropped: nothing left to check


@pytest.mark.parametrize('poison', POISONS)
def test_writes_inside_the_interior_pass_the_check(poison):
    guard = guarded.Guard(poison, cpu=True)
    t = guard.empty(33, dtype=torch.uint8)
    t.fill_(0)
    u = guard.empty((0, 4), dtype=torch.float32)          # an empty tensor has bands too
    assert u.shape == (0, 4)
    guard.check()


def test_a_read_outside_an_uploaded_input_shows_between_the_two_poisons():
    data = numpy.arange(10, dtype=numpy.uint8)

    def sloppy(x):                                        # sums 4-byte words and takes one byte too many
        return int(torch.as_strided(x, (11,), (1,)).to(torch.int64).sum())

    def tidy(x):
        return int(x.to(torch.int64).sum())
    results = {}
    for poison in POISONS:
        guard = guarded.Guard(poison, cpu=True)
        x = guard.upload(data, device='cpu')
        assert numpy.array_equal(x.numpy(), data) and x.is_contiguous() and x.data_ptr() % 4096 == 0
        results[poison] = (sloppy(x), tidy(x))
        guard.check()                                     # a read leaves the bands alone: only the comparison shows it
    assert results[0xFF][1] == results[0x7F][1] == 45
    assert results[0xFF][0] != results[0x7F][0]


@pytest.mark.parametrize('poison', POISONS)
def test_layout_values_and_views(poison):
    guard = guarded.Guard(poison, cpu=True)
    x = guard.empty(2, 3, 128, dtype=torch.float32)
    tensors = [x, guard.empty((5, 7), dtype=torch.int16), guard.empty(torch.Size((3,)), dtype=torch.float64),
               guard.empty_like(x, dtype=torch.int16), guard.zeros((4, 9), dtype=torch.int32), guard.zeros(6, dtype=torch.int64),
               guard.zeros_like(x), guard.full((3, 3), 2.5, dtype=torch.float32), guard.full_like(x, 7, dtype=torch.uint8),
               guard.upload(numpy.ones((3, 5), dtype=numpy.float32), device='cpu')]
    for t in tensors:
        assert t.is_contiguous() and t.data_ptr() % 4096 == 0
    assert tensors[3].shape == x.shape and tensors[3].dtype == torch.int16
    assert tensors[4].shape == (4, 9) and int(tensors[4].abs().sum()) == 0 and int(tensors[5].abs().sum()) == 0
    assert tensors[6].dtype == torch.float32 and float(tensors[6].abs().sum()) == 0.
    assert (tensors[7] == 2.5).all() and (tensors[8] == 7).all() and tensors[8].shape == x.shape
    for a in guard._live:                                # bands and interior start at multiples of 4096, the bands are poisoned
        assert (a.raw.data_ptr() + a.start) % 4096 == 0
        (lower, upper) = guard._bands(a)
        assert lower.numel() == upper.numel() == 4096 and (lower == poison).all() and (upper == poison).all()
        assert (lower.data_ptr() % 4096, upper.data_ptr() - a.raw.data_ptr() - a.start) == (0, a.nbytes)
    guard.check()


def test_requests_that_pass_through_are_plain_torch_tensors():
    guard = guarded.Guard(0xFF, passthrough_bytes=1024, cpu=True)
    big = guard.zeros(1025, dtype=torch.uint8)
    small = guard.zeros(1024, dtype=torch.uint8)
    assert len(guard._live) == 1 and big.untyped_storage().nbytes() == 1025 and small.untyped_storage().nbytes() > 2*4096
    host_only = guarded.Guard(0xFF)                        # the default: host requests are torch's own
    plain = host_only.zeros(1, dtype=torch.int32)
    assert not host_only._live and plain.untyped_storage().nbytes() == 4 and plain.tolist() == [0]
    assert host_only.empty((2, 2)).shape == (2, 2) and host_only.full((2,), 3).tolist() == [3, 3] and not host_only._live
    assert host_only.upload(numpy.arange(3), device='cpu').tolist() == [0, 1, 2] and not host_only._live


def _fake_module():
    module = types.ModuleType('fake_device')
    module.torch = torch
    exec('def make(n):\n    return torch.empty(n, dtype=torch.int32, device=torch.device("cpu")), torch.arange(n)', module.__dict__)
    return module


def test_guarded_swaps_torch_and_restores_it():
    (a, b) = (_fake_module(), _fake_module())
    with guarded.guarded((a, b), 0xFF, cpu=True) as guard:
        assert a.torch is not torch and b.torch is a.torch
        (t, r) = a.make(4)
        assert t.tolist() == [-1]*4 and r.tolist() == [0, 1, 2, 3]          # the allocation is the guard's, the rest is torch's
        assert guard._live[0].caller == 'make'
    assert a.torch is torch and b.torch is torch
    with pytest.raises(KeyError):
        with guarded.guarded((a, b), 0x7F, cpu=True):
            a.make(2)
            raise KeyError('inside')
    assert a.torch is torch and b.torch is torch


def test_guarded_checks_the_bands_on_exit():
    a = _fake_module()
    with pytest.raises(AssertionError, match='offset 16 of the interior'):
        with guarded.guarded((a,), 0xFF, cpu=True) as guard:
            a.make(4)
            (raw, start, nbytes) = _raw_of(guard)
            raw[start + nbytes] = 1
    assert a.torch is torch


def test_the_package_modules_have_a_swappable_torch():
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), 0xFF):
        assert device.torch is pipeline.torch and device.torch is not torch
        assert device.torch.float32 is torch.float32 and device.torch.cuda is torch.cuda
    assert device.torch is torch and pipeline.torch is torch


@pytest.mark.parametrize('poison', POISONS)
def test_check_keep_verifies_without_dropping(poison):
    """`check(keep=True)` between the steps of a resident codec: the bands are verified, the allocations stay for the next check, and
    an overrun between two checks is reported by the later one."""
    guard = guarded.Guard(poison, cpu=True)
    t = guard.empty(10, dtype=torch.uint8)
    guard.check(keep=True)
    assert len(guard._live) == 1
    u = guard.zeros(3, dtype=torch.int32)
    guard.check(keep=True)
    assert [a.nbytes for a in guard._live] == [10, 12]           # in the order they were made
    (raw, start, nbytes) = _raw_of(guard, 0)
    raw[start + nbytes + 5] = 1
    with pytest.raises(AssertionError, match='offset 15 of the interior'):
        guard.check(keep=True)
    assert not guard._live and t.numel() == 10 and u.tolist() == [0, 0, 0]      # a failed check drops the references
    guard.check()
