"""Poisoned buffers between guard bands for the kernel parity tests (a plain helper module: import it, no fixture lives here).

The parity tests compare what a kernel wrote with an oracle. They do not control the memory the kernel writes into or reads next to:
an output from `torch.empty` very likely still holds the previous, correct, answer of the same shape (the caching allocator hands
the block out again), a store one position past a ragged edge lands in the allocator's slack, and a load past the last image reads
whatever the pool holds, usually zeros. `Guard` closes the three gaps:

* every allocation is `band + nbytes + band` bytes, ALL of them filled with a poison byte first, and the interior is returned as a
  contiguous view of the requested dtype and shape: an element the kernel never writes keeps the poison and fails the test's own
  bit-exact comparison;
* `check()` asserts that both bands of every allocation still hold the poison: a write outside the tensor is reported with the
  allocation and the first changed offset relative to the interior;
* inputs go between bands as well (`upload`), and a test runs under two poisons: a kernel whose defined outputs differ between the
  two runs reads outside its inputs.

Poison bytes: 0xFF reads as NaN in float32 / float64, 255 as uint8 and -1 as int16 / int32 / int64; 0x7F as 3.4e38 in float32, 1.4e306
in float64, 127 as uint8, 32639 as int16. (Not 0xA5 for floats: as float32 it is -2.9e-16, which an O(1) FMA chain absorbs without
changing a bit.)

What this does NOT catch: the bands are `band_bytes` = 4096 bytes wide on each side -- wider than any single store or load group of
these kernels (the largest are 16 bytes x 64 lanes = 1 KB) and a multiple of every alignment the ABI asks for -- so an overrun that
JUMPS further than 4096 bytes beyond a tensor lands outside them and is not seen; neither is an out-of-tensor READ that happens to
give the same defined outputs under both poisons. Requests above `passthrough_bytes`, pinned ones, (unless `cpu=True`) host ones
and those made while the current stream captures a graph (the poison fill would be recorded, not run) go to torch unchanged. The
guard keeps every allocation alive until `check()`, so a test that bounds the peak of allocated memory sees what the guard holds.

`guarded(modules, poison)` swaps the module-global `torch` of the listed package modules (device, pipeline; container where a test
needs it; codec where the resident codecs' slots are to lie between bands, tests/test_gpu_codec_slots.py) for a proxy that forwards
everything to torch except the six allocation functions, and checks the bands on exit. A new
kernel test should allocate through it: add the module-level autouse fixture the kernel-level GPU modules carry, and upload the
inputs with `Guard.upload` where reads matter.
"""
import contextlib
import math
import os
import sys

import torch

ALIGN = 4096
ALLOCATORS = ('empty', 'zeros', 'full', 'empty_like', 'zeros_like', 'full_like')


def _shape(size):
    """torch's size arguments: empty(2, 3), empty((2, 3)), empty(torch.Size(...)), empty(5)."""
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def _caller():
    """Name of the function that asked for the allocation: the nearest frame outside this file."""
    frame = sys._getframe(1)
    here = os.path.abspath(__file__)
    while frame is not None and os.path.abspath(frame.f_code.co_filename) == here:
        frame = frame.f_back
    return frame.f_code.co_name if frame is not None else '?'


class _Allocation(object):
    def __init__(self, raw, start, nbytes, shape, dtype, caller):
        (self.raw, self.start, self.nbytes, self.shape, self.dtype, self.caller) = (raw, start, nbytes, shape, dtype, caller)

    def describe(self):
        return '{0} {1} allocated in {2}()'.format(self.shape, self.dtype, self.caller)


class Guard(object):
    """Allocator of poisoned buffers between guard bands; see the module's docstring. cpu=True guards host tensors too (the guard's
    own tests); by default only device requests are guarded."""

    def __init__(self, poison_byte, band_bytes=4096, passthrough_bytes=256 << 20, cpu=False):
        if not 0 <= int(poison_byte) <= 255:
            raise ValueError('`poison_byte` must be one byte')
        if band_bytes <= 0 or band_bytes % ALIGN:
            raise ValueError('`band_bytes` must be a positive multiple of {}'.format(ALIGN))
        self.poison = int(poison_byte)
        self.band = int(band_bytes)
        self.passthrough_bytes = int(passthrough_bytes)
        self.cpu = bool(cpu)
        self._live = []

    # ---- the layout ------------------------------------------------------------------------------------------------------------
    def _passes_through(self, nbytes, device, kwargs):
        if kwargs.get('pin_memory') or kwargs.get('out') is not None or kwargs.get('requires_grad'):
            return True
        if kwargs.get('layout', torch.strided) is not torch.strided:
            return True
        if kwargs.get('memory_format', torch.contiguous_format) not in (torch.contiguous_format, torch.preserve_format):
            return True
        if nbytes > self.passthrough_bytes:
            return True
        if torch.device(device).type == 'cpu':
            return not self.cpu
        # inside a graph capture the poison fill would be recorded, not run: the bands would hold whatever the pool held
        return torch.cuda.is_current_stream_capturing()

    def _allocate(self, shape, dtype, device, value=None):
        """[slack to the next 4096-byte address][band][interior, nbytes][band]: band and interior start at multiples of 4096 and
        the upper band starts at the interior's last byte + 1. Everything is poisoned; `value` then goes into the interior."""
        itemsize = torch.empty((), dtype=dtype).element_size()
        nbytes = int(math.prod(shape))*itemsize
        raw = torch.empty(ALIGN + 2*self.band + nbytes, dtype=torch.uint8, device=device)
        raw.fill_(self.poison)
        start = (-raw.data_ptr()) % ALIGN + self.band
        interior = raw[start:start + nbytes].view(dtype).view(shape)
        if value is not None:
            interior.fill_(value)
        self._live.append(_Allocation(raw, start, nbytes, shape, dtype, _caller()))
        return interior

    def _new(self, name, shape, value, dtype, device, kwargs):
        if dtype is None:
            dtype = torch.full((), value).dtype if name == 'full' else torch.get_default_dtype()
        device = device if device is not None else 'cpu'
        itemsize = torch.empty((), dtype=dtype).element_size()
        if self._passes_through(int(math.prod(shape))*itemsize, device, kwargs):
            if name == 'full':
                return torch.full(shape, value, dtype=dtype, device=device, **kwargs)
            return getattr(torch, name)(shape, dtype=dtype, device=device, **kwargs)
        kwargs.pop('memory_format', None)
        kwargs.pop('layout', None)
        kwargs.pop('pin_memory', None)
        kwargs.pop('requires_grad', None)
        kwargs.pop('out', None)
        if kwargs:
            raise TypeError('guarded.{0}: unexpected arguments {1}'.format(name, sorted(kwargs)))
        return self._allocate(shape, dtype, device, value)

    # ---- torch's six allocation functions -----------------------------------------------------------------------------------------
    def empty(self, *size, dtype=None, device=None, **kwargs):
        return self._new('empty', _shape(size), None, dtype, device, kwargs)

    def zeros(self, *size, dtype=None, device=None, **kwargs):
        return self._new('zeros', _shape(size), 0, dtype, device, kwargs)

    def full(self, size, fill_value, dtype=None, device=None, **kwargs):
        return self._new('full', _shape((size,)), fill_value, dtype, device, kwargs)

    def empty_like(self, x, dtype=None, device=None, **kwargs):
        return self._new('empty', tuple(x.shape), None, dtype if dtype is not None else x.dtype, device if device is not None else x.device, kwargs)

    def zeros_like(self, x, dtype=None, device=None, **kwargs):
        return self._new('zeros', tuple(x.shape), 0, dtype if dtype is not None else x.dtype, device if device is not None else x.device, kwargs)

    def full_like(self, x, fill_value, dtype=None, device=None, **kwargs):
        return self._new('full', tuple(x.shape), fill_value, dtype if dtype is not None else x.dtype,
                         device if device is not None else x.device, kwargs)

    def upload(self, array, device='cuda'):
        """A numpy array as an input between bands on `device`: host data in the interior, poison all around."""
        import numpy
        host = torch.from_numpy(numpy.ascontiguousarray(array))
        if self._passes_through(host.numel()*host.element_size(), device, {}):
            return host.to(device)
        interior = self._allocate(tuple(host.shape), host.dtype, device)
        interior.copy_(host)
        return interior

    # ---- the check ----------------------------------------------------------------------------------------------------------------
    def _bands(self, a):
        return a.raw[a.start - self.band:a.start], a.raw[a.start + a.nbytes:a.start + a.nbytes + self.band]

    def check(self, keep=False):
        """Asserts that every band of every allocation since the last check still holds the poison byte, then drops the references.
        On failure: the allocation (shape, dtype, the function that allocated it) and the first changed offset relative to the
        interior (negative: in front of it; >= nbytes: behind it).
        keep=True: the bands are verified and the allocations stay with the guard -- a test that checks after every step of a resident
        codec (tests/test_gpu_codec_slots.py) learns which step overran, and the exit's check still covers the slots' buffers. A failed
        check drops the references either way."""
        (live, self._live) = (self._live, [])
        if not live:
            return
        flags = {}
        for a in live:                         # one comparison per allocation, one device -> host copy per device
            (lower, upper) = self._bands(a)
            flags.setdefault(a.raw.device, []).append((torch.count_nonzero(lower != self.poison) + torch.count_nonzero(upper != self.poison)).reshape(1))
        touched = []
        for (device, parts) in flags.items():
            touched += torch.cat(parts).cpu().tolist()
        order = [a for device in flags for a in live if a.raw.device == device]
        failures = []
        for (a, count) in zip(order, touched):
            if not count:
                continue
            (lower, upper) = self._bands(a)
            changed = torch.nonzero(lower != self.poison)
            offset = int(changed[0, 0]) - self.band if changed.numel() else a.nbytes + int(torch.nonzero(upper != self.poison)[0, 0])
            failures.append('{0}: {1} band bytes changed, the first at offset {2} of the interior ({3} bytes)'.format(
                a.describe(), count, offset, a.nbytes))
        assert not failures, 'written outside a tensor (poison 0x{0:02X}):\n  '.format(self.poison) + '\n  '.join(failures)
        if keep:
            self._live = live + self._live


class _TorchProxy(object):
    """`torch` for a package module: every attribute is torch's except the six allocation functions."""

    def __init__(self, guard):
        self._guard = guard

    def __getattr__(self, name):
        if name in ALLOCATORS:
            return getattr(self._guard, name)
        return getattr(torch, name)


@contextlib.contextmanager
def guarded(modules, poison, **guard_arguments):
    """Replaces the module-global `torch` of each module in `modules` with a proxy whose six allocation functions are a `Guard`'s;
    yields the Guard. On exit the modules get their `torch` back (also after an exception) and, when the body did not raise, the
    bands are checked. Objects captured at import (device._raw_stream) are unaffected."""
    guard = Guard(poison, **guard_arguments)
    proxy = _TorchProxy(guard)
    saved = [(module, module.torch) for module in modules]
    for (module, _) in saved:
        module.torch = proxy
    try:
        yield guard
    except BaseException:
        guard._live = []
        raise
    finally:
        for (module, original) in saved:
            module.torch = original
    guard.check()
