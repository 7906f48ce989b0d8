"""The whole hot path for a batch of images as one asynchronous call: what the body of `fix_gamma`
(kodak_tensorflow/reconstructing_eae_kodak.py:144-147, 170-225) does per image with `sess.run`, numpy and 127 Cython
calls, issued here as a dozen launches over arrays that stay in HBM:

    conv1+GDN1 -> conv2+GDN2 -> conv3 -> [GDN3 -> centre / quantise / int16 symbols / dead-map flags -> IGDN4]
    -> exception-map histograms
    -> (side stream) lossless coder: encode every map, decode it back, compare                 lossless/compression.py:84-154
    -> tconv1+IGDN5 -> tconv2+IGDN6 -> tconv3 + BT.601 cast + squared error against the input  tools.py:61-93, 831-881

`BatchCodec.submit` only enqueues; `Ticket.result()` returns, per image, the quantities `fix_gamma` stores: the number
of bits of the lossless code (coder bits of the 127 ordinary maps + ceil(h*w*entropy) of the exception map,
compression.py:68-81), the squared error (-> `tls.psnr_2d`), the number of dead maps (`tls.count_nb_deads`), and, on
request, the uint8 reconstruction. The values equal those of the reference-shaped functions of `kodak/` on the same
inputs (tests/test_gpu_codec.py); `bench.py` times exactly this class.

Concurrency: the coder is a few latency-bound wavefronts, so its launches go to side streams and overlap the synthesis
transforms of the same batch and the analysis transforms of the next ones; `nb_in_flight` batches of coder work may be
pending. Buffers that cross streams are preallocated per slot (`_Slot`: everything one step in flight owns); results reach
the host through a kernel that writes pinned memory (no hipMemcpyAsync on the launch thread) and a worker thread turns them
into per-image numbers; it polls its events and sleeps in between instead of spinning in `synchronize()` (eight ranks share one host CPU quota). For small batches the
step can be replayed as three hipGraphs per slot (`use_graphs`) over several transform streams (`nb_transform_streams`).
"""
import contextlib
import os
import queue
import threading
import time
import weakref

import numpy
import torch

from . import colour as colour_rules
from . import container as container_format
from . import device as dev
from . import pipeline
from .kodak.eae.graph import constants as csts
from .kodak.lossless import compression as lossless_compression

# HIP multiplexes streams onto 4 hardware queues: side streams are shared by every codec of the process so that a coder
# stream never ends up on the hardware queue of the stream the transforms run on. One list per device AND kind: a codec's
# coder streams are coder streams for every other codec too, whatever their `nb_in_flight`.
_SIDE_STREAMS = {}          # (device index, kind) -> list of streams
# The result worker polls its events and sleeps in between: `Event.synchronize()` was measured to spin a whole CPU per
# process (with blocking events too), and eight ranks share one 16-CPU quota. 0 restores synchronize().
_POLL_SECONDS = float(os.environ.get('EAE_WORKER_POLL_SECONDS', '0.0002'))
# How the result worker learns that a batch is through. 'sequence' (default): the last launch of the coder side and of the synthesis
# side bumps a step counter that lands in pinned host memory (device.publish_sequence); the worker, which knows how many times the
# slot has been submitted, reads that word -- no HIP call and no event recorded for it, so the worker can never disturb a stream
# capture (`_capture_all`), and a poll is a load. Measured against 'events' (round 3-4's way: one event per side per step,
# `event.query()` every 0.2 ms; profiles/r05_wait_modes.log, r05_host_cpu_threads.log): same throughput within 0.5 %, the worker's
# own CPU 0.7-0.9 ms per 3.0 ms step either way, and the 2.85 ms per step the HIP runtime's signal thread spends in
# kfd_wait_on_events (system time) does NOT move: it does not come from the host's events.
_WAIT_MODE = os.environ.get('EAE_WORKER_WAIT', 'sequence')
if _WAIT_MODE not in ('sequence', 'events'):
    raise ValueError('EAE_WORKER_WAIT={0!r}: expected "sequence" or "events"'.format(_WAIT_MODE))
# Where a batch's coder work starts. The coder's first kernel is wide (binarise: one wavefront per map, 3,048 of them for 24 Kodak
# images) and, launched the moment the symbols exist, runs exactly while transpose_conv_1 does -- the shortest of the conv GEMM
# launches, which it stretched from 0.29 to 0.34 ms. '1': the coder stream waits for transpose_conv_1 instead (its wide pass then
# falls into transpose_conv_2's 1.07 ms: tconv1 0.339 -> 0.304 ms, 0.66 -> 0.73 of peak; the step is the same within 0.1 %,
# profiles/r05_coder_behind_tconv1.log). For one or two images per batch the step IS the coder's chain and starting it a launch
# later only adds to it (one image 1.23 -> 1.37 ms): there the coder starts as soon as the symbols exist. '0' / '1' force either.
_CODER_BEHIND_TCONV1 = os.environ.get('EAE_CODER_BEHIND_TCONV1')
# (0.1 ms between polls, behind the one long sleep of `_Worker._wait_sequence`: one image at a time 1.09 -> 1.05 ms against 0.2 ms, 0.03 ms more CPU per step)
_SEQUENCE_POLL_SECONDS = float(os.environ.get('EAE_WORKER_SEQUENCE_POLL_SECONDS', '0.0001'))
_SEQUENCE_TIMEOUT_SECONDS = float(os.environ.get('EAE_WORKER_SEQUENCE_TIMEOUT_SECONDS', '60'))
_LONG_SLEEP = os.environ.get('EAE_WORKER_LONG_SLEEP', '1') != '0'      # the one long sleep in front of the polls (`_Worker._wait_sequence`)
# `Ticket.result()` called before anybody has started on the ticket's step does the waiting and the bookkeeping ITSELF (the caller is
# blocked anyway: no wake-up of the worker, no hand-over back), and around the moment the step is expected it watches the step counter
# without sleeping, for at most this long (seconds of one CPU per call; 0 = never: sleeps and polls like the worker)
_RESULT_SPIN_SECONDS = float(os.environ.get('EAE_RESULT_SPIN_SECONDS', '0.00015'))
_RESULT_BY_CALLER = os.environ.get('EAE_RESULT_BY_CALLER', '1') != '0'      # 0: results are always formed by the worker thread (rounds 1-5)
_EARLY_PUBLISH = os.environ.get('EAE_EARLY_PUBLISH', '1') != '0'            # 0: a small step's analysis-side blocks reach the host with the coder's only


def _short_sleeps_for_this_thread():
    """PR_SET_TIMERSLACK = 1 us for the calling thread (Linux rounds a sleep up by the slack, 50 us by default)."""
    try:
        import ctypes
        ctypes.CDLL(None, use_errno=True).prctl(29, 1000, 0, 0, 0)
    except Exception:
        pass


# Stream priorities (experiments: scratch/r04): EAE_TRANSFORM_STREAM_PRIORITY / EAE_CODER_STREAM_PRIORITY, torch's numbering
# (-1 high, 0 normal); unset = the runtime's default for both.
def _priority(name):
    """Parsed once at import: a malformed value fails here, not inside some constructor later."""
    text = os.environ.get(name)
    if text is None:
        return None
    try:
        return int(text)
    except ValueError:
        raise ValueError('{0}={1!r}: expected an integer stream priority (-1 high, 0 normal)'.format(name, text))


_PRIORITY = {'transform': _priority('EAE_TRANSFORM_STREAM_PRIORITY'), 'coder': _priority('EAE_CODER_STREAM_PRIORITY')}
# Codecs of this process that have not been closed, per device: a graph capture waits until the others are idle (`_capture_all`).
# Weak references: a codec dropped without close() is still collected (its __del__ closes it).
_LIVE = {}                  # device index -> weakref.WeakSet of BatchCodec
_LIVE_LOCK = threading.Lock()


def _side_streams(count, device, kind='coder'):
    """The first `count` streams of the process-wide list of the device for this kind ('coder' / 'transform')."""
    streams = _SIDE_STREAMS.setdefault((device.index, kind), [])
    while len(streams) < count:
        if _PRIORITY[kind] is not None:
            streams.append(torch.cuda.Stream(device=device, priority=_PRIORITY[kind]))
        else:
            streams.append(torch.cuda.Stream(device=device))
    return streams[:count]


def _step_streams(count, device):
    """`count` streams for `one_stream_steps`: the device's transform streams as far as they exist, then its existing coder streams,
    and only then new (transform) streams."""
    existing_transform = len(_SIDE_STREAMS.get((device.index, 'transform'), ()))
    from_coder = min(len(_SIDE_STREAMS.get((device.index, 'coder'), ())), max(0, count - existing_transform))
    return _side_streams(count - from_coder, device, kind='transform') + _side_streams(from_coder, device)


class Ticket(object):
    """Handle on one submitted batch."""

    def __init__(self, nb_images):
        self.nb_images = nb_images
        self._done = threading.Event()
        self._error = None
        self._values = None
        self.reconstruction_uint8 = None      # device tensor when the codec keeps reconstructions
        self.reconstruction_host = None       # numpy uint8 (a view of the slot's pinned buffer) with BatchCodec(fetch_reconstruction=True),
        #                                       after result(); valid until the slot comes round again (nb_slots submits later)
        self.fed_event = None                 # host input: recorded behind the host -> device copy (the caller's pinned batch may
        #                                       be rewritten once it has completed)
        self.decoded_event = None             # with keep_reconstruction: recorded behind the synthesis transform: wait for it on another
        #                                       stream before reading `reconstruction_uint8` there (valid until the slot comes round again)
        self._coder_span = None               # (start, stop) timing events on the coder stream (BatchCodec(time_coder=True))
        self._job = None                      # (_Job, _Worker) until somebody has started on the step's results
        self._container_parts = None          # with BatchCodec(emit_container=True): what `container()` is assembled from, owned by the ticket

    def coder_ms(self):
        """Milliseconds the coder launches of this batch took on their stream (from the moment the symbols were ready to the
        publication of the results), other work sharing the GPU. Only with `BatchCodec(time_coder=True)`, after `result()`."""
        if self._coder_span is None:
            raise RuntimeError('the codec was not built with time_coder=True')
        return self._coder_span[0].elapsed_time(self._coder_span[1])

    def result(self):
        """Blocks until the batch is through; dict of numpy arrays, one entry per image:
        'nb_bits' int64 (lossless code incl. the exception map's entropy cost), 'coder_bits' int64, 'exception_bits' int64,
        'sse' int64 (sum of squared uint8 differences), 'nb_deads' int64.
        When the result worker has not started on this step yet (one step at a time: the caller is here a few microseconds after
        `submit`), the calling thread waits for the device and forms the results itself (`_Worker.process`)."""
        _wait_for_ticket(self)
        return self._values

    def _parts(self):
        self.result()
        parts = self._container_parts
        if parts is None:
            raise RuntimeError('the codec was not built with emit_container=True')
        if parts['error'] is not None:
            raise parts['error']
        if parts['payload'] is None:
            raise ContainerOverflow('the payload of this step takes {0} bytes, the codec holds {1} per step '
                                    '(BatchCodec(container_capacity_bytes=...))'.format(parts['payload_bytes'], parts['capacity']))
        return parts

    def container(self):
        """Blocks like `result()` (and raises the step's error like it); the batch as one `EAE1` blob (container.py), the bytes
        `container.encode_images` gives for the same images (`EAT1`, and `encode_images(..., coding_tile=...)`, with
        `BatchCodec(coding_tile=...)`). The codec has decoded every stream in it and compared the symbols.
        Raises `ContainerOverflow` when the payload did not fit `container_capacity_bytes`. Only with
        `BatchCodec(emit_container=True)`; before or after `result()`."""
        parts = self._parts()
        return container_format.assemble_blob(*(parts['head'] + (parts['rows'], parts['bits'], parts['payload'])),
                                              coding_tile=parts['coding_tile'], image_size=parts.get('image_size'))[0]

    def image_containers(self):
        """Like `container()`: one single-image `EAE1` (`EAT1`) blob per image of the batch (the payload is image-major: slices of
        the batch's, each behind its own header)."""
        parts = self._parts()
        return container_format.assemble_image_blobs(*(parts['head'] + (parts['rows'], parts['bits'], parts['payload'])),
                                                     coding_tile=parts['coding_tile'], image_size=parts.get('image_size'))


class ContainerOverflow(RuntimeError):
    """The coded payload of a step is larger than the codec's `container_capacity_bytes`: the step's results stand, its container
    was not produced."""


class StepTimeout(RuntimeError):
    """The device did not report a submitted step within EAE_WORKER_SEQUENCE_TIMEOUT_SECONDS: the codec is unusable from here on."""


class _Claimable(object):
    """A step's job: whoever claims it first -- the result worker taking it off its queue, or the caller's `result()` -- waits for
    the device and forms the results."""
    __slots__ = ('_claimed',)

    def __init__(self):
        self._claimed = threading.Lock()

    def claim(self):
        return self._claimed.acquire(False)


def _wait_for_ticket(ticket):
    """`result()` of either kind of ticket: when nobody has started on the step yet, the calling thread waits for the device and forms
    the results itself (`process(job, by_caller=True)` of the ticket's worker); then the step's own error, if any, is raised."""
    pending = ticket._job
    if pending is not None:
        ticket._job = None
        (job, worker) = pending
        if _RESULT_BY_CALLER and not ticket._done.is_set() and job.claim():
            worker.process(job, by_caller=True)
    ticket._done.wait()
    if ticket._error is not None:
        raise ticket._error


class _Job(_Claimable):
    """What the results of one submitted step are made from; whoever claims it first -- the result worker taking it off its queue, or
    the caller's `Ticket.result()` -- waits for the device and forms the results.
    events: what `_Worker._wait` waits for ('events' wait mode; else empty); views: the slot's pinned blocks (results, histograms,
    overflow, flags, checks, squared errors) as host arrays; symbols_host: the pinned symbols (host coder) or None; recount:
    `BatchCodec._recount_exception_maps` of the slot; fetch: `BatchCodec._fetch_job` or None; sequence: (the slot's step counters in
    pinned memory, the values this step leaves there) or None; early_published: the synthesis side's publication carried the
    analysis side's blocks too (exception-map histograms, dead-map flags, range check): small steps, whose caller waits for each
    result -- `BatchCodec._early_publish`; emit: with `emit_container`, (the blob's fixed parts, capacity, the slot's pinned payload,
    exception rows and index words as host arrays), else None."""
    __slots__ = ('ticket', 'events', 'views', 'symbols_host', 'slot_free', 'recount', 'fetch', 'sequence', 'early_published', 'emit')

    def __init__(self, ticket, events, views, symbols_host, slot_free, recount, fetch, sequence, early_published=False, emit=None):
        super(_Job, self).__init__()
        self.ticket = ticket
        self.events = events
        self.views = views
        self.symbols_host = symbols_host
        self.slot_free = slot_free
        self.recount = recount
        self.fetch = fetch
        self.sequence = sequence
        self.early_published = bool(early_published)
        self.emit = emit


_THREAD = threading.local()


class _StepWorker(threading.Thread):
    """The thread, the queue of jobs and the waits for a step's counters that `BatchCodec`'s and `BatchDecoder`'s result workers
    share; a subclass says in `process(job, by_caller=False)` what a finished step's results are made of."""

    def __init__(self):
        super(_StepWorker, self).__init__(daemon=True)
        self.jobs = queue.Queue()

    @staticmethod
    def _wait(event):
        if _POLL_SECONDS > 0.:
            while not event.query():
                time.sleep(_POLL_SECONDS)
        else:
            event.synchronize()

    _typical_wait = 0.      # seconds this thread lately had to wait per job (a running mean): `_wait_sequence` sleeps through most of it
    _alone = 0              # consecutive jobs that found nothing queued behind them (one step at a time)
    failed = None           # StepTimeout: the device stopped reporting; the codec refuses further work (BatchCodec.submit)
    _sleep = staticmethod(time.sleep)          # (a test drives `_wait_sequence` with a clock of its own: tests/test_host_logic.py)
    _now = staticmethod(time.monotonic)

    _caller_waits = ()      # the last waits of `_wait_sequence_by_caller` (seconds)

    def _wait_sequence_by_caller(self, words, expected, early=None):
        """`_wait_sequence` for the thread that called `Ticket.result()` on a step nobody had started on: that thread is blocked
        anyway, so nothing is handed over and what is left is to notice the device's last write as soon as it lands. ONE sleep up to
        shortly before the moment the step is expected to be through -- the shortest of the last three such waits, less a third of the
        spin budget: a lower bound as long as the regime lasts, and a change of regime (another shape of use, steps queued behind each
        other) shows as waits that differ, which switches the sleep off --, then the step counter is read in a loop for at most
        EAE_RESULT_SPIN_SECONDS of CPU, then polls like the worker's.
        early: called once the LAST counter (the synthesis side, which reports long before the coder's chains end when the step is
        small) has been reached, if that happens inside the sleep: the part of the results that does not come from the coder is
        formed while the coder still runs (`process`: 0.06 of the 0.09 ms between the device's last write and `result()` returning)."""
        started = self._now()
        waits = self._caller_waits
        steady = _LONG_SLEEP and len(waits) == 3 and max(waits) < 1.25*min(waits)
        wake = started + (min(waits) - _RESULT_SPIN_SECONDS/3.) if steady else started
        deadline = None
        if early is not None and len(expected) > 1:
            last = len(expected) - 1
            while wake - self._now() > 2.*_SEQUENCE_POLL_SECONDS:
                if ((int(words[last]) - expected[last]) & 0xFFFFFFFF) < 0x80000000:
                    early()
                    early = None
                    break
                self._sleep(min(2.*_SEQUENCE_POLL_SECONDS, wake - self._now()))
        if wake - self._now() > _SEQUENCE_POLL_SECONDS:
            self._sleep(wake - self._now())
        spin_until = self._now() + _RESULT_SPIN_SECONDS
        for (index, value) in enumerate(expected):
            while ((int(words[index]) - value) & 0xFFFFFFFF) >= 0x80000000:      # words[index] < value, wrap-around safe
                now = self._now()
                if now < spin_until:
                    continue
                self._sleep(0.5*_SEQUENCE_POLL_SECONDS)
                if deadline is None:
                    deadline = now + _SEQUENCE_TIMEOUT_SECONDS
                elif now > deadline:
                    raise StepTimeout('the device has not reported step {0} of this slot after {1:.0f} s (step counter at {2}): the slot\'s '
                                      'buffers may still be written to, so this codec takes no further batches -- close it'.format(
                                          value, _SEQUENCE_TIMEOUT_SECONDS, int(words[index])))
        self._caller_waits = (waits + (min(self._now() - started, 0.05),))[-3:]

    def _wait_sequence(self, words, expected):
        """Until the step counters the device leaves in pinned memory (`words`: numpy int32 view) have reached `expected`. Every
        sleep is a system call and a wake-up of this thread (a fifth of its time per step at twelve polls a step): the first sleep
        is three quarters of what the wait has lately been, the polls come after it."""
        deadline = None
        started = self._now()
        # (only in a steady regime -- more jobs queued behind this one, or one job at a time for a while: the last batches of a pipelined
        # run have the GPU to themselves and come back sooner than the mean says, and sleeping through that cost 20-step blocks 3 %:
        # 2,990 against 3,080 Mpx/s)
        queued = self.jobs.qsize()
        self._alone = self._alone + 1 if queued == 0 else 0
        steady = _LONG_SLEEP and (queued >= 2 or self._alone >= 4) and self._typical_wait > 4.*_SEQUENCE_POLL_SECONDS
        first = 0.75*self._typical_wait if steady else 0.
        poll = 0.5*_SEQUENCE_POLL_SECONDS if self._alone >= 4 else _SEQUENCE_POLL_SECONDS      # one step at a time: the caller is waiting for this
        for (index, value) in enumerate(expected):
            while ((int(words[index]) - value) & 0xFFFFFFFF) >= 0x80000000:      # words[index] < value, wrap-around safe
                self._sleep(max(first, poll))
                first = 0.
                if deadline is None:
                    deadline = self._now() + _SEQUENCE_TIMEOUT_SECONDS
                elif self._now() > deadline:
                    raise StepTimeout('the device has not reported step {0} of this slot after {1:.0f} s (step counter at {2}): the slot\'s '
                                      'buffers may still be written to, so this codec takes no further batches -- close it'.format(
                                          value, _SEQUENCE_TIMEOUT_SECONDS, int(words[index])))
        waited = min(self._now() - started, 0.05)
        if queued >= 2 or self._alone >= 3:      # (a regime change shows in the mean after a few jobs: `first` is a lower bound by then)
            self._typical_wait = waited if self._alone == 3 else self._typical_wait + 0.25*(waited - self._typical_wait)
        elif self._typical_wait == 0.:
            self._typical_wait = waited

    def run(self):
        _short_sleeps_for_this_thread()
        while True:
            job = self.jobs.get()
            if job is None:
                return
            if job.claim():          # (else the caller's `Ticket.result()` got there first and does it itself)
                self.process(job)


class _Worker(_StepWorker):
    """The result worker of `BatchCodec`."""
    image_size = None       # of a codec that pads (`BatchCodec(pad=True)`): the real size its containers carry

    def __init__(self, map_size, nb_maps, host_probabilities, idx_map_exception, host_threads, coding_tile=None, payload_order=None):
        """coding_tile, payload_order: of a codec that codes in tiles (`coding_tile_layout`): the slot's results are in run order,
        and `payload_order` (int64, one index per stream) takes them into the order of the payload."""
        super(_Worker, self).__init__()
        self.coding_tile = coding_tile
        self.payload_order = payload_order
        self.map_size = map_size
        self.nb_maps = nb_maps
        self.host_probabilities = host_probabilities
        self.idx_map_exception = idx_map_exception
        self.host_threads = host_threads

    def _exception_map_error(self, results):
        """The exception the first failed exception map of a step stands for, or None."""
        exception_maps = numpy.arange(self.idx_map_exception, results.shape[1], self.nb_maps)
        bad = exception_maps[results[2, exception_maps] != 0]
        if bad.size == 0:
            return None
        if int(results[2, bad[0]]) == 6:
            return AssertionError('\nArrays are not equal\nThe lossless compression has altered the centered quantized data.')
        from .kodak.lossless import interface_cython
        try:
            interface_cython.raise_for_status(int(results[2, bad[0]]), int(results[3, bad[0]]))
        except Exception as exc:
            return exc
        return None

    def process(self, job, by_caller=False):
        """Waits until the device is through with the step, then forms the ticket's results from the slot's pinned blocks (or the
        exception `result()` raises), frees the slot. On the worker thread, or on the caller's (`Ticket.result()`)."""
        ticket = job.ticket
        try:
            if by_caller and not getattr(_THREAD, 'short_sleeps', False):
                _short_sleeps_for_this_thread()
                _THREAD.short_sleeps = True
            (results, hist, overflow, flags, checks, sse) = [v if isinstance(v, numpy.ndarray) else v.numpy() for v in job.views]
            early = {}

            def early_part():
                """Everything that does not come from the coder: in pinned memory once the synthesis side has reported, i.e. while the
                coder's chains still run when the step is small. Nothing is raised from here (the slot is still in use): an
                exception is kept and raised behind the waits, after the ones the old order put in front of it."""
                # the last word of the squared-error block: tiles that a cut conv launch of this batch left unfinished
                # (device.conv_workspace_collect); nothing of this batch can be trusted then
                early['unfinished'] = int(sse[-1])
                early['sse'] = sse[:-1].astype(numpy.int64).copy()
                early['out_of_range'] = int(checks[0]) != 0
                early['nb_deads'] = (flags == 0).sum(axis=1).astype(numpy.int64)
                early['exception_bits'] = numpy.zeros(ticket.nb_images, dtype=numpy.int64)
                try:
                    if hist.size and early['unfinished'] == 0 and not early['out_of_range']:
                        rows = hist
                        if int(overflow.sum()) != 0:
                            # a symbol beyond +-hist_radius: the reference's histogram runs from the smallest to the largest symbol
                            # whatever they are (lossless/compression.py:68-75, tools.py:376-388), so count again over all of int16
                            rows = job.recount()
                        early['exception_bits'] = lossless_compression.exception_maps_nb_bits(rows.astype(numpy.int64), self.map_size)
                except Exception as exc:
                    early['error'] = exc

            if job.sequence is not None:
                if by_caller:
                    self._wait_sequence_by_caller(*job.sequence, early=early_part if job.early_published else None)
                else:
                    self._wait_sequence(*job.sequence)
            for event in job.events:
                self._wait(event)
            if job.fetch is not None:
                # The copy back is issued HERE, behind events that have completed: on this runtime an asynchronous copy
                # whose stream still waits for an event holds the calling thread until it can start (the launch thread would
                # submit the next step only after this one is decoded: 4.5 instead of 3.2 ms per step).
                (reconstruction, pinned, stream) = job.fetch
                with torch.cuda.device(reconstruction.device), torch.cuda.stream(stream):
                    pinned.copy_(reconstruction, non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record()
                self._wait(copied)
                ticket.reconstruction_host = pinned.numpy()
            if not early:
                early_part()
            if early['unfinished'] != 0:
                raise dev.SplitHandOffTimeout('{} tiles of a cut conv launch were not handed over: the results of this batch '
                                              'are invalid (the workspace has been reset; later batches are unaffected)'.format(early['unfinished']))
            if job.symbols_host is not None:
                # encode + decode + compare per map on the host cores, like compress_lossless + the caller's assert
                (_, nb_bits) = lossless_compression.code_planar_symbols(job.symbols_host.numpy(), self.host_probabilities,
                                                                       self.idx_map_exception, nb_threads=self.host_threads,
                                                                       roundtrip=True, verify_only=True)
                results = numpy.zeros_like(results)
                results[0] = nb_bits.reshape(-1)
            if self.payload_order is not None:
                # the coder's batches keep the tiles of one shape side by side; everything below (the first failing stream, the sums
                # per image, the container's bit counts) is in the payload's order: image -> tile -> map
                results = results.take(self.payload_order, axis=1)
            status = results[2]
            exception_coded = job.emit is not None and self.idx_map_exception >= 0
            container_error = None
            if exception_coded:
                # the exception maps are coded for the container only: the step's results are those of a codec that leaves them
                # out, so a failure of theirs is the container's (`Ticket.container()` raises it)
                status = status.copy()
                status[self.idx_map_exception::self.nb_maps] = 0
                container_error = self._exception_map_error(results)
            if status.any():
                bad = int(numpy.flatnonzero(status)[0])
                if int(results[2, bad]) == 6:
                    raise AssertionError('\nArrays are not equal\nThe lossless compression has altered the centered quantized data.')
                from .kodak.lossless import interface_cython
                interface_cython.raise_for_status(int(results[2, bad]), int(results[3, bad]))
            if early['out_of_range']:
                raise AssertionError('The rounded array elements cannot be represented as 16-bit signed integers.')
            if 'error' in early:
                raise early['error']
            n = ticket.nb_images
            map_bits = (results[0].astype(numpy.int64) + results[1].astype(numpy.int64)).reshape(n, -1, self.nb_maps)      # [image, tile, map]
            if exception_coded:
                map_bits[:, :, self.idx_map_exception] = 0       # charged by its entropy, as without `emit_container`
            coder_bits = map_bits.sum(axis=(1, 2))
            exception_bits = early['exception_bits']
            ticket._values = {'nb_bits': coder_bits + exception_bits, 'coder_bits': coder_bits,
                              'exception_bits': exception_bits, 'sse': early['sse'], 'nb_deads': early['nb_deads']}
            if job.emit is not None:
                # out of the slot's pinned buffers into objects the ticket owns, while the slot is still this step's
                (head, capacity, payload, rows, index) = job.emit
                payload_bytes = int(index[0])
                ticket._values['container_bytes'] = index[2:].astype(numpy.int64)
                ticket._container_parts = {
                    'head': head, 'capacity': capacity, 'payload_bytes': payload_bytes, 'error': container_error, 'coding_tile': self.coding_tile,
                    'image_size': self.image_size,
                    'rows': rows.copy() if self.idx_map_exception >= 0 else rows[:0].copy(),
                    'bits': numpy.stack([results[0], results[1]], axis=1).astype(numpy.uint32),
                    'payload': payload[:payload_bytes].tobytes() if int(index[1]) == 0 else None}
            self._finish(job)
        except StepTimeout as exc:    # nothing says the device is through with this slot: no later submit may reuse it
            self.failed = exc
            ticket._error = exc
        except Exception as exc:      # surfaced by Ticket.result()
            ticket._error = exc
        finally:
            job.slot_free.set()
            ticket._done.set()


    def _finish(self, job):
        """What a subclass adds to a step's results while the slot is still the step's (`_BudgetWorker`); raises like `process`."""


def default_nb_in_flight(h_in, w_in):
    """Batches of coder work to keep in flight when the caller does not say. A feature map is ONE serial chain (its symbols x
    about 0.2-0.4 us each to encode, the same again to decode, stretched next to the transforms), whatever the batch; the
    transforms of a batch take a time that grows with the batch instead. Measured on MI355X in the product mode
    (profiles/r03_depth_sweep.txt, profiles/r03_i_bench.json): 24 Kodak-sized images per step (maps of 1,536 symbols): three
    to five in flight are equal within 1 % at 0.2 bpp, five is the best at 1.4 bpp and 16 % ahead of three at 3.2 bpp; 64
    images of 256x256 (maps of 256 symbols: short chains, short steps) lose 10 % with five against three; a 2048x2048 image
    has maps of 16,384 symbols and needs eight. Round 5, on the shorter chains of that round's cores (profiles/r05_coder_waves_per_block.log):
    six against five for Kodak-sized maps is equal within noise up to 2 bpp and 2 % ahead at 3.2 bpp (seven no better), so: six."""
    map_size = (-(-h_in//csts.STRIDE_PROD))*(-(-w_in//csts.STRIDE_PROD))      # of the coded size (`BatchCodec(pad=True)`: any h_in, w_in)
    return int(min(8, 3 + map_size//512))


def default_coder_chunks(n_maps):
    """Launches the coder's serial chains are cut into (`BatchCodec(coder_chunks=None)`): ONE, i.e. off. For one or two images a
    step is as long as the coder's chains laid end to end (binarise, encoder core, emit, decoder core, debinarise: 0.65 of the 1.2 ms
    one Kodak image takes), and cut into chunks on three streams the decoder trails the encoder -- but on this runtime every
    cross-stream hop costs 60-100 us (launched directly or replayed as a hipGraph), more than a chunk saves at the headline's entropy:
    one image's round trip 0.65 ms whole, 0.84 / 0.95 / 1.24 ms in 2 / 3 / 4 chunks; at 2 bpp 2.46 ms whole, 2.29 / 2.18 in 4 / 8
    chunks (profiles/r05_trailing_alone.log). So the chunked form stays an option (`coder_chunks`, EAE_CODER_CHUNKS) for long chains."""
    forced = os.environ.get('EAE_CODER_CHUNKS')
    if forced:
        return max(1, min(16, int(forced)))
    return 1


PRODUCT_TRANSFORM_STREAMS = 3      # 2 / 3 / 4 / 5 streams: 3,020 / 3,075 / 3,060 / 3,030 Mpx/s for 24 Kodak images per step, 2,550 / 2,770 / 2,740
#                                    for 64 images of 256x256 (profiles/r03_transform_streams2.txt)


def product_mode(h_in, w_in):
    """The keyword arguments of the mode a deployment (and `bench.py`'s headline) runs `BatchCodec` in: consecutive batches go
    round three private transform streams, the step is replayed as three hipGraphs, the number of coder batches in flight follows
    the map size. `BatchCodec(..., **codec.product_mode(h, w))`; the constructor's own defaults are the conservative ones (every
    launch on the caller's stream, kernel by kernel: what the per-launch hooks and the roofline leg need)."""
    return {'nb_in_flight': default_nb_in_flight(h_in, w_in), 'nb_transform_streams': PRODUCT_TRANSFORM_STREAMS, 'use_graphs': True}


_BUDGET_WARNED = [False]


def stream_budget(nb_transform_streams, nb_in_flight, hw_queues=None, copies=0):
    """Caps a codec's busy streams to the hardware queues the process has: -> (nb_transform_streams, nb_in_flight, message or None).

    The HIP runtime gives a process GPU_MAX_HW_QUEUES hardware queues (4 unless the variable says otherwise; the package sets 16 at
    import when it still can: `__init__._configure_hw_queues`); streams beyond that share queues, busy ones with busy ones, which was
    measured to cost the product mode up to 30 %. One queue is left to the caller's own stream, `copies` to the feed / fetch streams.
    Coder streams (batches in flight) go first, down to two; then the transform streams, down to one; then the coder streams again."""
    if hw_queues is None:
        from autoencoder_based_image_compression_amd import HW_QUEUES
        hw_queues = HW_QUEUES[0]
    (nt, nf) = (max(1, int(nb_transform_streams)), max(1, int(nb_in_flight)))
    budget = max(2, int(hw_queues) - 1 - int(copies))
    (nt0, nf0) = (nt, nf)
    while nt + nf > budget and nf > 2:
        nf -= 1
    while nt + nf > budget and nt > 1:
        nt -= 1
    while nt + nf > budget and nf > 1:
        nf -= 1
    message = None
    if (nt, nf) != (nt0, nf0):
        message = ('BatchCodec: {0} transform + {1} coder streams asked for, but this process has {2} hardware queues (GPU_MAX_HW_QUEUES; '
                   'streams beyond them share queues and serialise): running {3} + {4}. Set GPU_MAX_HW_QUEUES=16 in the environment before '
                   'the first GPU call, or import this package before anything initialises the GPU.'.format(nt0, nf0, hw_queues, nt, nf))
    return (nt, nf, message)


def _no_hook(name, fn):
    return fn()


def coding_tile_layout(batch_size, h, w, coding_tile, idx_map_exception=-1):
    """Where everything of a step of `BatchCodec(coding_tile=...)` lies; numpy only, the same for every step of a codec (DESIGN.md
    section 15). batch_size images of an h x w latent plane, coding_tile=(th, tw) latents, clamped to the plane. An ENTRY is one
    (image, tile): 128 maps, 128 pairs of streams. The payload, the header's bit counts and the results take the entries in
    PAYLOAD order (image -> tile, row-major); the coder takes the entries of one shape class as one batch of maps of one size, so
    the symbols, the streams, the coder's results and the offsets lie in RUN order: class after class, payload order within a
    class -- `container._group_layout` of the one group that holds every entry of the step. -> dict:
    'coding_tile' (clamped), 'nb_tiles', 'tiles' and 'classes' (`container.coding_tile_grid`), 'entries' [(image, tile)] in payload
    order, 'runs' [((rows, cols) of the class, entries, first stream, first symbol element)], class runs starting on 128-element
    boundaries, 'elements' of the symbol buffer, 'offsets' int64 [entries] (element offset of every payload-order entry's map 0),
    'plan' int64 [entries, 6] (the rows of `device.tile_symbols_gather`), 'prob_row' int32 [n_streams] in run order (map m -> row
    m, the exception map of image i -> row 128 + i), 'run_entry' int64 [entries] (run-order index of every payload-order entry),
    'payload_entry' (its inverse), 'payload_order' int64 [n_streams] (run-order stream of every payload-order stream: what
    `numpy.take` turns run-order results into payload order with), 'n_streams' = batch_size * nb_tiles * 128."""
    batch_size = container_format._positive_int(batch_size, '`batch_size`')
    (th, tw) = container_format._positive_pair(coding_tile, '`coding_tile`')
    coding_tile = (min(th, h), min(tw, w))
    (tiles, classes) = container_format.coding_tile_grid(h, w, coding_tile)
    nb_tiles = tiles.shape[0]
    nb_maps = csts.NB_MAPS_3
    entries = [(i, t) for i in range(batch_size) for t in range(nb_tiles)]
    (group_runs, offsets, elements) = container_format._group_layout(entries, tiles, classes)
    payload_entry = numpy.concatenate([numpy.asarray(ks, dtype=numpy.int64) for (_, ks, _) in group_runs])
    run_entry = numpy.empty(len(entries), dtype=numpy.int64)
    run_entry[payload_entry] = numpy.arange(len(entries), dtype=numpy.int64)
    (runs, first_entry) = ([], 0)
    for (cls, ks, first_element) in group_runs:
        runs.append((tuple(classes[cls]), len(ks), first_entry*nb_maps, int(first_element)))
        first_entry += len(ks)
    prob_row = numpy.concatenate([container_format._prob_rows(entries, ks, idx_map_exception) for (_, ks, _) in group_runs])
    payload_order = (run_entry[:, None]*nb_maps + numpy.arange(nb_maps, dtype=numpy.int64)[None, :]).reshape(-1)
    return {'coding_tile': coding_tile, 'nb_tiles': nb_tiles, 'tiles': tiles, 'classes': classes, 'entries': entries, 'runs': runs,
            'elements': int(elements), 'offsets': offsets, 'plan': container_format._symbols_plan(entries, tiles, offsets),
            'prob_row': prob_row.astype(numpy.int32), 'run_entry': run_entry, 'payload_entry': payload_entry,
            'payload_order': payload_order, 'n_streams': len(entries)*nb_maps}


def _class_batches(runs, results, tile_major, rows, offsets, length, device):
    """The coder's batches of a step in tiles, one per shape class of `runs` (`coding_tile_layout`'s or `region_layout`'s): a
    `device.CoderStreams` whose results are that class's columns of the ONE block `results`, and that class's run of the tile-major
    buffer, of the probability `rows` and of the `offsets`. The classes run one after the other on the step's stream, so one
    workspace of the largest class serves them all. -> ([(streams, tiles, rows, offsets)], bytes of that workspace)."""
    (classes, need) = ([], 0)
    for ((tile_rows, tile_cols), count, first_stream, first_element) in runs:
        (n, size) = (count*csts.NB_MAPS_3, tile_rows*tile_cols)
        streams = dev.CoderStreams(n, size, length, device, results=results[:, first_stream:first_stream + n])
        classes.append((streams, tile_major[first_element:first_element + n*size].view(n, size), rows[first_stream:first_stream + n],
                        offsets[first_stream:first_stream + n]))
        need = max(need, dev.coder_workspace_bytes(n, size, length))
    return classes, need


class _Slot(object):
    """Everything one step in flight owns; `BatchCodec` goes round `nb_slots` of them. Made once: no launch and no submit cuts a view."""
    __slots__ = ('block', 'out', 'results', 'hist', 'overflow', 'flags', 'checks', 'sse', 'unfinished', 'pinned_out', 'pinned_sse',
                 'host_views', 'symbols', 'symbols_2d', 'coder_streams', 'workspace', 'conv_ws', 'seq_dev', 'pinned_seq', 'seq_host',
                 'coder_seq', 'synthesis_seq', 'counts', 'free', 'pinned_symbols', 'staging', 'pinned_rec', 'graphs', 'table', 'exception_rows',
                 'index', 'payload_bytes', 'offsets', 'payload', 'pinned_payload', 'emit_tail', 'pinned_emit', 'emit_host', 'gathered',
                 'classes')

    def __init__(self, codec):
        (batch_size, nb_maps, device) = (codec.batch_size, codec.nb_maps, codec.device)
        n_maps = batch_size*nb_maps
        n_streams = codec._n_streams      # pairs of streams the coder leaves results for: n_maps, times the tiles of a map with a coding tile
        nb_hist = batch_size if codec.idx_map_exception >= 0 else 0
        hist_width = 2*codec.hist_radius + 1
        layout = (4*n_streams, nb_hist*hist_width, nb_hist, n_maps, 4)
        nb_words = sum(layout)
        assert nb_words % 2 == 0

        def cut(block):
            """[coder results 4 x n_streams | exception histograms | overflow | flags | checks(4)], on the device or in pinned memory."""
            (results, hist, overflow, flags, checks) = torch.split(block, layout)
            return (results.view(4, n_streams), hist.view(nb_hist, hist_width) if nb_hist else hist, overflow, flags.view(batch_size, nb_maps), checks)

        # the block for the host, followed by the squared errors (int64 per image, published on their own once the synthesis
        # transform is through) and behind them one more 64-bit word whose low half is the conv workspace's error word of the step
        self.block = torch.zeros(nb_words + 2*batch_size + 2, dtype=torch.int32, device=device)
        self.out = self.block[:nb_words]
        (self.results, self.hist, self.overflow, self.flags, self.checks) = cut(self.out)
        self.sse = self.block[nb_words:].view(torch.int64)           # [batch_size] errors + [1] status
        self.unfinished = self.block[nb_words + 2*batch_size:nb_words + 2*batch_size + 1]
        self.pinned_out = torch.zeros(nb_words, dtype=torch.int32).pin_memory()
        self.pinned_sse = torch.zeros(batch_size + 1, dtype=torch.int64).pin_memory()
        # what the result worker reads (`_Job.views`)
        self.host_views = tuple(t.numpy() for t in cut(self.pinned_out) + (self.pinned_sse,))
        self.symbols = torch.empty((batch_size, nb_maps, codec.map_size), dtype=torch.int16, device=device)
        self.symbols_2d = self.symbols.view(n_maps, codec.map_size)
        (self.gathered, self.classes) = (None, None)
        if codec.coding_tile is None:
            self.coder_streams = dev.CoderStreams(n_maps, codec.map_size, codec.truncated_unary_length, device, results=self.results)
            make_workspace = dev.coder_trailing_workspace if codec.coder_chunks > 1 else dev.coder_workspace
            self.workspace = make_workspace(n_maps, codec.map_size, codec.truncated_unary_length, device)
        else:
            # The step's (image, tile) entries in run order (`coding_tile_layout`): the tile-major symbols, and per shape class one
            # batch of streams whose results are that class's columns of the ONE results block; the classes run one after the other
            # on the step's coder stream, so one workspace of the largest class serves them all.
            tiled = codec._tile_layout
            self.coder_streams = None
            # (one tile per map: the planar symbols ARE the tile-major buffer, and nothing is gathered)
            self.gathered = self.symbols.view(-1) if tiled['nb_tiles'] == 1 else torch.empty(tiled['elements'], dtype=torch.int16, device=device)
            self.offsets = torch.zeros((n_streams, 2), dtype=torch.int64, device=device)
            (self.classes, need) = _class_batches(tiled['runs'], self.results, self.gathered, codec._tile_prob_row, self.offsets,
                                                  codec.truncated_unary_length, device)
            self.workspace = torch.empty(need, dtype=torch.uint8, device=device)
        # scratch that lets the conv GEMM launches cut their last tiles (device.conv_workspace): a slot's launches never overlap each other
        self.conv_ws = dev.conv_workspace(device)
        # step counters: [coder side, synthesis side] on the device (+ the two ticket words of device.publish_step), their published
        # values in pinned memory, and how many times the host has submitted each side (what the result worker waits for)
        self.seq_dev = torch.zeros(4, dtype=torch.int32, device=device)
        self.pinned_seq = torch.zeros(2, dtype=torch.int32).pin_memory()
        self.seq_host = self.pinned_seq.numpy()
        # (tickets, counter, published word) of `device.publish_step`, for the coder side and for the synthesis side
        self.coder_seq = (self.seq_dev[2:3], self.seq_dev[0:1], self.pinned_seq[0:1])
        self.synthesis_seq = (self.seq_dev[3:4], self.seq_dev[1:2], self.pinned_seq[1:2])
        self.counts = [0, 0]
        self.free = threading.Event()
        self.free.set()
        self.pinned_symbols = torch.empty((batch_size, nb_maps, codec.map_size), dtype=torch.int16).pin_memory() if codec.coder == 'host' else None
        self.staging = None          # device copy of a host batch (made at the slot's first host batch)
        self.pinned_rec = (torch.empty((batch_size, codec.h_image, codec.w_image), dtype=torch.uint8).pin_memory()
                           if codec.fetch_reconstruction else None)
        self.graphs = None           # (graphs, static input, latents, reconstruction) once captured (`BatchCodec._capture_all`)
        self.emit_host = None
        if codec.emit_container:
            # One float64 block: [the codec's probability table | one row per image for its exception map | index words (int64: payload
            # bytes, overflow flag, bytes per image)]. The coder reads the first two parts as its table; the last two go to the host.
            length = codec.truncated_unary_length
            (table_words, row_words) = (nb_maps*length, batch_size*length)
            block = torch.zeros(table_words + row_words + 2 + batch_size, dtype=torch.float64, device=device)
            self.table = block[:table_words + row_words].view(nb_maps + batch_size, length)
            self.table[:nb_maps].copy_(codec.probabilities)
            self.exception_rows = self.table[nb_maps:]
            self.index = block[table_words + row_words:].view(torch.int64)
            self.payload_bytes = self.index[0:1]
            self.emit_tail = block[table_words:]
            self.pinned_emit = torch.zeros(row_words + 2 + batch_size, dtype=torch.float64).pin_memory()
            if codec.coding_tile is None:
                self.offsets = torch.zeros((n_maps, 2), dtype=torch.int64, device=device)
            self.payload = torch.zeros(codec.container_capacity_bytes, dtype=torch.uint8, device=device)
            self.pinned_payload = torch.zeros(codec.container_capacity_bytes, dtype=torch.uint8).pin_memory()
            # what the result worker copies from (`_Job.emit`)
            self.emit_host = (codec._container_head, codec.container_capacity_bytes, self.pinned_payload.numpy(),
                              self.pinned_emit[:row_words].view(batch_size, length).numpy(), self.pinned_emit[row_words:].view(torch.int64).numpy())


class BatchCodec(object):
    """Encode -> quantise -> entropy-code (with round trip) -> decode -> squared error for batches of a fixed shape."""
    (_ticket_class, _worker_class) = (Ticket, _Worker)      # what a subclass replaces (`BudgetCodec`)

    def __init__(self, variables, are_bin_widths_learned, bin_widths_test, map_mean, binary_probabilities, idx_map_exception,
                 batch_size, h_in, w_in, device='cuda', nb_in_flight=None, keep_reconstruction=False, launch_hook=None,
                 coder='device', host_coder_threads=0, hist_radius=2047, nb_transform_streams=1, use_graphs=False,
                 time_coder=False, fuse_latent=False, fetch_reconstruction=False, coder_chunks=None, one_stream_steps=False,
                 emit_container=False, container_capacity_bytes=None, coding_tile=None, rdo_lambda=None, pad=False):
        """coder: 'device' (the coder kernels on side streams), 'host' (ONE device -> host copy of the symbols per batch, then
        the host C-ABI coder `eae_coder_compress_maps` on `host_coder_threads` threads: the shape BASELINE.json sketches) or
        'none' (transforms only; the bit counts come back as zeros).
        nb_in_flight: batches whose coder work may be pending at once, each on its own side stream (None:
        `default_nb_in_flight(h_in, w_in)`).
        nb_transform_streams: 1 = the transforms run on the caller's current stream; more = consecutive batches alternate
        between that many private streams (worth it only for small batches, whose kernels leave most of the GPU idle).
        one_stream_steps: a step's coder runs on the step's transform stream, behind its synthesis transform, instead of beside it on a
        coder stream: ONE graph launch per step, no event between streams. For one or two images per step, where consecutive steps on
        `nb_transform_streams` streams are what fills the GPU and a hop between streams costs 60-100 us on this runtime (one Kodak
        image per step on 14 streams: 0.295 -> 0.252 ms per image, the launching thread 0.15 -> 0.06 ms; a single step takes the
        coder's 0.2 ms longer).
        use_graphs: capture the launches of one step into three hipGraphs per slot on first use (analysis side, coder,
        synthesis side) and replay them afterwards: three host launches per step instead of about twenty. For small batches, where the launch thread is the
        bottleneck (one Kodak image per step); `launch_hook` is not called for replayed steps. Not for coder='host'.
        fuse_latent: run the latent stage (gdn_3, quantiser, inverse_gdn_4) as the epilogue of the conv_3 launch instead of as
        its own kernel (device.conv5x5s2_latent; same bits). One launch fewer, but at Kodak batch sizes conv_3 has one tile per
        SIMD and nothing to hide that epilogue behind: 3.41 against 3.44 ms per 24 images, with the conv_3 launch at 0.36 ms
        instead of 0.27 + 0.12. Pays for batches that give conv_3 several tiles per SIMD.
        fetch_reconstruction: the uint8 reconstructions are copied to pinned host memory by the result worker (on a stream of its
        own, once the batch is decoded) and `Ticket.reconstruction_host` holds them after `result()`: the fetch of the reference's
        `decode_mini_batches` (eae/batching.py:49-53). The feed is `submit()` with a pinned HOST tensor.
        coder_chunks: 2..16 cuts the coder's serial chains into that many launches each, so that the emit pass and the decoder run
        while the encoder core is still at work (`device.coder_roundtrip_trailing`; same results). None: `default_coder_chunks`
        (off: on this runtime the hops between the three streams cost more than the overlap saves, except for long chains).
        hist_radius: the exception map's entropy is formed from an exact histogram of its symbols over [-hist_radius,
        hist_radius]; when a symbol falls outside, the result worker counts that batch's exception maps again over the whole
        int16 range (like the image-by-image functions of `kodak/`; the reference's histogram has no bound,
        lossless/compression.py:68-75).
        emit_container: every step also leaves its `EAE1` container (container.py) with the ticket: `Ticket.container()`,
        `Ticket.image_containers()`, and 'container_bytes' per image in `result()`; everything else `result()` returns is what the
        same codec without it returns. The offsets, the packing and the exception maps' probability rows are formed on the device,
        behind the coder's launches and in front of the publication of its results; the exception map is then
        coded too (with a row measured on it, as `container.encode_images` does), which needs `hist_radius >= L`. Needs the device coder.
        container_capacity_bytes: the payload bytes a step may take (rounded up to 16; a device and a pinned buffer of that size per
        slot). None: batch_size*h_in*w_in, i.e. 8 bits per pixel. A step beyond it keeps its results; its `Ticket.container()` raises
        `ContainerOverflow`.
        coding_tile: (th, tw) in latents, with `emit_container`: every (image, tile, map) is coded as its own pair of streams and
        the step's container is the tile-indexed `EAT1` -- `Ticket.container()` / `image_containers()` are byte for byte what
        `container.encode_images(..., coding_tile=(th, tw))` writes, so `container.decode_region` reads a crop out of them. The tile
        is clamped to the latent plane. 'coder_bits' sums an image's tiles (every tile's streams pay their own termination, so it is
        larger than without tiles); 'sse', 'nb_deads' and 'exception_bits' do not change. The serial chains are then a tile long
        instead of a map. At most 65,535 (image, tile) pairs per step; not with `coder_chunks`.
        rdo_lambda: None, or a non-negative float in squared latent units per bit: the step's symbols are chosen by the
        rate-distortion optimised quantiser instead of by nearest rounding: conv_3, gdn_3 as a launch of its
        own, then `device.latent_quantize_rdo` with `ratecontrol.rdo_thresholds` of this rate point. Everything behind the symbols is
        unchanged and `result()` has the same keys; the containers are byte for byte `container.encode_images(..., rdo_lambda=...)`.
        0.0 gives the results of None. Not with `fuse_latent` or the host coder.
        pad: h_in x w_in is the REAL size of the images, any positive integers. `submit` takes
        (batch_size, h_in, w_in); the step runs at the coded size -- both sides rounded up to multiples of 16 -- on the batch
        extended by edge replication (`device.frame_pad_u8`, one launch in front of the analysis transform: on the graph path where the
        batch is copied into the step's static input), in every mode above. `result()` has the same keys and, 'sse' apart, the values
        of the same codec at the coded size on the numpy-edge-padded batch; 'sse' is over the real pixels (`device.frame_sse_u8`
        behind transpose_conv_3, which then skips its fused error). The containers carry the real size in their `crop` byte: byte for
        byte `container.encode_images(..., pad=True)`. `Ticket.reconstruction_uint8` / `reconstruction_host` are (batch_size, h_in,
        w_in), the top-left of the coded planes. `h_in`, `w_in` of the codec are the coded size then, `h_image`, `w_image` the real."""
        if coder not in ('device', 'host', 'none'):
            raise ValueError('`coder` is neither "device" nor "host" nor "none".')
        self.pad = bool(pad)
        (self.h_image, self.w_image) = (h_in, w_in)
        if self.pad:
            (h_in, w_in) = container_format.coded_size(container_format._positive_int(h_in, '`h_in`'), container_format._positive_int(w_in, '`w_in`'))
        self.rdo_lambda = None
        if rdo_lambda is not None:
            # refused in front of every allocation
            if fuse_latent:
                raise ValueError('`rdo_lambda` does not go with `fuse_latent`: the fused latent stage rounds to the nearest symbol.')
            if coder == 'host':
                raise ValueError('`rdo_lambda` needs the coder on the device (or none).')
            self.rdo_lambda = float(rdo_lambda)
            if not numpy.isfinite(self.rdo_lambda) or self.rdo_lambda < 0.:
                raise ValueError('`rdo_lambda` must be a finite number that is not negative.')
        if use_graphs and coder == 'host':
            raise ValueError('`use_graphs` needs the coder on the device (or none).')
        if h_in % csts.STRIDE_PROD != 0 or w_in % csts.STRIDE_PROD != 0:
            raise ValueError('The image size is not divisible by the product of the three strides.')
        self.coding_tile = None
        if coding_tile is not None:
            # refused in front of every allocation
            if not emit_container:
                raise ValueError('`coding_tile` needs `emit_container=True`: the tiles are those of the step\'s `EAT1` container.')
            if coder != 'device':
                raise ValueError('`coding_tile` needs the coder on the device.')
            if int(default_coder_chunks(batch_size*csts.NB_MAPS_3) if coder_chunks is None else coder_chunks) > 1:
                raise ValueError('`coding_tile` does not go with `coder_chunks` > 1: the chunked coder codes whole maps.')
            coding_tile = container_format._positive_pair(coding_tile, '`coding_tile`')
            if max(coding_tile) > 0xFFFF:
                raise ValueError('A side of `coding_tile` does not fit the container (65535 latents at most).')
            (h_map, w_map) = (h_in//csts.STRIDE_PROD, w_in//csts.STRIDE_PROD)
            self.coding_tile = (min(coding_tile[0], h_map), min(coding_tile[1], w_map))
            if batch_size*container_format._nb_tiles(h_map, w_map, self.coding_tile) > 65535:
                raise ValueError('`batch_size` images of {0} coding tiles each are more than the 65535 (image, tile) pairs a step can hold.'.format(
                    container_format._nb_tiles(h_map, w_map, self.coding_tile)))
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if self.device.index != torch.cuda.current_device():      # launches go to the current device's streams (device._stream)
            raise ValueError('`device` is {0} but the current device is cuda:{1}: build and use the codec under '
                             '`torch.cuda.device({0!r})`.'.format(self.device, torch.cuda.current_device()))
        self.learned = are_bin_widths_learned
        self.encoder = pipeline.DeviceEncoder(variables, are_bin_widths_learned, self.device)
        self.decoder = pipeline.DeviceDecoder(variables, are_bin_widths_learned, self.device)
        self.batch_size = batch_size
        (self.h_in, self.w_in) = (h_in, w_in)
        self.nb_maps = csts.NB_MAPS_3
        self.map_size = (h_in//csts.STRIDE_PROD)*(w_in//csts.STRIDE_PROD)
        self.idx_map_exception = idx_map_exception if 0 <= idx_map_exception < self.nb_maps else -1
        probabilities = numpy.ascontiguousarray(binary_probabilities, dtype=numpy.float64)
        if probabilities.ndim != 2 or probabilities.shape[0] != self.nb_maps:
            raise ValueError('`binary_probabilities` must have one row per map.')
        self.truncated_unary_length = probabilities.shape[1]
        if self.truncated_unary_length > 255:
            raise OverflowError('value too large to convert to numpy.uint8_t')   # interface_cython.pyx:49
        self.emit_container = bool(emit_container)
        if self.emit_container and coder != 'device':
            raise ValueError('`emit_container` needs the coder on the device: the container is made of its streams.')
        if self.emit_container and self.idx_map_exception >= 0 and int(hist_radius) < self.truncated_unary_length:
            raise ValueError('`emit_container` with an exception map needs `hist_radius` >= the truncated unary length: the map\'s '
                             'probability row is formed from its histogram.')
        if container_capacity_bytes is None:
            container_capacity_bytes = batch_size*h_in*w_in
        self.container_capacity_bytes = max(16, -(-int(container_capacity_bytes)//16)*16)
        bin_widths_host = numpy.ascontiguousarray(bin_widths_test, dtype=numpy.float32)
        map_mean_host = numpy.ascontiguousarray(map_mean, dtype=numpy.float32)
        # the parts of a step's container that no step changes (container.assemble_blob's leading arguments)
        self._container_head = (bool(are_bin_widths_learned), batch_size, h_in, w_in, self.idx_map_exception, bin_widths_host.copy(),
                                map_mean_host.copy(), probabilities.copy())
        # with `pad`: the dense real-size copy of the batch a replayed step's squared error is taken against, one per slot, made at the
        # capture (`_capture_all`) -- the codec's, not the slots': a slot holds what every mode needs
        self._frame_references = None
        self.bin_widths = torch.from_numpy(bin_widths_host).to(self.device)
        self.map_mean = torch.from_numpy(map_mean_host).to(self.device)
        self.probabilities = torch.from_numpy(probabilities).to(self.device)
        if self.rdo_lambda is not None:
            # what `device.latent_quantize_rdo` takes beyond the latents: one rate point, which every image takes
            from . import ratecontrol
            self._rdo_bin_widths = self.bin_widths.reshape(1, self.nb_maps)
            self._rdo_thresholds = torch.from_numpy(ratecontrol.rdo_thresholds(bin_widths_host[None], probabilities[None], self.rdo_lambda,
                                                                               self.idx_map_exception)).to(self.device)
            self._rdo_point = torch.zeros(batch_size, dtype=torch.int32, device=self.device)
        prob_row = torch.arange(self.nb_maps, dtype=torch.int32).repeat(batch_size)
        if self.idx_map_exception >= 0:
            prob_row[self.idx_map_exception::self.nb_maps] = -1        # costed from its histogram (compression.py:68-75)
        self.prob_row = prob_row.to(self.device)
        self._emit_prob_row = None
        if self.emit_container:
            # image i's exception map is coded with row nb_maps + i of the slot's table (`_Slot.exception_rows`)
            emit_prob_row = torch.arange(self.nb_maps, dtype=torch.int32).repeat(batch_size)
            if self.idx_map_exception >= 0:
                emit_prob_row[self.idx_map_exception::self.nb_maps] = self.nb_maps + torch.arange(batch_size, dtype=torch.int32)
            self._emit_prob_row = emit_prob_row.to(self.device)
        self.fetch_reconstruction = bool(fetch_reconstruction)
        self.keep_reconstruction = bool(keep_reconstruction) or self.fetch_reconstruction
        self.hist_radius = int(hist_radius)
        self.coder = coder
        self.time_coder = bool(time_coder)      # Ticket.coder_ms(): the launch-by-launch path only
        self.fuse_latent = bool(fuse_latent)
        self.one_stream_steps = bool(one_stream_steps)
        # launch_hook(name, fn): called for every timed launch of the launch-by-launch path with name in ('conv1_gdn1',
        # 'conv2_gdn2', 'conv3', 'latent', 'tconv1_igdn5', 'tconv2_igdn6', 'tconv3', 'coder_encode', 'coder_decode') on the
        # stream the launch goes to (bench.py brackets them with HIP events); it must return fn()
        self.launch_hook = launch_hook if launch_hook is not None else _no_hook
        n_maps = batch_size*self.nb_maps
        self._n_maps = n_maps
        self._n_streams = n_maps          # pairs of streams per step: what sizes the head of a slot's result block
        self._tile_layout = None
        if self.coding_tile is not None:
            # everything a step in tiles needs beyond its symbols is the same for every step: made once, shared by the slots
            tiled = coding_tile_layout(batch_size, h_in//csts.STRIDE_PROD, w_in//csts.STRIDE_PROD, self.coding_tile, self.idx_map_exception)
            self._tile_layout = tiled
            self._n_streams = tiled['n_streams']
            self._tile_plan_host = tiled['plan']
            self._tile_plan = torch.from_numpy(tiled['plan']).to(self.device)
            self._tile_prob_row = torch.from_numpy(tiled['prob_row']).to(self.device)
            # `device.coder_index_tiles`: per payload-order entry, its run-order index and half the stream stride of its class
            half_stride = numpy.array([dev.coder_stream_stride_bytes(int(tiled['tiles'][t, 2]*tiled['tiles'][t, 3]), self.truncated_unary_length)//2
                                       for (_, t) in tiled['entries']], dtype=numpy.int64)
            self._tile_table = torch.from_numpy(numpy.stack([tiled['run_entry'], half_stride], axis=1)).to(self.device)
        if nb_in_flight is None:
            nb_in_flight = default_nb_in_flight(h_in, w_in)
        if coder == 'device' and not one_stream_steps and os.environ.get('EAE_IGNORE_HW_QUEUES') != '1':
            # no more busy streams than the process has hardware queues (said once; EAE_IGNORE_HW_QUEUES=1: the experiments' switch)
            (nb_transform_streams, nb_in_flight, message) = stream_budget(nb_transform_streams, nb_in_flight,
                                                                          copies=1 if fetch_reconstruction else 0)
            if message is not None and not _BUDGET_WARNED[0]:
                _BUDGET_WARNED[0] = True
                import warnings
                warnings.warn(message, RuntimeWarning, stacklevel=2)
        self.nb_in_flight = nb_in_flight
        self.nb_transform_streams = nb_transform_streams
        self.nb_slots = nb_in_flight + 2
        nb_private = nb_transform_streams if (nb_transform_streams > 1 or use_graphs) else 0      # replays never go to the caller's stream
        if self.one_stream_steps:
            # no coder streams; the steps' streams come from both of the process's lists, so that a process that has run other codecs
            # makes as few new streams as it can (streams beyond GPU_MAX_HW_QUEUES share hardware queues, busy ones with busy ones)
            self._streams = []
            self._transform_streams = _step_streams(nb_private, self.device)
        else:
            self._streams = _side_streams(nb_in_flight, self.device)
            self._transform_streams = _side_streams(nb_private, self.device, kind='transform')
        self._coder_behind_tconv1 = (n_maps > 256) if _CODER_BEHIND_TCONV1 is None else _CODER_BEHIND_TCONV1 != '0'
        # one or two images per step: the caller usually waits for each result, and what it waits for last is the coder. The analysis
        # side's blocks (exception-map histograms, dead-map flags, range check) then travel with the synthesis side's publication
        # already -- one more copy launch on the transform stream, 0.4 ms before the coder ends -- and `Ticket.result()` turns them into
        # their share of the results while the coder still runs (`_Worker.process`).
        # (not with `one_stream_steps`: that mode is for many small steps in flight, where the launching thread's time per step is the rate)
        self._early_publish = n_maps <= 256 and _EARLY_PUBLISH and not one_stream_steps
        self.coder_chunks = int(default_coder_chunks(n_maps) if coder_chunks is None else coder_chunks)
        if self.coder_chunks > 1 and coder != 'device':
            self.coder_chunks = 1
        self._slots = [_Slot(self) for _ in range(self.nb_slots)]
        self._index = 0
        self.use_graphs = bool(use_graphs)
        self._warm = False
        self._recount_stream = None
        # host in / host out: a copy stream each way
        self._feed_stream = None
        self._fetch_stream = torch.cuda.Stream(device=self.device) if self.fetch_reconstruction else None
        assert not self.use_graphs or self._transform_streams      # replays never go to the caller's stream
        # last but one: a constructor that raised above has no worker yet, and `close()` has nothing to wait for
        self._worker = self._worker_class(self.map_size, self.nb_maps, probabilities if coder == 'host' else None, self.idx_map_exception,
                               host_coder_threads, self.coding_tile, self._tile_layout['payload_order'] if self._tile_layout else None)
        if self.pad:
            self._worker.image_size = (self.h_image, self.w_image)
        self._worker.start()
        # last: a constructor that raised above leaves nothing half-built behind for another codec's `_capture_all` to drain
        with _LIVE_LOCK:
            _LIVE.setdefault(self.device.index, weakref.WeakSet()).add(self)

    def submit(self, luminances_uint8):
        """uint8 tensor (batch_size, h_in, w_in), on the device or in PINNED host memory -> Ticket. Everything is enqueued; nothing
        is waited for except a free slot (at most nb_in_flight + 2 batches are pending). A host batch is copied in on a copy
        stream of the codec's own (`Ticket.fed_event` is recorded behind the copy: leave the batch alone until then)."""
        if luminances_uint8.dtype != torch.uint8:
            raise TypeError('`luminances_uint8.dtype` is not equal to `torch.uint8`.')
        if tuple(luminances_uint8.shape) != (self.batch_size, self.h_image, self.w_image):
            raise ValueError('`luminances_uint8.shape` is not (batch_size, h_in, w_in).')
        if self._worker.failed is not None:
            raise StepTimeout('this codec stopped taking batches: {0}'.format(self._worker.failed))
        host = luminances_uint8.device.type == 'cpu'
        if host and not luminances_uint8.is_pinned():
            raise ValueError('a host batch must be in pinned memory (`torch.Tensor.pin_memory()`): its copy is asynchronous.')
        if self.use_graphs:
            # every slot's graphs are captured at the first call, after one ordinary step that gets every lazy initialisation out of
            # the way (`_capture_all`), and replayed afterwards
            if not self._warm:
                self._submit(luminances_uint8).result()          # first launches: function attributes, lazy module loads
                try:
                    self._capture_all(luminances_uint8)
                except BaseException:
                    for slot in self._slots:                         # a half-captured set is of no use: the next submit starts over
                        slot.graphs = None
                    raise
                self._warm = True
            return self._submit(luminances_uint8, replay=True)
        if not self._transform_streams:
            return self._submit(luminances_uint8)
        # small batches leave most of the GPU idle and a step is a chain of short dependent kernels: consecutive batches go
        # to different streams so that their chains overlap
        stream = self._transform_streams[self._index % len(self._transform_streams)]
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ticket = self._submit(luminances_uint8)
        if not host:
            luminances_uint8.record_stream(stream)
        return ticket

    def _feed(self, host_batch, device_batch, fresh=False):
        """Host -> device copy of a pinned batch on the codec's feed stream; the CURRENT stream waits for it. Returns the event
        recorded behind the copy (`Ticket.fed_event`). fresh: the destination has just come from the caching allocator, which
        may have handed out a block that kernels still queued on the current stream use (freed intermediates of the previous
        steps: safe to reuse in stream order only): the copy then goes behind everything the current stream holds."""
        if self._feed_stream is None:
            self._feed_stream = torch.cuda.Stream(device=self.device)
        if fresh:
            self._feed_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._feed_stream):
            device_batch.copy_(host_batch, non_blocking=True)
            fed = torch.cuda.Event()
            fed.record()
        torch.cuda.current_stream().wait_event(fed)
        return fed

    def _submit(self, luminances_uint8, replay=False):
        """One step: claims the next slot, launches the step (`_replay_step` / `_launch_step`), hands its job to the result worker.
        Which events exist: `coded` / `decoded` are what the worker waits for in the 'events' wait mode; in 'sequence' mode it reads
        the slot's step counters, and an event is only made for whom it serves (`time_coder`: the launch-by-launch path only; a
        caller reading the reconstruction on another stream waits for `decoded`)."""
        index = self._index
        self._index += 1
        slot = self._slots[index % self.nb_slots]
        slot.free.wait()
        slot.free.clear()
        sequence_mode = _WAIT_MODE == 'sequence'
        expected = (slot.counts[0] + 1, slot.counts[1] + 1)      # what the slot's step counters will show behind this step
        timed = self.time_coder and not replay
        try:
            ticket = self._ticket_class(self.batch_size)
            coded = torch.cuda.Event(enable_timing=timed) if (timed or not sequence_mode) else None
            if timed:
                ticket._coder_span = (torch.cuda.Event(enable_timing=True), coded)
            if not sequence_mode or self.keep_reconstruction:
                ticket.decoded_event = torch.cuda.Event()
            reconstruction = (self._replay_step if replay else self._launch_step)(luminances_uint8, slot, index, ticket, coded)
            if self.pad:
                reconstruction = reconstruction[:, :self.h_image, :self.w_image]      # a view: the top-left of the coded planes
            if self.keep_reconstruction:
                ticket.reconstruction_uint8 = reconstruction       # valid until this slot comes round again
            job = _Job(ticket, () if sequence_mode else (coded, ticket.decoded_event), slot.host_views, slot.pinned_symbols, slot.free,
                       lambda: self._recount_exception_maps(slot), self._fetch_job(slot, reconstruction),
                       (slot.seq_host, expected) if sequence_mode else None, self._early_publish, slot.emit_host)
            ticket._job = (job, self._worker)
            self._worker.jobs.put(job)
            slot.counts = list(expected)
            return ticket
        except BaseException:
            self._resync(slot)
            slot.free.set()       # nobody will report on this slot: without this, drain() / close() wait for ever
            raise

    def _replay_step(self, luminances_uint8, slot, index, ticket, coded):
        """One step = three hipGraph launches: the analysis side (conv1 .. symbols) and the synthesis side on a transform
        stream, the coder on a coder stream between two events, exactly the stream structure of the launch-by-launch path.
        A slot owns its buffers (symbols, streams, result blocks), so it owns its three graphs too. Records `coded` and the
        ticket's events where they exist; returns the slot's reconstruction."""
        stream = self._transform_streams[index % len(self._transform_streams)]
        coder_stream = self._streams[index % len(self._streams)] if self._streams else None
        caller = torch.cuda.current_stream()
        if slot.graphs is None:
            raise RuntimeError('slot {} has no captured graphs (a capture failed earlier)'.format(index % self.nb_slots))
        (graphs, static_input, _, reconstruction) = slot.graphs
        # the launch thread's time is what the pipelined small-batch rate is made of: the current stream is switched directly
        # (`with torch.cuda.stream(...)` costs three device-index resolutions per entry and exit) and restored in the `finally`
        try:
            torch.cuda.set_stream(stream)
            # (with `pad` the batch goes into the slot's real-size reference, and the pad kernel fills the static input from it)
            batch_input = self._frame_references[index % self.nb_slots] if self.pad else static_input
            if luminances_uint8.device.type == 'cpu':
                ticket.fed_event = self._feed(luminances_uint8, batch_input)
            else:
                stream.wait_stream(caller)
                batch_input.copy_(luminances_uint8, non_blocking=True)
            if self.pad:
                dev.frame_pad_u8(batch_input, out=static_input)
            graphs[0].replay()
            if self.one_stream_steps:
                if coded is not None:                         # the whole step is graphs[0]: both of the worker's events behind it
                    coded.record(stream)
            else:
                quantized = torch.cuda.Event()
                quantized.record(stream)
                torch.cuda.set_stream(coder_stream)
                coder_stream.wait_event(quantized)
                graphs[1].replay()
                if coded is not None:
                    coded.record(coder_stream)
                torch.cuda.set_stream(stream)
                graphs[2].replay()
            if ticket.decoded_event is not None:
                ticket.decoded_event.record(stream)
        finally:
            torch.cuda.set_stream(caller)
        if ticket.fed_event is None:
            luminances_uint8.record_stream(stream)
        return reconstruction

    def _capture_all(self, like):
        """Captures the three graphs of EVERY slot now, while nothing of THIS codec is in flight and its result worker is idle
        (other codecs of the process share the side streams: capture before they are busy, or give them other streams): a capture that
        starts later shares its stream with replays whose events the worker is polling, and on this runtime a query of an
        event recorded on a capturing stream invalidates the capture (seen with one transform stream and 24 Kodak images:
        hipErrorStreamCaptureInvalidated at the first launch of the second slot's capture)."""
        # Codecs of this process share the device's side streams (and their slices move with `nb_in_flight`): one that is busy would
        # have its worker polling events on a stream this capture uses. Wait until every other live codec of the device is idle;
        # a caller that keeps submitting to another codec from another thread during a first submit here is outside the contract
        # (bring a device's codecs up one after the other).
        with _LIVE_LOCK:
            others = [c for c in _LIVE.get(self.device.index, ()) if c is not self and getattr(c, '_worker', None) is not None]
        for other in others:
            other.drain()
        torch.cuda.synchronize(self.device)
        if self.pad:
            self._frame_references = [torch.empty((self.batch_size, self.h_image, self.w_image), dtype=torch.uint8, device=self.device)
                                      for _ in self._slots]
        for (number, slot) in enumerate(self._slots):
            # any of the codec's streams will do for the capture: a replay runs on the stream it is launched into, which
            # `_replay_step` picks from the submission index (slots and streams go round at different periods)
            stream = self._transform_streams[number % len(self._transform_streams)]
            coder_stream = self._streams[number % len(self._streams)] if self._streams else None
            static_input = torch.empty((self.batch_size, self.h_in, self.w_in), dtype=torch.uint8, device=self.device)
            # what the synthesis side takes its squared error against: the static input itself, with `pad` the real-size batch
            reference = self._frame_references[number] if self.pad else static_input
            if self.one_stream_steps:
                graphs = [torch.cuda.CUDAGraph()]
                with torch.cuda.graph(graphs[0], stream=stream, capture_error_mode='thread_local'):
                    latents = self._launch_analysis(static_input, slot, _no_hook)
                    reconstruction = self._launch_synthesis(latents, reference, slot, _no_hook)
                    self._launch_coder(slot)
                slot.graphs = (graphs, static_input, latents, reconstruction)
                continue
            graphs = [torch.cuda.CUDAGraph() for _ in range(3)]
            with torch.cuda.graph(graphs[0], stream=stream, capture_error_mode='thread_local'):
                latents = self._launch_analysis(static_input, slot, _no_hook)
                if self._coder_behind_tconv1:
                    latents = self._launch_synthesis_head(latents, slot, _no_hook)
            with torch.cuda.graph(graphs[1], stream=coder_stream, capture_error_mode='thread_local'):
                self._launch_coder(slot)
            with torch.cuda.graph(graphs[2], stream=stream, capture_error_mode='thread_local'):
                reconstruction = self._launch_synthesis(latents, reference, slot, _no_hook, head_done=self._coder_behind_tconv1)
            slot.graphs = (graphs, static_input, latents, reconstruction)

    def _launch_step(self, luminances_uint8, slot, index, ticket, coded):
        """One step launch by launch: the transforms on the current stream, the coder on a coder stream beside the synthesis
        transform (`one_stream_steps`: behind it, on the current stream). Records `coded` and the ticket's events where they exist;
        returns the reconstruction."""
        hook = self.launch_hook
        stream = self._streams[index % len(self._streams)] if self._streams else None
        if luminances_uint8.device.type == 'cpu':
            fresh = slot.staging is None
            if fresh:
                slot.staging = torch.empty((self.batch_size, self.h_image, self.w_image), dtype=torch.uint8, device=self.device)
            ticket.fed_event = self._feed(luminances_uint8, slot.staging, fresh)
            luminances_uint8 = slot.staging
        # with `pad` the transforms see the batch extended to the coded size (an allocator temporary), the squared error the batch itself
        latents = self._launch_analysis(dev.frame_pad_u8(luminances_uint8) if self.pad else luminances_uint8, slot, hook)
        head_done = self._coder_behind_tconv1 and not self.one_stream_steps
        if head_done:
            latents = self._launch_synthesis_head(latents, slot, hook)
        if self.one_stream_steps:                          # the coder behind the synthesis transform, on this stream
            reconstruction = self._launch_synthesis(latents, luminances_uint8, slot, hook)
        else:
            quantized = torch.cuda.Event()
            quantized.record()
        with (contextlib.nullcontext() if self.one_stream_steps else torch.cuda.stream(stream)):
            if not self.one_stream_steps:
                stream.wait_event(quantized)
            if ticket._coder_span is not None:
                ticket._coder_span[0].record()
            self._launch_coder(slot, hook)
            if coded is not None:
                coded.record()
        if not self.one_stream_steps:
            reconstruction = self._launch_synthesis(latents, luminances_uint8, slot, hook, head_done=head_done)
        if ticket.decoded_event is not None:
            ticket.decoded_event.record()
        return reconstruction

    def _resync(self, slot):
        """A submit that raised may have launched some of its step: wait for whatever it did launch and take the slot's step
        counters from the device, so that the next job on this slot waits for the right values."""
        try:
            torch.cuda.synchronize(self.device)
            slot.counts = [int(v) for v in slot.seq_dev[:2].cpu().tolist()]
            slot.seq_dev[2:].zero_()                    # ticket words of a publish that never ran to its end
            slot.block[4*self._n_streams:].zero_()      # accumulators a publish would have cleared
        except Exception:      # the device itself is in trouble: the next submit will say so
            pass

    def _fetch_job(self, slot, reconstruction):
        """What the result worker needs to copy the slot's reconstruction to the host (None: not asked for)."""
        if not self.fetch_reconstruction:
            return None
        reconstruction.record_stream(self._fetch_stream)
        return (reconstruction, slot.pinned_rec, self._fetch_stream)

    def _recount_exception_maps(self, slot):
        """Histograms of the slot's exception maps over all of int16, as a host array [batch, 65535] (called by the result
        worker while it still owns the slot, on its own stream, when a symbol fell outside `hist_radius`)."""
        with torch.cuda.device(self.device):
            if self._recount_stream is None:
                self._recount_stream = torch.cuda.Stream(device=self.device)
            with torch.cuda.stream(self._recount_stream):
                (hist, overflow) = dev.symbol_histograms(slot.symbols_2d, 32767, first_map=self.idx_map_exception, map_step=self.nb_maps)
                host = hist.cpu().numpy()
                if int(overflow.sum().item()) != 0:          # -32768: cast_float_to_int16 never produces it (tools.py:95-133)
                    raise RuntimeError('exception-map symbol outside [-32767, 32767]')
        return host

    def _launch_analysis(self, luminances_uint8, slot, hook):
        """conv1+GDN1 -> conv2+GDN2 -> conv3 -> latent stage (symbols, dead-map flags, decoder input) -> exception-map
        histograms, on the current stream. Returns the synthesis transform's input."""
        enc = self.encoder
        v = enc.v
        d = self.decoder.v
        gdn_1 = hook('conv1_gdn1', lambda: dev.conv9x9s4_u8(luminances_uint8, enc.w1, v['encoder/biases_1'], enc.g[1], v['encoder/beta_1']))
        ws = slot.conv_ws
        gdn_2 = hook('conv2_gdn2', lambda: dev.conv5x5s2(gdn_1, enc.w2, v['encoder/biases_2'], dev.NORM_GDN, enc.g[2], v['encoder/beta_2'], workspace=ws))
        # (histograms, overflow, flags, checks, squared errors are accumulated into: zero when the slot is made, and zeroed again by the
        # launches that publish them, `_launch_coder` / `_launch_synthesis`)
        gdn_in = None if self.learned else (enc.g[3], v['encoder/beta_3'])
        igdn_out = None if self.learned else (self.decoder.g[4], d['decoder/beta_4'])
        if self.fuse_latent:
            # conv_3 with the latent stage as its epilogue: one launch, the latents never go through HBM in between
            q = hook('conv3', lambda: dev.conv5x5s2_latent(gdn_2, enc.w3, v['encoder/biases_3'], self.bin_widths, self.map_mean, gdn_in=gdn_in,
                                                           igdn_out=igdn_out, want_flags=True, out_symbols=slot.symbols,
                                                           out_flags=slot.flags, out_checks=slot.checks[:3], workspace=ws))
        elif self.rdo_lambda is not None:
            # conv_3 -> gdn_3 as its own launch -> the quantiser that weighs every symbol's bits against its error (+ inverse_gdn_4)
            y = hook('conv3', lambda: dev.conv5x5s2(gdn_2, enc.w3, v['encoder/biases_3'], dev.NORM_NONE, workspace=ws))
            if not self.learned:
                y = hook('gdn3', lambda: dev.gdn(y, enc.g[3], v['encoder/beta_3']))
            q = hook('latent', lambda: dev.latent_quantize_rdo(y, self._rdo_bin_widths, self._rdo_thresholds, self._rdo_point,
                                                               self.truncated_unary_length, self.map_mean, igdn_out=igdn_out,
                                                               want_shifted=self.learned, want_symbols=True, want_flags=True,
                                                               out_symbols=slot.symbols, out_flags=slot.flags, out_checks=slot.checks[:3]))
        else:
            y_raw = hook('conv3', lambda: dev.conv5x5s2(gdn_2, enc.w3, v['encoder/biases_3'], dev.NORM_NONE, workspace=ws))
            # gdn_3 -> centre / quantise / symbols / dead-map flags -> de-centre -> inverse_gdn_4: one pass over the latents
            q = hook('latent', lambda: dev.latent_stage(y_raw, self.bin_widths, self.map_mean, gdn_in=gdn_in, igdn_out=igdn_out,
                                                        want_shifted=self.learned, want_symbols=True, want_flags=True,
                                                        out_symbols=slot.symbols, out_flags=slot.flags, out_checks=slot.checks[:3]))
        if self.idx_map_exception >= 0:
            dev.symbol_histograms(slot.symbols_2d, self.hist_radius, out=(slot.hist, slot.overflow),
                                  first_map=self.idx_map_exception, map_step=self.nb_maps, zero=False)
        if self._early_publish:
            # The analysis side's blocks are final here and reach pinned memory at once (the coder's publication, which also zeroes them
            # for the slot's next step, copies them again): in FRONT of the event the coder's stream waits for, so the zeroing cannot
            # overtake this copy. The host looks at them when the synthesis side has reported (`_Worker.process`).
            first = 4*self._n_streams
            dev.publish_to_host(slot.out[first:], slot.pinned_out[first:])
        return q['shifted'] if self.learned else q['t']

    def _coder_table(self, slot):
        """What the step's coder runs on -> (the probability table, the rows of it the streams take: one tensor for whole maps, one per
        shape class of `slot.classes` with a coding tile, where the exception maps' rows of the table go: None without a container)."""
        if not self.emit_container:
            return (self.probabilities, self.prob_row, None)
        rows = self._emit_prob_row if self.coding_tile is None else [rows for (_, _, rows, _) in slot.classes]
        return (slot.table, rows, slot.exception_rows)

    def _launch_coder(self, slot, hook=_no_hook):
        """The lossless coder over the slot's symbols (encode every map, decode it back, compare) and the publication of the
        slot's result block, on the current stream."""
        symbols = slot.symbols_2d
        (table, prob_row, exception_rows) = self._coder_table(slot)
        if exception_rows is not None and self.idx_map_exception >= 0:
            # the histograms are final since the analysis side and are zeroed only by this side's `publish_step`
            dev.exception_rows(slot.hist, slot.overflow, self.map_size, self.truncated_unary_length, out=exception_rows)
        if self.coding_tile is not None:
            # (image, tile) entries instead of whole maps: the symbols tile-major, one coder batch per shape
            # class, then the index over all of them and one pack per class into the one payload
            length = self.truncated_unary_length
            if slot.gathered.data_ptr() != slot.symbols.data_ptr():
                dev.tile_symbols_gather(slot.symbols, slot.gathered, self._tile_plan, self._tile_plan_host, self.h_in//csts.STRIDE_PROD,
                                        self.w_in//csts.STRIDE_PROD)
            for ((streams, tiles, _, _), rows) in zip(slot.classes, prob_row):
                hook('coder_encode', lambda: dev.coder_encode_batch(tiles, table, rows, length, out=streams, workspace=slot.workspace))
                hook('coder_decode', lambda: dev.coder_decode_batch(streams, table, rows, expected=tiles, workspace=slot.workspace))
            dev.coder_index_tiles(slot.results[0], slot.results[1], self._tile_table, self.nb_maps, self._tile_layout['nb_tiles'],
                                  self.container_capacity_bytes, offsets=slot.offsets, index=slot.index)
            for (streams, _, _, offsets) in slot.classes:
                dev.coder_pack_indexed(streams, offsets, slot.index, slot.payload)
            self._publish_coder_side(slot)
            return
        if self.coder == 'device' and self.coder_chunks > 1:
            hook('coder_roundtrip', lambda: dev.coder_roundtrip_trailing(symbols, table, prob_row, self.truncated_unary_length,
                                                                         chunks=self.coder_chunks, out=slot.coder_streams, workspace=slot.workspace))
        elif self.coder == 'device':
            hook('coder_encode', lambda: dev.coder_encode_batch(symbols, table, prob_row, self.truncated_unary_length,
                                                                out=slot.coder_streams, workspace=slot.workspace))
            hook('coder_decode', lambda: dev.coder_decode_batch(slot.coder_streams, table, prob_row, expected=symbols,
                                                                workspace=slot.workspace))
        elif self.coder == 'host':
            slot.pinned_symbols.copy_(slot.symbols, non_blocking=True)
        else:
            slot.results.zero_()
        if self.emit_container:
            # offsets and sizes from the bit counts, then the streams packed
            dev.coder_index_streams(slot.coder_streams, self.nb_maps, self.container_capacity_bytes, offsets=slot.offsets, index=slot.index)
            dev.coder_pack_indexed(slot.coder_streams, slot.offsets, slot.index, slot.payload)
        self._publish_coder_side(slot)

    def _publish_coder_side(self, slot, beside=()):
        """With a container, the payload's prefix and the index words into pinned memory; `beside`: (device block, pinned block) pairs
        a subclass publishes with them; then the step counter: all in front of it, so whoever sees the counter finds them on the host."""
        if self.emit_container:
            dev.publish_prefix(slot.payload, slot.pinned_payload, slot.payload_bytes)
            dev.publish_to_host(slot.emit_tail, slot.pinned_emit)
        for (block, pinned) in beside:
            dev.publish_to_host(block, pinned)
        dev.publish_step(slot.out, slot.pinned_out, 4*self._n_streams, *slot.coder_seq)

    def _launch_synthesis_head(self, latents, slot, hook):
        """tconv1+IGDN5 on the current stream (the first launch of the synthesis side, apart: `_coder_behind_tconv1`)."""
        dec = self.decoder
        d = dec.v
        return hook('tconv1_igdn5', lambda: dev.tconv5x5s2(latents, dec.w4, d['decoder/biases_4'], dev.NORM_IGDN, dec.g[5], d['decoder/beta_5'],
                                                           workspace=slot.conv_ws))

    def _launch_synthesis(self, latents, luminances_uint8, slot, hook, head_done=False):
        """tconv1+IGDN5 -> tconv2+IGDN6 -> tconv3 + BT.601 cast + squared error against the input, and the publication of the
        squared errors, on the current stream. Returns the uint8 reconstruction. head_done: `latents` is already tconv1's output.
        luminances_uint8: what the error is taken against; with `pad` the real-size batch (the reconstruction is of the coded size)."""
        dec = self.decoder
        d = dec.v
        ws = slot.conv_ws
        t = latents if head_done else self._launch_synthesis_head(latents, slot, hook)
        t = hook('tconv2_igdn6', lambda: dev.tconv5x5s2(t, dec.w5, d['decoder/biases_5'], dev.NORM_IGDN, dec.g[6], d['decoder/beta_6'], workspace=ws))
        if self.pad:
            # the error over the real pixels only: transpose_conv_3 without its fused error, then one launch over the top-left h x w
            (_, reconstruction, _) = hook('tconv3', lambda: dev.tconv9x9s4_luma(t, dec.w6, want_f32=False, want_u8=True))
            dev.frame_sse_u8(reconstruction, luminances_uint8, out=slot.sse[:self.batch_size])
        else:
            (_, reconstruction, _) = hook('tconv3', lambda: dev.tconv9x9s4_luma(t, dec.w6, want_f32=False, want_u8=True, ref_u8=luminances_uint8,
                                                                                sse=slot.sse[:self.batch_size]))
        # every conv launch of this step (analysis side too: same stream, same workspace) is behind us: its error word, and a
        # clean workspace for the slot's next step
        dev.publish_step(slot.sse, slot.pinned_sse, 0, *slot.synthesis_seq, conv_ws=ws, error_word=slot.unfinished)
        return reconstruction

    def drain(self):
        """Waits until every submitted batch is through."""
        torch.cuda.synchronize(self.device)
        for slot in self._slots:
            slot.free.wait()

    def close(self):
        """Waits for the pending batches (whether or not their tickets failed) and joins the result worker: a worker still
        unwinding while the interpreter finalises aborts the process at exit. Idempotent."""
        if getattr(self, '_worker', None) is None:      # closed already, or a constructor that raised before the worker existed
            return
        try:
            self.drain()
        finally:
            self._worker.jobs.put(None)
            self._worker.join()
            self._worker = None
            with _LIVE_LOCK:
                _LIVE.get(self.device.index, weakref.WeakSet()).discard(self)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, traceback):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: nothing left to report to
            pass


# ---- the other half: containers in, reconstructions out ---------------------------------------------------

def _pack_head(shapes):
    """[(name, dtype, shape)] of a step head -> (fields {name: (byte offset, dtype, shape)}, bytes of the block): the fields one
    behind the other, each on an 8-byte boundary, the block rounded up to 16 bytes."""
    (fields, pos) = ({}, 0)
    for (name, dtype, shape) in shapes:
        pos = -(-pos//8)*8
        fields[name] = (pos, numpy.dtype(dtype), shape)
        pos += numpy.dtype(dtype).itemsize*int(numpy.prod(shape))
    return fields, -(-pos//16)*16


def _head_views(head, fields, nbytes):
    """The `fields` of `_pack_head` as numpy views of `head` (uint8, contiguous, at least `nbytes`, 8-byte aligned)."""
    if head.dtype != numpy.uint8 or head.ndim != 1 or head.size < nbytes:
        raise ValueError('`head` must be a flat uint8 array of at least {0} bytes.'.format(nbytes))
    return {name: head[pos:pos + dtype.itemsize*int(numpy.prod(shape))].view(dtype).reshape(shape) for (name, (pos, dtype, shape)) in fields.items()}


def _decode_head_fields(batch_size, nb_maps, truncated_unary_length, n_streams=None):
    n_maps = batch_size*nb_maps if n_streams is None else int(n_streams)
    return (('bits', numpy.uint32, (n_maps, 2)), ('prob_row', numpy.int32, (n_maps,)), ('bin_widths', numpy.float32, (batch_size, nb_maps)),
            ('map_mean', numpy.float32, (batch_size, nb_maps)), ('table', numpy.float64, (batch_size, nb_maps + 1, truncated_unary_length)),
            ('payload_bytes', numpy.uint64, (1,)))


def decode_head_layout(batch_size, nb_maps, truncated_unary_length, n_streams=None):
    """The "step head" of `BatchDecoder`: everything of a step's blobs but their payload, in one fixed-size block that crosses to the
    device with one copy. -> (fields {name: (byte offset, dtype, shape)}, bytes of the block, a multiple of 16):
    'bits' uint32 [n_maps][2] (arithmetic-coded stream, bypass stream), 'prob_row' int32 [n_maps] (row of 'table' a map is coded
    with, -1: not coded), 'bin_widths' and 'map_mean' float32 [batch][nb_maps], 'table' float64 [batch][nb_maps + 1][L] (every
    image's own probabilities, then the row of its exception map), 'payload_bytes' uint64 [1].
    n_streams: pairs of streams per step, None = batch_size*nb_maps, one per map. A decoder of coding tiles has one per (image, tile,
    map), `coding_tile_layout(...)['n_streams']`: 'bits' and 'prob_row' then hold that many entries, in RUN order."""
    return _pack_head(_decode_head_fields(batch_size, nb_maps, truncated_unary_length, n_streams))


def decode_head_views(head, batch_size, nb_maps, truncated_unary_length, n_streams=None):
    """The fields of `decode_head_layout` as numpy views of `head` (uint8, contiguous, at least the block's bytes, 8-byte aligned)."""
    return _head_views(head, *decode_head_layout(batch_size, nb_maps, truncated_unary_length, n_streams))


def plan_decode_step(blobs, batch_size, h_in, w_in, truncated_unary_length, are_bin_widths_learned, capacity, head, payload,
                     nb_maps=csts.NB_MAPS_3, coding_tile=None, layout=None, image_size=None):
    """The host side of one `BatchDecoder` step; numpy only. blobs: one `EAE1` blob or a sequence of them, 1..batch_size images in
    all, in the order of the step's images. Every header is parsed and checked (`container.read_header`, then the decoder's own
    height, width, truncated unary length and model kind, the number of images, the payload against `capacity`) BEFORE a byte of
    `head` or `payload` is written: a refused step (ValueError) leaves both as they were. Then `head` (uint8: `decode_head_layout`)
    is filled -- image i's map m is coded with row i*(nb_maps + 1) + m of the table, its exception map with row
    i*(nb_maps + 1) + nb_maps, the maps of absent images get -1 -- and the payloads go to `payload` (uint8) one behind the other.
    coding_tile=(th, tw) latents: the step of a decoder of coding tiles. The blobs are then `EAT1` blobs whose
    coding tile, clamped to the latent plane, is the decoder's clamped tile: anything else (an `EAE1` blob, another tile) is refused
    like the rest, with a ValueError that names `coding_tile`. `head` is `decode_head_layout(..., n_streams)`: the headers' bit
    counts, which are in payload order (image -> tile -> map), go to 'bits' in RUN order through the one static index array
    `layout['payload_order']`, and so do the rows of 'prob_row' -- every stream of image i, map m gets row i*(nb_maps + 1) + m, the
    exception map of the image's blob row i*(nb_maps + 1) + nb_maps in every tile, every stream of an absent image -1 and zero bits.
    The other fields and the payload are as without tiles: payload order is image-major, so blobs one behind the other are images one
    behind the other. layout: `coding_tile_layout(batch_size, h_in/16, w_in/16, coding_tile)` when the caller has it (it is the same
    for every step: its clamped tile is then the step's, and `coding_tile` is not looked at again), else it is computed here.
    h_in, w_in: the CODED size. image_size: None, or the real (h, w) of a decoder that crops (`BatchDecoder(pad=True)`): every blob's
    real size (its header's `crop` byte, container.py) must be that one -- without it the coded size, i.e. a crop of 0.
    -> (images, payload bytes)."""
    if isinstance(blobs, (bytes, bytearray, memoryview)):
        blobs = [blobs]
    blobs = list(blobs)
    if not blobs:
        raise ValueError('A step needs at least one blob.')
    (h_map, w_map) = (h_in//csts.STRIDE_PROD, w_in//csts.STRIDE_PROD)
    if layout is not None:
        coding_tile = layout['coding_tile']          # validated and clamped once, by whoever made the layout
    elif coding_tile is not None:
        (th, tw) = container_format._positive_pair(coding_tile, '`coding_tile`')
        coding_tile = (min(th, h_map), min(tw, w_map))
    headers = []
    for blob in blobs:
        if coding_tile is None and bytes(blob[:4]) == container_format.TILE_MAGIC:
            raise ValueError('An EAT1 container codes tiles: BatchDecoder takes EAE1 blobs only, use container.decode_region.')
        header = container_format.read_header(blob)
        if (header['height'], header['width']) != (h_in, w_in):
            raise ValueError('The container holds {0} x {1} images, the decoder was built for {2} x {3}.'.format(
                header['height'], header['width'], h_in, w_in))
        if (header['image_height'], header['image_width']) != ((h_in, w_in) if image_size is None else tuple(image_size)):
            raise ValueError('The container holds images of {0} x {1} pixels inside its {2} x {3} planes (the `crop` byte of its header), '
                             'the decoder {4}.'.format(header['image_height'], header['image_width'], h_in, w_in,
                                                       'does not crop (`BatchDecoder(..., pad=True)` does)' if image_size is None else
                                                       'was built for {0} x {1}'.format(*image_size)))
        if header['truncated_unary_length'] != truncated_unary_length:          # (`read_header` has refused anything but `nb_maps` maps)
            raise ValueError('The container was coded with a truncated unary length of {0}, the decoder was built for {1}.'.format(
                header['truncated_unary_length'], truncated_unary_length))
        if header['are_bin_widths_learned'] != bool(are_bin_widths_learned):
            raise ValueError('The container was written by the other kind of model (learned / fixed bin widths).')
        if coding_tile is not None:
            if header.get('format') != 'EAT1':
                raise ValueError('This decoder was built with `coding_tile`={0}: it takes EAT1 blobs of that coding tile, this is an EAE1 '
                                 'blob (a decoder built without `coding_tile` reads it).'.format(coding_tile))
            blob_tile = (min(header['coding_tile'][0], h_map), min(header['coding_tile'][1], w_map))
            if blob_tile != coding_tile:
                raise ValueError('The container was coded in tiles of {0} latents, the decoder was built with `coding_tile`={1}.'.format(
                    blob_tile, coding_tile))
        headers.append(header)
    nb_images = sum(header['nb_images'] for header in headers)
    if nb_images > batch_size:
        raise ValueError('The blobs hold {0} images, a step of this decoder takes {1} at most.'.format(nb_images, batch_size))
    sizes = [len(blob) - header['payload_offset'] for (blob, header) in zip(blobs, headers)]
    payload_bytes = sum(sizes)
    if payload_bytes > capacity or payload_bytes > payload.size:
        raise ValueError('The payload of this step takes {0} bytes, the decoder holds {1} per step '
                         '(BatchDecoder(payload_capacity_bytes=...)).'.format(payload_bytes, min(capacity, payload.size)))
    if coding_tile is None:
        views = decode_head_views(head, batch_size, nb_maps, truncated_unary_length)
    else:
        if layout is None:
            layout = coding_tile_layout(batch_size, h_map, w_map, coding_tile)
        nb_tiles = layout['nb_tiles']
        views = decode_head_views(head, batch_size, nb_maps, truncated_unary_length, layout['n_streams'])
        # the step in payload order, the order of the headers; one scatter each takes them to run order behind the loop
        ordered_bits = numpy.zeros((batch_size, nb_tiles, nb_maps, 2), dtype=numpy.uint32)
        ordered_rows = numpy.full((batch_size, nb_tiles, nb_maps), -1, dtype=numpy.int32)
    (first, pos) = (0, 0)
    for (blob, header, size) in zip(blobs, headers, sizes):
        n = header['nb_images']
        rows = (numpy.arange(first, first + n, dtype=numpy.int32)*(nb_maps + 1))[:, None] + numpy.arange(nb_maps, dtype=numpy.int32)[None, :]
        exception = header['idx_map_exception']
        if exception >= 0:
            rows[:, exception] = numpy.arange(first, first + n, dtype=numpy.int32)*(nb_maps + 1) + nb_maps
            views['table'][first:first + n, nb_maps] = header['exception_probabilities']
        else:
            views['table'][first:first + n, nb_maps] = 0.5
        if coding_tile is None:
            views['bits'][first*nb_maps:(first + n)*nb_maps] = header['bits']
            views['prob_row'][first*nb_maps:(first + n)*nb_maps] = rows.reshape(-1)
        else:
            ordered_bits[first:first + n] = header['bits']
            ordered_rows[first:first + n] = rows[:, None, :]
        views['bin_widths'][first:first + n] = header['bin_widths']
        views['map_mean'][first:first + n] = header['map_mean']
        views['table'][first:first + n, :nb_maps] = header['binary_probabilities']
        payload[pos:pos + size] = numpy.frombuffer(blob, dtype=numpy.uint8, count=size, offset=header['payload_offset'])
        first += n
        pos += size
    if coding_tile is None:
        views['bits'][nb_images*nb_maps:] = 0
        views['prob_row'][nb_images*nb_maps:] = -1
    else:
        views['bits'][layout['payload_order']] = ordered_bits.reshape(-1, 2)
        views['prob_row'][layout['payload_order']] = ordered_rows.reshape(-1)
    views['bin_widths'][nb_images:] = 0.
    views['map_mean'][nb_images:] = 0.
    views['table'][nb_images:] = 0.5
    views['payload_bytes'][0] = payload_bytes
    return nb_images, payload_bytes


# Streams of a `BatchDecoder` whose caller does not say (`nb_in_flight` is then two more than the streams it runs, so that the host
# fills the next slots' pinned buffers while the streams are busy). From a sweep in a process with 16 hardware queues
# (profiles/batch_decoder.md; graphs on, bin width 1.0): 1 / 2 / 3 / 4 streams take 2.12 / 1.84 / 1.73 / 1.68 ms per 24 Kodak images
# and 0.52 / 0.30 / 0.26 / 0.23 ms per single image; four is the most that was measured. A process with fewer queues runs what
# `stream_budget` leaves (two streams on four queues).
DECODER_STREAMS = 4


def _refuse_shape(batch_size, h_in, w_in, truncated_unary_length, coding_tile):
    """What every resident decoder refuses of its shape (ValueError) -> `coding_tile` as a pair of positive ints, or None."""
    if h_in % csts.STRIDE_PROD != 0 or w_in % csts.STRIDE_PROD != 0 or h_in < 1 or w_in < 1:
        raise ValueError('The image size is not divisible by the product of the three strides.')
    if not 1 <= int(truncated_unary_length) <= 255:
        raise ValueError('The truncated unary length does not belong to [1, 255].')
    if batch_size < 1:
        raise ValueError('`batch_size` is not positive.')
    if coding_tile is None:
        return None
    coding_tile = container_format._positive_pair(coding_tile, '`coding_tile`')
    if max(coding_tile) > 0xFFFF:
        raise ValueError('A side of `coding_tile` does not fit the container (65535 latents at most).')
    return coding_tile


def _decoder_device(device):
    """The device of a resident decoder: the current one, by name or by default (launches go to the current device's streams)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if device.index != torch.cuda.current_device():
        raise ValueError('`device` is {0} but the current device is cuda:{1}: build and use the decoder under '
                         '`torch.cuda.device({0!r})`.'.format(device, torch.cuda.current_device()))
    return device


def _decoder_streams(nb_streams, name):
    """The streams a resident decoder (`BatchDecoder`, `RegionDecoder`) runs: what the caller asked for, or `DECODER_STREAMS`, capped
    to the hardware queues of the process."""
    asked = nb_streams is not None
    nb_streams = max(1, int(nb_streams)) if asked else DECODER_STREAMS
    if os.environ.get('EAE_IGNORE_HW_QUEUES') != '1':
        # (a decoder has no coder streams: the one `stream_budget` always leaves for them is the margin here)
        (capped, _, _) = stream_budget(nb_streams, 1)
        # (the default is capped without a word: the caller asked for nothing)
        if asked and capped != nb_streams and not _BUDGET_WARNED[0]:
            _BUDGET_WARNED[0] = True
            import warnings
            warnings.warn('{2}: {0} streams asked for, running {1}: this process has too few hardware queues '
                          '(GPU_MAX_HW_QUEUES; streams beyond them share queues and serialise).'.format(nb_streams, capped, name),
                          RuntimeWarning, stacklevel=4)          # whoever called the constructor, behind `_build` and `__init__`
        nb_streams = capped
    return nb_streams


class DecodeTicket(object):
    """Handle on one submitted `BatchDecoder` step."""

    def __init__(self, nb_images):
        self.nb_images = nb_images
        self.errors = None                    # after result(): one entry per image, None or the exception of its first failing map
        self._done = threading.Event()
        self._error = None                    # the step's own failure (StepTimeout, a hand-off failure of the transforms)
        self._value = None
        self._job = None

    def result(self, raise_errors=True):
        """Blocks until the step is through; uint8 (nb_images, h_in, w_in): a numpy view of the slot's pinned buffer
        (`fetch_reconstruction=True`) or the device tensor, valid until the slot comes round again. Raises the first image's error
        unless `raise_errors` is False: `errors` then says which images of the array to leave alone."""
        _wait_for_ticket(self)
        if raise_errors:
            for error in self.errors:
                if error is not None:
                    raise error
        return self._value


class _DecodeJob(_Claimable):
    __slots__ = ('ticket', 'slot', 'sequence', 'payload_bytes', 'detail')

    def __init__(self, ticket, slot, sequence, payload_bytes, detail):
        """detail: per image (or crop) of the step, the column ranges [(first, end)] of the slot's results that hold its streams, in
        the order in which its first failing stream is looked for."""
        super(_DecodeJob, self).__init__()
        (self.ticket, self.slot, self.sequence, self.payload_bytes, self.detail) = (ticket, slot, sequence, payload_bytes, detail)


def _first_failure(results, ranges):
    """What `interface_cython.raise_for_status` raises for the first failing stream among the column `ranges` [(first, end)] of the
    coder's `results` (rows 2 and 3: status and stage), taken in order; None when every stream of them is fine."""
    for (first, end) in ranges:
        status = results[2, first:end]
        if status.any():
            from .kodak.lossless import interface_cython
            bad = first + int(numpy.flatnonzero(status)[0])
            try:
                interface_cython.raise_for_status(int(results[2, bad]), int(results[3, bad]))
            except Exception as exc:
                return exc
            return None
    return None


class _DecodeWorker(_StepWorker):
    """The result worker of `BatchDecoder` and `RegionDecoder`."""

    def __init__(self, payload_order=None):
        """payload_order: of a `BatchDecoder` of coding tiles (`coding_tile_layout`): the slot's results are in run order, and this
        index array takes them into the order of the payload, image -> tile -> map, which the ranges of a job then refer to."""
        super(_DecodeWorker, self).__init__()
        self.payload_order = payload_order

    def process(self, job, by_caller=False):
        (ticket, slot) = (job.ticket, job.slot)
        try:
            if by_caller and not getattr(_THREAD, 'short_sleeps', False):
                _short_sleeps_for_this_thread()
                _THREAD.short_sleeps = True
            if by_caller:
                self._wait_sequence_by_caller(*job.sequence)
            else:
                self._wait_sequence(*job.sequence)
            if int(slot.unfinished_host[0]) != 0:
                raise dev.SplitHandOffTimeout('{} tiles of a cut conv launch were not handed over: the reconstructions of this step '
                                              'are invalid (later steps are unaffected)'.format(int(slot.unfinished_host[0])))
            if int(slot.index_host[0]) != job.payload_bytes or int(slot.index_host[1]) != 0:
                raise RuntimeError('the device placed {0} payload bytes, the headers of the step announce {1}'.format(
                    int(slot.index_host[0]), job.payload_bytes))
            self._form(job)
        except StepTimeout as exc:
            self.failed = exc
            ticket._error = exc
        except Exception as exc:
            ticket._error = exc
        finally:
            if ticket.errors is None:
                ticket.errors = [ticket._error]*ticket.nb_images
            slot.free.set()
            ticket._done.set()

    def _form(self, job):
        """The ticket's errors and value from the slot's pinned blocks, once the step is through and its byte count agrees."""
        (ticket, slot) = (job.ticket, job.slot)
        results = slot.results_host
        if self.payload_order is not None:
            # status and stage of every stream in payload order: an image's first failing stream is the first of its first
            # failing tile, as `container.decode_images` meets them in the image's own blob
            results = results.take(self.payload_order, axis=1)
        ticket.errors = [_first_failure(results, ranges) for ranges in job.detail]
        ticket._value = slot.value(ticket.nb_images)


class _DecodeLane(object):
    """The device side of one slot of a resident decoder: the stream its steps run on and every device buffer between a step's
    first and last launch (the largest are the activations of the synthesis transform, 17 MB per Kodak image). No two steps in flight
    share a buffer. What differs between the decoders it reads off `decoder` (`BatchDecoder._lay_out`): the head's fields, the
    streams of a step, the class runs of a step in tiles, the latent window that is synthesised, the images the index counts."""

    def __init__(self, decoder, stream):
        (batch_size, nb_maps, device, length) = (decoder.batch_size, decoder.nb_maps, decoder.device, decoder.truncated_unary_length)
        # pairs of streams per step: batch_size*nb_maps, times the tiles of a map with a coding tile; `RegionDecoder`: the slots' maps
        n_maps = decoder._n_streams
        (rows, cols) = decoder.window
        self.stream = stream
        (fields, head_bytes) = _pack_head(decoder._head_fields)
        self.head = torch.zeros(head_bytes, dtype=torch.uint8, device=device)

        def field(name, dtype):
            """The torch twin of `_head_views`; None for a field this decoder's head does not have."""
            if name not in fields:
                return None
            (pos, numpy_dtype, shape) = fields[name]
            return self.head[pos:pos + numpy_dtype.itemsize*int(numpy.prod(shape))].view(dtype).view(shape)

        self.head_bits = field('bits', torch.int32)
        self.prob_row = field('prob_row', torch.int32)
        (self.placement, self.crop_origin) = (field('placement', torch.int32), field('crop_origin', torch.int32))      # `RegionDecoder`
        self.bin_widths = field('bin_widths', torch.float32)
        self.map_mean = field('map_mean', torch.float32)
        self.table = field('table', torch.float64).view(batch_size*(nb_maps + 1), length)
        self.payload_bytes = field('payload_bytes', torch.int64)
        self.head_bytes = torch.full((1,), head_bytes, dtype=torch.int64, device=device)
        self.payload = torch.zeros(decoder.payload_capacity_bytes, dtype=torch.uint8, device=device)
        # what goes to the host behind a step: [coder results 4 x n_maps | index words (int64: payload bytes, overflow flag, bytes per
        # image of the index -- `RegionDecoder`'s slots are the entries of ONE image, so the bytes again)]
        self.status = torch.zeros(4*n_maps + 2*(2 + decoder._index_images), dtype=torch.int32, device=device)
        self.results = self.status[:4*n_maps].view(4, n_maps)
        self.index = self.status[4*n_maps:].view(torch.int64)
        self.offsets = torch.zeros((n_maps, 2), dtype=torch.int64, device=device)
        (self.coder_streams, self.symbols, self.decoded, self.classes) = (None, None, None, None)
        if decoder._runs is None:
            self.coder_streams = dev.CoderStreams(n_maps, rows*cols, length, device, results=self.results)
            self.workspace = dev.coder_workspace(n_maps, rows*cols, length, device)
            self.symbols = torch.zeros((batch_size, nb_maps, rows*cols), dtype=torch.int16, device=device)
        else:
            # The buffers of `BatchCodec`'s slot (`_Slot`), read the other way: the step's entries in run order, every shape class
            # decoded into its run of the tile-major buffer (`_class_batches`).
            self.decoded = torch.zeros(decoder._elements, dtype=torch.int16, device=device)
            (self.classes, need) = _class_batches(decoder._runs, self.results, self.decoded, self.prob_row, self.offsets, length, device)
            self.workspace = torch.empty(need, dtype=torch.uint8, device=device)
        # a plane per image, or a window per crop
        self.shifted = torch.zeros((batch_size, rows, cols, nb_maps), dtype=torch.float32, device=device)
        (self.scratch, self.unfinished) = decoder.decoder.model.decode_scratch(batch_size, rows, cols)


class _DecodeSlot(object):
    """What one step in flight of a resident decoder owns: its device buffers (`lane`), the pinned buffers the host fills and reads,
    the planes (of the images, or of the crops' windows), for a `RegionDecoder` the crops, the step counter, the captured graph.
    Made once."""

    def __init__(self, decoder, lane):
        (batch_size, device, fetch) = (decoder.batch_size, decoder.device, decoder.fetch_reconstruction)
        n_maps = decoder._n_streams
        (rows, cols) = decoder.window
        self.lane = lane
        self.region = decoder.region
        self.pinned_head = torch.zeros(lane.head.numel(), dtype=torch.uint8).pin_memory()
        self.pinned_payload = torch.zeros(decoder.payload_capacity_bytes, dtype=torch.uint8).pin_memory()
        (self.head_host, self.payload_host) = (self.pinned_head.numpy(), self.pinned_payload.numpy())
        self.pinned_status = torch.zeros(lane.status.numel(), dtype=torch.int32).pin_memory()
        self.results_host = self.pinned_status[:4*n_maps].view(4, n_maps).numpy()
        self.index_host = self.pinned_status[4*n_maps:].view(torch.int64).numpy()
        self.pinned_unfinished = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.unfinished_host = self.pinned_unfinished.numpy()
        self.planes = torch.zeros((batch_size, 16*rows, 16*cols), dtype=torch.uint8, device=device)
        # what a ticket returns: the planes, fetched or not; of a `RegionDecoder` the crops, cut into pinned memory or on the device
        (self.pinned_rec, self.crops, self.pinned_crops) = (None, None, None)
        if self.region is None:
            if fetch:
                self.pinned_rec = torch.zeros((batch_size, 16*rows, 16*cols), dtype=torch.uint8).pin_memory()
        else:
            crop_bytes = -(-batch_size*self.region[0]*self.region[1]//16)*16          # whole 16-byte words: `device.publish_crops`
            if fetch:
                self.pinned_crops = torch.zeros(crop_bytes, dtype=torch.uint8).pin_memory()
            else:
                self.crops = torch.zeros(crop_bytes, dtype=torch.uint8, device=device)
        self.rec_host = self.pinned_rec.numpy() if self.pinned_rec is not None else None
        self.crops_host = self.pinned_crops.numpy() if self.pinned_crops is not None else None
        self.seq_dev = torch.zeros(2, dtype=torch.int32, device=device)      # [step counter, ticket word of device.publish_step]
        self.pinned_seq = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.seq_host = self.pinned_seq.numpy()
        self.count = 0
        self.free = threading.Event()
        self.free.set()
        self.graph = None

    def value(self, n):
        """What the ticket of a step of n images (crops) returns."""
        if self.region is None:
            return self.rec_host[:n] if self.rec_host is not None else self.planes[:n]
        (rh, rw) = self.region
        return (self.crops_host if self.crops_host is not None else self.crops)[:n*rh*rw].reshape(n, rh, rw)


class BatchDecoder(object):
    """`EAE1` containers -> uint8 reconstructions for steps of a fixed shape, resident and pipelined: what `container.decode_images`
    computes (same bytes), with every buffer made once, the host work of a step in `plan_decode_step`, and the step as one chain of
    launches on one of `nb_streams` private streams (one hipGraph per slot with `use_graphs`). DESIGN.md section 14. With
    `coding_tile`: the same for the tile-indexed `EAT1` containers of that coding tile (section 16)."""
    (pad, image_size) = (False, None)      # `BatchDecoder(pad=True)`; a `RegionDecoder` never crops to a real size

    def __init__(self, variables, are_bin_widths_learned, batch_size, h_in, w_in, truncated_unary_length, device='cuda', nb_in_flight=None,
                 nb_streams=None, use_graphs=False, payload_capacity_bytes=None, fetch_reconstruction=True, coding_tile=None, pad=False,
                 keep_reconstruction=False):
        """nb_streams: consecutive steps go round that many private streams, so that one step's serial decoder core runs beside
        another step's synthesis transform. nb_in_flight: steps that may be pending at once (= slots: pinned buffers and planes).
        None: `DECODER_STREAMS` streams, or as many of them as the process's hardware queues allow (`stream_budget`; streams asked
        for explicitly are capped too, with a warning), and two more steps in flight than streams.
        use_graphs: capture the step of every slot into a hipGraph at the first submit and replay it afterwards.
        payload_capacity_bytes: payload bytes a step may hold (rounded up to 16; a device buffer per stream and a pinned one per
        slot). None: batch_size*h_in*w_in. fetch_reconstruction: the planes reach pinned host memory inside the step and `result()`
        is a numpy view of them; False: `result()` is the slot's device tensor.
        coding_tile: (th, tw) in latents: the decoder reads `EAT1` blobs coded in that tile (clamped to the latent plane) -- what
        `BatchCodec(emit_container=True, coding_tile=(th, tw))` and `container.encode_images(..., coding_tile=(th, tw))` write --
        and nothing else: an `EAE1` blob or another tile is refused by `submit` (ValueError). Every (image, tile, map) is a pair of
        streams of its own, so the decoder core's serial chains are a tile long instead of a map. At most 65,535 (image, tile) pairs
        per step. None: `EAE1` blobs only.
        pad: h_in x w_in is the REAL size of the images, any positive integers: the decoder takes the blobs
        whose coded size is that size rounded up to multiples of 16 and whose `crop` byte gives exactly it -- what
        `container.encode_images(..., pad=True)` and `BatchCodec(..., pad=True)` write --, refuses every other (`plan_decode_step`), and
        `result()` is uint8 (n, h_in, w_in), the top-left of the coded planes, cut by `device.publish_crops` at the end of the step
        (into pinned memory with `fetch_reconstruction`). A decoder without `pad` refuses a blob whose `crop` is not 0.
        keep_reconstruction: as `BatchCodec`'s: every ticket gets, at submit time, `decoded_event`, recorded on the slot's stream
        behind the step, and `reconstruction_uint8`, the slot's planes on the device -- `planes[:n, :h_in, :w_in]` with `pad`, the
        top-left view of the coded planes, `planes[:n]` without --, valid until the slot comes round again: another stream waits for
        the event and reads them there (`ColourDecoder`). False: neither attribute exists and no event is made."""
        (self.pad, self.image_size) = (bool(pad), None)
        if self.pad:
            self.image_size = (container_format._positive_int(h_in, '`h_in`'), container_format._positive_int(w_in, '`w_in`'))
            (h_in, w_in) = container_format.coded_size(*self.image_size)
        self._lay_out(batch_size, h_in, w_in, truncated_unary_length, payload_capacity_bytes, coding_tile)
        if self.pad:
            self.region = self.image_size          # what a slot cuts out of its planes for the ticket (`_DecodeSlot`), at the origin
        self._build(variables, are_bin_widths_learned, device, nb_in_flight, nb_streams, use_graphs, fetch_reconstruction, keep_reconstruction)

    def _lay_out(self, batch_size, h_in, w_in, truncated_unary_length, payload_capacity_bytes, coding_tile):
        """The first half of construction: refuses what no decoder can be built for, then lays a step out -- everything `_build`,
        `_DecodeLane` and `_DecodeSlot` size their buffers by. numpy only: nothing is allocated, so every refusal lies in front of
        every allocation."""
        coding_tile = _refuse_shape(batch_size, h_in, w_in, truncated_unary_length, coding_tile)
        (h_map, w_map) = (h_in//csts.STRIDE_PROD, w_in//csts.STRIDE_PROD)
        # whole images: no crops, and the latents that are synthesised are the plane
        (self.coding_tile, self.region, self.window, self.map_size) = (None, None, (h_map, w_map), h_map*w_map)
        # pairs of streams of a step, one per map; in tiles the class runs [((rows, cols), entries, first stream, first element)] too
        (self._n_streams, self._runs, self._elements) = (int(batch_size)*csts.NB_MAPS_3, None, None)
        self._tile_layout = None
        if coding_tile is not None:
            self.coding_tile = (min(coding_tile[0], h_map), min(coding_tile[1], w_map))
            if int(batch_size)*container_format._nb_tiles(h_map, w_map, self.coding_tile) > 65535:
                raise ValueError('`batch_size` images of {0} coding tiles each are more than the 65535 (image, tile) pairs a step can hold.'.format(
                    container_format._nb_tiles(h_map, w_map, self.coding_tile)))
            # everything a step in tiles needs beyond its blobs is the same for every step: made once, shared by the slots
            self._tile_layout = tiled = coding_tile_layout(int(batch_size), h_map, w_map, self.coding_tile)
            (self._n_streams, self._runs, self._elements) = (tiled['n_streams'], tiled['runs'], tiled['elements'])
        self._payload_order = self._tile_layout['payload_order'] if self._tile_layout else None
        self._index_images = int(batch_size)          # images whose bytes the index counts
        self._head_fields = _decode_head_fields(int(batch_size), csts.NB_MAPS_3, int(truncated_unary_length), self._n_streams)
        # what the worker scans for an image's first failing stream (`_DecodeJob.detail`): its streams, in payload order
        per_image = self._n_streams//int(batch_size)
        self._image_ranges = [[(i*per_image, (i + 1)*per_image)] for i in range(int(batch_size))]
        self._set_sizes(batch_size, h_in, w_in, truncated_unary_length, payload_capacity_bytes, int(batch_size)*int(h_in)*int(w_in))

    def _set_sizes(self, batch_size, h_in, w_in, truncated_unary_length, payload_capacity_bytes, default_capacity):
        """The end of `_lay_out`: the last refusal, and the sizes every resident decoder has."""
        if payload_capacity_bytes is None:
            payload_capacity_bytes = default_capacity
        if int(payload_capacity_bytes) < 1:
            raise ValueError('`payload_capacity_bytes` is not positive.')
        self.payload_capacity_bytes = -(-int(payload_capacity_bytes)//16)*16
        (self.batch_size, self.h_in, self.w_in) = (int(batch_size), int(h_in), int(w_in))
        self.nb_maps = csts.NB_MAPS_3
        self.truncated_unary_length = int(truncated_unary_length)

    def _build(self, variables, are_bin_widths_learned, device, nb_in_flight, nb_streams, use_graphs, fetch_reconstruction,
               keep_reconstruction=False):
        """The second half of construction, of a decoder `_lay_out` has accepted: the device, the model, the streams, the static
        tables, the slots, the worker."""
        self.device = _decoder_device(device)
        self.learned = bool(are_bin_widths_learned)
        self.decoder = pipeline.DeviceDecoder(variables, are_bin_widths_learned, self.device)
        self.fetch_reconstruction = bool(fetch_reconstruction)
        self.keep_reconstruction = bool(keep_reconstruction)
        self.use_graphs = bool(use_graphs)
        self.nb_streams = nb_streams = _decoder_streams(nb_streams, type(self).__name__)
        self.nb_in_flight = max(1, int(nb_in_flight)) if nb_in_flight is not None else nb_streams + 2
        self.nb_slots = self.nb_in_flight
        self._upload_tables()
        streams = _step_streams(self.nb_streams, self.device)
        self._slots = [_DecodeSlot(self, _DecodeLane(self, streams[k % self.nb_streams])) for k in range(self.nb_slots)]
        self._index = 0
        self._warm = False
        self._worker = _DecodeWorker(self._payload_order)
        self._worker.start()
        with _LIVE_LOCK:
            _LIVE.setdefault(self.device.index, weakref.WeakSet()).add(self)

    def _upload_tables(self):
        """What the launches of every step read beside the slot's buffers: on the device once, shared by the slots."""
        tiled = self._tile_layout
        if tiled is not None:
            self._tile_plan_host = tiled['plan']
            self._tile_plan = torch.from_numpy(tiled['plan']).to(self.device)
            # `device.coder_index_tiles`: per payload-order entry, its run-order index and half the stream stride of its class
            half_stride = numpy.array([dev.coder_stream_stride_bytes(int(tiled['tiles'][t, 2]*tiled['tiles'][t, 3]), self.truncated_unary_length)//2
                                       for (_, t) in tiled['entries']], dtype=numpy.int64)
            self._tile_table = torch.from_numpy(numpy.stack([tiled['run_entry'], half_stride], axis=1)).to(self.device)
        if self.pad:
            # `device.publish_crops`: every image's crop starts at (0, 0)
            self._crop_origins = torch.zeros((self.batch_size, 2), dtype=torch.int32, device=self.device)

    def submit(self, blobs):
        """One `EAE1` blob of 1..batch_size images, or a sequence of `EAE1` blobs holding that many in all -> DecodeTicket
        (`EAT1` blobs of the decoder's coding tile, and only those, for a decoder built with `coding_tile`).
        Everything is checked on the host first (`plan_decode_step`: ValueError, nothing launched); then the step is enqueued and
        nothing is waited for except a free slot."""
        if self._worker is None:
            raise RuntimeError('this decoder is closed')
        if self._worker.failed is not None:
            raise StepTimeout('this decoder stopped taking steps: {0}'.format(self._worker.failed))
        if self.use_graphs and not self._warm:
            # one ordinary step first (lazy module loads, function attributes), then every slot's graph, while nothing is in flight
            ticket = self._submit(blobs, replay=False)
            ticket.result(raise_errors=False)
            try:
                self._capture_all()
            except BaseException:
                for slot in self._slots:
                    slot.graph = None
                raise
            self._warm = True
            return ticket
        return self._submit(blobs, replay=self.use_graphs)

    def _submit(self, blobs, replay):
        slot = self._slots[self._index % self.nb_slots]
        slot.free.wait()
        (nb_images, payload_bytes, detail) = self._plan_step(slot, blobs)
        slot.free.clear()
        self._index += 1
        expected = slot.count + 1
        try:
            ticket = DecodeTicket(nb_images)
            caller = torch.cuda.current_stream()
            try:
                torch.cuda.set_stream(slot.lane.stream)
                if replay:
                    if slot.graph is None:
                        raise RuntimeError('this slot has no captured graph (a capture failed earlier)')
                    slot.graph.replay()
                else:
                    self._launch_step(slot)
                if self.keep_reconstruction:
                    # behind the step on the slot's stream, never inside `_launch_step`, which is what a graph captures
                    ticket.decoded_event = torch.cuda.Event()
                    ticket.decoded_event.record(slot.lane.stream)
                    ticket.reconstruction_uint8 = self._kept(slot, nb_images)
            finally:
                torch.cuda.set_stream(caller)
            job = _DecodeJob(ticket, slot, (slot.seq_host, (expected,)), payload_bytes, detail)
            ticket._job = (job, self._worker)
            self._worker.jobs.put(job)
            slot.count = expected
            return ticket
        except BaseException:
            try:
                torch.cuda.synchronize(self.device)
                slot.count = int(slot.seq_dev[0].item())
                slot.seq_dev[1:].zero_()
            except Exception:
                pass
            slot.free.set()
            raise

    def _kept(self, slot, nb_images):
        """`reconstruction_uint8` of a ticket (`keep_reconstruction`): what of the slot another stream reads behind `decoded_event`."""
        return slot.planes[:nb_images, :self.image_size[0], :self.image_size[1]] if self.pad else slot.planes[:nb_images]

    def _plan_step(self, slot, blobs):
        """The host side of a step, into the slot's pinned head and payload -> (images, payload bytes, detail for the worker).
        Raises ValueError, with the slot untouched, for a step it refuses."""
        (nb_images, payload_bytes) = plan_decode_step(blobs, self.batch_size, self.h_in, self.w_in, self.truncated_unary_length, self.learned,
                                                      self.payload_capacity_bytes, slot.head_host, slot.payload_host, self.nb_maps,
                                                      self.coding_tile, self._tile_layout, self.image_size)
        return nb_images, payload_bytes, self._image_ranges[:nb_images]

    def _capture_all(self):
        """Every slot's step as one hipGraph, while nothing of this decoder is in flight (and the other codecs of the device are
        idle: they share the process's streams, `BatchCodec._capture_all`)."""
        with _LIVE_LOCK:
            others = [c for c in _LIVE.get(self.device.index, ()) if c is not self and getattr(c, '_worker', None) is not None]
        for other in others:
            other.drain()
        torch.cuda.synchronize(self.device)
        for slot in self._slots:
            slot.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(slot.graph, stream=slot.lane.stream, capture_error_mode='thread_local'):
                self._launch_step(slot)

    def _launch_step(self, slot):
        """The step of `slot` on the current stream: one chain, no argument of which depends on the step's contents."""
        lane = slot.lane
        dev.fetch_prefix(slot.pinned_head, lane.head, lane.head_bytes)                      # the head: a fixed size
        dev.fetch_prefix(slot.pinned_payload, lane.payload, lane.payload_bytes)             # the payload: the bytes the head announces
        lane.results[:2].copy_(lane.head_bits.view(-1, 2).t())                              # [n_maps][2] -> the coder's two arrays
        self._launch_latents(slot)
        self.decoder.model.decode_into(lane.shifted, slot.planes, lane.scratch)
        self._launch_output(slot)
        dev.publish_to_host(lane.unfinished, slot.pinned_unfinished)
        dev.publish_step(lane.status, slot.pinned_status, lane.status.numel(), slot.seq_dev[1:2], slot.seq_dev[0:1], slot.pinned_seq)

    @staticmethod
    def _launch_classes(lane):
        """One unpack and one decoder batch per shape class of a step in tiles, into the tile-major buffer."""
        for (streams, tiles, rows, offsets) in lane.classes:
            dev.coder_unpack_into(streams, lane.payload, offsets)
            dev.coder_decode_batch(streams, lane.table, rows, workspace=lane.workspace, out=tiles)

    def _launch_latents(self, slot):
        """The first half of a step: the fetched bit counts and payload -> the dequantised latents in `lane.shifted`."""
        lane = slot.lane
        if self.coding_tile is None:
            streams = lane.coder_streams
            dev.coder_index_streams(streams, self.nb_maps, self.payload_capacity_bytes, offsets=lane.offsets, index=lane.index)
            dev.coder_unpack_into(streams, lane.payload, lane.offsets)
            dev.coder_decode_batch(streams, lane.table, lane.prob_row, workspace=lane.workspace, out=lane.symbols.view(-1, self.map_size))
            dev.dequantize_maps_rows(lane.symbols, lane.bin_widths, lane.map_mean, out_shifted=lane.shifted)
        else:
            # (image, tile) entries instead of whole maps: the bit counts lie in run order, the index takes the
            # offsets in payload order, then one unpack and one decoder batch per shape class into the tile-major buffer, and one
            # launch dequantises every tile of the step, with its image's rows, into the latents (every latent is in exactly one tile)
            dev.coder_index_tiles(lane.results[0], lane.results[1], self._tile_table, self.nb_maps, self._tile_layout['nb_tiles'],
                                  self.payload_capacity_bytes, offsets=lane.offsets, index=lane.index)
            self._launch_classes(lane)
            dev.tile_symbols_dequantize_rows(lane.decoded, self._tile_plan, self._tile_plan_host, lane.bin_widths, lane.map_mean, lane.shifted)

    def _launch_output(self, slot):
        """The second half of a step, behind the synthesis transform: what the ticket returns reaches the host (if it is to)."""
        if self.pad:
            (h, w) = self.image_size
            dev.publish_crops(slot.planes, self._crop_origins, slot.pinned_crops if slot.pinned_crops is not None else slot.crops, h, w)
        elif slot.pinned_rec is not None:
            dev.publish_to_host(slot.planes, slot.pinned_rec)

    def drain(self):
        """Waits until every submitted step is through."""
        torch.cuda.synchronize(self.device)
        for slot in self._slots:
            slot.free.wait()

    def close(self):
        """Waits for the pending steps and joins the result worker. Idempotent."""
        if getattr(self, '_worker', None) is None:
            return
        try:
            self.drain()
        finally:
            self._worker.jobs.put(None)
            self._worker.join()
            self._worker = None
            with _LIVE_LOCK:
                _LIVE.get(self.device.index, weakref.WeakSet()).discard(self)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, traceback):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- crops out of EAT1 containers, resident and pipelined --------------------------------------------------

class RegionSource(object):
    """An `EAT1` (or `EAE1`) container a `RegionDecoder` cuts crops out of: a bytes-like blob or a seekable binary file object. The
    header is parsed and checked ONCE, here (`container.read_header`'s checks; of a file only the header is read); what stays is
    `header`, and per (image, tile) entry the byte offset `starts` and the byte length `sizes` of its streams in the source, int64
    [nb_images, nb_tiles]. `read(entries)` returns the bytes of [(image, tile)] entries.
    pad: a source whose header's `crop` byte is not 0 -- images of `image_height` x `image_width` pixels, the top-left of coded planes
    of `header['height']` x `header['width']` -- is accepted, for a `RegionDecoder(pad=True)` of that real size; False: refused."""

    def __init__(self, source, pad=False):
        (self.header, self._blob) = container_format._source_header(source)
        self._source = source
        header = self.header
        self.pad = bool(pad)
        (self.image_height, self.image_width) = (header['image_height'], header['image_width'])
        if not self.pad and (header['image_height'], header['image_width']) != (header['height'], header['width']):
            raise ValueError('The source holds images of {0} x {1} pixels inside {2} x {3} planes (the `crop` byte of its header): '
                             '`RegionSource` / `RegionDecoder` do not crop to a real size; `container.decode_region` does.'.format(
                                 header['image_height'], header['image_width'], header['height'], header['width']))
        (self.h_map, self.w_map) = (header['height']//csts.STRIDE_PROD, header['width']//csts.STRIDE_PROD)
        (tile, bits) = container_format._tile_layout(header)
        self.coding_tile = (min(tile[0], self.h_map), min(tile[1], self.w_map))          # clamped, as `coding_tile_grid` cuts the plane
        self.bits = bits                                                                 # uint32 [nb_images, nb_tiles, nb_maps, 2]
        self.sizes = container_format._entry_bytes(bits)
        flat = self.sizes.reshape(-1)
        self.starts = (header['payload_offset'] + numpy.cumsum(flat) - flat).reshape(self.sizes.shape)
        # the rows the coder decodes an image's maps with, the exception map's last: float64 [nb_images, nb_maps + 1, L]
        (nb_images, nb_maps, length) = (header['nb_images'], header['nb_maps'], header['truncated_unary_length'])
        self.table = numpy.full((nb_images, nb_maps + 1, length), 0.5, dtype=numpy.float64)
        self.table[:, :nb_maps] = header['binary_probabilities']
        self.prob_row = numpy.arange(nb_maps, dtype=numpy.int32)
        if header['idx_map_exception'] >= 0:
            self.table[:, nb_maps] = header['exception_probabilities']
            self.prob_row[header['idx_map_exception']] = nb_maps

    def read(self, entries):
        """One bytes-like chunk per (image, tile) of `entries`: slices of an in-memory blob; of a file, adjacent ranges in one read
        (`container.fetch_region`'s reader)."""
        ranges = [(int(self.starts[i, t]), int(self.starts[i, t] + self.sizes[i, t])) for (i, t) in entries]
        return container_format._read_ranges(self._source, self._blob, ranges)


def region_window(h, w, region):
    """(Rs, Cs): the latent rows and columns of the window a `RegionDecoder` synthesises for crops of region = (rh, rw) pixels out
    of an h x w latent plane: the region's latents, one more where it is not aligned to 16, and `pipeline.DECODER_HALO` around them,
    clamped to the plane."""
    (before, after) = pipeline.DECODER_HALO
    return (min(h, (region[0] + 14)//16 + 1 + before + after), min(w, (region[1] + 14)//16 + 1 + before + after))


def region_origin(h, w, Rs, Cs, y0, x0):
    """(r0, c0): where the Rs x Cs window of the crop at pixel (y0, x0) starts in the h x w latent plane. The window contains
    `container.region_plan`'s minimal sub-plane, and where it was shifted to stay inside the plane its edge is the plane's edge."""
    before = pipeline.DECODER_HALO[0]
    return (min(max(y0//16 - before, 0), h - Rs), min(max(x0//16 - before, 0), w - Cs))


def _axis_kinds(size, tile, window):
    """One axis of the coding-tile grid against a window of `window` latents at every position: (kind of every grid index -- 0: a
    full tile, 1: the shorter last one --, per kind the most tiles of it any position touches)."""
    count = -(-size//tile)
    kinds = [1 if (k == count - 1 and size % tile) else 0 for k in range(count)]
    most = [0, 0]
    for start in range(size - window + 1):
        touched = kinds[start//tile:(start + window - 1)//tile + 1]
        most = [max(most[0], touched.count(0)), max(most[1], touched.count(1))]
    return kinds, most


def region_layout(batch_size, h, w, coding_tile, Rs, Cs):
    """Where everything of a `RegionDecoder` step lies; numpy only, the same for every step. batch_size crops,
    each an Rs x Cs window of an h x w latent plane coded in `coding_tile` = (th, tw) latents (clamped to the plane). The grid has
    two kinds of tile rows (full, last) and of tile columns, so at most four shape classes; a crop gets, per class, as many SLOTS as
    the most tile rows of the class's row kind any window position touches, times the same of the columns. A slot is one (crop,
    tile) of a step, or absent. Run order -- the order of the streams, the results, the offsets, the tile-major `decoded` buffer AND
    of the payload -- is class -> crop -> slot. -> dict: 'coding_tile' (clamped), 'h', 'w', 'window' (Rs, Cs), 'batch_size', 'tiles'
    and 'classes' (`container.coding_tile_grid`), 'class_slots' [slots per crop of every class], 'class_first' [run index of every
    class's first slot], 'slots_per_crop', 'n_slots', 'n_streams' = n_slots*128, 'runs' [((rows, cols), slots of the class, first
    stream, first element)] as `coding_tile_layout`'s, class runs on 128-element boundaries, 'elements' of the `decoded` buffer,
    'slots' int64 [n_slots, 3] (rows, cols, element offset: `device.tile_symbols_dequantize_placed`'s static half)."""
    batch_size = container_format._positive_int(batch_size, '`batch_size`')
    (th, tw) = container_format._positive_pair(coding_tile, '`coding_tile`')
    coding_tile = (min(th, h), min(tw, w))
    if not (1 <= Rs <= h and 1 <= Cs <= w):
        raise ValueError('The window does not fit the latent plane.')
    (tiles, classes) = container_format.coding_tile_grid(h, w, coding_tile)
    (row_kinds, most_rows) = _axis_kinds(h, coding_tile[0], Rs)
    (col_kinds, most_cols) = _axis_kinds(w, coding_tile[1], Cs)
    tiles_per_row = len(col_kinds)
    class_slots = [0]*len(classes)
    for (i, rk) in enumerate(row_kinds):
        for (j, ck) in enumerate(col_kinds):
            class_slots[int(tiles[i*tiles_per_row + j, 4])] = most_rows[rk]*most_cols[ck]
    nb_maps = csts.NB_MAPS_3
    (runs, class_first, slots, first, pos) = ([], [], [], 0, 0)
    for (cls, (rows, cols)) in enumerate(classes):
        count = batch_size*class_slots[cls]
        runs.append(((rows, cols), count, first*nb_maps, pos))
        class_first.append(first)
        slots += [(rows, cols, pos + k*nb_maps*rows*cols) for k in range(count)]
        first += count
        pos = (pos + count*nb_maps*rows*cols + 127)//128*128
    return {'coding_tile': coding_tile, 'h': h, 'w': w, 'window': (Rs, Cs), 'batch_size': batch_size, 'tiles': tiles, 'classes': classes,
            'tiles_per_row': tiles_per_row, 'class_slots': class_slots, 'class_first': class_first, 'slots_per_crop': sum(class_slots),
            'n_slots': first, 'n_streams': first*nb_maps, 'runs': runs, 'elements': max(pos, 128),
            'slots': numpy.array(slots, dtype=numpy.int64).reshape(-1, 3)}


def _region_head_fields(batch_size, n_slots, truncated_unary_length, nb_maps=csts.NB_MAPS_3):
    n_streams = int(n_slots)*nb_maps
    return (('bits', numpy.uint32, (n_streams, 2)), ('prob_row', numpy.int32, (n_streams,)), ('placement', numpy.int32, (int(n_slots), 4)),
            ('crop_origin', numpy.int32, (batch_size, 2)), ('bin_widths', numpy.float32, (batch_size, nb_maps)),
            ('map_mean', numpy.float32, (batch_size, nb_maps)), ('table', numpy.float64, (batch_size, nb_maps + 1, truncated_unary_length)),
            ('payload_bytes', numpy.uint64, (1,)))


def region_head_layout(batch_size, n_slots, truncated_unary_length, nb_maps=csts.NB_MAPS_3):
    """The step head of `RegionDecoder`, in the manner of `decode_head_layout`: one fixed-size block, one copy. -> (fields {name:
    (byte offset, dtype, shape)}, bytes of the block, a multiple of 16): 'bits' uint32 [n_streams][2] and 'prob_row' int32
    [n_streams] in run order, n_streams = n_slots*nb_maps (an absent slot: zero bits, -1); 'placement' int32 [n_slots][4] (crop or
    -1, tile origin row and col in the crop's window, 0); 'crop_origin' int32 [batch][2] (the crop in its window's reconstruction);
    'bin_widths', 'map_mean' float32 [batch][nb_maps]; 'table' float64 [batch][nb_maps + 1][L] (each crop's own source's rows,
    the exception map's last); 'payload_bytes' uint64 [1]."""
    return _pack_head(_region_head_fields(batch_size, n_slots, truncated_unary_length, nb_maps))


def region_head_views(head, batch_size, n_slots, truncated_unary_length, nb_maps=csts.NB_MAPS_3):
    """The fields of `region_head_layout` as numpy views of `head` (uint8, contiguous, at least the block's bytes, 8-byte aligned)."""
    return _head_views(head, *region_head_layout(batch_size, n_slots, truncated_unary_length, nb_maps))


def place_region(layout, y0, x0):
    """The grid tiles the window of the crop at pixel (y0, x0) meets, and where they go -> ((r0, c0), [(tile, slot of the crop's
    class-major slots: (class, index within the class), tile origin row - r0, tile origin col - c0)]) in tile row-major order."""
    ((Rs, Cs), (th, tw), tiles) = (layout['window'], layout['coding_tile'], layout['tiles'])
    (r0, c0) = region_origin(layout['h'], layout['w'], Rs, Cs, y0, x0)
    used = [0]*len(layout['classes'])
    placed = []
    for i in range(r0//th, (r0 + Rs - 1)//th + 1):
        for j in range(c0//tw, (c0 + Cs - 1)//tw + 1):
            t = i*layout['tiles_per_row'] + j
            cls = int(tiles[t, 4])
            if used[cls] >= layout['class_slots'][cls]:
                raise AssertionError('the window at ({0}, {1}) needs more slots of class {2} than the layout holds'.format(r0, c0, cls))
            placed.append((t, (cls, used[cls]), int(tiles[t, 0]) - r0, int(tiles[t, 1]) - c0))
            used[cls] += 1
    return (r0, c0), placed


def _refuse_region_request(source, image, y0, x0, layout, region, truncated_unary_length, are_bin_widths_learned, image_size=None):
    """What `plan_region_step` refuses (ValueError) of one request by its source's header alone: nothing is read, nothing written."""
    (h, w) = (layout['h'], layout['w'])
    (rh, rw) = region
    header = source.header
    if (source.h_map, source.w_map) != (h, w):
        raise ValueError('The source holds {0} x {1} images, the decoder was built for {2} x {3}.'.format(
            header['height'], header['width'], 16*h, 16*w))
    if header.get('format') != 'EAT1':
        raise ValueError('This decoder takes EAT1 sources of `coding_tile`={0}: this is an EAE1 source, whose maps are coded whole '
                         '(container.decode_region reads a crop out of it).'.format(layout['coding_tile']))
    if source.coding_tile != layout['coding_tile']:
        raise ValueError('The source was coded in tiles of {0} latents, the decoder was built with `coding_tile`={1}.'.format(
            source.coding_tile, layout['coding_tile']))
    if header['truncated_unary_length'] != truncated_unary_length:
        raise ValueError('The source was coded with a truncated unary length of {0}, the decoder was built for {1}.'.format(
            header['truncated_unary_length'], truncated_unary_length))
    if header['are_bin_widths_learned'] != bool(are_bin_widths_learned):
        raise ValueError('The source was written by the other kind of model (learned / fixed bin widths).')
    if not 0 <= image < header['nb_images']:
        raise ValueError('The source holds {0} images: there is no image {1}.'.format(header['nb_images'], image))
    real = (header['image_height'], header['image_width'])
    if image_size is None:
        if real != (header['height'], header['width']):
            raise ValueError('The source holds images of {0} x {1} pixels inside {2} x {3} planes: a decoder built without `pad` '
                             'does not crop to a real size.'.format(real[0], real[1], header['height'], header['width']))
    elif real != tuple(image_size):
        raise ValueError('The source holds images of {0} x {1} pixels, the decoder was built for {2} x {3}.'.format(
            real[0], real[1], image_size[0], image_size[1]))
    if y0 < 0 or x0 < 0 or y0 + rh > real[0] or x0 + rw > real[1]:
        raise ValueError('The region {0} leaves the {1} x {2} image.'.format((int(y0), int(x0), rh, rw), real[0], real[1]))


def plan_region_step(requests, layout, head, payload, capacity, region, truncated_unary_length, are_bin_widths_learned,
                     nb_maps=csts.NB_MAPS_3, image_size=None):
    """The host side of one `RegionDecoder` step; numpy only (and the sources' own reads). requests: 1..batch_size of (RegionSource,
    image, y0, x0); layout: `region_layout`; region = (rh, rw) pixels. EVERYTHING is checked -- and every byte range is read -- before
    a byte of `head` (uint8: `region_head_layout`) or `payload` (uint8) is written: a refused step (ValueError) leaves both as they
    were. Refused: no request or more than the layout's batch; a source of another size, of another clamped coding tile, of another
    truncated unary length, of the other model kind, or an `EAE1` one; an image the source does not hold; a region that leaves the
    image; a payload beyond `capacity`. Then the head is filled -- crop k's map m decodes with row k*(nb_maps + 1) + m of the table,
    its exception map with row k*(nb_maps + 1) + nb_maps; absent slots get zero bits, row -1 and crop -1, absent crops zero bin
    widths and means and rows of 0.5 -- and the placed entries' bytes go to `payload` in run order, one behind the other.
    image_size: None, or the REAL size (h, w) of the images of a `RegionDecoder(pad=True)`, the top-left of the coded plane the
    layout was made for: a source of another real size is refused, and a region must lie inside the real image. None: a source
    whose real size is not its coded size (`RegionSource(pad=True)` of a padded container) is refused.
    -> (crops, payload bytes, per crop the run-order slots of its tiles in tile row-major order)."""
    requests = list(requests)
    (batch_size, n_slots) = (layout['batch_size'], layout['n_slots'])
    if not requests:
        raise ValueError('A step needs at least one request.')
    if len(requests) > batch_size:
        raise ValueError('{0} requests, a step of this decoder takes {1} at most.'.format(len(requests), batch_size))
    (steps, payload_bytes) = ([], 0)
    for request in requests:
        if not isinstance(request, (tuple, list)) or len(request) != 4 or not isinstance(request[0], RegionSource):
            raise ValueError('A request is (RegionSource, image, y0, x0).')
        (source, image, y0, x0) = request
        for x in (image, y0, x0):
            if isinstance(x, bool) or not isinstance(x, (int, numpy.integer)):
                raise ValueError('A request is (RegionSource, image, y0, x0) in integers.')
        _refuse_region_request(source, image, y0, x0, layout, region, truncated_unary_length, are_bin_widths_learned, image_size)
        ((r0, c0), placed) = place_region(layout, int(y0), int(x0))
        payload_bytes += int(sum(source.sizes[image, t] for (t, _, _, _) in placed))
        steps.append((source, int(image), (int(y0) - 16*r0, int(x0) - 16*c0), placed))
    if payload_bytes > capacity or payload_bytes > payload.size:
        raise ValueError('The payload of this step takes {0} bytes, the decoder holds {1} per step '
                         '(RegionDecoder(payload_capacity_bytes=...)).'.format(payload_bytes, min(capacity, payload.size)))
    views = region_head_views(head, batch_size, n_slots, truncated_unary_length, nb_maps)
    # every range is read before anything is written: a truncated file refuses the step too
    pieces = []                                          # (run-order slot, chunk)
    crop_slots = []
    for (k, (source, image, _, placed)) in enumerate(steps):
        chunks = source.read([(image, t) for (t, _, _, _) in placed])
        runs = [layout['class_first'][cls] + k*layout['class_slots'][cls] + s for (_, (cls, s), _, _) in placed]
        for (run, chunk, (t, _, _, _)) in zip(runs, chunks, placed):
            if len(chunk) != source.sizes[image, t]:
                raise ValueError('A payload range does not match the bit counts of the header.')
            pieces.append((run, chunk))
        crop_slots.append(runs)
    bits = views['bits'].reshape(n_slots, nb_maps, 2)
    prob_row = views['prob_row'].reshape(n_slots, nb_maps)
    bits[:] = 0
    prob_row[:] = -1
    views['placement'][:] = (-1, 0, 0, 0)
    views['crop_origin'][:] = 0
    for (k, ((source, image, origin, placed), runs)) in enumerate(zip(steps, crop_slots)):
        for (run, (t, _, row, col)) in zip(runs, placed):
            bits[run] = source.bits[image, t]
            prob_row[run] = source.prob_row + k*(nb_maps + 1)
            views['placement'][run] = (k, row, col, 0)
        views['crop_origin'][k] = origin
        views['bin_widths'][k] = source.header['bin_widths']
        views['map_mean'][k] = source.header['map_mean']
        views['table'][k] = source.table[image]
    n = len(steps)
    views['bin_widths'][n:] = 0.
    views['map_mean'][n:] = 0.
    views['table'][n:] = 0.5
    views['payload_bytes'][0] = payload_bytes
    pos = 0
    for (_, chunk) in sorted(pieces, key=lambda piece: piece[0]):
        payload[pos:pos + len(chunk)] = numpy.frombuffer(chunk, dtype=numpy.uint8)
        pos += len(chunk)
    return n, payload_bytes, crop_slots


class _KeepNeedsDeviceCrops(ValueError, TypeError):
    """`RegionDecoder(keep_reconstruction=True)` with the crops fetched to the host: a ValueError. Until `RegionDecoder` took the
    keyword, passing it at all was a TypeError, and whoever caught that still does."""


class RegionDecoder(BatchDecoder):
    """(RegionSource, image, y0, x0) requests -> uint8 crops of one fixed size, resident and pipelined: what
    `container.decode_region(source, decoder, (y0, x0, rh, rw), images=[image])[0]` computes (same bytes), with `BatchDecoder`'s
    machinery -- slots made once, the host work of a step in `plan_region_step`, the step as one chain of launches on one of
    `nb_streams` private streams, one hipGraph per slot with `use_graphs` -- around a step whose SHAPE is static (`region_layout`)
    while its PLACEMENT changes with every step and reaches the kernels through device memory. DESIGN.md section 17.
    `submit(requests)` takes 1..batch_size requests (RegionSource, image, y0, x0), the sources the same or not -> DecodeTicket, whose
    `result()` is uint8 (n, rh, rw), crop k the pixels [y0, y0 + rh) x [x0, x0 + rw) of its image, valid until the slot comes round
    again. Everything is checked on the host first (`plan_region_step`: ValueError, nothing written, nothing launched)."""

    def __init__(self, variables, are_bin_widths_learned, batch_size, h_in, w_in, truncated_unary_length, coding_tile, region,
                 device='cuda', nb_in_flight=None, nb_streams=None, use_graphs=False, payload_capacity_bytes=None, fetch_reconstruction=True,
                 pad=False, keep_reconstruction=False):
        """h_in, w_in: the size of the SOURCE images, fixed for the decoder's lifetime like `coding_tile` = (th, tw) latents
        (clamped to the latent plane) and region = (rh, rw) pixels, the size of every crop. Only the window around a crop is
        synthesised (`region_window`: the region's latents and the decoder's halo), so the source may be larger than the untiled
        synthesis takes; the window must not be. At most 65,535 slots per step (`batch_size` times `region_layout`'s slots per crop).
        payload_capacity_bytes: payload bytes a step may hold (rounded up to 16); None: 16 bits per symbol of the step's slots.
        fetch_reconstruction: the crops reach pinned host memory inside the step and `result()` is a numpy view of them; False:
        `result()` is a view of the slot's device tensor. The other arguments as `BatchDecoder`'s.
        pad: h_in x w_in is the REAL size of the source images, any positive integers (DESIGN.md sections 25, 28): the layout is that
        of the coded size, both sides rounded up to multiples of 16, and the real image is the top-left of the coded plane, so the
        window and the placement of a crop are what they are without `pad`. The sources are `RegionSource(..., pad=True)` of exactly
        that real size, a region lies inside the REAL image, and `result()` is `container.decode_region`'s of the padded container.
        False: a source whose `crop` byte is not 0 is refused.
        keep_reconstruction: every ticket gets, at submit time, `decoded_event`, recorded on the slot's stream behind the step, and
        `reconstruction_uint8`, the slot's crops on the device as (n, rh, rw), valid until the slot comes round again: another stream
        waits for the event and reads them there (`ColourRegionDecoder`). The crops must then stay on the device:
        `fetch_reconstruction=True` with it is refused (ValueError; the error is a TypeError as well, which passing this keyword was
        before `RegionDecoder` took it)."""
        (self.pad, self.image_size) = (bool(pad), None)
        if keep_reconstruction and fetch_reconstruction:
            raise _KeepNeedsDeviceCrops('`keep_reconstruction` keeps the crops on the device for another stream: it needs '
                                        '`fetch_reconstruction=False`.')
        if self.pad:
            self.image_size = (container_format._positive_int(h_in, '`h_in`'), container_format._positive_int(w_in, '`w_in`'))
            region = container_format._positive_pair(region, '`region`')
            if region[0] > self.image_size[0] or region[1] > self.image_size[1]:
                raise ValueError('`region` = {0} is larger than the {1} x {2} images.'.format(region, self.image_size[0], self.image_size[1]))
            (h_in, w_in) = container_format.coded_size(*self.image_size)
        self._lay_out(batch_size, h_in, w_in, truncated_unary_length, payload_capacity_bytes, coding_tile, region)
        self._build(variables, are_bin_widths_learned, device, nb_in_flight, nb_streams, use_graphs, fetch_reconstruction, keep_reconstruction)

    def _lay_out(self, batch_size, h_in, w_in, truncated_unary_length, payload_capacity_bytes, coding_tile, region):
        coding_tile = _refuse_shape(batch_size, h_in, w_in, truncated_unary_length, coding_tile)
        region = container_format._positive_pair(region, '`region`')
        if region[0] > h_in or region[1] > w_in:
            raise ValueError('`region` = {0} is larger than the {1} x {2} images.'.format(region, h_in, w_in))
        (h_map, w_map) = (h_in//csts.STRIDE_PROD, w_in//csts.STRIDE_PROD)
        (Rs, Cs) = region_window(h_map, w_map, region)
        if 16*Rs*Cs*512 > 0x7FFFFFFF:
            raise ValueError('`region` = {0} needs a window of {1} x {2} latents, more than the untiled synthesis takes.'.format(region, Rs, Cs))
        layout = region_layout(int(batch_size), h_map, w_map, coding_tile, Rs, Cs)
        if layout['n_slots'] > 65535:
            raise ValueError('`batch_size` crops of {0} slots each are more than the 65535 slots a step can hold.'.format(layout['slots_per_crop']))
        (self.coding_tile, self.region, self.window) = (layout['coding_tile'], region, (Rs, Cs))
        # everything a step needs beyond its requests is the same for every step: made once, shared by the slots
        self._layout = layout
        (self._n_streams, self._runs, self._elements) = (layout['n_streams'], layout['runs'], layout['elements'])
        self._payload_order = None                    # the payload of a step lies in run order
        self._index_images = 1                        # every slot is an entry of one "image"
        self._head_fields = _region_head_fields(int(batch_size), layout['n_slots'], int(truncated_unary_length))
        # what the worker scans (`_DecodeJob.detail`): the streams of every run-order slot, picked per step by the crops' placement
        self._slot_ranges = [(k*csts.NB_MAPS_3, (k + 1)*csts.NB_MAPS_3) for k in range(layout['n_slots'])]
        self._set_sizes(batch_size, h_in, w_in, truncated_unary_length, payload_capacity_bytes, 2*layout['elements'])

    def _upload_tables(self):
        layout = self._layout
        self._slots_host = layout['slots']
        self._slots_device = torch.from_numpy(layout['slots']).to(self.device)
        # `device.coder_index_tiles`: the payload is in run order, so every slot is its own entry, clamped to half its class's stride
        half_stride = numpy.concatenate([numpy.full(count, dev.coder_stream_stride_bytes(rows*cols, self.truncated_unary_length)//2, dtype=numpy.int64)
                                         for ((rows, cols), count, _, _) in layout['runs']])
        self._entry_table = torch.from_numpy(numpy.stack([numpy.arange(layout['n_slots'], dtype=numpy.int64), half_stride], axis=1)).to(self.device)

    def _plan_step(self, slot, requests):
        """As `BatchDecoder._plan_step`; a crop's streams are those of its tiles' slots, its tiles in row-major order as
        `container.decode_region` meets them, the maps of a tile in order."""
        (crops, payload_bytes, crop_slots) = plan_region_step(requests, self._layout, slot.head_host, slot.payload_host, self.payload_capacity_bytes,
                                                              self.region, self.truncated_unary_length, self.learned, self.nb_maps,
                                                              self.image_size)
        ranges = self._slot_ranges
        return crops, payload_bytes, [[ranges[run] for run in runs] for runs in crop_slots]

    def _kept(self, slot, nb_images):
        return slot.value(nb_images)          # the crops on the device: `keep_reconstruction` came with `fetch_reconstruction=False`

    def _launch_latents(self, slot):
        lane = slot.lane
        # every slot is an entry of one "image": the offsets of its pieces in the payload, which lies in run order
        dev.coder_index_tiles(lane.results[0], lane.results[1], self._entry_table, self.nb_maps, self._layout['n_slots'],
                              self.payload_capacity_bytes, offsets=lane.offsets, index=lane.index)
        self._launch_classes(lane)
        # the placed tiles cover every latent of a present crop's window exactly once
        dev.tile_symbols_dequantize_placed(lane.decoded, self._slots_device, self._slots_host, lane.placement, lane.bin_widths, lane.map_mean,
                                           lane.shifted)

    def _launch_output(self, slot):
        (rh, rw) = self.region
        dev.publish_crops(slot.planes, slot.lane.crop_origin, slot.pinned_crops if slot.pinned_crops is not None else slot.crops, rh, rw)


# ---- a rate point per image, chosen on the device to a byte budget -----------------------------------------

class BudgetTicket(Ticket):
    """Handle on one submitted `BudgetCodec` step: `result()` also says where every image landed; `image_containers()` gives every
    image's blob at its own rate point."""

    def container(self):
        """Always raises: one `EAE1` blob holds one rate point, the images of a step each have their own."""
        raise RuntimeError('a BudgetCodec step has one rate point per image and one EAE1 blob holds one: use `image_containers()`')

    def image_containers(self):
        """Blocks like `result()`; one single-image `EAE1` blob per image (`EAT1` from a `TiledBudgetCodec`), byte for byte what
        `container.encode_images` writes for that image at the point `result()['rate_point']` names. Raises `ContainerOverflow` like
        `Ticket.container()`."""
        parts = self._parts()
        (learned, _, height, width, exception, ladder) = parts['head']
        (bits, rows, view) = (parts['bits'], parts['rows'], memoryview(parts['payload']))
        nb_maps = ladder.bin_widths_points.shape[1]
        per_image = bits.shape[0]//self.nb_images            # nb_maps, times the tiles of an image with a coding tile (payload order)
        image_bytes = container_format._entry_bytes(bits.reshape(self.nb_images, per_image//nb_maps, nb_maps, 2)).sum(axis=1)
        stops = numpy.cumsum(image_bytes)
        blobs = []
        for (i, k) in enumerate(parts['rate_point'].tolist()):
            blobs.append(container_format.assemble_blob(learned, 1, height, width, exception, ladder.bin_widths_points[k], ladder.map_mean,
                                                        ladder.binary_probabilities_points[k], rows[i:i + 1] if exception >= 0 else rows[:0],
                                                        bits[i*per_image:(i + 1)*per_image], view[int(stops[i] - image_bytes[i]):int(stops[i])],
                                                        coding_tile=parts['coding_tile'], image_size=parts.get('image_size'))[0])
        return blobs


def _staged_block(batch_size, device):
    """One int64 per image that `_stage` writes into pinned memory and a kernel inside the step's chain fetches -> (the pinned block,
    its numpy view, the device's copy, the block's size in bytes on the device, as `device.fetch_prefix` takes it)."""
    padded = batch_size + batch_size % 2                       # `device.fetch_prefix` copies multiples of 16 bytes
    pinned = torch.zeros(padded, dtype=torch.int64).pin_memory()
    return (pinned, pinned.numpy(), torch.zeros(padded, dtype=torch.int64, device=device),
            torch.full((1,), 8*padded, dtype=torch.int64, device=device))


class _BudgetSlot(object):
    """What one `BudgetCodec` step in flight owns beyond its `_Slot`, and the base of what the other rate-control codecs' steps own:
    the ladder's accumulators, the step's budgets, the choice and the coder's table, on the device and in pinned memory. Made once;
    tests/budget_slot_buffers.py says what a step may find in every attribute when it starts."""
    __slots__ = ('accum', 'hist', 'bypass_bits', 'range_errors', 'pinned_budgets', 'budgets_host', 'budgets', 'budgets_nbytes', 'select',
                 'upper', 'point', 'flags', 'prob_row', 'pinned_select', 'select_host', 'table', 'points_table', 'exception_rows',
                 'pinned_rows', 'rows_host')

    def __init__(self, codec, extra_words=0):
        """extra_words: 32-bit words behind `flags` in `select` and `pinned_select`, on an 8-byte boundary, for what a subclass
        publishes together with the selection."""
        (batch_size, nb_maps, device, ladder) = (codec.batch_size, codec.nb_maps, codec.device, codec.ladder)
        (nb_points, length) = (ladder.nb_points, ladder.truncated_unary_length)
        (counts_shape, rows_shape) = self._shapes(codec)
        # the ladder's accumulators, zeroed by one launch at the head of every step: [bypass bits int64 | histograms int32 | range
        # errors int32]
        nb_bits = int(numpy.prod(counts_shape))
        nb_bins = nb_bits*(length + 1)
        self.accum = torch.zeros(2*nb_bits + nb_bins + nb_points, dtype=torch.int32, device=device)
        (bypass_bits, hist, self.range_errors) = torch.split(self.accum, [2*nb_bits, nb_bins, nb_points])
        self.bypass_bits = bypass_bits.view(torch.int64).view(counts_shape)
        self.hist = hist.view(counts_shape + (length + 1,))
        # the step's budgets (`BudgetCodec._stage`)
        (self.pinned_budgets, self.budgets_host, self.budgets, self.budgets_nbytes) = _staged_block(batch_size, device)
        # what the selection leaves for the host: [upper int64 N x K | point int32 N | flags int32 N | the subclass's words]
        layout = [2*batch_size*nb_points, batch_size, batch_size, extra_words]
        self.select = torch.zeros(sum(layout), dtype=torch.int32, device=device)
        (upper, self.point, self.flags, _) = torch.split(self.select, layout)
        self.upper = upper.view(torch.int64).view(batch_size, nb_points)
        self.pinned_select = torch.zeros(sum(layout), dtype=torch.int32).pin_memory()
        (upper, point, flags, _) = torch.split(self.pinned_select, layout)
        # what the result worker reads (`_BudgetWorker._finish`)
        self.select_host = (upper.view(torch.int64).view(batch_size, nb_points).numpy(), point.numpy(), flags.numpy())
        # the coder's table: [the K x 128 rows of the ladder | one row per image for its exception map]
        self.table = torch.zeros((nb_points*nb_maps + batch_size, length), dtype=torch.float64, device=device)
        (self.points_table, self.exception_rows) = (self.table[:nb_points*nb_maps], self.table[nb_points*nb_maps:])
        self.points_table.copy_(torch.from_numpy(ladder.binary_probabilities_points.reshape(nb_points*nb_maps, length)))
        self.pinned_rows = torch.zeros((batch_size, length), dtype=torch.float64).pin_memory()
        self.rows_host = self.pinned_rows.numpy()
        # the coder's row of every stream of the step, chosen by `device.ladder_select` or `device.ladder_select_tiles`
        self.prob_row = torch.zeros(rows_shape, dtype=torch.int32, device=device)

    @staticmethod
    def _shapes(codec):
        """(the shape of the ladder's counts, the shape of `prob_row`): here one count and one row per (image, [point,] map)."""
        return ((codec.batch_size, codec.ladder.nb_points, codec.nb_maps), (codec.batch_size, codec.nb_maps))

    @property
    def selected(self):
        """The block `device.ladder_select` writes every image's point into."""
        return self.point


class _BudgetHead(object):
    """The first element of a `BudgetCodec` slot's `emit_host` (what `_Worker.process` keeps as the container's 'head'): the fixed
    parts of the step's blobs and the host views of the slot's `_BudgetSlot`."""
    __slots__ = ('fixed', 'budget_slot', 'header_bytes')

    def __init__(self, fixed, budget_slot, header_bytes):
        (self.fixed, self.budget_slot, self.header_bytes) = (fixed, budget_slot, header_bytes)


class _BudgetWorker(_Worker):
    """The result worker of `BudgetCodec`."""

    def _finish(self, job):
        """The step's choice out of the slot's pinned blocks into the ticket, while the slot is still the step's."""
        (ticket, head) = (job.ticket, job.emit[0])
        (upper, point, flags) = head.budget_slot.select_host
        n = ticket.nb_images
        budgets = head.budget_slot.budgets_host[:n].copy()
        rate_point = point[:n].astype(numpy.int64)
        blob_bytes = head.header_bytes + ticket._values['container_bytes']
        ticket._values.update({'rate_point': rate_point, 'upper_bound_bytes': upper[:n].copy(), 'budget_bytes': budgets,
                               'blob_bytes': blob_bytes, 'promised': (flags[:n] & 1) != 0, 'fits': blob_bytes <= budgets})
        parts = ticket._container_parts
        parts['head'] = head.fixed
        parts['rate_point'] = rate_point
        if self.idx_map_exception >= 0:
            parts['rows'] = head.budget_slot.rows_host.copy()


class BudgetCodec(BatchCodec):
    """`BatchCodec` with a rate point per image, chosen inside the step, on the device, so that the image's blob fits a byte budget
    (DESIGN.md section 19): "N bytes per image" as a property of a step of the resident codec."""
    (_ticket_class, _worker_class) = (BudgetTicket, _BudgetWorker)
    # what the subclasses flip: whether `coding_tile` is taken (and in what words it is refused), and the class of the per-step state
    # beyond `_Slot`
    (_takes_coding_tile, _budget_slot_class) = (False, _BudgetSlot)
    # `pad` stays refused by every public rate-control codec; `_PlaneBudgetCodec`, a plane of a colour
    # picture inside `ColourBudgetCodec`, flips this
    _takes_pad = False
    _no_coding_tile = '`BudgetCodec` does not take `coding_tile`: the bounds are those of whole maps (EAE1).'

    def __init__(self, variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, budget_bytes=None, **batch_codec_options):
        """ladder: a `ratecontrol.RateLadder`, finest point first, of at most `device.ladder_max_points(L)` points. A ladder with a
        price (`RateLadder(..., rdo_lambda=...)`) makes the step count, bound, probe and code the symbols of the
        rate-distortion optimised quantiser: `Ticket.image_containers()[i]` is then `container.encode_images(..., rdo_lambda=
        ladder.rdo_lambdas[k])` at the image's point k, everything else reads the same. The keyword `rdo_lambda` itself is refused:
        the price belongs to the ladder. budget_bytes: the
        budget of a `submit` that names none (a scalar or one value per image). batch_codec_options: `BatchCodec`'s keyword arguments
        (device, nb_in_flight, keep_reconstruction, use_graphs, nb_transform_streams, one_stream_steps, hist_radius,
        container_capacity_bytes, ...); `emit_container` is always on; `coding_tile`, `fuse_latent`, a coder other than 'device' and
        `coder_chunks` > 1 are refused.
        Per image, in ladder order, the step takes the first point whose symbols fit int16 and whose UPPER BOUND on the size of the
        image's single-image EAE1 blob (ratecontrol.upper_bounds_fixed) is within the budget; if none is, the last valid point.
        `Ticket.result()` gains 'rate_point' int64 (N,), 'upper_bound_bytes' int64 (N, K), 'budget_bytes' int64 (N,), 'blob_bytes'
        int64 (N,) (the length of the image's blob), 'promised' bool (N,) (the bound of the point taken was within the budget) and
        'fits' bool (N,) (blob_bytes <= budget); 'nb_bits', 'coder_bits', 'exception_bits', 'sse', 'nb_deads' and 'container_bytes'
        are those of the image's own point. `Ticket.image_containers()[i]` is byte for byte `container.encode_images` of image i at
        its point; `Ticket.container()` raises. An image without a valid point fails the step's range check as in `BatchCodec`."""
        from . import ratecontrol
        if not isinstance(ladder, ratecontrol.RateLadder):
            raise TypeError('`ladder` is not a `ratecontrol.RateLadder`.')
        # refused in front of every allocation
        options = dict(batch_codec_options)
        if not options.pop('emit_container', True):
            raise ValueError('`BudgetCodec` always emits containers: the budget is that of the image\'s blob.')
        if options.get('coding_tile') is not None and not self._takes_coding_tile:
            raise ValueError(self._no_coding_tile)
        if options.get('fuse_latent'):
            raise ValueError('`BudgetCodec` does not take `fuse_latent`: the point is chosen between conv_3 and the quantiser.')
        if options.get('rdo_lambda') is not None:
            raise ValueError('The rate-control codecs do not take `rdo_lambda`: the price of a bit comes with the ladder '
                             '(`ratecontrol.RateLadder(..., rdo_lambda=...)`), a point at a time.')
        if options.get('pad') and not self._takes_pad:
            raise ValueError('The rate-control codecs do not take `pad`: their bounds and probes are over the coded plane, and a PSNR floor '
                             'would need the real pixel count (DESIGN.md section 25). `BatchCodec(..., pad=True)` pads.')
        if options.get('coder', 'device') != 'device':
            raise ValueError('`BudgetCodec` needs the coder on the device.')
        chunks = options.get('coder_chunks')
        if int(default_coder_chunks(batch_size*csts.NB_MAPS_3) if chunks is None else chunks) > 1:
            raise ValueError('`BudgetCodec` does not go with `coder_chunks` > 1.')
        for name in ('bin_widths_test', 'map_mean', 'binary_probabilities', 'idx_map_exception'):
            if name in options:
                raise TypeError('`{0}` comes with the ladder.'.format(name))
        length = ladder.truncated_unary_length
        if ladder.nb_points > dev.ladder_max_points(length):
            raise ValueError('The ladder has {0} points, one pass takes {1} at a truncated unary length of {2} '
                             '(`device.ladder_max_points`).'.format(ladder.nb_points, dev.ladder_max_points(length), length))
        self.ladder = ladder
        self._default_budgets = None if budget_bytes is None else self._budgets_of(budget_bytes, batch_size)
        # (the base class's own rate point, which no launch of this class reads, is the ladder's first)
        super(BudgetCodec, self).__init__(variables, are_bin_widths_learned, ladder.bin_widths_points[0], ladder.map_mean,
                                          ladder.binary_probabilities_points[0], ladder.idx_map_exception, batch_size, h_in, w_in,
                                          emit_container=True, **options)
        try:
            to_device = lambda array: torch.from_numpy(numpy.ascontiguousarray(array)).to(self.device)
            # (the coded size, not the arguments: with `pad`, which only `_takes_pad` lets through, they are the real size)
            self._header_bytes = ratecontrol.header_bytes(ladder, self.h_in, self.w_in, self.coding_tile)
            if self._tile_layout is not None:
                # `device.ladder_select_tiles`: the image of every (image, tile) entry in the run order the coder takes them in
                tiled = self._tile_layout
                self._entry_image = to_device(numpy.array([tiled['entries'][p][0] for p in tiled['payload_entry'].tolist()], dtype=numpy.int32))
            self._bin_widths_points = to_device(ladder.bin_widths_points)
            # a ladder with a price (`RateLadder(rdo_lambda=...)`): the thresholds of its points in the
            # quantiser's layout [K, 128, 16] and in the count's [K, 16, 128]; None: every launch is that of nearest rounding
            self._rdo_thresholds_points = self._rdo_by_magnitude = None
            if ladder.rdo_thresholds_points is not None:
                self._rdo_thresholds_points = to_device(ladder.rdo_thresholds_points)
                self._rdo_by_magnitude = dev.rdo_thresholds_by_magnitude(self._rdo_thresholds_points)
            # (32-bit words: torch has no arithmetic on uint32, and none is asked of it)
            self._fixed_costs = to_device(ratecontrol.fixed_costs(ladder).view(numpy.int32))
            self._log2_tables = to_device(ratecontrol.log2_tables(self.map_size).view(numpy.int32)) if self.idx_map_exception >= 0 else None
            self._budget_slots = {}
            fixed = (bool(are_bin_widths_learned), 1, self.h_in, self.w_in, self.idx_map_exception, ladder)
            for slot in self._slots:
                budget_slot = self._budget_slot_class(self)
                self._budget_slots[id(slot)] = budget_slot
                slot.emit_host = (_BudgetHead(fixed, budget_slot, self._header_bytes),) + slot.emit_host[1:]
            self._staged = None
        except BaseException:
            self.close()
            raise

    @staticmethod
    def _budgets_of(budget_bytes, batch_size):
        budgets = numpy.asarray(budget_bytes)
        if budgets.dtype.kind not in 'iu' or budgets.ndim > 1 or (budgets.ndim == 1 and budgets.shape[0] != batch_size):
            raise ValueError('`budget_bytes` must be an integer or one integer per image.')
        return numpy.ascontiguousarray(numpy.broadcast_to(budgets.astype(numpy.int64), (batch_size,)))

    def submit(self, luminances_uint8, budget_bytes=None):
        """`BatchCodec.submit` with the step's budgets: a scalar or one value per image, bytes of the image's whole blob (header
        included); None: the constructor's `budget_bytes`."""
        budgets = self._budgets_for(budget_bytes)
        if budgets is None:
            raise ValueError('no `budget_bytes`, and the codec was built without a default.')
        return self._submit_staged(luminances_uint8, (budgets,))

    def _budgets_for(self, budget_bytes):
        """The budgets of a step as int64 (batch_size,): those it names, else the constructor's; None when there are none."""
        return self._default_budgets if budget_bytes is None else self._budgets_of(budget_bytes, self.batch_size)

    def _submit_staged(self, luminances_uint8, staged):
        """`BatchCodec.submit` of a step whose `_stage` finds `staged`, one int64 (batch_size,) per pinned block it fills."""
        self._staged = staged
        try:
            return super(BudgetCodec, self).submit(luminances_uint8)
        finally:
            self._staged = None

    def _stage(self, slot):
        """The step's budgets into the slot's pinned block (the slot is this step's: `_submit` has claimed it)."""
        self._budget_slots[id(slot)].budgets_host[:self.batch_size] = self._staged[0]

    def _launch_step(self, luminances_uint8, slot, index, ticket, coded):
        self._stage(slot)
        return super(BudgetCodec, self)._launch_step(luminances_uint8, slot, index, ticket, coded)

    def _replay_step(self, luminances_uint8, slot, index, ticket, coded):
        self._stage(slot)
        return super(BudgetCodec, self)._replay_step(luminances_uint8, slot, index, ticket, coded)

    def _launch_analysis(self, luminances_uint8, slot, hook):
        """conv1+GDN1 -> conv2+GDN2 -> conv3 -> gdn_3 -> the ladder's histograms -> the step's budgets -> the point of every image
        -> the quantiser with every image's own bin widths (+ inverse_gdn_4) -> exception-map histograms, on the current stream.
        Everything that varies from step to step travels through device memory: no argument of any launch depends on it."""
        budget = self._budget_slots[id(slot)]
        y = self._launch_selection(luminances_uint8, slot, budget, hook)
        return self._launch_quantiser(y, slot, budget, hook)

    def _launch_selection(self, luminances_uint8, slot, budget, hook):
        """`_launch_analysis` up to the point of every image; returns the latents the quantiser sees."""
        enc = self.encoder
        v = enc.v
        budget.accum.zero_()                             # the ladder's accumulators: the head of the step
        gdn_1 = hook('conv1_gdn1', lambda: dev.conv9x9s4_u8(luminances_uint8, enc.w1, v['encoder/biases_1'], enc.g[1], v['encoder/beta_1']))
        ws = slot.conv_ws
        gdn_2 = hook('conv2_gdn2', lambda: dev.conv5x5s2(gdn_1, enc.w2, v['encoder/biases_2'], dev.NORM_GDN, enc.g[2], v['encoder/beta_2'], workspace=ws))
        y = hook('conv3', lambda: dev.conv5x5s2(gdn_2, enc.w3, v['encoder/biases_3'], dev.NORM_NONE, workspace=ws))
        if not self.learned:
            y = hook('gdn3', lambda: dev.gdn(y, enc.g[3], v['encoder/beta_3']))
        hook('ladder', lambda: self._launch_ladder(y, budget))
        self._launch_budgets(budget)
        hook('select', lambda: self._launch_select(budget))
        return y

    def _launch_budgets(self, budget):
        """The step's budgets out of the slot's pinned block into its device block, in front of the selection."""
        dev.fetch_prefix(budget.pinned_budgets, budget.budgets, budget.budgets_nbytes)

    def _launch_quantiser(self, y, slot, budget, hook):
        """`_launch_analysis` from the quantiser on, at `budget.point`; returns the synthesis transform's input."""
        d = self.decoder.v
        igdn_out = None if self.learned else (self.decoder.g[4], d['decoder/beta_4'])
        outputs = dict(igdn_out=igdn_out, want_shifted=self.learned, want_symbols=True, want_flags=True, out_symbols=slot.symbols,
                       out_flags=slot.flags, out_checks=slot.checks[:3])
        q = hook('latent', lambda: self._quantise_at(y, budget.point, **outputs))
        if self.idx_map_exception >= 0:
            dev.symbol_histograms(slot.symbols_2d, self.hist_radius, out=(slot.hist, slot.overflow),
                                  first_map=self.idx_map_exception, map_step=self.nb_maps, zero=False)
        if self._early_publish:
            first = 4*self._n_streams
            dev.publish_to_host(slot.out[first:], slot.pinned_out[first:])
        return q['shifted'] if self.learned else q['t']

    def _quantise_at(self, y, point, **outputs):
        """The quantiser with every image's own row (`point` int32 [N] on the device): `device.latent_quantize_rows`, or for a ladder
        with a price `device.latent_quantize_rdo` with the thresholds of the same row."""
        if self._rdo_thresholds_points is None:
            return dev.latent_quantize_rows(y, self._bin_widths_points, point, self.map_mean, **outputs)
        return dev.latent_quantize_rdo(y, self._bin_widths_points, self._rdo_thresholds_points, point, self.truncated_unary_length,
                                       self.map_mean, **outputs)

    def _launch_ladder(self, y, budget):
        out = (budget.hist, budget.bypass_bits, budget.range_errors)
        if self._rdo_thresholds_points is None:
            dev.ladder_histograms(y, self._bin_widths_points, self.map_mean, self.truncated_unary_length, out=out)
        else:                                            # the symbols counted are the symbols `_quantise_at` writes
            dev.ladder_histograms_rdo(y, self._bin_widths_points, self._rdo_thresholds_points, self.map_mean, self.truncated_unary_length,
                                      out=out, by_magnitude=self._rdo_by_magnitude)

    def _launch_select(self, budget):
        dev.ladder_select(budget.hist, budget.bypass_bits, self._fixed_costs, self._log2_tables, self.idx_map_exception, self._header_bytes,
                          self.map_size, budget.budgets[:self.batch_size], self.ladder.nb_points*self.nb_maps,
                          out={'point': budget.selected, 'prob_row': budget.prob_row, 'upper': budget.upper, 'flags': budget.flags})

    def _coder_table(self, slot):
        """The table of every point's rows, the rows `ladder_select` chose and the table's own exception rows."""
        budget = self._budget_slots[id(slot)]
        return (budget.table, budget.prob_row.view(-1), budget.exception_rows)

    def _publish_coder_side(self, slot):
        """`BatchCodec._publish_coder_side` with the choice, and with an exception map its rows, beside the payload and the index."""
        budget = self._budget_slots[id(slot)]
        rows = ((budget.exception_rows, budget.pinned_rows),) if self.idx_map_exception >= 0 else ()
        super(BudgetCodec, self)._publish_coder_side(slot, ((budget.select, budget.pinned_select),) + rows)


class _PlaneBudgetCodec(BudgetCodec):
    """`BudgetCodec` as one plane of a colour picture inside `ColourBudgetCodec`; private: the public
    rate-control codecs go on refusing `pad`. Two things are its own.
    `pad=True` is taken: h_in x w_in is the plane's REAL size, the step runs at the coded size as `BatchCodec(pad=True)` runs it, the
    bounds, the header and the blobs are those of the coded plane with the real size in the `crop` byte -- `container.encode_images(...,
    pad=True)` at the image's point, byte for byte -- and 'sse' is over the real pixels.
    budgets_on_device=True: `submit(images, budget_bytes)` also takes an int64 device tensor (batch_size,) that was written earlier
    on the caller's stream. The step copies it into its slot's `budgets` block on the step's own stream, behind that stream's wait for
    the caller's and in front of the selection, launches no `fetch_prefix` of budgets, and publishes `budgets` into the slot's
    `pinned_budgets` together with the selection: 'budget_bytes' of `result()` is what the device used. A host array or a scalar goes
    the same way, through the slot's pinned block. The slot's `budgets` block is free then: `_submit` has waited for the slot, so the
    step that used it last has published its counters, behind its selection."""
    _takes_pad = True

    def __init__(self, variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, budget_bytes=None, budgets_on_device=False,
                 **batch_codec_options):
        self.budgets_on_device = bool(budgets_on_device)
        super(_PlaneBudgetCodec, self).__init__(variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, budget_bytes,
                                                **batch_codec_options)

    def _budgets_for(self, budget_bytes):
        if not isinstance(budget_bytes, torch.Tensor):
            return super(_PlaneBudgetCodec, self)._budgets_for(budget_bytes)
        if not self.budgets_on_device:
            raise ValueError('`budget_bytes` as a tensor needs `budgets_on_device=True`.')
        if budget_bytes.dtype != torch.int64 or tuple(budget_bytes.shape) != (self.batch_size,) or not budget_bytes.is_contiguous() \
                or budget_bytes.device != self.device:
            raise ValueError('`budget_bytes` as a tensor must be int64 (batch_size,), contiguous, on the codec\'s device.')
        return budget_bytes

    def _stage(self, slot):
        """With `budgets_on_device`: the step's budgets into the slot's DEVICE block, on the current stream (the step's own)."""
        if not self.budgets_on_device:
            return super(_PlaneBudgetCodec, self)._stage(slot)
        (budget, staged, n) = (self._budget_slots[id(slot)], self._staged[0], self.batch_size)
        if isinstance(staged, torch.Tensor):
            budget.budgets[:n].copy_(staged, non_blocking=True)
            staged.record_stream(torch.cuda.current_stream())
        else:
            budget.budgets_host[:n] = staged
            budget.budgets[:n].copy_(budget.pinned_budgets[:n], non_blocking=True)

    def _replay_step(self, luminances_uint8, slot, index, ticket, coded):
        if not self.budgets_on_device:
            return super(_PlaneBudgetCodec, self)._replay_step(luminances_uint8, slot, index, ticket, coded)
        # the stream `BatchCodec._replay_step` replays this step's graphs on: the budgets go there in front of them
        stream = self._transform_streams[index % len(self._transform_streams)]
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            self._stage(slot)
        return BatchCodec._replay_step(self, luminances_uint8, slot, index, ticket, coded)

    def _launch_budgets(self, budget):
        if not self.budgets_on_device:                   # (else `_stage` has put them there: nothing is launched, captured or eager)
            super(_PlaneBudgetCodec, self)._launch_budgets(budget)

    def _publish_coder_side(self, slot):
        if self.budgets_on_device:
            budget = self._budget_slots[id(slot)]
            dev.publish_to_host(budget.budgets, budget.pinned_budgets)
        super(_PlaneBudgetCodec, self)._publish_coder_side(slot)


# ---- the same for tile-indexed containers: counts, bounds and streams per coding tile ------------------------

class _TiledRows(object):
    """What makes a `_BudgetSlot` or a `_QualitySlot` the one of a codec with a coding tile (in front of it among the bases): the
    ladder's accumulators per coding tile and the coder's rows per stream of the step."""
    __slots__ = ()              # (`class_rows` is a slot of the two classes below: two bases that both add slots do not combine)

    def __init__(self, codec):
        super(_TiledRows, self).__init__(codec)
        # `prob_row` holds the rows in RUN order (`device.ladder_select_tiles`): every shape class's run of them
        self.class_rows = [self.prob_row[first:first + count*codec.nb_maps] for (_, count, first, _) in codec._tile_layout['runs']]

    @staticmethod
    def _shapes(codec):
        tiled = codec._tile_layout
        return ((codec.batch_size, codec.ladder.nb_points, tiled['nb_tiles'], codec.nb_maps), (tiled['n_streams'],))


class _TiledBudgetSlot(_TiledRows, _BudgetSlot):
    """What one `TiledBudgetCodec` step in flight owns beyond its `_Slot`: `_BudgetSlot`'s state with `_TiledRows`' shapes. Made once;
    tests/tiled_budget_slot_buffers.py says what a step may find in every attribute when it starts. The accumulators take
    N K T 128 (L + 1) 4 bytes per slot (and an eleventh of that for the bypass bits): 7.3 MB at 24 Kodak images, K = 9 and tiles of
    16, 29 MB at tiles of 8."""
    __slots__ = ('class_rows',)


class _TiledRateControl(object):
    """The tiled pieces of a rate-control step, in front of `BudgetCodec` or `QualityCodec` among the bases: the counts and the
    bounds per coding tile, and the coder's rows per shape class."""
    _takes_coding_tile = True

    def _launch_ladder(self, y, budget):
        plane = y.view(self.batch_size, self.h_in//csts.STRIDE_PROD, self.w_in//csts.STRIDE_PROD, self.nb_maps)
        out = (budget.hist, budget.bypass_bits, budget.range_errors)
        if self._rdo_thresholds_points is None:
            dev.ladder_histograms_tiles(plane, self._bin_widths_points, self.coding_tile, self.map_mean, self.truncated_unary_length, out=out)
        else:
            dev.ladder_histograms_rdo_tiles(plane, self._bin_widths_points, self._rdo_thresholds_points, self.coding_tile, self.map_mean,
                                            self.truncated_unary_length, out=out, by_magnitude=self._rdo_by_magnitude)

    def _launch_select(self, budget):
        dev.ladder_select_tiles(budget.hist, budget.bypass_bits, self._fixed_costs, self._log2_tables, self.idx_map_exception,
                                self._header_bytes, self.map_size, budget.budgets[:self.batch_size], self._entry_image,
                                self.ladder.nb_points*self.nb_maps,
                                out={'point': budget.selected, 'prob_row': budget.prob_row, 'upper': budget.upper, 'flags': budget.flags})

    def _coder_table(self, slot):
        """The table of every point's rows, every shape class's run of the rows `ladder_select_tiles` chose and the table's own
        exception rows."""
        budget = self._budget_slots[id(slot)]
        return (budget.table, budget.class_rows, budget.exception_rows)


class TiledBudgetCodec(_TiledRateControl, BudgetCodec):
    """`BudgetCodec` for tile-indexed containers: a byte budget per image whose blob is the single-image `EAT1`
    blob `container.encode_images(..., coding_tile=coding_tile)` writes, so that crops come out of it (`container.decode_region`,
    `RegionDecoder`) and its serial chains are a tile long."""
    _budget_slot_class = _TiledBudgetSlot

    def __init__(self, variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, coding_tile, budget_bytes=None, **batch_codec_options):
        """coding_tile: (th, tw) in latents, clamped to the latent plane, as `BatchCodec(coding_tile=...)` takes it; everything else
        as `BudgetCodec`. Refused in front of every allocation: `fuse_latent`, a coder other than 'device', `coder_chunks` > 1, a
        ladder longer than `device.ladder_max_points(L)`, and `batch_size` times the tiles of an image beyond 65535.
        The step counts per (image, point, tile, map) (`device.ladder_histograms_tiles`), bounds every image's `EAT1` blob at every
        point with every tile stream's own closing bits and byte padding (`device.ladder_select_tiles`:
        ratecontrol.upper_bounds_fixed_tiles) and codes the tiles with the rows of the image's point. `Ticket.result()` has
        `BudgetCodec`'s keys, 'coder_bits' summed over an image's tiles; `Ticket.image_containers()[i]` is byte for byte
        `container.encode_images(image i, ..., coding_tile=coding_tile)` at `rate_point[i]`; `Ticket.container()` raises."""
        coding_tile = container_format._positive_pair(coding_tile, '`coding_tile`')
        super(TiledBudgetCodec, self).__init__(variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, budget_bytes=budget_bytes,
                                               coding_tile=coding_tile, **batch_codec_options)


# ---- a PSNR floor per image, searched on the device ----------------------------------------------------------

class _QualitySlot(_BudgetSlot):
    """What one `QualityCodec` step in flight owns beyond its `_Slot`: `_BudgetSlot`'s state -- its `point` is called `first` here,
    the finest point the search may take --, the step's thresholds, the bisection's state and trace behind the selection in `select`
    (published with it), the accumulator and the latent buffer of the probes. Made once; tests/quality_slot_buffers.py says what a
    step may find in every attribute when it starts."""
    __slots__ = ('first', 'pinned_max_sse', 'max_sse_host', 'max_sse', 'max_sse_nbytes', 'trace_sse', 'met', 'state', 'trace_point',
                 'search_host', 'probe_acc', 'probe_latent')

    def __init__(self, codec):
        (batch_size, nb_rounds, device) = (codec.batch_size, codec.nb_rounds, codec.device)
        # behind [upper | first | flags]: [trace_sse int64 N x R | point int32 N | met int32 N | state int32 N x 2 | trace_point int32 N x R]
        search = [2*batch_size*nb_rounds, batch_size, batch_size, 2*batch_size, batch_size*nb_rounds]
        super(_QualitySlot, self).__init__(codec, extra_words=sum(search))
        own = self.select.numel() - sum(search)
        # what `device.ladder_select` writes keeps its place and gives its name to the search's own block: the point the step codes at
        self.first = self.point
        (trace_sse, self.point, self.met, state, trace_point) = torch.split(self.select[own:], search)
        self.trace_sse = trace_sse.view(torch.int64).view(batch_size, nb_rounds)
        self.state = state.view(batch_size, 2)
        self.trace_point = trace_point.view(batch_size, nb_rounds)
        (trace_sse, point, met, state, trace_point) = torch.split(self.pinned_select[own:], search)
        # what the result worker reads (`_QualityWorker._finish`): (point, met, trace_point, trace_sse)
        self.search_host = (point.numpy(), met.numpy(), trace_point.view(batch_size, nb_rounds).numpy(),
                            trace_sse.view(torch.int64).view(batch_size, nb_rounds).numpy())
        # the step's thresholds (`QualityCodec._stage`)
        (self.pinned_max_sse, self.max_sse_host, self.max_sse, self.max_sse_nbytes) = _staged_block(batch_size, device)
        # what a probe's `tconv9x9s4_luma` adds its squared errors into, and what its quantiser writes for its synthesis pass
        self.probe_acc = torch.zeros(batch_size, dtype=torch.int64, device=device)
        self.probe_latent = torch.empty((batch_size, codec.h_in//csts.STRIDE_PROD, codec.w_in//csts.STRIDE_PROD, codec.nb_maps),
                                        dtype=torch.float32, device=device)

    @property
    def selected(self):
        return self.first


class _QualityWorker(_BudgetWorker):
    """The result worker of `QualityCodec`."""

    def _finish(self, job):
        """`_BudgetWorker._finish`, whose point is the finest the search could take, then the step's search out of the slot's pinned
        blocks into the ticket."""
        super(_QualityWorker, self)._finish(job)
        (ticket, quality) = (job.ticket, job.emit[0].budget_slot)
        (point, met, trace_point, trace_sse) = quality.search_host
        (n, values) = (ticket.nb_images, ticket._values)
        rate_point = point[:n].astype(numpy.int64)
        values.update({'rate_point': rate_point, 'first_point': values['rate_point'], 'met': (met[:n] & 1) != 0,
                       'max_sse': quality.max_sse_host[:n].copy(), 'probe_points': trace_point[:n].astype(numpy.int64),
                       'probe_sse': trace_sse[:n].copy(),
                       'promised': values['upper_bound_bytes'][numpy.arange(n), rate_point] <= values['budget_bytes']})
        ticket._container_parts['rate_point'] = rate_point


class QualityCodec(BudgetCodec):
    """`BudgetCodec` with the rate point of every image found inside the step, on the device, so that the image keeps a PSNR floor at
    the smallest size the ladder allows: "this much quality per image" as a property of a step of the
    resident codec."""
    (_ticket_class, _worker_class) = (BudgetTicket, _QualityWorker)
    _budget_slot_class = _QualitySlot
    _no_coding_tile = ('`QualityCodec` does not take `coding_tile`: the coder\'s rows per stream would need the run order of '
                       '`device.ladder_select_tiles`.')
    NO_BUDGET = 1 << 62            # what a step without a budget stages: every valid point's bound is within it

    def __init__(self, variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, target_psnr=None, max_sse=None, budget_bytes=None,
                 **batch_codec_options):
        """ladder, batch_codec_options: as `BudgetCodec`; `coding_tile`, `fuse_latent`, a coder other than 'device' and `coder_chunks`
        > 1 are refused. target_psnr (dB) or max_sse (the largest squared error against the input, an integer): the threshold of a
        `submit` that names none, a scalar or one value per image, at most one of the two; target_psnr becomes
        `ratecontrol.max_sse_for_psnr(target_psnr, h_in*w_in)`. budget_bytes: the budget of a `submit` that names none; None: no budget.
        Per image the step bisects the ladder, in `ratecontrol.quality_rounds(K)` rounds, for the COARSEST point whose squared error
        against the input is within the threshold (`ratecontrol.select_by_quality`; the squared error is assumed not to decrease along
        the ladder, which is not checked), starting from the point `BudgetCodec` takes for the budget -- without a budget the first
        point whose symbols fit int16 --: quality is met at the smallest size, inside the budget where there is one. An image whose
        finest allowed point misses the threshold is coded at that point and reported in 'met'. A round quantises every image at its
        probe point, runs the synthesis transform and takes the exact squared error; the point finally taken is then quantised, coded
        and synthesised as in `BudgetCodec`.
        `Ticket.result()` has `BudgetCodec`'s keys and 'met' bool (N,), 'max_sse' int64 (N,), 'probe_points' and 'probe_sse' int64
        (N, R) (what every round probed and found) and 'first_point' int64 (N,) (the finest point the search could take);
        'rate_point' is the point taken, 'promised' says upper_bound_bytes[i, rate_point[i]] <= budget, 'budget_bytes' is 2^62
        without a budget. `Ticket.image_containers()[i]` is byte for byte `container.encode_images` of image i at its point;
        `Ticket.container()` raises."""
        # refused in front of every allocation, as everything `BudgetCodec.__init__` refuses
        self._nb_pixels = h_in*w_in
        self._default_max_sse = self._max_sse_of(target_psnr, max_sse, batch_size)
        super(QualityCodec, self).__init__(variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, budget_bytes=budget_bytes,
                                           **batch_codec_options)

    @property
    def nb_rounds(self):
        """The rounds of a step's bisection."""
        from . import ratecontrol
        return ratecontrol.quality_rounds(self.ladder.nb_points)

    def _max_sse_of(self, target_psnr, max_sse, batch_size):
        """The thresholds of a step as int64 (batch_size,), from one of the two ways to name them; None when neither is given."""
        from . import ratecontrol
        if target_psnr is not None and max_sse is not None:
            raise ValueError('give `target_psnr` or `max_sse`, not both.')
        if target_psnr is not None:
            targets = numpy.asarray(target_psnr, dtype=numpy.float64)
            if targets.ndim > 1 or (targets.ndim == 1 and targets.shape[0] != batch_size):
                raise ValueError('`target_psnr` must be a number or one number per image.')
            max_sse = ratecontrol.max_sse_for_psnr(targets, self._nb_pixels)
        if max_sse is None:
            return None
        thresholds = numpy.asarray(max_sse)
        if thresholds.dtype.kind not in 'iu' or thresholds.ndim > 1 or (thresholds.ndim == 1 and thresholds.shape[0] != batch_size):
            raise ValueError('`max_sse` must be an integer or one integer per image.')
        return numpy.ascontiguousarray(numpy.broadcast_to(thresholds.astype(numpy.int64), (batch_size,)))

    def submit(self, luminances_uint8, target_psnr=None, max_sse=None, budget_bytes=None):
        """`BatchCodec.submit` with the step's thresholds (`target_psnr` or `max_sse`, a scalar or one value per image; neither: the
        constructor's) and budgets (None: the constructor's `budget_bytes`; none there either: no budget)."""
        if target_psnr is None and max_sse is None:
            thresholds = self._default_max_sse
            if thresholds is None:
                raise ValueError('neither `target_psnr` nor `max_sse`, and the codec was built without a default.')
        else:
            thresholds = self._max_sse_of(target_psnr, max_sse, self.batch_size)
        budgets = self._budgets_for(budget_bytes)
        if budgets is None:
            budgets = numpy.full(self.batch_size, self.NO_BUDGET, dtype=numpy.int64)
        return self._submit_staged(luminances_uint8, (budgets, thresholds))

    def _stage(self, slot):
        """`BudgetCodec._stage`, and the step's thresholds into their pinned block."""
        super(QualityCodec, self)._stage(slot)
        self._budget_slots[id(slot)].max_sse_host[:self.batch_size] = self._staged[1]

    def _launch_round(self, quality, round):
        dev.quality_search(quality.first, quality.max_sse[:self.batch_size], quality.state, quality.probe_acc, quality.point, quality.prob_row,
                           quality.trace_point, quality.trace_sse, quality.met, self.ladder.nb_points, round, self.idx_map_exception,
                           self.ladder.nb_points*self.nb_maps)

    def _launch_analysis(self, luminances_uint8, slot, hook):
        """`BudgetCodec._launch_analysis` with the search between the point for the budget and the quantiser: ... -> the point of every
        image for its budget (`first`) -> the step's thresholds -> round 0 -> R times [the quantiser at every image's probe point (no
        symbols, flags or checks) -> tconv1+IGDN5 -> tconv2+IGDN6 -> tconv3 + BT.601 cast + squared error against the input -> round
        r] -> the quantiser at the point taken -> exception-map histograms, on the current stream. A linear chain whose launches
        and arguments are the same every step: the rounds differ by a scalar, the step's contents travel through device memory."""
        quality = self._budget_slots[id(slot)]
        y = self._launch_selection(luminances_uint8, slot, quality, hook)
        self._launch_thresholds(quality)
        hook('search', lambda: self._launch_round(quality, 0))
        dec = self.decoder
        d = dec.v
        ws = slot.conv_ws                         # the slot's: its error word, collected behind the synthesis side, covers the probes
        igdn_out = None if self.learned else (dec.g[4], d['decoder/beta_4'])
        (out_shifted, out_t) = (quality.probe_latent, None) if self.learned else (None, quality.probe_latent)
        for r in range(1, self.nb_rounds + 1):
            hook('probe_latent', lambda: self._quantise_at(y, quality.point, igdn_out=igdn_out, want_shifted=self.learned, want_symbols=False,
                                                           want_checks=False, out_shifted=out_shifted, out_t=out_t))
            t = hook('probe_tconv1_igdn5', lambda: dev.tconv5x5s2(quality.probe_latent, dec.w4, d['decoder/biases_4'], dev.NORM_IGDN, dec.g[5],
                                                                  d['decoder/beta_5'], workspace=ws))
            t = hook('probe_tconv2_igdn6', lambda: dev.tconv5x5s2(t, dec.w5, d['decoder/biases_5'], dev.NORM_IGDN, dec.g[6], d['decoder/beta_6'],
                                                                  workspace=ws))
            hook('probe_tconv3', lambda: self._launch_probe_error(t, luminances_uint8, quality))
            hook('search', lambda: self._launch_round(quality, r))
        return self._launch_quantiser(y, slot, quality, hook)

    def _launch_thresholds(self, quality):
        """The step's thresholds out of the slot's pinned block into its device block, in front of round 0."""
        dev.fetch_prefix(quality.pinned_max_sse, quality.max_sse, quality.max_sse_nbytes)

    def _launch_probe_error(self, t, luminances_uint8, quality):
        """A probe's transpose_conv_3 without a plane: its squared error against the step's input, added into `probe_acc`."""
        return dev.tconv9x9s4_luma(t, self.decoder.w6, want_f32=False, want_u8=False, ref_u8=luminances_uint8, sse=quality.probe_acc)


class _PlaneQualityCodec(QualityCodec):
    """`QualityCodec` as one plane of a colour picture inside `ColourQualityCodec`; private: the public
    rate-control codecs go on refusing `pad`. Two things are its own, as two are `_PlaneBudgetCodec`'s.
    `pad=True` is taken: h_in x w_in is the plane's REAL size, the step runs at the coded size as `BatchCodec(pad=True)` runs it, and
    EVERY squared error of the step is over the real pixels: the final one as `BatchCodec(pad=True)` takes it, a probe's out of the
    epilogue of its own transpose_conv_3 (`device.tconv9x9s4_luma_frame`) against the padded frame the analysis side was given, so
    that 'probe_sse' at the point taken IS 'sse' and `sse <= max_sse` stands on the count `max_sse_for_psnr(T, h_in*w_in)` assumes.
    The bounds, the header and the blobs are those of the coded plane with the real size in the `crop` byte.
    thresholds_on_device=True: `submit(images, max_sse=...)` also takes an int64 device tensor (batch_size,) that was written earlier
    on the caller's stream. The step copies it into its slot's `max_sse` block on the step's own stream, behind that stream's wait for
    the caller's and in front of round 0, launches no `fetch_prefix` of thresholds, eager or replayed, and publishes `max_sse` into
    the slot's `pinned_max_sse` together with the selection: 'max_sse' of `result()` is what the device used. A host array or a scalar
    goes the same way, through the slot's pinned block. The slot's `max_sse` block is free then: `_submit` has waited for the slot."""
    _takes_pad = True

    def __init__(self, variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, target_psnr=None, max_sse=None, budget_bytes=None,
                 thresholds_on_device=False, **batch_codec_options):
        self.thresholds_on_device = bool(thresholds_on_device)
        super(_PlaneQualityCodec, self).__init__(variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, target_psnr=target_psnr,
                                                 max_sse=max_sse, budget_bytes=budget_bytes, **batch_codec_options)

    def _max_sse_of(self, target_psnr, max_sse, batch_size):
        if not isinstance(max_sse, torch.Tensor):
            return super(_PlaneQualityCodec, self)._max_sse_of(target_psnr, max_sse, batch_size)
        if target_psnr is not None:
            raise ValueError('give `target_psnr` or `max_sse`, not both.')
        if not self.thresholds_on_device:
            raise ValueError('`max_sse` as a tensor needs `thresholds_on_device=True`.')
        if max_sse.dtype != torch.int64 or tuple(max_sse.shape) != (batch_size,) or not max_sse.is_contiguous() or max_sse.device != self.device:
            raise ValueError('`max_sse` as a tensor must be int64 (batch_size,), contiguous, on the codec\'s device.')
        return max_sse

    def _stage(self, slot):
        """With `thresholds_on_device`: the step's thresholds into the slot's DEVICE block, on the current stream (the step's own);
        its budgets as ever."""
        if not self.thresholds_on_device:
            return super(_PlaneQualityCodec, self)._stage(slot)
        BudgetCodec._stage(self, slot)
        (quality, staged, n) = (self._budget_slots[id(slot)], self._staged[1], self.batch_size)
        if isinstance(staged, torch.Tensor):
            quality.max_sse[:n].copy_(staged, non_blocking=True)
            staged.record_stream(torch.cuda.current_stream())
        else:
            quality.max_sse_host[:n] = staged
            quality.max_sse[:n].copy_(quality.pinned_max_sse[:n], non_blocking=True)

    def _replay_step(self, luminances_uint8, slot, index, ticket, coded):
        if not self.thresholds_on_device:
            return super(_PlaneQualityCodec, self)._replay_step(luminances_uint8, slot, index, ticket, coded)
        # the stream `BatchCodec._replay_step` replays this step's graphs on: the thresholds go there in front of them
        stream = self._transform_streams[index % len(self._transform_streams)]
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            self._stage(slot)
        return BatchCodec._replay_step(self, luminances_uint8, slot, index, ticket, coded)

    def _launch_thresholds(self, quality):
        if not self.thresholds_on_device:                # (else `_stage` has put them there: nothing is launched, captured or eager)
            super(_PlaneQualityCodec, self)._launch_thresholds(quality)

    def _launch_probe_error(self, t, luminances_uint8, quality):
        """The probe's error over the plane's real pixels, out of the transposed conv's own epilogue: `luminances_uint8` is the padded
        frame here (`BatchCodec._launch_step` / the graph's static input)."""
        return dev.tconv9x9s4_luma_frame(t, self.decoder.w6, (self.h_image, self.w_image), want_f32=False, want_u8=False,
                                         ref_u8=luminances_uint8, sse=quality.probe_acc)

    def _publish_coder_side(self, slot):
        if self.thresholds_on_device:
            quality = self._budget_slots[id(slot)]
            dev.publish_to_host(quality.max_sse, quality.pinned_max_sse)
        super(_PlaneQualityCodec, self)._publish_coder_side(slot)


# ---- the same for tile-indexed containers: the search's rows per stream, in the coder's run order -----------

def tile_prob_rows(layout, points, idx_map_exception=-1, exception_row_base=None):
    """The coder's row of every stream of a step in coding tiles whose image i is coded at `points[i]`, in the run order of `layout`
    (`coding_tile_layout`'s dict): what `device.quality_search_tiles` writes. Map m of run-order entry e, an (image, tile), takes row
    points[image]*128 + m; the exception map takes `exception_row_base + image` (None: behind the K = max(points) + 1 points'
    rows). -> int32 [n_streams]. With every point 0 it is `layout['prob_row']`."""
    nb_maps = csts.NB_MAPS_3
    points = numpy.asarray(points, dtype=numpy.int64)
    if exception_row_base is None:
        exception_row_base = (int(points.max()) + 1)*nb_maps
    images = numpy.array([layout['entries'][p][0] for p in layout['payload_entry'].tolist()], dtype=numpy.int64)
    rows = points[images][:, None]*nb_maps + numpy.arange(nb_maps, dtype=numpy.int64)[None, :]
    if idx_map_exception >= 0:
        rows[:, idx_map_exception] = exception_row_base + images
    return rows.reshape(-1).astype(numpy.int32)


class _TiledQualitySlot(_TiledRows, _QualitySlot):
    """What one `TiledQualityCodec` step in flight owns beyond its `_Slot`: `_QualitySlot`'s state with `_TiledRows`' shapes, as
    `_TiledBudgetSlot` is `_BudgetSlot`'s; every round of `device.quality_search_tiles` writes `prob_row` again. Made once;
    tests/tiled_quality_slot_buffers.py says what a step may find in every attribute when it starts."""
    __slots__ = ('class_rows',)


class TiledQualityCodec(_TiledRateControl, QualityCodec):
    """`QualityCodec` for tile-indexed containers: a PSNR floor per image whose blob is the single-image `EAT1`
    blob `container.encode_images(..., coding_tile=coding_tile)` writes, so that crops come out of it (`container.decode_region`,
    `RegionDecoder`) and its serial chains are a tile long."""
    _budget_slot_class = _TiledQualitySlot

    def __init__(self, variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, coding_tile, target_psnr=None, max_sse=None,
                 budget_bytes=None, **batch_codec_options):
        """coding_tile: (th, tw) in latents, clamped to the latent plane, as `BatchCodec(coding_tile=...)` takes it; everything else
        as `QualityCodec`. Refused in front of every allocation: what `QualityCodec` and `TiledBudgetCodec` refuse.
        The step is `QualityCodec`'s with the tiled pieces of `TiledBudgetCodec`: the counts per (image, point, tile, map), the
        bounds of every image's `EAT1` blob for the finest point the search may take, the search -- a point's squared error does not
        depend on the coding tile: the probes are `QualityCodec`'s --, every round leaving the coder's rows per stream of the step
        (`device.quality_search_tiles`), and the coder in tiles. `Ticket.result()` has `QualityCodec`'s keys, 'coder_bits' summed over
        an image's tiles, 'upper_bound_bytes' the `EAT1` bounds; `Ticket.image_containers()[i]` is byte for byte
        `container.encode_images(image i, ..., coding_tile=coding_tile)` at `rate_point[i]`; `Ticket.container()` raises."""
        coding_tile = container_format._positive_pair(coding_tile, '`coding_tile`')
        super(TiledQualityCodec, self).__init__(variables, are_bin_widths_learned, ladder, batch_size, h_in, w_in, target_psnr=target_psnr,
                                                max_sse=max_sse, budget_bytes=budget_bytes, coding_tile=coding_tile, **batch_codec_options)
        try:
            # `device.quality_search_tiles`: where the coder takes every (image, tile) entry from, in payload order
            self._run_entry = torch.from_numpy(self._tile_layout['run_entry'].astype(numpy.int32)).to(self.device)
        except BaseException:
            self.close()
            raise

    def _launch_round(self, quality, round):
        dev.quality_search_tiles(quality.first, quality.max_sse[:self.batch_size], quality.state, quality.probe_acc, quality.point,
                                 quality.prob_row, quality.trace_point, quality.trace_sse, quality.met, self._run_entry,
                                 self._tile_layout['nb_tiles'], self.ladder.nb_points, round, self.idx_map_exception,
                                 self.ladder.nb_points*self.nb_maps)


# ---- colour pictures: three planes through two luminance codecs ------------------------------------------------

class ColourTicket(object):
    """Handle on one submitted batch of colour pictures: the three plane tickets (`tickets`: Y, Cb, Cr) and what the colour layer adds."""

    def __init__(self, tickets, image_size, step):
        self.nb_images = tickets[0].nb_images
        self.tickets = tuple(tickets)
        self.image_size = image_size
        self.reconstruction_rgb = None        # device tensor (N, h, w, 3): the merged pictures
        self.reconstruction_host = None       # numpy uint8 (N, h, w, 3), a view of the colour slot's pinned buffer, with fetch_reconstruction,
        #                                       after result(): the same pictures, written by a merge launch of their own straight into
        #                                       pinned memory. Both are valid until the colour slot comes round (`ColourCodec.depth` submits
        #                                       later); everything `result()` returns is the ticket's own and stays valid
        self.fed_event = None                 # host input: recorded behind the host -> device copy (the caller's pinned batch may be
        #                                       rewritten once it has completed)
        self.merged_event = None              # recorded behind the merge and the publication of 'sse_rgb': wait for it on another stream
        #                                       before reading `reconstruction_rgb` there
        self._step = step
        self._sse = None                      # 'sse_rgb', copied out of the colour slot's pinned words: by `result()`, or by the `submit`
        #                                       that takes the slot for its next step (`_keep_sse`), whichever comes first
        self._values = None

    def _keep_sse(self):
        """Behind `merged_event`: the step's squared errors leave the slot's pinned words for the ticket."""
        if self._sse is None:
            self._sse = self._step.sse_host.copy()

    def result(self):
        """Blocks until the three planes and the merge are through (and raises a plane's error as `Ticket.result()` does); every key of
        `BatchCodec.result()` as an array (N, 3) in the order Y, Cb, Cr, and 'sse_rgb' int64 (N,): the squared error of the merged
        picture against the input over its 3 h w samples. Only waits: everything was enqueued by `submit`. Valid at any later time, like
        `Ticket.result()`: nothing it returns stays in a slot."""
        if self._values is None:
            results = [ticket.result() for ticket in self.tickets]
            self.merged_event.synchronize()
            values = {key: numpy.stack([r[key] for r in results], axis=1) for key in results[0]}
            self._keep_sse()
            values['sse_rgb'] = self._sse
            if self._step.pinned_rgb is not None:
                self.reconstruction_host = self._step.pinned_rgb.numpy()
            self._values = values
        return self._values

    def container(self):
        """The step as one `EAC1` blob (container.py): byte for byte `container.encode_colour_images` of the same pictures. Blocks and
        raises like the three `Ticket.container()` it is made of (`ContainerOverflow` included). Needs `emit_container=True`."""
        return container_format.assemble_colour_blob(self.image_size, *(ticket.container() for ticket in self.tickets))

    def image_containers(self):
        """Like `container()`: one `EAC1` blob per picture, made of the three single-image plane blobs."""
        return [container_format.assemble_colour_blob(self.image_size, *blobs)
                for blobs in zip(*(ticket.image_containers() for ticket in self.tickets))]


class _ColourStep(object):
    """What one colour step in flight owns beside the inner codecs' slots; `ColourCodec` goes round `depth` of them."""

    def __init__(self, codec):
        (n, h, w, device) = (codec.batch_size, codec.h, codec.w, codec.device)
        (hc, wc) = (codec.hc, codec.wc)
        self.rgb_in = torch.empty((n, h, w, 3), dtype=torch.uint8, device=device)          # the device copy of the batch: split from, compared with
        self.planes = (torch.empty((n, h, w), dtype=torch.uint8, device=device), torch.empty((n, hc, wc), dtype=torch.uint8, device=device),
                       torch.empty((n, hc, wc), dtype=torch.uint8, device=device))
        self.pinned_rgb = torch.empty((n, h, w, 3), dtype=torch.uint8).pin_memory() if codec.fetch_reconstruction else None
        self.rgb_out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=device)
        self.sse = torch.zeros(n, dtype=torch.int64, device=device)
        self.pinned_sse = torch.zeros(n, dtype=torch.int64).pin_memory()
        self.sse_host = self.pinned_sse.numpy()
        self.merged = None                    # the event behind the last merge that used this entry
        self.ticket = None                    # that step's ticket, until the entry's next step has taken its squared errors out for it


class ColourCodec(object):
    """RGB pictures of any height and width through the luminance model, 4:2:0 (colour.py), pipelined: two `BatchCodec(pad=True,
    keep_reconstruction=True)` of batch size `batch_size` -- `luma` at (h, w), `chroma` at (hc, wc) = ceil(h/2) x ceil(w/2) -- and,
    around them, the split kernel, the merge kernel and rings of buffers of this class's own. Neither inner codec is modified.

    A colour step is one step of `luma` and two consecutive steps of `chroma`, Cb then Cr; the three `Ticket.container()`s are the
    three plane blobs of the step's `EAC1`. `submit` enqueues, in this order: the copy of the batch into the step's device buffer (a
    pinned batch on a feed stream, `ColourTicket.fed_event` behind it), the split into the step's three plane buffers on the caller's
    stream, the three inner submits, and, on a stream of this codec's own behind the three tickets' `decoded_event`s, the merge
    (`device.colour_merge_420`) of the three kept reconstructions into the step's RGB output with the squared error against the device
    copy of the input -- with `fetch_reconstruction` a second merge launch, of the picture alone, straight into the step's pinned
    output --, then the publication of the errors and `merged_event`.

    Ring depth. An inner slot's reconstruction is valid "until the slot comes round": the inner codecs order the reuse of a slot
    against their own result worker, not against a merge on another stream. `luma` holds `luma.nb_slots` steps, `chroma`
    `chroma.nb_slots` of which a colour step takes two consecutive ones, so the inner rings hold
        depth = min(luma.nb_slots, chroma.nb_slots // 2)
    colour steps: the plane of step i is overwritten by step i + luma.nb_slots at the earliest, Cb and Cr of step i (inner steps 2i,
    2i + 1) by inner step 2i + chroma.nb_slots, which belongs to colour step i + chroma.nb_slots // 2 for either parity. `submit`
    therefore waits on the host for the merge event of step i - depth before it enqueues anything of step i, and this class's own rings
    (batch copies, plane buffers, RGB outputs, squared errors) are `depth` long: the same wait frees entry i % depth, and behind it
    `submit` hands the entry's squared errors to the ticket of step i - depth, so a `ColourTicket.result()` collected at any later
    time is its own step's. A configuration whose chroma codec cannot hold one colour step (depth 0) is refused. A `submit` that
    raises half way (an inner codec's error) drains both inner codecs and the merge stream before it re-raises: whatever it did
    enqueue is through, and the next step starts on idle rings whichever parity the chroma ring is left at.

    chroma: None (Cb and Cr take the luminance rate point) or (bin_widths_test, map_mean, binary_probabilities, idx_map_exception).
    batch_codec_options go to both inner codecs; chroma_options override them for `chroma` (`codec.product_mode(hc, wc)`). Unless
    given there, the chroma codec's `nb_in_flight` is 2 * `luma.nb_in_flight` + 2 -- as many colour steps as `luma`'s slots hold --
    cut to what `codec.stream_budget` leaves of it in this process, quietly, since nobody asked for the larger number: with 4 hardware
    queues that is 2, and depth = 2. A value the caller gives is budgeted, and warned about, by `BatchCodec` as ever.
    `fetch_reconstruction` is this codec's: the merged pictures in pinned memory as well. `pad` and `keep_reconstruction` are fixed."""

    # what `ColourBudgetCodec` replaces: the ring entry, the ticket and (`_build`'s `make_inner`, `_submit_planes`) the inner codecs
    (_step_class, _ticket_class) = (_ColourStep, ColourTicket)

    def __init__(self, variables, are_bin_widths_learned, bin_widths_test, map_mean, binary_probabilities, idx_map_exception, batch_size,
                 h, w, chroma=None, chroma_options=None, **batch_codec_options):
        (self.luma, self.chroma) = (None, None)
        luma_point = (bin_widths_test, map_mean, binary_probabilities, idx_map_exception)
        chroma_point = luma_point if chroma is None else tuple(chroma)
        if len(chroma_point) != 4:
            raise ValueError('`chroma` must be (bin_widths_test, map_mean, binary_probabilities, idx_map_exception).')
        self._build(batch_size, h, w, chroma_options, batch_codec_options,
                    lambda is_chroma, height, width, **options: BatchCodec(variables, are_bin_widths_learned, *(chroma_point if is_chroma else luma_point),
                                                                           self.batch_size, height, width, pad=True, keep_reconstruction=True,
                                                                           **options))

    def _build(self, batch_size, h, w, chroma_options, batch_codec_options, make_inner):
        """Everything the constructor does behind its own arguments: the options' refusals, the two inner codecs --
        make_inner(is_chroma, height, width, **options) -> the luminance codec, then the chroma codec --, the ring and the merge stream."""
        (self.luma, self.chroma) = (None, None)
        options = dict(batch_codec_options)
        chroma_options = dict(chroma_options or {})
        for fixed in ('pad', 'keep_reconstruction'):
            if fixed in options or fixed in chroma_options:
                raise ValueError('`{0}` is not an option of ColourCodec: its inner codecs run with {0}=True.'.format(fixed))
        for shared in ('fetch_reconstruction', 'emit_container', 'device'):
            if shared in chroma_options:
                raise ValueError('`{0}` is the colour codec\'s, not the chroma codec\'s alone.'.format(shared))
        self.fetch_reconstruction = bool(options.pop('fetch_reconstruction', False))
        self.batch_size = container_format._positive_int(batch_size, '`batch_size`')
        (self.h, self.w) = (container_format._positive_int(h, '`h`'), container_format._positive_int(w, '`w`'))
        (self.hc, self.wc) = dev.chroma_size(self.h, self.w)
        for_chroma = dict(options)
        for_chroma.update(chroma_options)
        self.emit_container = bool(options.get('emit_container', False))
        try:
            self.luma = make_inner(False, self.h, self.w, **options)
            if chroma_options.get('nb_in_flight') is None:
                # two inner steps per colour step: as many colour steps as the luminance codec's nb_in_flight + 2 slots hold, as far as
                # this process's hardware queues go (the condition is `BatchCodec`'s own, so it finds nothing left to cut or to say)
                wanted = 2*int(self.luma.nb_in_flight) + 2
                if for_chroma.get('coder', 'device') == 'device' and not for_chroma.get('one_stream_steps') \
                        and os.environ.get('EAE_IGNORE_HW_QUEUES') != '1':
                    (_, wanted, _) = stream_budget(for_chroma.get('nb_transform_streams', 1), wanted)
                for_chroma['nb_in_flight'] = wanted
            self.chroma = make_inner(True, self.hc, self.wc, **for_chroma)
            self.device = self.luma.device
            self.depth = min(self.luma.nb_slots, self.chroma.nb_slots//2)
            if self.depth < 1:
                raise ValueError('the chroma codec has {0} slot(s): it cannot hold the two steps (Cb, Cr) of one colour step.'.format(
                    self.chroma.nb_slots))
            self._steps = [self._step_class(self) for _ in range(self.depth)]
            self._merge_stream = torch.cuda.Stream(device=self.device)
            self._feed_stream = None
            self._index = 0
        except BaseException:
            self.close()
            raise

    def submit(self, rgb_uint8):
        """uint8 tensor (batch_size, h, w, 3), on the device or in PINNED host memory -> ColourTicket. Everything is enqueued; the host
        waits only for free inner slots and for the merge of the step `depth` submits ago (class docstring)."""
        if rgb_uint8.dtype != torch.uint8:
            raise TypeError('`rgb_uint8.dtype` is not equal to `torch.uint8`.')
        if tuple(rgb_uint8.shape) != (self.batch_size, self.h, self.w, 3):
            raise ValueError('`rgb_uint8.shape` is not (batch_size, h, w, 3).')
        host = rgb_uint8.device.type == 'cpu'
        if host and not rgb_uint8.is_pinned():
            raise ValueError('a host batch must be in pinned memory (`torch.Tensor.pin_memory()`): its copy is asynchronous.')
        step = self._steps[self._index % self.depth]
        self._index += 1
        if step.merged is not None:
            # the merge that read this entry, and the inner reconstructions that come round with this step, is through
            step.merged.synchronize()
        if step.ticket is not None:
            step.ticket._keep_sse()           # before this step's merge rewrites the entry's pinned words
            step.ticket = None
        try:
            return self._enqueue(step, rgb_uint8, host)
        except BaseException:
            # part of the step may be enqueued (an inner submit raised): wait for all of it, so that the next step finds idle rings
            step.merged = None
            try:
                self.drain()
            except Exception:                 # the device itself is in trouble: the next submit will say so
                pass
            raise

    def _enqueue(self, step, rgb_uint8, host):
        """The launches of one colour step on ring entry `step` (class docstring) -> its ticket."""
        fed = None
        if host:
            if self._feed_stream is None:
                self._feed_stream = torch.cuda.Stream(device=self.device)
            with torch.cuda.stream(self._feed_stream):
                step.rgb_in.copy_(rgb_uint8, non_blocking=True)
                fed = torch.cuda.Event()
                fed.record()
            torch.cuda.current_stream().wait_event(fed)
        else:
            step.rgb_in.copy_(rgb_uint8, non_blocking=True)
        dev.colour_split_420(step.rgb_in, out=step.planes)
        tickets = self._submit_planes(step)
        ticket = self._ticket_class(tickets, (self.h, self.w), step)
        ticket.fed_event = fed
        with torch.cuda.stream(self._merge_stream):
            for inner in tickets:
                self._merge_stream.wait_event(inner.decoded_event)
                inner.reconstruction_uint8.record_stream(self._merge_stream)
            step.sse.zero_()
            planes = tuple(inner.reconstruction_uint8 for inner in tickets)
            dev.colour_merge_420(*planes, (self.h, self.w), out=step.rgb_out, reference=step.rgb_in, sse=step.sse)
            if step.pinned_rgb is not None:
                dev.colour_merge_420(*planes, (self.h, self.w), out=step.pinned_rgb)      # the picture alone, straight into pinned memory
            step.pinned_sse.copy_(step.sse, non_blocking=True)
            step.merged = torch.cuda.Event()
            step.merged.record()
        ticket.merged_event = step.merged
        ticket.reconstruction_rgb = step.rgb_out
        step.ticket = ticket
        return ticket

    def _submit_planes(self, step):
        """The three inner submits of the step whose planes `step.planes` holds, on the current stream -> the tickets (Y, Cb, Cr)."""
        return (self.luma.submit(step.planes[0]), self.chroma.submit(step.planes[1]), self.chroma.submit(step.planes[2]))

    def drain(self):
        """Waits until every submitted batch is through, the merges included."""
        for inner in (self.luma, self.chroma):
            if inner is not None:
                inner.drain()
        if getattr(self, '_merge_stream', None) is not None:
            self._merge_stream.synchronize()

    def close(self):
        """Waits for the pending batches and closes both inner codecs. Idempotent."""
        try:
            self.drain()
        finally:
            for inner in (self.luma, self.chroma):
                if inner is not None:
                    inner.close()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, traceback):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: nothing left to report to
            pass


# ---- a byte budget per colour picture ---------------------------------------------------------------------------

class ColourBudgetTicket(ColourTicket):
    """Handle on one submitted `ColourBudgetCodec` step."""
    _picture_budgets = None                   # int64 (N,): the step's budgets per picture, the ticket's own copy

    def result(self):
        """`ColourTicket.result()` over the three `BudgetCodec.result()`s -- every key (N, 3, ...) in the order Y, Cb, Cr, 'budget_bytes'
        the budgets the planes' selections used, and 'sse_rgb' -- plus, per picture, int64 / bool (N,): 'picture_budget_bytes';
        'picture_blob_bytes', 48 plus the three 'blob_bytes': the length of `image_containers()[i]`; 'picture_promised': all three
        planes are promised, and then 48 plus the three bounds taken is within the budget; 'picture_fits': the blob is."""
        if self._values is None:
            values = super(ColourBudgetTicket, self).result()
            values['picture_budget_bytes'] = self._picture_budgets
            values['picture_blob_bytes'] = container_format.COLOUR_HEADER_BYTES + values['blob_bytes'].sum(axis=1)
            values['picture_promised'] = values['promised'].all(axis=1)
            values['picture_fits'] = values['picture_blob_bytes'] <= self._picture_budgets
        return self._values

    def container(self):
        """Always raises, as `BudgetTicket.container()`: every picture of the step has rate points of its own."""
        raise RuntimeError('a ColourBudgetCodec step has rate points per picture and one EAC1 blob holds one per plane: use `image_containers()`')


class _ColourBudgetStep(_ColourStep):
    """`_ColourStep` with the step's budgets: the pictures' in a pinned block and on the device, the luminance planes' on the device."""

    def __init__(self, codec):
        super(_ColourBudgetStep, self).__init__(codec)
        n = codec.batch_size
        self.pinned_budgets = torch.zeros(n, dtype=torch.int64).pin_memory()
        self.budgets_host = self.pinned_budgets.numpy()
        self.budgets = torch.zeros(n, dtype=torch.int64, device=codec.device)
        self.luma_budgets = torch.zeros(n, dtype=torch.int64, device=codec.device)      # written by `device.colour_budget_rest`


class ColourBudgetCodec(ColourCodec):
    """`ColourCodec` with ONE byte budget per picture: that of the picture's single-picture `EAC1` blob, shared between its three
    planes on the device inside the step (the rule is `ratecontrol.colour_chroma_budgets` /
    `colour_luma_budgets`, its synchronous sibling `container.encode_colour_images_to_budget`). The inner codecs are two
    `_PlaneBudgetCodec(pad=True, keep_reconstruction=True)`, `luma` with `budgets_on_device=True`; the ring depth, the drain when a
    submit raises, `close`, `fetch_reconstruction` and the merge are `ColourCodec`'s.

    `submit(rgb, budget_bytes)` enqueues, in this order: the batch copy and the split; Cb and Cr into `chroma`, each with the
    host-computed budget c = (P * share_q16) >> 17; on the caller's stream, behind both chroma steps' `decoded_event`, ONE
    `device.colour_budget_rest` launch, which reads the picture budgets (uploaded from the step's pinned block) and the `upper` and
    `point` blocks of the two chroma slots and writes r = max(P - ub_cb - ub_cr, 0) into the step's own buffer; Y into `luma` with that
    buffer as its budgets; the merge. The luminance budget never visits the host, and no launch argument depends on it.
    The chroma blocks read stay valid until their slot comes round, which `ColourCodec`'s depth rule puts behind this step's merge,
    hence behind the launch that read them (DESIGN.md section 29 has the whole argument). The luminance analysis of a colour step
    runs behind its chroma steps; steps of the ring overlap as in `ColourCodec`.

    ladder, chroma_ladder (None: `ladder`): `ratecontrol.RateLadder`s of the same number of points and the same truncated unary
    length; chroma_share: the fraction of the payload both chroma planes together may take, in ]0, 1[ (0.25: a starting value, not a
    measured one). budget_bytes: the budget of a `submit` that names none. Refused: `coding_tile`, the keyword `rdo_lambda` (a ladder
    with a price is fine), `pad` / `keep_reconstruction` as options, and what `BudgetCodec` refuses."""
    (_step_class, _ticket_class) = (_ColourBudgetStep, ColourBudgetTicket)

    def __init__(self, variables, are_bin_widths_learned, ladder, batch_size, h, w, budget_bytes=None, chroma_ladder=None, chroma_share=0.25,
                 chroma_options=None, **batch_codec_options):
        from . import ratecontrol
        (self.luma, self.chroma) = (None, None)
        chroma_ladder = ladder if chroma_ladder is None else chroma_ladder
        if not isinstance(ladder, ratecontrol.RateLadder) or not isinstance(chroma_ladder, ratecontrol.RateLadder):
            raise TypeError('`ladder` and `chroma_ladder` must be `ratecontrol.RateLadder`s.')
        # refused in front of every allocation
        for options in (batch_codec_options, chroma_options or {}):
            if options.get('coding_tile') is not None:
                raise ValueError('`ColourBudgetCodec` does not take `coding_tile`: the bounds are those of whole maps (EAE1 plane blobs).')
            if options.get('rdo_lambda') is not None:
                raise ValueError('`ColourBudgetCodec` does not take `rdo_lambda`: the price of a bit comes with the ladder '
                                 '(`ratecontrol.RateLadder(..., rdo_lambda=...)`).')
            if 'budgets_on_device' in options:
                raise ValueError('`budgets_on_device` is not an option of ColourBudgetCodec: its luminance codec runs with it.')
        if chroma_ladder.nb_points != ladder.nb_points:
            raise ValueError('`ladder` and `chroma_ladder` hold {0} and {1} rate points: the same number is needed.'.format(
                ladder.nb_points, chroma_ladder.nb_points))
        if chroma_ladder.truncated_unary_length != ladder.truncated_unary_length:
            raise ValueError('`ladder` and `chroma_ladder` have truncated unary lengths {0} and {1}: the same is needed.'.format(
                ladder.truncated_unary_length, chroma_ladder.truncated_unary_length))
        ratecontrol.colour_chroma_budgets(0, chroma_share)             # refuses a share outside ]0, 1[
        self.chroma_share = float(chroma_share)
        (self.ladder, self.chroma_ladder) = (ladder, chroma_ladder)
        self._default_budgets = None if budget_bytes is None else BudgetCodec._budgets_of(budget_bytes, container_format._positive_int(batch_size, '`batch_size`'))
        self._submitting = None
        self._build(batch_size, h, w, chroma_options, batch_codec_options,
                    lambda is_chroma, height, width, **options: _PlaneBudgetCodec(
                        variables, are_bin_widths_learned, chroma_ladder if is_chroma else ladder, self.batch_size, height, width, pad=True,
                        keep_reconstruction=True, budgets_on_device=not is_chroma, **options))
        self.emit_container = True

    def submit(self, rgb_uint8, budget_bytes=None):
        """`ColourCodec.submit` with the step's budgets: a scalar or one value per picture, bytes of the picture's whole single-picture
        `EAC1` blob (its 48-byte header included); None: the constructor's `budget_bytes`."""
        from . import ratecontrol
        budgets = self._default_budgets if budget_bytes is None else BudgetCodec._budgets_of(budget_bytes, self.batch_size)
        if budgets is None:
            raise ValueError('no `budget_bytes`, and the codec was built without a default.')
        self._submitting = (budgets, ratecontrol.colour_chroma_budgets(budgets, self.chroma_share))
        try:
            return super(ColourBudgetCodec, self).submit(rgb_uint8)
        finally:
            self._submitting = None

    def _submit_planes(self, step):
        (budgets, chroma_budgets) = self._submitting
        # the entry is this step's: `submit` has waited for the merge of the step that used it last, which lies behind that step's
        # `colour_budget_rest` and luminance selection
        step.budgets_host[:] = budgets
        step.budgets.copy_(step.pinned_budgets, non_blocking=True)
        chroma_slots = []
        chroma_tickets = []
        for plane in step.planes[1:]:
            slot = self.chroma._slots[self.chroma._index % self.chroma.nb_slots]       # the slot this inner step takes (`BatchCodec._submit`)
            chroma_slots.append(self.chroma._budget_slots[id(slot)])
            chroma_tickets.append(self.chroma.submit(plane, chroma_budgets))
        caller = torch.cuda.current_stream()
        for inner in chroma_tickets:
            caller.wait_event(inner.decoded_event)
        (of_cb, of_cr) = chroma_slots
        dev.colour_budget_rest(step.budgets, of_cb.upper, of_cb.point, of_cr.upper, of_cr.point, step.luma_budgets)
        luma_ticket = self.luma.submit(step.planes[0], step.luma_budgets)
        return (luma_ticket,) + tuple(chroma_tickets)

    def _enqueue(self, step, rgb_uint8, host):
        ticket = super(ColourBudgetCodec, self)._enqueue(step, rgb_uint8, host)
        ticket._picture_budgets = self._submitting[0].copy()
        return ticket


# ---- a PSNR floor per colour picture ----------------------------------------------------------------------------

class ColourQualityTicket(ColourTicket):
    """Handle on one submitted `ColourQualityCodec` step."""
    _picture_max_sse = None                   # int64 (N,): the step's thresholds per picture, the ticket's own copy

    def result(self):
        """`ColourTicket.result()` over the three `QualityCodec.result()`s -- every key (N, 3, ...) in the order Y, Cb, Cr, 'max_sse'
        the thresholds the planes' searches used, and 'sse_rgb' (information: the rule does not read it) -- plus, per picture, int64 /
        bool (N,): 'picture_max_sse', M; 'picture_sse', the three 'sse' summed: the squared error over all samples of the 4:2:0 form;
        'picture_met': picture_sse <= M; 'picture_blob_bytes', 48 plus the three 'blob_bytes': the length of `image_containers()[i]`."""
        if self._values is None:
            values = super(ColourQualityTicket, self).result()
            values['picture_max_sse'] = self._picture_max_sse
            values['picture_sse'] = values['sse'].astype(numpy.int64).sum(axis=1)
            values['picture_met'] = values['picture_sse'] <= self._picture_max_sse
            values['picture_blob_bytes'] = container_format.COLOUR_HEADER_BYTES + values['blob_bytes'].sum(axis=1)
        return self._values

    def container(self):
        """Always raises, as `BudgetTicket.container()`: every picture of the step has rate points of its own."""
        raise RuntimeError('a ColourQualityCodec step has rate points per picture and one EAC1 blob holds one per plane: use `image_containers()`')


class _ColourQualityStep(_ColourStep):
    """`_ColourStep` with the step's thresholds: the pictures' in a pinned block and on the device, the luminance planes' on the device."""

    def __init__(self, codec):
        super(_ColourQualityStep, self).__init__(codec)
        n = codec.batch_size
        self.pinned_max_sse = torch.zeros(n, dtype=torch.int64).pin_memory()
        self.max_sse_host = self.pinned_max_sse.numpy()
        self.max_sse = torch.zeros(n, dtype=torch.int64, device=codec.device)
        self.luma_max_sse = torch.zeros(n, dtype=torch.int64, device=codec.device)      # written by `device.colour_quality_rest`


class ColourQualityCodec(ColourCodec):
    """`ColourCodec` with ONE PSNR floor per picture: over all S = h w + 2 hc wc samples of its 4:2:0 form, shared between its three
    planes on the device inside the step (the rule is `ratecontrol.colour_chroma_max_sse` /
    `colour_luma_max_sse`, its synchronous sibling `container.encode_colour_images_to_quality`). The inner codecs are two
    `_PlaneQualityCodec(pad=True, keep_reconstruction=True)`, `luma` with `thresholds_on_device=True`; the ring depth, the drain when a
    submit raises, `close`, `fetch_reconstruction` and the merge are `ColourCodec`'s.

    `submit(rgb, target_psnr=None, max_sse=None)` enqueues, in this order: the batch copy and the split; Cb and Cr into `chroma`, each
    with the host-computed threshold a = (M * share_q16) >> 17; on the caller's stream, behind both chroma steps' `decoded_event`, ONE
    `device.colour_quality_rest` launch, which reads the picture thresholds (uploaded from the step's pinned block) and the two chroma
    slots' published 'sse' -- the real squared errors of the points taken, which the synthesis side's `publish_step` writes into the
    slot's pinned words in front of that event (the device's own words are cleared by the same launch) -- and writes max(M - sse_cb -
    sse_cr, 0) into the step's own buffer; Y into `luma` with that buffer as its thresholds; the merge. The luminance threshold never
    visits the host, and no launch argument depends on it. The words read stay valid until their slot comes round, which
    `ColourCodec`'s depth rule puts behind this step's merge, hence behind the launch that read them. The luminance analysis of a
    colour step runs behind its chroma steps; steps of the ring overlap as in `ColourCodec`.

    ladder, chroma_ladder (None: `ladder`): `ratecontrol.RateLadder`s of the same number of points and the same truncated unary
    length; chroma_share: the fraction of the picture's squared error both chroma planes together may take, in ]0, 1[ (1/3, the
    chroma planes' share of the samples: a starting value nobody has measured on a trained model). target_psnr (dB, over the S
    samples: `ratecontrol.max_sse_for_psnr(T, colour_nb_samples(h, w))`) or max_sse (an integer in [0, 2^62]): the threshold of a
    `submit` that names none, a scalar or one value per picture, at most one of the two. Refused in front of every allocation:
    `budget_bytes` (a budget under a floor is out of scope), `coding_tile`, the keyword `rdo_lambda` (a ladder with a price is
    fine), `pad` / `keep_reconstruction` / `thresholds_on_device` as options, and what `QualityCodec` refuses.
    MONOTONICITY IS ASSUMED AND NOT CHECKED, per plane, as in `ratecontrol.select_by_quality`."""
    (_step_class, _ticket_class) = (_ColourQualityStep, ColourQualityTicket)

    def __init__(self, variables, are_bin_widths_learned, ladder, batch_size, h, w, target_psnr=None, max_sse=None, chroma_ladder=None,
                 chroma_share=1./3., chroma_options=None, **batch_codec_options):
        from . import ratecontrol
        (self.luma, self.chroma) = (None, None)
        chroma_ladder = ladder if chroma_ladder is None else chroma_ladder
        if not isinstance(ladder, ratecontrol.RateLadder) or not isinstance(chroma_ladder, ratecontrol.RateLadder):
            raise TypeError('`ladder` and `chroma_ladder` must be `ratecontrol.RateLadder`s.')
        # refused in front of every allocation
        for options in (batch_codec_options, chroma_options or {}):
            if 'budget_bytes' in options:
                raise ValueError('`ColourQualityCodec` does not take `budget_bytes`: a byte budget under a quality floor is out of scope.')
            if options.get('coding_tile') is not None:
                raise ValueError('`ColourQualityCodec` does not take `coding_tile`: the plane blobs are those of whole maps (EAE1).')
            if options.get('rdo_lambda') is not None:
                raise ValueError('`ColourQualityCodec` does not take `rdo_lambda`: the price of a bit comes with the ladder '
                                 '(`ratecontrol.RateLadder(..., rdo_lambda=...)`).')
            if 'thresholds_on_device' in options:
                raise ValueError('`thresholds_on_device` is not an option of ColourQualityCodec: its luminance codec runs with it.')
        if chroma_ladder.nb_points != ladder.nb_points:
            raise ValueError('`ladder` and `chroma_ladder` hold {0} and {1} rate points: the same number is needed.'.format(
                ladder.nb_points, chroma_ladder.nb_points))
        if chroma_ladder.truncated_unary_length != ladder.truncated_unary_length:
            raise ValueError('`ladder` and `chroma_ladder` have truncated unary lengths {0} and {1}: the same is needed.'.format(
                ladder.truncated_unary_length, chroma_ladder.truncated_unary_length))
        ratecontrol.colour_chroma_max_sse(0, chroma_share)             # refuses a share outside ]0, 1[
        self.chroma_share = float(chroma_share)
        (self.ladder, self.chroma_ladder) = (ladder, chroma_ladder)
        self.batch_size = container_format._positive_int(batch_size, '`batch_size`')
        self._nb_samples = ratecontrol.colour_nb_samples(container_format._positive_int(h, '`h`'), container_format._positive_int(w, '`w`'))
        self._default_max_sse = self._max_sse_of(target_psnr, max_sse)
        self._submitting = None
        self._build(batch_size, h, w, chroma_options, batch_codec_options,
                    lambda is_chroma, height, width, **options: _PlaneQualityCodec(
                        variables, are_bin_widths_learned, chroma_ladder if is_chroma else ladder, self.batch_size, height, width, pad=True,
                        keep_reconstruction=True, thresholds_on_device=not is_chroma, **options))
        self.emit_container = True

    def _max_sse_of(self, target_psnr, max_sse):
        """The thresholds of a step as int64 (batch_size,), from one of the two ways to name them; None when neither is given."""
        from . import ratecontrol
        if target_psnr is not None and max_sse is not None:
            raise ValueError('give `target_psnr` or `max_sse`, not both.')
        if target_psnr is not None:
            targets = numpy.asarray(target_psnr, dtype=numpy.float64)
            if targets.ndim > 1 or (targets.ndim == 1 and targets.shape[0] != self.batch_size):
                raise ValueError('`target_psnr` must be a number or one number per picture.')
            max_sse = ratecontrol.max_sse_for_psnr(targets, self._nb_samples)
        if max_sse is None:
            return None
        thresholds = ratecontrol._colour_max_sse(max_sse)              # refuses what is no integer in [0, 2^62]
        if numpy.ndim(max_sse) == 1 and thresholds.shape[0] != self.batch_size:
            raise ValueError('`max_sse` must be an integer or one integer per picture.')
        return numpy.ascontiguousarray(numpy.broadcast_to(thresholds, (self.batch_size,)))

    def submit(self, rgb_uint8, target_psnr=None, max_sse=None):
        """`ColourCodec.submit` with the step's thresholds: `target_psnr` (dB over the picture's S samples) or `max_sse` (the largest
        sse_Y + sse_Cb + sse_Cr), a scalar or one value per picture; neither: the constructor's."""
        from . import ratecontrol
        if target_psnr is None and max_sse is None:
            thresholds = self._default_max_sse
            if thresholds is None:
                raise ValueError('neither `target_psnr` nor `max_sse`, and the codec was built without a default.')
        else:
            thresholds = self._max_sse_of(target_psnr, max_sse)
        self._submitting = (thresholds, ratecontrol.colour_chroma_max_sse(thresholds, self.chroma_share))
        try:
            return super(ColourQualityCodec, self).submit(rgb_uint8)
        finally:
            self._submitting = None

    def _submit_planes(self, step):
        (thresholds, chroma_thresholds) = self._submitting
        # the entry is this step's: `submit` has waited for the merge of the step that used it last, which lies behind that step's
        # `colour_quality_rest` and luminance search
        step.max_sse_host[:] = thresholds
        step.max_sse.copy_(step.pinned_max_sse, non_blocking=True)
        n = self.batch_size
        chroma_slots = []
        chroma_tickets = []
        for plane in step.planes[1:]:
            chroma_slots.append(self.chroma._slots[self.chroma._index % self.chroma.nb_slots])     # the slot this inner step takes (`BatchCodec._submit`)
            chroma_tickets.append(self.chroma.submit(plane, max_sse=chroma_thresholds))
        caller = torch.cuda.current_stream()
        for inner in chroma_tickets:
            caller.wait_event(inner.decoded_event)
        (of_cb, of_cr) = chroma_slots
        dev.colour_quality_rest(step.max_sse, of_cb.pinned_sse[:n], of_cr.pinned_sse[:n], step.luma_max_sse)
        luma_ticket = self.luma.submit(step.planes[0], max_sse=step.luma_max_sse)
        return (luma_ticket,) + tuple(chroma_tickets)

    def _enqueue(self, step, rgb_uint8, host):
        ticket = super(ColourQualityCodec, self)._enqueue(step, rgb_uint8, host)
        ticket._picture_max_sse = self._submitting[0].copy()
        return ticket


# ---- colour pictures out of EAC1 containers, resident and pipelined --------------------------------------------

class ColourDecodeTicket(object):
    """Handle on one submitted `ColourDecoder` step: the three plane tickets (`tickets`: Y, Cb, Cr), `nb_images`, and `merged_event`,
    recorded behind the merge: wait for it on another stream before reading the device result there."""

    def __init__(self, tickets, step, image_size):
        self.nb_images = tickets[0].nb_images
        self.tickets = tuple(tickets)
        self.merged_event = None
        self.errors = None                    # after result(): per picture, None or the first error among its Y, Cb and Cr planes
        self._step = step
        self._image_size = image_size
        self._value = None

    def result(self, raise_errors=True):
        """Blocks until the three planes and the merge are through; uint8 (nb_images, h, w, 3): a numpy view of the colour slot's pinned
        buffer (`fetch_reconstruction=True`) or the device tensor, valid until the colour slot comes round `ColourDecoder.depth`
        submits later. Raises the first picture's error unless `raise_errors` is False: `errors` then says which pictures of the
        array to leave alone. Only waits: everything was enqueued by `submit`."""
        if self.errors is None:
            for ticket in self.tickets:
                ticket.result(raise_errors=False)
            self.merged_event.synchronize()
            self.errors = [next((ticket.errors[i] for ticket in self.tickets if ticket.errors[i] is not None), None)
                           for i in range(self.nb_images)]
            (h, w) = self._image_size
            buffer = self._step.host if self._step.host is not None else self._step.device
            self._value = buffer[:self.nb_images*h*w*3].reshape(self.nb_images, h, w, 3)
        if raise_errors:
            for error in self.errors:
                if error is not None:
                    raise error
        return self._value


class _ColourDecodeStep(object):
    """What one colour step in flight owns beside the inner decoders' slots: the buffer its merge writes, whole 16-byte words of it
    (`device.colour_merge_420_words`), pinned or on the device; `ColourDecoder` goes round `depth` of them."""

    def __init__(self, decoder):
        nbytes = dev.colour_words_bytes(decoder.batch_size, decoder.h, decoder.w)
        (self.pinned, self.host, self.device) = (None, None, None)
        if decoder.fetch_reconstruction:
            self.pinned = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
            self.host = self.pinned.numpy()
        else:
            self.device = torch.zeros(nbytes, dtype=torch.uint8, device=decoder.device)
        self.merged = None                    # the event behind the last merge that used this entry


class ColourDecoder(object):
    """`EAC1` containers -> uint8 RGB pictures (n, h, w, 3), resident and pipelined: what `container.decode_colour_images` computes
    (same bytes), the mirror of `ColourCodec`. Two unmodified `BatchDecoder(pad=True, keep_reconstruction=True,
    fetch_reconstruction=False)` of batch size `batch_size` -- `luma` at (h, w), `chroma` at (hc, wc) = ceil(h/2) x ceil(w/2) -- and,
    on a stream of this decoder's own behind the three tickets' `decoded_event`s, ONE `device.colour_merge_420_words` launch over the
    step's pictures, straight into the colour slot's pinned buffer (`fetch_reconstruction`) or into its device buffer; both hold
    `batch_size` pictures rounded up to 16 bytes. `merged_event` is recorded behind it.

    A colour step is one step of `luma` and two consecutive steps of `chroma`, Cb then Cr. The ring rule is `ColourCodec`'s, for the
    same reason: the inner decoders free a slot against their own worker, not against a merge on another stream, so the inner rings
    hold depth = min(luma.nb_slots, chroma.nb_slots // 2) colour steps, `submit` of step i first waits on the host for the merge event
    of step i - depth, and the colour ring is `depth` long. A depth of 0 is refused. A `submit` that raises half way drains both
    inner decoders and the merge stream before it re-raises.

    chroma_options: `nb_in_flight`, `nb_streams`, `payload_capacity_bytes`, `truncated_unary_length` of the chroma decoder, where they
    differ from the luminance decoder's. `coding_tile` goes to both and each clamps it to its own latent plane, as
    `container.encode_colour_images(coding_tile=...)` writes them. Unless given, chroma's `nb_in_flight` is 2 * `luma.nb_in_flight`,
    and the two decoders share what `stream_budget` leaves this process after one stream for the merge (4 + 4 streams at 16 hardware
    queues, 1 + 1 at 4), quietly, since nobody asked; numbers the caller gives are capped, and warned about, by `BatchDecoder`."""
    CHROMA_OPTIONS = ('nb_in_flight', 'nb_streams', 'payload_capacity_bytes', 'truncated_unary_length')

    def __init__(self, variables, are_bin_widths_learned, batch_size, h, w, truncated_unary_length, device='cuda', nb_in_flight=None,
                 nb_streams=None, use_graphs=False, payload_capacity_bytes=None, fetch_reconstruction=True, coding_tile=None,
                 chroma_options=None):
        (self.luma, self.chroma, self._merge_stream, self._closed) = (None, None, None, False)
        chroma_options = dict(chroma_options or {})
        for name in chroma_options:
            if name not in self.CHROMA_OPTIONS:
                raise ValueError('`{0}` is not an option of the chroma decoder alone: `chroma_options` takes {1}.'.format(
                    name, ', '.join(self.CHROMA_OPTIONS)))
        self.batch_size = container_format._positive_int(batch_size, '`batch_size`')
        (self.h, self.w) = (container_format._positive_int(h, '`h`'), container_format._positive_int(w, '`w`'))
        (self.hc, self.wc) = dev.chroma_size(self.h, self.w)
        self.fetch_reconstruction = bool(fetch_reconstruction)
        for_luma = {'nb_in_flight': nb_in_flight, 'nb_streams': nb_streams, 'payload_capacity_bytes': payload_capacity_bytes}
        for_chroma = dict(for_luma, nb_in_flight=None)      # chroma's slots follow the luminance decoder's unless given
        for_chroma.update({name: value for (name, value) in chroma_options.items() if name != 'truncated_unary_length'})
        if os.environ.get('EAE_IGNORE_HW_QUEUES') != '1':
            # one stream is the merge's; the two decoders share the rest
            (luma_streams, chroma_streams, _) = stream_budget(DECODER_STREAMS, DECODER_STREAMS, copies=1)
            if for_luma['nb_streams'] is None:
                for_luma['nb_streams'] = luma_streams
            if for_chroma['nb_streams'] is None:
                for_chroma['nb_streams'] = chroma_streams
        shared = {'device': device, 'use_graphs': use_graphs, 'fetch_reconstruction': False, 'coding_tile': coding_tile, 'pad': True,
                  'keep_reconstruction': True}
        try:
            self.luma = BatchDecoder(variables, are_bin_widths_learned, self.batch_size, self.h, self.w, truncated_unary_length,
                                     **shared, **for_luma)
            if for_chroma['nb_in_flight'] is None:
                for_chroma['nb_in_flight'] = 2*self.luma.nb_in_flight      # two inner steps per colour step
            self.chroma = BatchDecoder(variables, are_bin_widths_learned, self.batch_size, self.hc, self.wc,
                                       chroma_options.get('truncated_unary_length', truncated_unary_length), **shared, **for_chroma)
            self.device = self.luma.device
            self.depth = min(self.luma.nb_slots, self.chroma.nb_slots//2)
            if self.depth < 1:
                raise ValueError('the chroma decoder has {0} slot(s): it cannot hold the two steps (Cb, Cr) of one colour step.'.format(
                    self.chroma.nb_slots))
            self._steps = [_ColourDecodeStep(self) for _ in range(self.depth)]
            self._merge_stream = torch.cuda.Stream(device=self.device)
            self._index = 0
        except BaseException:
            self.close()
            raise

    def submit(self, blobs):
        """One `EAC1` blob of 1..batch_size pictures, or a sequence of `EAC1` blobs holding that many in all -> ColourDecodeTicket.
        The blobs are split and checked on the host first (`container.split_colour_blob`, then the decoder's own size and batch:
        ValueError, nothing launched; the inner `plan_decode_step` refuses what does not fit its decoder); then everything is enqueued,
        and the host waits only for free inner slots and for the merge of the step `depth` submits ago."""
        if self._closed:
            raise RuntimeError('this decoder is closed')
        if isinstance(blobs, (bytes, bytearray, memoryview)):
            blobs = [blobs]
        blobs = list(blobs)
        if not blobs:
            raise ValueError('A step needs at least one blob.')
        planes = ([], [], [])
        nb_images = 0
        for blob in blobs:
            (header, *plane_blobs) = container_format.split_colour_blob(blob)
            if (header['image_height'], header['image_width']) != (self.h, self.w):
                raise ValueError('The colour container holds {0} x {1} pictures, the decoder was built for {2} x {3}.'.format(
                    header['image_height'], header['image_width'], self.h, self.w))
            nb_images += header['nb_images']
            for (plane, plane_blob) in zip(planes, plane_blobs):
                plane.append(plane_blob)
        if nb_images > self.batch_size:
            raise ValueError('The blobs hold {0} pictures, the decoder takes {1} per step.'.format(nb_images, self.batch_size))
        step = self._steps[self._index % self.depth]
        self._index += 1
        if step.merged is not None:
            # the merge that wrote this entry, and read the inner reconstructions that come round with this step, is through
            step.merged.synchronize()
        try:
            return self._enqueue(step, planes)
        except BaseException:
            # part of the step may be enqueued (an inner submit raised): wait for all of it, so that the next step finds idle rings
            step.merged = None
            try:
                self.drain()
            except Exception:                 # the device itself is in trouble: the next submit will say so
                pass
            raise

    def _enqueue(self, step, planes):
        """The launches of one colour step on ring entry `step` (class docstring) -> its ticket."""
        tickets = (self.luma.submit(planes[0]), self.chroma.submit(planes[1]), self.chroma.submit(planes[2]))
        ticket = ColourDecodeTicket(tickets, step, (self.h, self.w))
        with torch.cuda.stream(self._merge_stream):
            for inner in tickets:
                self._merge_stream.wait_event(inner.decoded_event)
            dev.colour_merge_420_words(*(inner.reconstruction_uint8 for inner in tickets), (self.h, self.w),
                                       out=step.pinned if step.pinned is not None else step.device)
            step.merged = torch.cuda.Event()
            step.merged.record()
        ticket.merged_event = step.merged
        return ticket

    def drain(self):
        """Waits until every submitted step is through, the merges included."""
        for inner in (self.luma, self.chroma):
            if inner is not None:
                inner.drain()
        if self._merge_stream is not None:
            self._merge_stream.synchronize()

    def close(self):
        """Waits for the pending steps and closes both inner decoders. Idempotent."""
        self._closed = True
        try:
            self.drain()
        finally:
            for inner in (self.luma, self.chroma):
                if inner is not None:
                    inner.close()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, traceback):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: nothing left to report to
            pass


# ---- crops of colour pictures out of tile-indexed EAC1 containers, resident and pipelined ------------------------

class ColourRegionSource(object):
    """An `EAC1` container a `ColourRegionDecoder` cuts RGB crops out of: a bytes-like blob or a seekable binary file object. The
    48-byte header and the three plane headers are parsed and checked ONCE, here (of a file nothing else is read: every plane is read
    in place through a view of its byte range); what stays is `header` (`container.read_colour_header`), `nb_images`, `image_height`,
    `image_width` and `planes`: the three `RegionSource(..., pad=True)` of Y, Cb and Cr."""

    def __init__(self, source):
        (self.header, plane_sources) = container_format.colour_source(source)
        self.planes = tuple(RegionSource(plane, pad=True) for plane in plane_sources)
        container_format.check_colour_planes(self.header, [plane.header for plane in self.planes])
        (self.nb_images, self.image_height, self.image_width) = (self.header['nb_images'], self.header['image_height'],
                                                                 self.header['image_width'])


class ColourRegionTicket(object):
    """Handle on one submitted `ColourRegionDecoder` step: the three plane tickets (`tickets`: Y, Cb, Cr), `nb_images` (the crops of the
    step), and `merged_event`, recorded behind the merge: wait for it on another stream before reading the device result there."""

    def __init__(self, tickets, step, region):
        self.nb_images = tickets[0].nb_images
        self.tickets = tuple(tickets)
        self.merged_event = None
        self.errors = None                    # after result(): per crop, None or the first error among its Y, Cb and Cr planes
        self._step = step
        self._region = region
        self._value = None

    def result(self, raise_errors=True):
        """Blocks until the three planes and the merge are through; uint8 (nb_images, rh, rw, 3): a numpy view of the colour slot's
        pinned buffer (`fetch_reconstruction=True`) or the device tensor, valid until the colour slot comes round
        `ColourRegionDecoder.depth` submits later. Raises the first crop's error unless `raise_errors` is False: `errors` then says
        which crops of the array to leave alone. Only waits: everything was enqueued by `submit`."""
        if self.errors is None:
            for ticket in self.tickets:
                ticket.result(raise_errors=False)
            self.merged_event.synchronize()
            self.errors = [next((ticket.errors[i] for ticket in self.tickets if ticket.errors[i] is not None), None)
                           for i in range(self.nb_images)]
            (rh, rw) = self._region
            buffer = self._step.host if self._step.host is not None else self._step.device
            self._value = buffer[:self.nb_images*rh*rw*3].reshape(self.nb_images, rh, rw, 3)
        if raise_errors:
            for error in self.errors:
                if error is not None:
                    raise error
        return self._value


class _ColourRegionStep(object):
    """What one colour crop step in flight owns beside the inner decoders' slots: the pinned pixel origins of its crops, int32
    [batch][2], which the merge reads from memory, and the buffer the merge writes, whole 16-byte words of it
    (`device.colour_merge_420_crops`), pinned or on the device; `ColourRegionDecoder` goes round `depth` of them."""

    def __init__(self, decoder):
        nbytes = dev.colour_words_bytes(decoder.batch_size, *decoder.region)
        self.pinned_origins = torch.zeros((decoder.batch_size, 2), dtype=torch.int32).pin_memory()
        self.origins_host = self.pinned_origins.numpy()
        (self.pinned, self.host, self.device) = (None, None, None)
        if decoder.fetch_reconstruction:
            self.pinned = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
            self.host = self.pinned.numpy()
        else:
            self.device = torch.zeros(nbytes, dtype=torch.uint8, device=decoder.device)
        self.merged = None                    # the event behind the last merge that used this entry


class ColourRegionDecoder(object):
    """(ColourRegionSource, image, y0, x0) requests -> uint8 RGB crops (n, rh, rw, 3) of one fixed size, resident and pipelined: what
    `container.decode_colour_region(source, decoder, (y0, x0, rh, rw), images=[image])[0]` computes (same bytes). Built the way
    `ColourDecoder` is, around two `RegionDecoder(pad=True, keep_reconstruction=True, fetch_reconstruction=False)` of batch size
    `batch_size`: `luma` at (h, w) with `region`, `chroma` at (hc, wc) with the chroma rectangle `colour.chroma_region` gives every
    crop of that region, whose size does not depend on where the crop lies. A colour step is one step of `luma` and two consecutive
    steps of `chroma`, Cb then Cr, each at its crops' chroma origins; then, on a stream of this decoder's own behind the three
    tickets' `decoded_event`s, ONE `device.colour_merge_420_crops` launch, which reads the crops' pixel origins from the ring entry's
    pinned block and writes straight into its pinned buffer (`fetch_reconstruction`) or its device buffer. `merged_event` is
    recorded behind it. The merge is not captured into a graph; `use_graphs` is the inner decoders'.

    The ring rule, `chroma_options`, the stream budget and what a failing `submit` does are `ColourDecoder`'s:
    depth = min(luma.nb_slots, chroma.nb_slots // 2), `submit` of step i first waits for the merge of step i - depth."""
    CHROMA_OPTIONS = ColourDecoder.CHROMA_OPTIONS

    def __init__(self, variables, are_bin_widths_learned, batch_size, h, w, truncated_unary_length, coding_tile, region, device='cuda',
                 nb_in_flight=None, nb_streams=None, use_graphs=False, payload_capacity_bytes=None, fetch_reconstruction=True,
                 chroma_options=None):
        (self.luma, self.chroma, self._merge_stream, self._closed) = (None, None, None, False)
        chroma_options = dict(chroma_options or {})
        for name in chroma_options:
            if name not in self.CHROMA_OPTIONS:
                raise ValueError('`{0}` is not an option of the chroma decoder alone: `chroma_options` takes {1}.'.format(
                    name, ', '.join(self.CHROMA_OPTIONS)))
        self.batch_size = container_format._positive_int(batch_size, '`batch_size`')
        (self.h, self.w) = (container_format._positive_int(h, '`h`'), container_format._positive_int(w, '`w`'))
        (self.hc, self.wc) = dev.chroma_size(self.h, self.w)
        self.region = container_format._positive_pair(region, '`region`')
        if self.region[0] > self.h or self.region[1] > self.w:
            raise ValueError('`region` = {0} is larger than the {1} x {2} pictures.'.format(self.region, self.h, self.w))
        self.chroma_region = dev.chroma_region_size((self.h, self.w), self.region)
        self.fetch_reconstruction = bool(fetch_reconstruction)
        for_luma = {'nb_in_flight': nb_in_flight, 'nb_streams': nb_streams, 'payload_capacity_bytes': payload_capacity_bytes}
        for_chroma = dict(for_luma, nb_in_flight=None)      # chroma's slots follow the luminance decoder's unless given
        for_chroma.update({name: value for (name, value) in chroma_options.items() if name != 'truncated_unary_length'})
        if os.environ.get('EAE_IGNORE_HW_QUEUES') != '1':
            # one stream is the merge's; the two decoders share the rest
            (luma_streams, chroma_streams, _) = stream_budget(DECODER_STREAMS, DECODER_STREAMS, copies=1)
            if for_luma['nb_streams'] is None:
                for_luma['nb_streams'] = luma_streams
            if for_chroma['nb_streams'] is None:
                for_chroma['nb_streams'] = chroma_streams
        shared = {'device': device, 'use_graphs': use_graphs, 'fetch_reconstruction': False, 'pad': True, 'keep_reconstruction': True}
        try:
            self.luma = RegionDecoder(variables, are_bin_widths_learned, self.batch_size, self.h, self.w, truncated_unary_length,
                                      coding_tile, self.region, **shared, **for_luma)
            if for_chroma['nb_in_flight'] is None:
                for_chroma['nb_in_flight'] = 2*self.luma.nb_in_flight      # two inner steps per colour step
            self.chroma = RegionDecoder(variables, are_bin_widths_learned, self.batch_size, self.hc, self.wc,
                                        chroma_options.get('truncated_unary_length', truncated_unary_length), coding_tile,
                                        self.chroma_region, **shared, **for_chroma)
            self.device = self.luma.device
            self.depth = min(self.luma.nb_slots, self.chroma.nb_slots//2)
            if self.depth < 1:
                raise ValueError('the chroma decoder has {0} slot(s): it cannot hold the two steps (Cb, Cr) of one colour step.'.format(
                    self.chroma.nb_slots))
            self._steps = [_ColourRegionStep(self) for _ in range(self.depth)]
            self._merge_stream = torch.cuda.Stream(device=self.device)
            self._index = 0
        except BaseException:
            self.close()
            raise

    def _plan(self, requests):
        """The host checks of a step -> (pixel origins int32 [n][2], the requests of the Y, Cb and Cr steps). Raises ValueError for
        what the headers of the sources alone refuse; nothing is read, written or launched."""
        requests = list(requests)
        if not requests:
            raise ValueError('A step needs at least one request.')
        if len(requests) > self.batch_size:
            raise ValueError('{0} requests, a step of this decoder takes {1} at most.'.format(len(requests), self.batch_size))
        origins = numpy.zeros((len(requests), 2), dtype=numpy.int32)
        planes = ([], [], [])
        for (k, request) in enumerate(requests):
            if not isinstance(request, (tuple, list)) or len(request) != 4 or not isinstance(request[0], ColourRegionSource):
                raise ValueError('A request is (ColourRegionSource, image, y0, x0).')
            (source, image, y0, x0) = request
            for x in (image, y0, x0):
                if isinstance(x, bool) or not isinstance(x, (int, numpy.integer)):
                    raise ValueError('A request is (ColourRegionSource, image, y0, x0) in integers.')
            (image, y0, x0) = (int(image), int(y0), int(x0))
            if (source.image_height, source.image_width) != (self.h, self.w):
                raise ValueError('The source holds {0} x {1} pictures, the decoder was built for {2} x {3}.'.format(
                    source.image_height, source.image_width, self.h, self.w))
            if not 0 <= image < source.nb_images:
                raise ValueError('The source holds {0} pictures: there is no picture {1}.'.format(source.nb_images, image))
            if y0 < 0 or x0 < 0 or y0 + self.region[0] > self.h or x0 + self.region[1] > self.w:
                raise ValueError('The region {0} leaves the {1} x {2} picture.'.format((y0, x0) + self.region, self.h, self.w))
            (_, (cy0, cx0)) = colour_rules.chroma_region(self.h, self.w, self.region, y0, x0)
            origins[k] = (y0, x0)
            for (plane, inner, at, requests_of_plane) in zip(source.planes, (self.luma, self.chroma, self.chroma),
                                                             ((y0, x0), (cy0, cx0), (cy0, cx0)), planes):
                _refuse_region_request(plane, image, at[0], at[1], inner._layout, inner.region, inner.truncated_unary_length, inner.learned,
                                       inner.image_size)
                requests_of_plane.append((plane, image, at[0], at[1]))
        return origins, planes

    def submit(self, requests):
        """1..batch_size requests (ColourRegionSource, image, y0, x0), the sources the same or not -> ColourRegionTicket, whose
        `result()` is uint8 (n, rh, rw, 3), crop k the pixels [y0, y0 + rh) x [x0, x0 + rw) of its picture. Everything the headers
        say is checked on the host first (ValueError, nothing launched; a payload beyond an inner decoder's capacity is refused by that
        decoder's own plan, and `submit` then drains before it re-raises); then everything is enqueued, and the host waits only for
        free inner slots and for the merge of the step `depth` submits ago."""
        if self._closed:
            raise RuntimeError('this decoder is closed')
        (origins, planes) = self._plan(requests)
        step = self._steps[self._index % self.depth]
        self._index += 1
        if step.merged is not None:
            # the merge that wrote this entry, read its origins and the inner crops that come round with this step, is through
            step.merged.synchronize()
        try:
            return self._enqueue(step, origins, planes)
        except BaseException:
            # part of the step may be enqueued (an inner submit raised): wait for all of it, so that the next step finds idle rings
            step.merged = None
            try:
                self.drain()
            except Exception:                 # the device itself is in trouble: the next submit will say so
                pass
            raise

    def _enqueue(self, step, origins, planes):
        """The launches of one colour step on ring entry `step` (class docstring) -> its ticket."""
        n = len(origins)
        step.origins_host[:n] = origins
        tickets = (self.luma.submit(planes[0]), self.chroma.submit(planes[1]), self.chroma.submit(planes[2]))
        ticket = ColourRegionTicket(tickets, step, self.region)
        with torch.cuda.stream(self._merge_stream):
            for inner in tickets:
                self._merge_stream.wait_event(inner.decoded_event)
            dev.colour_merge_420_crops(*(inner.reconstruction_uint8 for inner in tickets), (self.h, self.w), step.pinned_origins[:n],
                                       out=step.pinned if step.pinned is not None else step.device)
            step.merged = torch.cuda.Event()
            step.merged.record()
        ticket.merged_event = step.merged
        return ticket

    (drain, close) = (ColourDecoder.drain, ColourDecoder.close)          # the same two inner decoders and merge stream

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, traceback):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: nothing left to report to
            pass
