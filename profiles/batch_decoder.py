#!/usr/bin/env python
"""What `codec.BatchDecoder` gives over `container.decode_images` (profiles/batch_decoder.md).

24 Kodak-sized synthetic images per step (bench.py's images, model and statistics), per bin width; the blobs come from
`codec.BatchCodec(emit_container=True)`: the step's blob and its 24 single-image blobs. In ONE process, in alternating blocks:
`BatchDecoder` at its defaults with graphs (24 images per step, pipelined), a loop of `decode_images` on the 24-image blob, a loop of
`decode_images` image by image, `BatchDecoder` with one image per step (pipelined, and submit -> result one at a time). Per block
the wall time and the process CPU time per step; medians are of the blocks, with the smallest and the largest beside them. Then
the sweep that the defaults come from: `nb_streams` 1..4, graphs on and off, for both batch sizes. One JSON line per measurement
on stdout; the tables go to profiles/batch_decoder.md.

    python profiles/batch_decoder.py [--blocks 5] [--steps 20] [--bin-widths 1.0 0.05] [--no-sweep]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
import autoencoder_based_image_compression_amd as package  # noqa: E402
from autoencoder_based_image_compression_amd import codec, container, pipeline  # noqa: E402
from autoencoder_based_image_compression_amd import device as dev  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats  # noqa: E402


def summary(values):
    ordered = sorted(values)
    return {'median': round(ordered[(len(ordered) - 1)//2], 4), 'min': round(ordered[0], 4), 'max': round(ordered[-1], 4)}


def timed(fn, count):
    """-> (wall ms, process CPU ms) per unit of `count`."""
    torch.cuda.synchronize()
    (t0, c0) = (time.perf_counter(), time.process_time())
    fn()
    return (time.perf_counter() - t0)/count*1e3, (time.process_time() - c0)/count*1e3


def stop_on_errors(tickets):
    """A run in which a step failed measures nothing: say which step, which images, which exception, and stop."""
    failed = []
    for (step, ticket) in enumerate(tickets):
        if ticket._error is not None:          # the step's own failure (copied into every entry of `errors`)
            failed.append('step {0}: the whole step: {1}: {2}'.format(step, type(ticket._error).__name__, ticket._error))
            continue
        for (image, error) in enumerate(ticket.errors or ()):
            if error is not None:
                failed.append('step {0}, image {1}: {2}: {3}'.format(step, image, type(error).__name__, error))
    if failed:
        raise SystemExit('BatchDecoder reported errors on valid blobs ({0} in {1} steps):\n  '.format(len(failed), len(tickets))
                         + '\n  '.join(failed[:40]))


def pipelined(decoder, blobs, steps, expected=None):
    """expected(k): what step k must decode to; the LAST step's result is compared (it is still valid behind the drain)."""
    kept = []

    def run():
        tickets = [decoder.submit(blobs[k % len(blobs)]) for k in range(steps)]
        decoder.drain()
        kept.extend(tickets)
    out = timed(run, steps)
    stop_on_errors(kept)
    if expected is not None and not numpy.array_equal(kept[-1].result(), expected(steps - 1)):
        raise SystemExit('BatchDecoder: the last step of a block does not decode to the codec\'s reconstruction')
    return out


def one_at_a_time(decoder, blobs, steps, expected):
    wrong = []

    def run():
        for k in range(steps):
            if not numpy.array_equal(decoder.submit(blobs[k % len(blobs)]).result(), expected(k)):
                wrong.append(k)
    out = timed(run, steps)
    if wrong:
        raise SystemExit('BatchDecoder, submit -> result: steps {0} do not decode to the codec\'s reconstruction'.format(wrong))
    return out


def decode_images_loop(blobs, decoder_model, count, expected):
    last = []

    def run():
        for k in range(count):
            last[:] = [container.decode_images(blobs[k % len(blobs)], decoder_model)]
    out = timed(run, count)
    if not numpy.array_equal(last[0], expected(count - 1)):
        raise SystemExit('decode_images: the last call of a block does not decode to the codec\'s reconstruction')
    return out


def make_blobs(variables, bin_widths, map_mean, probabilities, images, batch, h, w):
    with codec.BatchCodec(variables, False, bin_widths, map_mean, probabilities, bench.IDX_MAP_EXCEPTION, batch, h, w, emit_container=True,
                          keep_reconstruction=True, container_capacity_bytes=2*batch*h*w, **codec.product_mode(h, w)) as c:
        ticket = c.submit(images)
        ticket.result()
        return ticket.container(), ticket.image_containers(), ticket.reconstruction_uint8.cpu().numpy()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--blocks', type=int, default=5)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--batch', type=int, default=24)
    parser.add_argument('--height', type=int, default=512)
    parser.add_argument('--width', type=int, default=768)
    parser.add_argument('--bin-widths', type=float, nargs='+', default=[1.0, 0.05])
    parser.add_argument('--no-sweep', action='store_true')
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'batch_decoder.md'))
    args = parser.parse_args()
    (batch, h, w, steps) = (args.batch, args.height, args.width, args.steps)
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    images_host = bench.synthetic_images(1000, batch, h, w)
    images = torch.from_numpy(images_host).to(device)
    (pixels, length) = (batch*h*w, bench.TRUNCATED_UNARY_LENGTH)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for bin_width in args.bin_widths:
        variables = bench.synthetic_model(bin_width)
        bin_widths = variables[var.BIN_WIDTHS_NAME]
        encoder = pipeline.DeviceEncoder(variables, False, device)
        y0 = encoder(images)
        map_mean = dev.map_means(y0).cpu().numpy()
        probabilities = lossless_stats.compute_binary_probabilities(y0.cpu().numpy(), bin_widths, map_mean, length)
        del y0, encoder
        (blob, image_blobs, reconstruction) = make_blobs(variables, bin_widths, map_mean, probabilities, images, batch, h, w)
        payload = len(blob) - container.read_header(blob)['payload_offset']
        capacity = 2*pixels
        model = pipeline.DeviceDecoder(variables, False, device)
        assert numpy.array_equal(container.decode_images(blob, model), reconstruction)

        def build(n, **arguments):
            return codec.BatchDecoder(variables, False, n, h, w, length, device=device, payload_capacity_bytes=capacity*n//batch, **arguments)

        full = build(batch, use_graphs=True)
        single = build(1, use_graphs=True)
        assert numpy.array_equal(full.submit(blob).result(), reconstruction)
        assert numpy.array_equal(single.submit(image_blobs[3]).result(), reconstruction[3:4])
        def whole(k):
            return reconstruction

        def one(k):
            return reconstruction[k % batch:k % batch + 1]

        legs = {
            'BatchDecoder, batch per step, pipelined': (batch, lambda: pipelined(full, [blob], steps, whole)),
            'decode_images, batch per call': (batch, lambda: decode_images_loop([blob], model, 3, whole)),
            'BatchDecoder, 1 per step, pipelined': (1, lambda: pipelined(single, image_blobs, 4*steps, one)),
            'BatchDecoder, 1 per step, submit -> result': (1, lambda: one_at_a_time(single, image_blobs, 2*steps, one)),
            'decode_images, 1 per call': (1, lambda: decode_images_loop(image_blobs, model, batch, one)),
        }
        images_per_unit = {name: n for (name, (n, _)) in legs.items()}
        legs = {name: fn for (name, (_, fn)) in legs.items()}
        for fn in legs.values():          # warm-up: graphs captured, lazy loads done
            fn()
        measured = {name: {'ms': [], 'cpu': []} for name in legs}
        gc.collect()
        gc.disable()
        try:
            for _ in range(args.blocks):
                for (name, fn) in legs.items():          # alternating: every leg sees the same box at the same time
                    (ms, cpu) = fn()
                    measured[name]['ms'].append(ms)
                    measured[name]['cpu'].append(cpu)
        finally:
            gc.enable()
        for (name, m) in measured.items():
            n = images_per_unit[name]
            emit({'what': name, 'bin_width': bin_width, 'images_per_step': n, 'height': h, 'width': w, 'blocks': args.blocks,
                  'payload_bits_per_pixel': round(8.*payload/pixels, 4), 'nb_streams': full.nb_streams, 'nb_in_flight': full.nb_in_flight,
                  'ms_per_step': summary(m['ms']), 'Mpx_per_s': summary([n*h*w/(ms*1e-3)/1e6 for ms in m['ms']]),
                  'process_cpu_ms_per_step': summary(m['cpu'])})
        full.close()
        single.close()
        if not args.no_sweep:
            for n in (batch, 1):
                for graphs in (True, False):
                    for nb_streams in (1, 2, 3, 4):
                        decoder = build(n, use_graphs=graphs, nb_streams=nb_streams, nb_in_flight=nb_streams + 2)
                        if decoder.nb_streams != nb_streams:      # too few hardware queues: this row would measure another one
                            print('sweep: {0} streams asked for, {1} run: skipped (set GPU_MAX_HW_QUEUES=16)'.format(nb_streams, decoder.nb_streams), flush=True)
                            decoder.close()
                            continue
                        blobs = [blob] if n == batch else image_blobs
                        count = steps if n == batch else 4*steps
                        pipelined(decoder, blobs, count, whole if n == batch else one)
                        ms = [pipelined(decoder, blobs, count, whole if n == batch else one) for _ in range(args.blocks)]
                        emit({'what': 'sweep', 'bin_width': bin_width, 'images_per_step': n, 'use_graphs': graphs, 'nb_streams_asked': nb_streams,
                              'nb_streams': decoder.nb_streams, 'nb_in_flight': decoder.nb_in_flight,
                              'ms_per_step': summary([v[0] for v in ms]), 'process_cpu_ms_per_step': summary([v[1] for v in ms])})
                        decoder.close()
                        del decoder
        del model
        torch.cuda.empty_cache()
    write_report(args.output, lines, args)


def write_report(path, lines, args):
    def cell(s):
        return '{0} ({1} .. {2})'.format(s['median'], s['min'], s['max'])

    out = ['# `codec.BatchDecoder` against `container.decode_images`', '',
           'Written by `profiles/batch_decoder.py` ({0} blocks per leg, alternating in one process; median (min .. max) of the blocks). '
           '{1} images of {2}x{3} per step, blobs from `codec.BatchCodec(emit_container=True)`; {4} hardware queues (GPU_MAX_HW_QUEUES, set by: {5}).'.format(
               args.blocks, args.batch, args.height, args.width, package.HW_QUEUES[0], package.HW_QUEUES[1]), '']
    for bin_width in args.bin_widths:
        legs = [line for line in lines if line['bin_width'] == bin_width and line['what'] != 'sweep']
        if not legs:
            continue
        out += ['## bin width {0} ({1} payload bits per pixel)'.format(bin_width, legs[0]['payload_bits_per_pixel']), '',
                '`BatchDecoder` legs: {0} streams, {1} steps in flight, graphs on.'.format(legs[0]['nb_streams'], legs[0]['nb_in_flight']), '',
                '| leg | ms per step | Mpixel/s | host CPU ms per step |', '|---|---|---|---|']
        for line in legs:
            out.append('| {0} | {1} | {2} | {3} |'.format(line['what'], cell(line['ms_per_step']), cell(line['Mpx_per_s']), cell(line['process_cpu_ms_per_step'])))
        by_name = {line['what']: line['ms_per_step']['median'] for line in legs}
        out += ['', 'Factors (medians): a batch per step {0:.1f}x `decode_images` per call; one image per step pipelined {1:.1f}x and submit -> result '
                '{2:.1f}x `decode_images` image by image.'.format(
                    by_name['decode_images, batch per call']/by_name['BatchDecoder, batch per step, pipelined'],
                    by_name['decode_images, 1 per call']/by_name['BatchDecoder, 1 per step, pipelined'],
                    by_name['decode_images, 1 per call']/by_name['BatchDecoder, 1 per step, submit -> result']), '']
        sweep = [line for line in lines if line['bin_width'] == bin_width and line['what'] == 'sweep']
        if sweep:
            out += ['Sweep (pipelined, `nb_in_flight` = `nb_streams` + 2; ms per step, host CPU ms per step):', '',
                    '| images per step | graphs | streams asked | streams run | ms per step | host CPU ms per step |', '|---|---|---|---|---|---|']
            for line in sweep:
                out.append('| {0} | {1} | {2} | {3} | {4} | {5} |'.format(line['images_per_step'], 'on' if line['use_graphs'] else 'off', line['nb_streams_asked'],
                                                                     line['nb_streams'], cell(line['ms_per_step']), cell(line['process_cpu_ms_per_step'])))
            out.append('')
    with open(path, 'w') as f:
        f.write('\n'.join(out))


if __name__ == '__main__':
    main()
