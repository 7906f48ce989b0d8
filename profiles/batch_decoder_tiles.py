#!/usr/bin/env python
"""What `codec.BatchDecoder(coding_tile=...)` gives (profiles/batch_decoder_tiles.md): against
`container.decode_images` on the same `EAT1` blobs, and against the untiled `BatchDecoder` on `EAE1` blobs of the same images.

24 Kodak-sized synthetic images per step (bench.py's images, model and statistics), per bin width and per coding tile; the `EAT1`
blobs come from `codec.BatchCodec(emit_container=True, coding_tile=...)`, the `EAE1` blobs from the same codec without a tile: the
step's blob and its 24 single-image blobs each. In ONE process, in alternating blocks, per decoder (untiled, and one per tile):
24 images per step pipelined, one image per step pipelined, one image per step submit -> result; per tile also a loop of
`decode_images` on the 24-image `EAT1` blob and one image by image. Every leg compares what it decoded with the codec's
reconstruction. Per block the wall time and the process CPU time per step; medians are of the blocks, with the smallest and the
largest beside them. One JSON line per measurement on stdout; the tables go to profiles/batch_decoder_tiles.md.

    python profiles/batch_decoder_tiles.py [--blocks 5] [--steps 20] [--bin-widths 1.0 0.05] [--tiles 16 8]
"""
import argparse
import gc
import json
import os
import sys

import numpy
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for path in (ROOT, HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

import batch_decoder as base  # noqa: E402
import bench  # noqa: E402
import autoencoder_based_image_compression_amd as package  # noqa: E402
from autoencoder_based_image_compression_amd import codec, container, pipeline  # noqa: E402
from autoencoder_based_image_compression_amd import device as dev  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats  # noqa: E402


def make_blobs(variables, bin_widths, map_mean, probabilities, images, batch, h, w, tile):
    with codec.BatchCodec(variables, False, bin_widths, map_mean, probabilities, bench.IDX_MAP_EXCEPTION, batch, h, w, emit_container=True,
                          keep_reconstruction=True, container_capacity_bytes=2*batch*h*w, coding_tile=tile, **codec.product_mode(h, w)) as c:
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
    parser.add_argument('--tiles', type=int, nargs='+', default=[16, 8])
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'batch_decoder_tiles.md'))
    args = parser.parse_args()
    (batch, h, w, steps) = (args.batch, args.height, args.width, args.steps)
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    images = torch.from_numpy(bench.synthetic_images(1000, batch, h, w)).to(device)
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
        model = pipeline.DeviceDecoder(variables, False, device)
        capacity = 2*pixels
        (legs, decoders, payload_bits) = ({}, [], {})

        def add(name, tile, blob, image_blobs, reconstruction):
            """The three `BatchDecoder` legs of one decoder kind (tile None: the untiled decoder on `EAE1`), and with a tile the two
            `decode_images` loops on the same blobs."""
            def build(n):
                return codec.BatchDecoder(variables, False, n, h, w, length, device=device, payload_capacity_bytes=capacity*n//batch,
                                          use_graphs=True, coding_tile=tile)

            def whole(k):
                return reconstruction

            def one(k):
                return reconstruction[k % batch:k % batch + 1]

            (full, single) = (build(batch), build(1))
            decoders.extend([full, single])
            assert numpy.array_equal(container.decode_images(blob, model), reconstruction)
            assert numpy.array_equal(full.submit(blob).result(), reconstruction)
            assert numpy.array_equal(single.submit(image_blobs[3]).result(), reconstruction[3:4])
            payload_bits[name] = round(8.*(len(blob) - container.read_header(blob)['payload_offset'])/pixels, 4)
            legs[(name, '{0} per step, pipelined'.format(batch))] = (batch, lambda: base.pipelined(full, [blob], steps, whole))
            legs[(name, '1 per step, pipelined')] = (1, lambda: base.pipelined(single, image_blobs, 4*steps, one))
            legs[(name, '1 per step, submit -> result')] = (1, lambda: base.one_at_a_time(single, image_blobs, 2*steps, one))
            if tile is not None:
                legs[(name, 'decode_images, {0} per call'.format(batch))] = (batch, lambda: base.decode_images_loop([blob], model, 2, whole))
                legs[(name, 'decode_images, 1 per call')] = (1, lambda: base.decode_images_loop(image_blobs, model, 8, one))
            return full

        first = add('EAE1, untiled', None, *make_blobs(variables, bin_widths, map_mean, probabilities, images, batch, h, w, None))
        for t in args.tiles:
            add('EAT1, tile {0}'.format(t), (t, t), *make_blobs(variables, bin_widths, map_mean, probabilities, images, batch, h, w, (t, t)))
        for (key, (_, fn)) in legs.items():          # warm-up: graphs captured, lazy loads done
            print('warm-up: {0}, {1}'.format(*key), file=sys.stderr, flush=True)
            fn()
        measured = {key: {'ms': [], 'cpu': []} for key in legs}
        gc.collect()
        gc.disable()
        try:
            for _ in range(args.blocks):
                for (key, (_, fn)) in legs.items():          # alternating: every leg sees the same box at the same time
                    (ms, cpu) = fn()
                    measured[key]['ms'].append(ms)
                    measured[key]['cpu'].append(cpu)
        finally:
            gc.enable()
        for ((name, leg), m) in measured.items():
            n = legs[(name, leg)][0]
            emit({'blobs': name, 'leg': leg, 'bin_width': bin_width, 'images_per_step': n, 'height': h, 'width': w, 'blocks': args.blocks,
                  'payload_bits_per_pixel': payload_bits[name], 'nb_streams': first.nb_streams, 'nb_in_flight': first.nb_in_flight,
                  'ms_per_step': base.summary(m['ms']), 'process_cpu_ms_per_step': base.summary(m['cpu'])})
        for decoder in decoders:
            decoder.close()
        del model, decoders, legs
        torch.cuda.empty_cache()
    write_report(args.output, lines, args)


def write_report(path, lines, args):
    def cell(s):
        return '{0} ({1} .. {2})'.format(s['median'], s['min'], s['max'])

    out = ['# `codec.BatchDecoder(coding_tile=...)` against `container.decode_images` and the untiled `BatchDecoder`', '',
           'Written by `profiles/batch_decoder_tiles.py` ({0} blocks per leg, alternating in one process; median (min .. max) of the blocks). '
           '{1} images of {2}x{3}, blobs from `codec.BatchCodec(emit_container=True[, coding_tile=...])`; every leg compares what it decoded with '
           'the codec\'s reconstruction. {4} hardware queues (GPU_MAX_HW_QUEUES, set by: {5}).'.format(
               args.blocks, args.batch, args.height, args.width, package.HW_QUEUES[0], package.HW_QUEUES[1]), '']
    for bin_width in args.bin_widths:
        rows = [line for line in lines if line['bin_width'] == bin_width]
        if not rows:
            continue
        out += ['## bin width {0}'.format(bin_width), '',
                '`BatchDecoder` legs: {0} streams, {1} steps in flight, graphs on.'.format(rows[0]['nb_streams'], rows[0]['nb_in_flight']), '',
                '| blobs | payload bits per pixel | leg | ms per step | host CPU ms per step |', '|---|---|---|---|---|']
        for line in rows:
            out.append('| {0} | {1} | {2} | {3} | {4} |'.format(line['blobs'], line['payload_bits_per_pixel'], line['leg'], cell(line['ms_per_step']),
                                                              cell(line['process_cpu_ms_per_step'])))
        out.append('')
        median = {(line['blobs'], line['leg']): line['ms_per_step']['median'] for line in rows}
        for name in sorted({line['blobs'] for line in rows if line['blobs'] != 'EAE1, untiled'}):
            parts = []
            for leg in sorted({leg for (blobs, leg) in median if blobs == 'EAE1, untiled'}):
                parts.append('{0}: {1:.2f}x the untiled decoder\'s time'.format(leg, median[(name, leg)]/median[('EAE1, untiled', leg)]))
            batch_leg = '{0} per step, pipelined'.format(args.batch)
            parts.append('`decode_images` per call / per step: {0:.1f}x for {1} images, {2:.1f}x for one image pipelined, {3:.1f}x submit -> result'.format(
                median[(name, 'decode_images, {0} per call'.format(args.batch))]/median[(name, batch_leg)],
                args.batch, median[(name, 'decode_images, 1 per call')]/median[(name, '1 per step, pipelined')],
                median[(name, 'decode_images, 1 per call')]/median[(name, '1 per step, submit -> result')]))
            out += ['{0} (medians): {1}.'.format(name, '; '.join(parts)), '']
    with open(path, 'w') as f:
        f.write('\n'.join(out))


if __name__ == '__main__':
    main()
