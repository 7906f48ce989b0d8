#!/usr/bin/env python
"""What decoding colour pictures costs (profiles/colour_decoder.md): `--batch` RGB pictures at each of `--sizes`
(512 x 768 and 500 x 750 by default), bench.py's synthetic images in every channel, its model and statistics.

1. The merge kernels, device events, median (min .. max) of `--repeat` launches each: `device.colour_merge_420_words` against the
   untouched `device.colour_merge_420`, both writing the SAME destination, once in device memory and once in pinned host memory, and a
   copy of as many bytes as the picture has to the same destination. Old and new alternate, twice, so that neither has the machine
   to itself; both rounds are printed. The results are compared with `colour.merge_420_numpy` first.
2. The pipelined step, in ONE process, in alternating blocks: `ColourDecoder(use_graphs=True)` on one `EAC1` blob of the batch
   against its three inner steps submitted alone to two plain `BatchDecoder(pad=True, use_graphs=True)` with the streams and slots of
   the colour decoder's inner ones, and against `container.decode_colour_images` of the same blob; then one picture, submit to
   result, through a `ColourDecoder` of batch size 1 against `decode_colour_images` of its blob. At every `--bin-widths`.
One JSON line per measurement on stdout; the tables go to `--output`, in front of its section `## Notes`, which is written by hand and
which a rerun keeps as it finds it. The hardware queues are the process's (GPU_MAX_HW_QUEUES): run it once per setting, with an
`--output` of its own.

    python profiles/colour_decoder.py [--blocks 5] [--steps 20] [--batch 24] [--sizes 512x768 500x750] [--bin-widths 1.0 0.05]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for path in (ROOT, HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

import batch_decoder as base  # noqa: E402
import bench  # noqa: E402
import colour as colour_profile  # noqa: E402
import autoencoder_based_image_compression_amd as package  # noqa: E402
from autoencoder_based_image_compression_amd import codec, colour, container, pipeline  # noqa: E402
from autoencoder_based_image_compression_amd import device as dev  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats  # noqa: E402

NOTES_HEADING = '\n## Notes'


def event_times(fn, repeat):
    """Microseconds of `repeat` launches of `fn`, each between two events of its own -> {'median', 'min', 'max'}."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        (start, stop) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop)*1e3)
    ordered = sorted(times)
    return {'median': round(ordered[(len(ordered) - 1)//2], 2), 'min': round(ordered[0], 2), 'max': round(ordered[-1], 2)}


def kernel_legs(rgb, repeat, device):
    (n, h, w, _) = rgb.shape
    planes = dev.colour_split_420(torch.from_numpy(rgb).to(device))
    merged = colour.merge_420_numpy(*(plane.cpu().numpy() for plane in planes))
    (picture, room) = (n*h*w*3, dev.colour_words_bytes(n, h, w))
    source = torch.from_numpy(merged).to(device).reshape(-1)
    result = []
    for (place, flat) in (('device', torch.zeros(room, dtype=torch.uint8, device=device)), ('pinned', torch.zeros(room, dtype=torch.uint8).pin_memory())):
        shaped = flat[:picture].view(n, h, w, 3)
        for (name, fn) in (('colour_merge_420', lambda: dev.colour_merge_420(*planes, (h, w), out=shaped)),
                           ('colour_merge_420_words', lambda: dev.colour_merge_420_words(*planes, (h, w), flat))):
            flat.zero_()
            fn()
            torch.cuda.synchronize()
            if not numpy.array_equal((flat.cpu() if flat.is_cuda else flat).numpy()[:picture], merged.reshape(-1)):
                raise SystemExit('{0} into {1} memory is not colour.merge_420_numpy'.format(name, place))
        legs = (('colour_merge_420 (the existing kernel)', lambda: dev.colour_merge_420(*planes, (h, w), out=shaped)),
                ('colour_merge_420_words', lambda: dev.colour_merge_420_words(*planes, (h, w), flat)))
        for round_index in range(2):
            for (name, fn) in legs:
                result.append({'leg': name, 'destination': place, 'round': round_index, 'picture_bytes': picture, 'microseconds': event_times(fn, repeat)})
        result.append({'leg': 'copy of the picture\'s bytes from device memory', 'destination': place, 'round': 0, 'picture_bytes': picture,
                       'microseconds': event_times(lambda: flat[:picture].copy_(source, non_blocking=True), repeat)})
    return result


def blocks_of(legs, blocks):
    """legs {name: fn -> ms}: one warm-up call each, then `blocks` rounds over all of them -> {name: [ms]}."""
    for fn in legs.values():
        fn()
    measured = {name: [] for name in legs}
    gc.collect()
    gc.disable()
    try:
        for _ in range(blocks):
            for (name, fn) in legs.items():          # alternating: every leg sees the same machine at the same time
                measured[name].append(fn())
    finally:
        gc.enable()
    return measured


def step_legs(variables, bin_widths, rgb, args, device):
    """-> the JSON lines of one size at one bin width."""
    (n, h, w, _) = rgb.shape
    (hc, wc) = dev.chroma_size(h, w)
    length = bench.TRUNCATED_UNARY_LENGTH
    planes = colour.split_420_numpy(rgb)
    (H, W) = dev.coded_size(h, w)
    padded = numpy.pad(planes[0], ((0, 0), (0, H - h), (0, W - w)), mode='edge')
    encoder = pipeline.DeviceEncoder(variables, False, device)
    decoder = pipeline.DeviceDecoder(variables, False, device)
    y0 = encoder(torch.from_numpy(padded).to(device))
    map_mean = dev.map_means(y0).cpu().numpy()
    probabilities = lossless_stats.compute_binary_probabilities(y0.cpu().numpy(), bin_widths, map_mean, length)
    del y0
    point = (bin_widths, map_mean, probabilities, bench.IDX_MAP_EXCEPTION)
    (blob, _) = container.encode_colour_images(rgb, encoder, *point)
    (one, _) = container.encode_colour_images(rgb[:1], encoder, *point)
    expected = container.decode_colour_images(blob, decoder)
    plane_blobs = container.split_colour_blob(blob)[1:]
    lines = []
    with codec.ColourDecoder(variables, False, n, h, w, length, use_graphs=True) as d:
        if not numpy.array_equal(d.submit(blob).result(), expected):
            raise SystemExit('ColourDecoder is not decode_colour_images')
        inner = {'nb_streams': d.luma.nb_streams, 'use_graphs': True, 'pad': True}
        with codec.BatchDecoder(variables, False, n, h, w, length, nb_in_flight=d.luma.nb_in_flight, **inner) as luma, \
                codec.BatchDecoder(variables, False, n, hc, wc, length, nb_in_flight=d.chroma.nb_in_flight, **inner) as chroma:
            for ticket in (luma.submit(plane_blobs[0]), chroma.submit(plane_blobs[1]), chroma.submit(plane_blobs[2])):
                ticket.result()

            def colour_steps():
                kept = []

                def run():
                    kept.extend(d.submit(blob) for _ in range(args.steps))
                    d.drain()
                out = base.timed(run, args.steps)[0]
                kept[-1].result()
                return out

            def inner_steps():
                kept = []

                def run():
                    for _ in range(args.steps):
                        kept.extend((luma.submit(plane_blobs[0]), chroma.submit(plane_blobs[1]), chroma.submit(plane_blobs[2])))
                    luma.drain()
                    chroma.drain()
                out = base.timed(run, args.steps)[0]
                for ticket in kept[-3:]:
                    ticket.result()
                return out

            def synchronous():
                return base.timed(lambda: container.decode_colour_images(blob, decoder), 1)[0]

            measured = blocks_of({'ColourDecoder step': colour_steps, 'its three inner steps alone': inner_steps,
                                  'container.decode_colour_images': synchronous}, args.blocks)
            for (name, values) in measured.items():
                lines.append({'what': 'step', 'leg': name, 'ms': base.summary(values), 'depth': d.depth,
                              'luma': [d.luma.nb_streams, d.luma.nb_in_flight], 'chroma': [d.chroma.nb_streams, d.chroma.nb_in_flight],
                              'blob_bytes': len(blob)})
    with codec.ColourDecoder(variables, False, 1, h, w, length, use_graphs=True) as single:
        if not numpy.array_equal(single.submit(one).result(), expected[:1]):
            raise SystemExit('ColourDecoder of one picture is not decode_colour_images')

        def pipelined():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            single.submit(one).result()
            return (time.perf_counter() - t0)*1e3

        measured = blocks_of({'ColourDecoder, one picture, submit to result': pipelined,
                              'container.decode_colour_images, one picture': lambda: base.timed(lambda: container.decode_colour_images(one, decoder), 1)[0]},
                             args.blocks*args.steps)
        for (name, values) in measured.items():
            lines.append({'what': 'one', 'leg': name, 'ms': base.summary(values), 'blob_bytes': len(one)})
    return lines


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--blocks', type=int, default=5)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--batch', type=int, default=24)
    parser.add_argument('--sizes', nargs='+', default=['512x768', '500x750'])
    parser.add_argument('--bin-widths', nargs='+', type=float, default=[1.0, 0.05])
    parser.add_argument('--repeat', type=int, default=30)
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'colour_decoder.md'))
    args = parser.parse_args()
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for size in args.sizes:
        (h, w) = (int(side) for side in size.split('x'))
        rgb = colour_profile.pictures(args.batch, h, w)
        for line in kernel_legs(rgb, args.repeat, device):
            emit(dict(line, what='kernel', size=size))
        for bin_width in args.bin_widths:
            variables = bench.synthetic_model(bin_width)
            for line in step_legs(variables, variables[var.BIN_WIDTHS_NAME], rgb, args, device):
                emit(dict(line, size=size, bin_width=bin_width))
            torch.cuda.empty_cache()
    write_report(args.output, lines, args)


def write_report(path, lines, args):
    def cell(s):
        return '{0} ({1} .. {2})'.format(s['median'], s['min'], s['max'])

    out = ['# Colour pictures out of EAC1 containers: the whole-word merge and the ColourDecoder step', '',
           'Written by `profiles/colour_decoder.py`: {0} pictures per batch; {1} hardware queues (GPU_MAX_HW_QUEUES, set by: {2}).'.format(
               args.batch, package.HW_QUEUES[0], package.HW_QUEUES[1]), '']
    for size in args.sizes:
        out += ['## {0}: the two merge kernels into the same destination'.format(size), '',
                'Device events, median (min .. max) of {0} launches each, in microseconds; the existing kernel and the new one alternate, '
                'twice.'.format(args.repeat), '', '| destination | round | launch | microseconds |', '|---|---|---|---|']
        out += ['| {0} | {1} | {2} | {3} |'.format(line['destination'], line['round'], line['leg'], cell(line['microseconds']))
                for line in lines if line['what'] == 'kernel' and line['size'] == size]
        for bin_width in args.bin_widths:
            rows = [line for line in lines if line['what'] == 'step' and line['size'] == size and line['bin_width'] == bin_width]
            if not rows:
                continue
            out += ['', '## {0}, bin width {1}: the step'.format(size, bin_width), '',
                    '{0} blocks of {1} steps per leg, alternating in one process; ms per step, median (min .. max) of the blocks; '
                    '`decode_colour_images` is one call per block. Luminance decoder {2} streams and {3} steps in flight, chroma decoder {4} and '
                    '{5}, graphs; ring depth {6}; the blob has {7} bytes.'.format(args.blocks, args.steps, rows[0]['luma'][0], rows[0]['luma'][1],
                                                                                rows[0]['chroma'][0], rows[0]['chroma'][1], rows[0]['depth'],
                                                                                rows[0]['blob_bytes']), '', '| leg | ms per step |', '|---|---|']
            out += ['| {0} | {1} |'.format(line['leg'], cell(line['ms'])) for line in rows]
            out += ['', 'One picture, submit to result, {0} times each, alternating; ms, median (min .. max):'.format(args.blocks*args.steps), '',
                    '| leg | ms |', '|---|---|']
            out += ['| {0} | {1} |'.format(line['leg'], cell(line['ms'])) for line in lines
                    if line['what'] == 'one' and line['size'] == size and line['bin_width'] == bin_width]
        out.append('')
    notes = ''
    if os.path.exists(path):              # the hand-written part of the document stays
        with open(path) as f:
            text = f.read()
        if NOTES_HEADING in text:
            notes = text[text.index(NOTES_HEADING):]
    with open(path, 'w') as f:
        f.write('\n'.join(out) + notes)


if __name__ == '__main__':
    main()
