#!/usr/bin/env python
"""What colour pictures cost (profiles/colour.md): `--batch` RGB pictures at each of `--sizes` (512 x 768 and
500 x 750 by default), bench.py's synthetic images in every channel, its model and statistics.

1. The two kernels against a plain copy, device events, median of `--repeat` launches: `device.colour_split_420` from a device source
   and from a pinned one, `device.colour_merge_420` with and without the reference, and, for each, a device-to-device copy that reads
   and writes as many bytes as the kernel does, in the same run. The results are compared with `colour.py` first.
2. The pipelined step against its inner steps, in ONE process, in alternating blocks: `ColourCodec(**product_mode(h, w),
   chroma_options=product_mode(hc, wc))` on the RGB batch against the same three inner submits -- the luminance plane to its `luma`
   codec, Cb and Cr to its `chroma` codec -- with no split and no merge. Per block the wall time per step; medians are of the blocks,
   with the smallest and the largest beside them. The difference is what the colour layer costs.
One JSON line per measurement on stdout; the tables go to profiles/colour.md, in front of its section `## Notes`, which is written
by hand (what bounds the kernels, and the headline's comparison with the parent commit, run with bench.py itself) and which a rerun
keeps as it finds it.

    python profiles/colour.py [--blocks 5] [--steps 20] [--batch 24] [--sizes 512x768 500x750] [--bin-width 1.0]
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
import frames  # noqa: E402
import autoencoder_based_image_compression_amd as package  # noqa: E402
from autoencoder_based_image_compression_amd import codec, colour, pipeline  # noqa: E402
from autoencoder_based_image_compression_amd import device as dev  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats  # noqa: E402


NOTES_HEADING = '\n## Notes'


def pictures(batch, h, w):
    (H, W) = dev.coded_size(h, w)
    return numpy.ascontiguousarray(numpy.stack([bench.synthetic_images(1000 + channel, batch, H, W)[:, :h, :w] for channel in range(3)], axis=3))


def kernel_legs(rgb, repeat, device):
    """-> [{leg, bytes read + written, microseconds, TB/s, the same for a copy of as many bytes}] for the batch `rgb` (uint8 [n, h, w, 3])."""
    (n, h, w, _) = rgb.shape
    (hc, wc) = dev.chroma_size(h, w)
    (picture, planes_bytes) = (n*h*w*3, n*h*w + 2*n*hc*wc)
    source = torch.from_numpy(rgb).to(device)
    pinned = torch.from_numpy(rgb).pin_memory()
    planes = dev.colour_split_420(source)
    expected = colour.split_420_numpy(rgb)
    for got in (planes, dev.colour_split_420(pinned)):
        if not all(numpy.array_equal(a.cpu().numpy(), b) for (a, b) in zip(got, expected)):
            raise SystemExit('colour_split_420 is not colour.split_420_numpy')
    (out, sse) = dev.colour_merge_420(*planes, (h, w), reference=source)
    merged = colour.merge_420_numpy(*expected)
    if not numpy.array_equal(out.cpu().numpy(), merged) or not numpy.array_equal(sse.cpu().numpy(), colour.sse_rgb_numpy(rgb, merged)):
        raise SystemExit('colour_merge_420 is not colour.merge_420_numpy')
    legs = (('colour_split_420, device source', lambda: dev.colour_split_420(source, out=planes), picture + planes_bytes),
            ('colour_split_420, pinned source', lambda: dev.colour_split_420(pinned, out=planes), picture + planes_bytes),
            ('colour_merge_420, picture only', lambda: dev.colour_merge_420(*planes, (h, w), out=out), planes_bytes + picture),
            ('colour_merge_420, picture and squared error', lambda: dev.colour_merge_420(*planes, (h, w), out=out, reference=source, sse=sse),
             planes_bytes + 2*picture),
            ('colour_merge_420, squared error only', lambda: dev.colour_merge_420(*planes, (h, w), out=False, reference=source, sse=sse),
             planes_bytes + picture))
    result = []
    for (name, fn, nbytes) in legs:
        half = torch.empty(nbytes//2, dtype=torch.uint8, device=device)
        other = torch.empty_like(half)
        us = frames.event_median(fn, repeat)
        copy_us = frames.event_median(lambda: other.copy_(half), repeat)
        result.append({'leg': name, 'bytes': nbytes, 'microseconds': us, 'terabytes_per_second': round(nbytes/us*1e-6, 3),
                       'copy_microseconds': copy_us, 'copy_terabytes_per_second': round(2*(nbytes//2)/copy_us*1e-6, 3)})
    return result


def colour_steps(c, batch, steps):
    kept = []

    def run():
        kept.extend(c.submit(batch) for _ in range(steps))
        c.drain()
    out = base.timed(run, steps)
    kept[-1].result()
    return out


def inner_steps(c, planes, steps):
    kept = []

    def run():
        for _ in range(steps):
            kept.extend((c.luma.submit(planes[0]), c.chroma.submit(planes[1]), c.chroma.submit(planes[2])))
        c.drain()
    out = base.timed(run, steps)
    for ticket in kept[-3:]:
        ticket.result()
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--blocks', type=int, default=5)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--batch', type=int, default=24)
    parser.add_argument('--sizes', nargs='+', default=['512x768', '500x750'])
    parser.add_argument('--bin-width', type=float, default=1.0)
    parser.add_argument('--repeat', type=int, default=30)
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'colour.md'))
    args = parser.parse_args()
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    length = bench.TRUNCATED_UNARY_LENGTH
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    variables = bench.synthetic_model(args.bin_width)
    bin_widths = variables[var.BIN_WIDTHS_NAME]
    for size in args.sizes:
        (h, w) = (int(side) for side in size.split('x'))
        (hc, wc) = dev.chroma_size(h, w)
        rgb = pictures(args.batch, h, w)
        for line in kernel_legs(rgb, args.repeat, device):
            emit(dict(line, what='kernel', shape=[args.batch, h, w, 3]))
        planes = colour.split_420_numpy(rgb)
        padded = numpy.pad(planes[0], ((0, 0), (0, dev.coded_size(h, w)[0] - h), (0, dev.coded_size(h, w)[1] - w)), mode='edge')
        y0 = pipeline.DeviceEncoder(variables, False, device)(torch.from_numpy(padded).to(device))
        map_mean = dev.map_means(y0).cpu().numpy()
        probabilities = lossless_stats.compute_binary_probabilities(y0.cpu().numpy(), bin_widths, map_mean, length)
        del y0
        rgb_d = torch.from_numpy(rgb).to(device)
        planes_d = [torch.from_numpy(plane).to(device) for plane in planes]
        with codec.ColourCodec(variables, False, bin_widths, map_mean, probabilities, bench.IDX_MAP_EXCEPTION, args.batch, h, w,
                               chroma_options=codec.product_mode(hc, wc), **codec.product_mode(h, w)) as c:
            ticket = c.submit(rgb_d)
            r = ticket.result()
            alone = [t.result() for t in (c.luma.submit(planes_d[0]), c.chroma.submit(planes_d[1]), c.chroma.submit(planes_d[2]))]
            if not all(numpy.array_equal(r[key][:, k], alone[k][key]) for key in alone[0] for k in range(3)):
                raise SystemExit('ColourCodec: a plane\'s results are not those of the plane submitted alone')
            legs = {'ColourCodec step': lambda: colour_steps(c, rgb_d, args.steps),
                    'its three inner steps alone': lambda: inner_steps(c, planes_d, args.steps)}
            for fn in legs.values():          # warm-up
                fn()
            measured = {name: [] for name in legs}
            gc.collect()
            gc.disable()
            try:
                for _ in range(args.blocks):
                    for (name, fn) in legs.items():          # alternating: every leg sees the same box at the same time
                        measured[name].append(fn()[0])
            finally:
                gc.enable()
            psnr = colour.psnr_from_sse(r['sse_rgb'], 3*h*w)
            for (name, values) in measured.items():
                emit({'what': 'step', 'leg': name, 'shape': [args.batch, h, w, 3], 'bin_width': args.bin_width, 'blocks': args.blocks,
                      'steps': args.steps, 'ms_per_step': base.summary(values), 'depth': c.depth,
                      'luma': [c.luma.nb_transform_streams, c.luma.nb_in_flight], 'chroma': [c.chroma.nb_transform_streams, c.chroma.nb_in_flight],
                      'mean_psnr_rgb': round(float(psnr.mean()), 2)})
        torch.cuda.empty_cache()
    write_report(args.output, lines, args)


def write_report(path, lines, args):
    def cell(s):
        return '{0} ({1} .. {2})'.format(s['median'], s['min'], s['max'])

    out = ['# Colour pictures: what the split, the merge and the colour step cost', '',
           'Written by `profiles/colour.py`: {0} pictures per batch; {1} hardware queues (GPU_MAX_HW_QUEUES, set by: {2}).'.format(
               args.batch, package.HW_QUEUES[0], package.HW_QUEUES[1]), '']
    for size in args.sizes:
        shape = [args.batch] + [int(side) for side in size.split('x')] + [3]
        out += ['## {0}: the kernels against a copy of as many bytes'.format(size), '',
                'Device events, median of {0} launches each; bytes read + written; the copy is device to device, half the bytes read and '
                'half written.'.format(args.repeat), '',
                '| launch | bytes | microseconds | TB/s | copy, microseconds | copy, TB/s | kernel / copy rate |', '|---|---|---|---|---|---|---|']
        for line in lines:
            if line['what'] == 'kernel' and line['shape'] == shape:
                out.append('| {0} | {1} | {2} | {3} | {4} | {5} | {6} |'.format(
                    line['leg'], line['bytes'], line['microseconds'], line['terabytes_per_second'], line['copy_microseconds'],
                    line['copy_terabytes_per_second'], round(line['terabytes_per_second']/line['copy_terabytes_per_second'], 2)))
        rows = [line for line in lines if line['what'] == 'step' and line['shape'] == shape]
        if rows:
            out += ['', '## {0}: the colour step against its inner steps'.format(size), '',
                    '{0} blocks of {1} steps per leg, alternating in one process; median (min .. max) of the blocks. Bin width {2}; luminance '
                    'codec {3} transform streams and {4} batches in flight, chroma codec {5} and {6}, graphs; ring depth {7}.'.format(
                        args.blocks, args.steps, args.bin_width, rows[0]['luma'][0], rows[0]['luma'][1], rows[0]['chroma'][0], rows[0]['chroma'][1],
                        rows[0]['depth']), '', '| leg | ms per step |', '|---|---|']
            out += ['| {0} | {1} |'.format(line['leg'], cell(line['ms_per_step'])) for line in rows]
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
