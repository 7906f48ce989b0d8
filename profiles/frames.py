#!/usr/bin/env python
"""What images of any height and width cost (profiles/frames.md): `--batch` images of `--height` x `--width`
(500 x 750 by default, coded as 512 x 752), bench.py's synthetic images, model and statistics, per bin width.

1. The two kernels alone, device events, median of `--repeat` launches: `device.frame_pad_u8` from a device source and from a pinned
   one, `device.frame_sse_u8`, and on as many bytes `device.publish_crops` at origin (0, 0) (the crop a padded decoder publishes,
   into device and into pinned memory) and a plain device-to-device copy of the padded planes. With the bytes each moves.
2. The pipelined step, in ONE process, in alternating blocks: `BatchCodec(pad=True, **product_mode(h, w))` on the real batch against
   `BatchCodec(**product_mode(H, W))` on the numpy-edge-padded batch (same transforms, same coder work), both with
   `emit_container=True`; and `BatchDecoder(pad=True)` against `BatchDecoder` on the blobs of the two. Per block the wall time per
   step; medians are of the blocks, with the smallest and the largest beside them. Every leg is compared with the other first.
One JSON line per measurement on stdout; the tables go to profiles/frames.md.

    python profiles/frames.py [--blocks 5] [--steps 20] [--batch 24] [--height 500] [--width 750] [--bin-widths 1.0 0.05]
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
from autoencoder_based_image_compression_amd import codec, pipeline  # noqa: E402
from autoencoder_based_image_compression_amd import device as dev  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats  # noqa: E402


def event_median(fn, repeat):
    """Microseconds of one launch of `fn`: the median over `repeat` launches, each between two events of its own."""
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
    return round(sorted(times)[(len(times) - 1)//2], 2)


def kernel_legs(images, repeat, device):
    """-> [{leg, bytes read + written, microseconds, TB/s}] for the batch `images` (numpy uint8 [n, h, w])."""
    (n, h, w) = images.shape
    (H, W) = dev.coded_size(h, w)
    (real, coded) = (n*h*w, n*H*W)
    source = torch.from_numpy(images).to(device)
    pinned = torch.from_numpy(images).pin_memory()
    padded = dev.frame_pad_u8(source)
    expected = numpy.pad(images, ((0, 0), (0, H - h), (0, W - w)), mode='edge')
    if not numpy.array_equal(padded.cpu().numpy(), expected) or not numpy.array_equal(dev.frame_pad_u8(pinned).cpu().numpy(), expected):
        raise SystemExit('frame_pad_u8 is not numpy.pad(..., mode="edge")')
    other = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device=device)
    sse = torch.zeros(n, dtype=torch.int64, device=device)
    want = ((images.astype(numpy.int64) - other.cpu().numpy()[:, :h, :w])**2).sum(axis=(1, 2))
    if not numpy.array_equal(dev.frame_sse_u8(other, source).cpu().numpy(), want):
        raise SystemExit('frame_sse_u8 is not numpy\'s sum over the real pixels')
    origins = torch.zeros((n, 2), dtype=torch.int32, device=device)
    words = -(-real//16)*16
    (crops, pinned_crops) = (torch.zeros(words, dtype=torch.uint8, device=device), torch.zeros(words, dtype=torch.uint8).pin_memory())
    copy = torch.empty_like(padded)
    legs = (('frame_pad_u8, device source', lambda: dev.frame_pad_u8(source, out=padded), real + coded),
            ('frame_pad_u8, pinned source', lambda: dev.frame_pad_u8(pinned, out=padded), real + coded),
            ('frame_sse_u8', lambda: dev.frame_sse_u8(other, source, out=sse), 2*real),
            ('publish_crops at (0, 0), to device memory', lambda: dev.publish_crops(other, origins, crops, h, w), 2*real),
            ('publish_crops at (0, 0), to pinned memory', lambda: dev.publish_crops(other, origins, pinned_crops, h, w), 2*real),
            ('copy of the padded planes, device to device', lambda: copy.copy_(padded), 2*coded))
    out = []
    for (name, fn, nbytes) in legs:
        us = event_median(fn, repeat)
        out.append({'leg': name, 'bytes': nbytes, 'microseconds': us, 'terabytes_per_second': round(nbytes/us*1e-6, 3)})
    return out


def codec_pipelined(c, batch, steps):
    kept = []

    def run():
        kept.extend(c.submit(batch) for _ in range(steps))
        c.drain()
    out = base.timed(run, steps)
    for ticket in kept[-1:]:
        ticket.result()
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--blocks', type=int, default=5)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--batch', type=int, default=24)
    parser.add_argument('--height', type=int, default=500)
    parser.add_argument('--width', type=int, default=750)
    parser.add_argument('--bin-widths', type=float, nargs='+', default=[1.0, 0.05])
    parser.add_argument('--repeat', type=int, default=30)
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'frames.md'))
    args = parser.parse_args()
    (batch, h, w, steps) = (args.batch, args.height, args.width, args.steps)
    (H, W) = dev.coded_size(h, w)
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    images = numpy.ascontiguousarray(bench.synthetic_images(1000, batch, H, W)[:, :h, :w])
    padded = numpy.pad(images, ((0, 0), (0, H - h), (0, W - w)), mode='edge')
    length = bench.TRUNCATED_UNARY_LENGTH
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for line in kernel_legs(images, args.repeat, device):
        emit(dict(line, what='kernel', shape=[batch, h, w], coded=[H, W]))
    (images_d, padded_d) = (torch.from_numpy(images).to(device), torch.from_numpy(padded).to(device))
    for bin_width in args.bin_widths:
        variables = bench.synthetic_model(bin_width)
        bin_widths = variables[var.BIN_WIDTHS_NAME]
        y0 = pipeline.DeviceEncoder(variables, False, device)(padded_d)
        map_mean = dev.map_means(y0).cpu().numpy()
        probabilities = lossless_stats.compute_binary_probabilities(y0.cpu().numpy(), bin_widths, map_mean, length)
        del y0
        common = (variables, False, bin_widths, map_mean, probabilities, bench.IDX_MAP_EXCEPTION, batch)
        more = {'emit_container': True, 'keep_reconstruction': True, 'container_capacity_bytes': 2*batch*H*W}
        with codec.BatchCodec(*common, h, w, pad=True, **more, **codec.product_mode(h, w)) as framed, \
                codec.BatchCodec(*common, H, W, **more, **codec.product_mode(H, W)) as plain, \
                codec.BatchDecoder(variables, False, batch, h, w, length, use_graphs=True, payload_capacity_bytes=2*batch*H*W, pad=True) as framed_decoder, \
                codec.BatchDecoder(variables, False, batch, H, W, length, use_graphs=True, payload_capacity_bytes=2*batch*H*W) as plain_decoder:
            (a, b) = (framed.submit(images_d), plain.submit(padded_d))
            (ra, rb) = (a.result(), b.result())
            for key in ra:
                if key != 'sse' and not numpy.array_equal(ra[key], rb[key]):
                    raise SystemExit('BatchCodec(pad=True): {0} is not the padded batch\'s'.format(key))
            whole = b.reconstruction_uint8.cpu().numpy()
            if not numpy.array_equal(a.reconstruction_uint8.cpu().numpy(), whole[:, :h, :w]):
                raise SystemExit('BatchCodec(pad=True): the reconstruction is not the crop')
            (blob, plain_blob) = (a.container(), b.container())
            if blob[:23] != plain_blob[:23] or blob[24:] != plain_blob[24:]:
                raise SystemExit('BatchCodec(pad=True): the container is not the padded batch\'s but for byte 23')
            if not numpy.array_equal(framed_decoder.submit(blob).result(), whole[:, :h, :w]) or \
                    not numpy.array_equal(plain_decoder.submit(plain_blob).result(), whole):
                raise SystemExit('the decoders do not give the codec\'s reconstruction')
            legs = {'BatchCodec(pad=True), {0} x {1}'.format(h, w): lambda: codec_pipelined(framed, images_d, steps),
                    'BatchCodec, {0} x {1} padded by hand'.format(H, W): lambda: codec_pipelined(plain, padded_d, steps),
                    'BatchDecoder(pad=True), {0} x {1}'.format(h, w): lambda: base.pipelined(framed_decoder, [blob], steps),
                    'BatchDecoder, {0} x {1}'.format(H, W): lambda: base.pipelined(plain_decoder, [plain_blob], steps)}
            for fn in legs.values():          # warm-up: graphs captured, lazy loads done
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
            bpp = round(8.*int(ra['container_bytes'].sum())/(batch*h*w), 4)
            for (name, values) in measured.items():
                emit({'what': 'step', 'leg': name, 'bin_width': bin_width, 'payload_bits_per_real_pixel': bpp, 'blocks': args.blocks, 'steps': steps,
                      'ms_per_step': base.summary(values), 'nb_in_flight': framed.nb_in_flight, 'nb_transform_streams': framed.nb_transform_streams})
        torch.cuda.empty_cache()
    write_report(args.output, lines, args, (H, W))


def write_report(path, lines, args, coded):
    def cell(s):
        return '{0} ({1} .. {2})'.format(s['median'], s['min'], s['max'])

    out = ['# Images of any height and width: what the pad, the error and the crop cost', '',
           'Written by `profiles/frames.py`: {0} images of {1} x {2}, coded as {3} x {4}; {5} hardware queues (GPU_MAX_HW_QUEUES, set by: '
           '{6}).'.format(args.batch, args.height, args.width, coded[0], coded[1], package.HW_QUEUES[0], package.HW_QUEUES[1]), '',
           '## the kernels alone', '', 'Device events, median of {0} launches each; bytes read + written.'.format(args.repeat), '',
           '| launch | bytes | microseconds | TB/s |', '|---|---|---|---|']
    for line in lines:
        if line['what'] == 'kernel':
            out.append('| {0} | {1} | {2} | {3} |'.format(line['leg'], line['bytes'], line['microseconds'], line['terabytes_per_second']))
    out.append('')
    for bin_width in args.bin_widths:
        rows = [line for line in lines if line['what'] == 'step' and line['bin_width'] == bin_width]
        if not rows:
            continue
        out += ['## the pipelined step, bin width {0} ({1} payload bits per real pixel)'.format(bin_width, rows[0]['payload_bits_per_real_pixel']), '',
                '{0} blocks of {1} steps per leg, alternating in one process; median (min .. max) of the blocks. Codecs in the product mode '
                '({2} transform streams, {3} batches in flight, graphs) with `emit_container=True`; decoders with graphs.'.format(
                    args.blocks, args.steps, rows[0]['nb_transform_streams'], rows[0]['nb_in_flight']), '',
                '| leg | ms per step |', '|---|---|']
        out += ['| {0} | {1} |'.format(line['leg'], cell(line['ms_per_step'])) for line in rows]
        out.append('')
    with open(path, 'w') as f:
        f.write('\n'.join(out))


if __name__ == '__main__':
    main()
