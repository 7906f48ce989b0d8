#!/usr/bin/env python
"""What `codec.BatchCodec(emit_container=True)` costs, and what it replaces (profiles/codec_container.md).

Product mode (`codec.product_mode(h, w)`), 24 Kodak-sized synthetic images per step (bench.py's images, model and statistics), per
bin width: blocks of `--steps` steps of a codec without and of a codec with `emit_container`, alternating on one box; per block the
wall time and the process CPU time per step. Then the same images through `container.encode_images`, the synchronous route to the
same bytes, per call. One JSON line per measurement; medians are of the blocks, with the smallest and the largest beside them.

    python profiles/codec_container.py [--blocks 7] [--steps 40] [--bin-widths 1.0 0.05]
    python profiles/codec_container.py --encode-images-only      # runs on a tree without emit_container too
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
from autoencoder_based_image_compression_amd import codec, container, pipeline  # noqa: E402
from autoencoder_based_image_compression_amd import device as dev  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats  # noqa: E402


def summary(values):
    ordered = sorted(values)
    return {'median': round(ordered[(len(ordered) - 1)//2], 4), 'min': round(ordered[0], 4), 'max': round(ordered[-1], 4)}


def block(the_codec, images, steps):
    """-> (wall ms per step, process CPU ms per step, the last step's results)."""
    torch.cuda.synchronize()
    (t0, c0) = (time.perf_counter(), time.process_time())
    tickets = [the_codec.submit(images) for _ in range(steps)]
    the_codec.drain()
    results = [t.result() for t in tickets]
    (wall, cpu) = (time.perf_counter() - t0, time.process_time() - c0)
    return wall/steps*1e3, cpu/steps*1e3, results[-1], tickets[-1]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--blocks', type=int, default=7)
    parser.add_argument('--steps', type=int, default=40)
    parser.add_argument('--warmup', type=int, default=10)
    parser.add_argument('--batch', type=int, default=24)
    parser.add_argument('--height', type=int, default=512)
    parser.add_argument('--width', type=int, default=768)
    parser.add_argument('--bin-widths', type=float, nargs='+', default=[1.0, 0.05])
    parser.add_argument('--encode-images-only', action='store_true')
    args = parser.parse_args()
    (batch, h, w) = (args.batch, args.height, args.width)
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    images_host = bench.synthetic_images(1000, batch, h, w)
    images = torch.from_numpy(images_host).to(device)
    pixels = batch*h*w
    for bin_width in args.bin_widths:
        variables = bench.synthetic_model(bin_width)
        bin_widths = variables[var.BIN_WIDTHS_NAME]
        encoder = pipeline.DeviceEncoder(variables, False, device)
        y0 = encoder(images)
        map_mean = dev.map_means(y0).cpu().numpy()
        probabilities = lossless_stats.compute_binary_probabilities(y0.cpu().numpy(), bin_widths, map_mean, bench.TRUNCATED_UNARY_LENGTH)
        del y0
        idx = bench.IDX_MAP_EXCEPTION
        if not args.encode_images_only:
            mode = codec.product_mode(h, w)
            codecs = {'emit_off': codec.BatchCodec(variables, False, bin_widths, map_mean, probabilities, idx, batch, h, w, device=device, **mode),
                      'emit_on': codec.BatchCodec(variables, False, bin_widths, map_mean, probabilities, idx, batch, h, w, device=device,
                                                  emit_container=True, container_capacity_bytes=2*pixels, **mode)}
            for c in codecs.values():
                for _ in range(args.warmup):
                    c.submit(images)
                c.drain()
            measured = {name: {'ms': [], 'cpu': []} for name in codecs}
            payload_bytes = None
            gc.collect()
            gc.disable()
            try:
                for _ in range(args.blocks):
                    for (name, c) in codecs.items():          # alternating: both see the same box at the same time
                        (ms, cpu, last, ticket) = block(c, images, args.steps)
                        measured[name]['ms'].append(ms)
                        measured[name]['cpu'].append(cpu)
                        if name == 'emit_on':
                            payload_bytes = int(last['container_bytes'].sum())
                            blob_bytes = len(ticket.container())
            finally:
                gc.enable()
            for c in codecs.values():
                c.close()
            for (name, m) in measured.items():
                line = {'what': 'product mode, ' + name, 'bin_width': bin_width, 'batch': batch, 'height': h, 'width': w, 'steps_per_block': args.steps,
                        'blocks': args.blocks, 'ms_per_step': summary(m['ms']), 'Mpx_per_s': summary([pixels/(ms*1e-3)/1e6 for ms in m['ms']]),
                        'process_cpu_ms_per_step': summary(m['cpu']), 'ms_per_step_blocks': [round(v, 4) for v in m['ms']]}
                if name == 'emit_on':
                    line.update({'payload_bytes_per_step': payload_bytes, 'container_bytes_per_step': blob_bytes,
                                 'bits_per_pixel_payload': round(8.*payload_bytes/pixels, 4)})
                print(json.dumps(line), flush=True)
        # the synchronous route to the same bytes
        for _ in range(2):
            (blob, info) = container.encode_images(images_host, encoder, bin_widths, map_mean, probabilities, idx)
        calls = []
        for _ in range(max(5, args.blocks)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (blob, info) = container.encode_images(images_host, encoder, bin_widths, map_mean, probabilities, idx)
            calls.append((time.perf_counter() - t0)*1e3)
        print(json.dumps({'what': 'container.encode_images, one call per batch', 'bin_width': bin_width, 'batch': batch, 'height': h, 'width': w,
                          'ms_per_batch': summary(calls), 'ms_per_image': round(summary(calls)['median']/batch, 4),
                          'payload_bytes': info['payload_bytes'], 'blob_bytes': len(blob)}), flush=True)


if __name__ == '__main__':
    main()
