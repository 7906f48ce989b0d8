#!/usr/bin/env python
"""What coding tiles cost and give inside `codec.BatchCodec` (profiles/codec_tiles.md).

bench.py's synthetic images, model and statistics at 512 x 768, per bin width, in ONE process, every comparison in alternating
blocks (each leg sees the same box at the same time); medians of the blocks with the smallest and the largest beside them.

1. one image, submit -> result, each waited for before the next is submitted: the single-image mode of the README's snippet (14
   streams, one graph launch per step) and the default one-image codec (one coder stream, graphs, early publish: bench.py's
   `single_image.latency_ms`); without containers, with `emit_container` and no coding tile, with tiles of 16 and of 8 latents.
   Beside them the coder's share: `Ticket.coder_ms()` of a launch-by-launch codec (`time_coder=True`), and the encode / decode
   launches under HIP events (`launch_hook`).
2. 24 images per step, product mode, `emit_container=True`: no tile against tiles of 16, blocks of 100 steps; then `nb_in_flight`
   3..6 with tiles of 16.
3. `device.coder_index_tiles` alone under device events at 24 x 6 and 24 x 64 entries, beside `device.coder_index_streams` at 24 x 1.
4. payload and header bytes of a 24-image step: `EAE1` against tiles of 32, 16 and 8.

    GPU_MAX_HW_QUEUES=16 python profiles/codec_tiles.py [--blocks 5] [--bin-widths 1.0 0.05]
"""
import argparse
import gc
import json
import os
import sys
import time
import types

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

VARIANTS = (('no container', None), ('container, no tile', {}), ('tile 16', {'coding_tile': (16, 16)}), ('tile 8', {'coding_tile': (8, 8)}))
ONE_IMAGE_MODES = (('README single-image mode (14 streams, one_stream_steps)',
                    {'nb_in_flight': 14, 'nb_transform_streams': 14, 'use_graphs': True, 'one_stream_steps': True}),
                   ('default one-image codec (1 coder stream, graphs, early publish)',
                    {'nb_in_flight': 1, 'nb_transform_streams': 1, 'use_graphs': True}))


def summary(values):
    ordered = sorted(values)
    return {'median': round(ordered[(len(ordered) - 1)//2], 4), 'min': round(ordered[0], 4), 'max': round(ordered[-1], 4)}


def timed(fn, count):
    """-> wall ms per unit of `count`."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0)/count*1e3


def emit_arguments(extra, pixels):
    return {} if extra is None else dict(extra, emit_container=True, container_capacity_bytes=2*pixels)


def alternating(legs, blocks):
    """legs {name: fn -> ms}: one warm-up call each, then `blocks` rounds over all of them -> {name: [ms]}."""
    for fn in legs.values():
        fn()
    measured = {name: [] for name in legs}
    gc.collect()
    gc.disable()
    try:
        for _ in range(blocks):
            for (name, fn) in legs.items():
                measured[name].append(fn())
    finally:
        gc.enable()
    return measured


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--blocks', type=int, default=5)
    parser.add_argument('--latency-steps', type=int, default=100)
    parser.add_argument('--steps', type=int, default=100)
    parser.add_argument('--bin-widths', type=float, nargs='+', default=[1.0, 0.05])
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'codec_tiles.md'))
    args = parser.parse_args()
    (batch, h, w) = (24, 512, 768)
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    images = torch.from_numpy(bench.synthetic_images(1000, batch, h, w)).to(device)
    length = bench.TRUNCATED_UNARY_LENGTH
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
        model = (variables, False, bin_widths, map_mean, probabilities, bench.IDX_MAP_EXCEPTION)

        # ---- 1. one image, submit -> result --------------------------------------------------------------------------------------
        one = images[:1]
        for (mode, mode_arguments) in ONE_IMAGE_MODES:
            codecs = {name: codec.BatchCodec(*model, 1, h, w, device=device, **mode_arguments, **emit_arguments(extra, h*w)) for (name, extra) in VARIANTS}

            def serial(c):
                def run():
                    for _ in range(args.latency_steps):
                        c.submit(one).result()
                return lambda: timed(run, args.latency_steps)
            measured = alternating({name: serial(c) for (name, c) in codecs.items()}, args.blocks)
            for (name, c) in codecs.items():
                ticket = c.submit(one)
                values = ticket.result()
                emit({'what': 'one image', 'mode': mode, 'variant': name, 'bin_width': bin_width, 'ms_per_image': summary(measured[name]),
                      'coder_bits': int(values['coder_bits'][0]),
                      'container_bytes': int(values['container_bytes'][0]) if 'container_bytes' in values else None})
                c.close()
            del codecs
        # the coder's share: launch by launch, one coder stream, each step waited for
        for (name, extra) in VARIANTS:
            spans = []

            def hook(label, fn):
                if not label.startswith('coder'):
                    return fn()
                (a, b) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                a.record()
                out = fn()
                b.record()
                spans.append((label, a, b))
                return out
            with codec.BatchCodec(*model, 1, h, w, device=device, nb_in_flight=1, time_coder=True, launch_hook=hook, **emit_arguments(extra, h*w)) as c:
                for _ in range(5):
                    c.submit(one).result()
                del spans[:]
                (coder_ms, step_ms) = ([], [])
                for _ in range(30):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ticket = c.submit(one)
                    ticket.result()
                    step_ms.append((time.perf_counter() - t0)*1e3)
                    torch.cuda.synchronize()
                    coder_ms.append(ticket.coder_ms())
                launches = {}
                for (label, a, b) in spans:
                    launches.setdefault(label, []).append(a.elapsed_time(b))
                # (with tiles the hook sees one encode and one decode per shape class: summed per step)
                per_step = {label: sum(v)/30. for (label, v) in launches.items()}
            emit({'what': 'coder share', 'variant': name, 'bin_width': bin_width, 'coder_ms': summary(coder_ms), 'step_ms_launch_by_launch': summary(step_ms),
                  'encode_launches_ms_per_step': round(per_step.get('coder_encode', 0.), 4), 'decode_launches_ms_per_step': round(per_step.get('coder_decode', 0.), 4),
                  'coder_launch_pairs_per_step': len(launches.get('coder_encode', ()))//30})

        # ---- 2. 24 images per step, product mode ------------------------------------------------------------------------------------
        def pipelined(c):
            def run():
                tickets = [c.submit(images) for _ in range(args.steps)]
                c.drain()
                for ticket in tickets:
                    ticket.result()
            return lambda: timed(run, args.steps)
        product = codec.product_mode(h, w)
        codecs = {name: codec.BatchCodec(*model, batch, h, w, device=device, **product, **emit_arguments(extra, batch*h*w))
                  for (name, extra) in VARIANTS[1:3]}
        measured = alternating({name: pipelined(c) for (name, c) in codecs.items()}, args.blocks)
        for (name, c) in codecs.items():
            emit({'what': '24 images', 'variant': name, 'bin_width': bin_width, 'nb_in_flight': c.nb_in_flight, 'steps': args.steps,
                  'ms_per_step': summary(measured[name]), 'Mpx_per_s': summary([batch*h*w/(ms*1e-3)/1e6 for ms in measured[name]])})
            c.close()
        del codecs
        sweep = {}
        for depth in (3, 4, 5, 6):
            c = codec.BatchCodec(*model, batch, h, w, device=device, **dict(product, nb_in_flight=depth), **emit_arguments({'coding_tile': (16, 16)}, batch*h*w))
            if c.nb_in_flight != depth:
                print('sweep: {0} in flight asked for, {1} run: skipped (set GPU_MAX_HW_QUEUES=16)'.format(depth, c.nb_in_flight), flush=True)
                c.close()
                continue
            sweep[depth] = c
        if sweep:
            measured = alternating({depth: pipelined(c) for (depth, c) in sweep.items()}, args.blocks)
            for (depth, c) in sweep.items():
                emit({'what': 'sweep', 'variant': 'tile 16', 'bin_width': bin_width, 'nb_in_flight': depth, 'ms_per_step': summary(measured[depth])})
                c.close()
        del sweep

        # ---- 4. payload and header bytes of one 24-image step -----------------------------------------------------------------------
        for (name, tile) in (('EAE1', None), ('tile 32', (32, 32)), ('tile 16', (16, 16)), ('tile 8', (8, 8))):
            extra = {} if tile is None else {'coding_tile': tile}
            with codec.BatchCodec(*model, batch, h, w, device=device, nb_in_flight=1, **emit_arguments(extra, batch*h*w)) as c:
                ticket = c.submit(images)
                blob = ticket.container()
                payload = int(ticket.result()['container_bytes'].sum())
            header = container.read_header(blob)
            assert len(blob) - header['payload_offset'] == payload
            emit({'what': 'bytes', 'variant': name, 'bin_width': bin_width, 'payload_bytes': payload, 'header_bytes': header['payload_offset'],
                  'tiles_per_image': 1 if tile is None else header['bits'].shape[1]})
        torch.cuda.empty_cache()

    # ---- 3. the index entry point alone ---------------------------------------------------------------------------------------------
    rng = numpy.random.RandomState(0)

    def events(fn, calls=200, repeats=7):
        out = []
        for _ in range(repeats):
            (a, b) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            fn()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b)/calls*1e3)
        return summary(out)
    for tiles in (1, 6, 64):
        entries = 24*tiles
        stride = dev.coder_stream_stride_bytes(1536//tiles if tiles < 64 else 64, length)
        counts = torch.from_numpy(rng.randint(0, 4*stride, size=(2, entries*128)).astype(numpy.int32)).to(device)
        table = torch.from_numpy(numpy.stack([rng.permutation(entries), numpy.full(entries, stride//2)], axis=1).astype(numpy.int64)).to(device)
        offsets = torch.empty((entries*128, 2), dtype=torch.int64, device=device)
        index = torch.empty(2 + 24, dtype=torch.int64, device=device)
        emit({'what': 'index', 'entry_point': 'eae_hip_coder_index_tiles', 'entries': '24 x {0}'.format(tiles), 'pieces': entries*256,
              'us_per_call': events(lambda: dev.coder_index_tiles(counts[0], counts[1], table, 128, tiles, 10**9, offsets=offsets, index=index))})
        if tiles == 1:
            streams = types.SimpleNamespace(n_maps=entries*128, stride=stride, bac_bits=counts[0], bypass_bits=counts[1])
            emit({'what': 'index', 'entry_point': 'eae_hip_coder_index_streams', 'entries': '24 x 1', 'pieces': entries*256,
                  'us_per_call': events(lambda: dev.coder_index_streams(streams, 128, 10**9, offsets=offsets, index=index))})
    write_report(args.output, lines, args)


def write_report(path, lines, args):
    def cell(s):
        return '{0} ({1} .. {2})'.format(s['median'], s['min'], s['max'])

    out = ['# Coding tiles inside `codec.BatchCodec`', '',
           'Written by `profiles/codec_tiles.py` ({0} alternating blocks per leg in one process; median (min .. max) of the blocks). 512 x 768 '
           'images, bench.py\'s synthetic images, model and statistics; {1} hardware queues (GPU_MAX_HW_QUEUES, set by: {2}).'.format(
               args.blocks, package.HW_QUEUES[0], package.HW_QUEUES[1]), '']
    for bin_width in args.bin_widths:
        mine = [line for line in lines if line.get('bin_width') == bin_width]
        if not mine:
            continue
        out += ['## bin width {0}'.format(bin_width), '', '### One image, submit -> result (blocks of {0} images, each waited for)'.format(args.latency_steps), '',
                '| mode | variant | ms per image | coder bits | payload bytes |', '|---|---|---|---|---|']
        for line in mine:
            if line['what'] == 'one image':
                out.append('| {0} | {1} | {2} | {3} | {4} |'.format(line['mode'], line['variant'], cell(line['ms_per_image']), line['coder_bits'],
                                                                   '-' if line['container_bytes'] is None else line['container_bytes']))
        out += ['', 'The coder\'s share (launch by launch, one coder stream, 30 steps each waited for; `Ticket.coder_ms()` spans the coder stream from the '
                'symbols to the publication; the launches are the `launch_hook`\'s `coder_encode` / `coder_decode`, summed over the shape classes):', '',
                '| variant | coder span ms | encode launches ms | decode launches ms | coder batches per step | step ms, launch by launch |', '|---|---|---|---|---|---|']
        for line in mine:
            if line['what'] == 'coder share':
                out.append('| {0} | {1} | {2} | {3} | {4} | {5} |'.format(line['variant'], cell(line['coder_ms']), line['encode_launches_ms_per_step'],
                                                                         line['decode_launches_ms_per_step'], line['coder_launch_pairs_per_step'],
                                                                         cell(line['step_ms_launch_by_launch'])))
        out += ['', '### 24 images per step, product mode, `emit_container=True` (blocks of {0} steps)'.format(args.steps), '',
                '| variant | coder batches in flight | ms per step | Mpixel/s |', '|---|---|---|---|']
        for line in mine:
            if line['what'] == '24 images':
                out.append('| {0} | {1} | {2} | {3} |'.format(line['variant'], line['nb_in_flight'], cell(line['ms_per_step']), cell(line['Mpx_per_s'])))
        out += ['', '`nb_in_flight` with tiles of 16 (alternating blocks, ms per step): ' +
                ', '.join('{0}: {1}'.format(line['nb_in_flight'], cell(line['ms_per_step'])) for line in mine if line['what'] == 'sweep'), '']
        sizes = [line for line in mine if line['what'] == 'bytes']
        if sizes:
            base = sizes[0]
            out += ['### Bytes of one 24-image step', '', '| format | tiles per image | payload bytes | against `EAE1` | header bytes | header / payload |',
                    '|---|---|---|---|---|---|']
            for line in sizes:
                out.append('| {0} | {1} | {2} | {3:+.2f} % | {4} | {5:.2f} % |'.format(
                    line['variant'], line['tiles_per_image'], line['payload_bytes'], 100.*(line['payload_bytes'] - base['payload_bytes'])/base['payload_bytes'],
                    line['header_bytes'], 100.*line['header_bytes']/line['payload_bytes']))
            out.append('')
    index = [line for line in lines if line['what'] == 'index']
    if index:
        out += ['## The index entry point alone (device events around 200 calls, 7 repeats)', '', '| entry point | entries | pieces | us per call |', '|---|---|---|---|']
        for line in index:
            out.append('| `{0}` | {1} | {2} | {3} |'.format(line['entry_point'], line['entries'], line['pieces'], cell(line['us_per_call'])))
        out.append('')
    with open(path, 'w') as f:
        f.write('\n'.join(out))


if __name__ == '__main__':
    main()
