#!/usr/bin/env python
"""What an RGB crop out of a large colour picture costs (profiles/colour_region_decoder.md): `--crops` crops of
`--region` at random positions out of `--pictures` pictures of `--size`, coded in tiles of `--coding-tile` latents; bench.py's synthetic
images in every channel, its model and statistics.

1. The merge kernels, device events, median (min .. max) of `--repeat` launches each: `device.colour_merge_420_crops` on the crops of a
   step against `device.colour_merge_420_words` on as many pictures of the region's size -- as many output bytes --, both into the
   same destination, once in device memory and once in pinned host memory. The two alternate, twice; both rounds are printed. The
   crops are compared with `colour.merge_420_region_numpy` first.
2. The pipelined step, in ONE process, in alternating blocks: `ColourRegionDecoder(use_graphs=True)` against its three inner steps
   submitted alone to two plain `RegionDecoder(pad=True, use_graphs=True)` with the streams and slots of the colour decoder's inner
   ones, against `container.decode_colour_region` of one request, and against `container.decode_colour_images` of the whole blob.
   Every step takes other positions; the first step's crops are compared with `decode_colour_region` first.
One JSON line per measurement on stdout; the tables go to `--output`, in front of its section `## Notes`, which is written by hand and
which a rerun keeps as it finds it.

    python profiles/colour_region_decoder.py [--blocks 5] [--steps 20] [--crops 8] [--size 2048x2048] [--region 256x256]
"""
import argparse
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
import colour as colour_profile  # noqa: E402
import colour_decoder as colour_decoder_profile  # noqa: E402
import autoencoder_based_image_compression_amd as package  # noqa: E402
from autoencoder_based_image_compression_amd import codec, colour, container, pipeline  # noqa: E402
from autoencoder_based_image_compression_amd import device as dev  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats  # noqa: E402

NOTES_HEADING = '\n## Notes'
(event_times, blocks_of) = (colour_decoder_profile.event_times, colour_decoder_profile.blocks_of)


def pair(text):
    (a, b) = (int(side) for side in text.split('x'))
    return (a, b)


def positions(rng, count, size, region):
    return [(int(rng.randint(0, size[0] - region[0] + 1)), int(rng.randint(0, size[1] - region[1] + 1))) for _ in range(count)]


def kernel_legs(args, device):
    (size, region, n) = (args.size, args.region, args.crops)
    rng = numpy.random.RandomState(3)
    chroma = dev.chroma_region_size(size, region)
    crops = [rng.randint(0, 256, size=(n,) + shape).astype(numpy.uint8) for shape in (region, chroma, chroma)]
    origins = numpy.array(positions(rng, n, size, region), dtype=numpy.int32)
    expected = colour.merge_420_region_numpy(*crops, size, origins).reshape(-1)
    on_device = [torch.from_numpy(plane).to(device) for plane in crops]
    whole = [torch.from_numpy(rng.randint(0, 256, size=(n,) + shape).astype(numpy.uint8)).to(device)
             for shape in (region, dev.chroma_size(*region), dev.chroma_size(*region))]
    (picture, room) = (expected.size, dev.colour_words_bytes(n, *region))
    result = []
    for (place, flat, where) in (('device', torch.zeros(room, dtype=torch.uint8, device=device), torch.from_numpy(origins).to(device)),
                                 ('pinned', torch.zeros(room, dtype=torch.uint8).pin_memory(), torch.from_numpy(origins.copy()).pin_memory())):
        dev.colour_merge_420_crops(*on_device, size, where, flat)
        torch.cuda.synchronize()
        if not numpy.array_equal((flat.cpu() if flat.is_cuda else flat).numpy()[:picture], expected):
            raise SystemExit('colour_merge_420_crops into {0} memory is not colour.merge_420_region_numpy'.format(place))
        legs = (('colour_merge_420_words, {0} pictures of the region\'s size'.format(n), lambda: dev.colour_merge_420_words(*whole, region, flat)),
                ('colour_merge_420_crops, {0} crops'.format(n), lambda: dev.colour_merge_420_crops(*on_device, size, where, flat)))
        for round_index in range(2):
            for (name, fn) in legs:
                result.append({'what': 'kernel', 'leg': name, 'destination': place, 'round': round_index, 'output_bytes': picture,
                               'microseconds': event_times(fn, args.repeat)})
    return result


def step_legs(variables, bin_widths, rgb, args, device):
    (count, h, w, _) = rgb.shape
    (size, region, n) = ((h, w), args.region, args.crops)
    length = bench.TRUNCATED_UNARY_LENGTH
    encoder = pipeline.DeviceEncoder(variables, False, device)
    decoder = pipeline.DeviceDecoder(variables, False, device)
    (H, W) = dev.coded_size(h, w)
    luma = numpy.pad(colour.split_420_numpy(rgb[:1])[0], ((0, 0), (0, H - h), (0, W - w)), mode='edge')
    y0 = encoder(torch.from_numpy(luma).to(device))
    map_mean = dev.map_means(y0).cpu().numpy()
    probabilities = lossless_stats.compute_binary_probabilities(y0.cpu().numpy(), bin_widths, map_mean, length)
    del y0
    (blob, _) = container.encode_colour_images(rgb, encoder, bin_widths, map_mean, probabilities, bench.IDX_MAP_EXCEPTION,
                                               coding_tile=args.coding_tile)
    source = codec.ColourRegionSource(blob)
    rng = numpy.random.RandomState(5)
    steps = [[(source, int(rng.randint(count))) + at for at in positions(rng, n, size, region)] for _ in range(args.steps)]
    lines = []
    with codec.ColourRegionDecoder(variables, False, n, h, w, length, args.coding_tile, region, use_graphs=True) as d:
        first = d.submit(steps[0]).result()
        for (k, (_, image, y0_, x0_)) in enumerate(steps[0]):
            if not numpy.array_equal(first[k], container.decode_colour_region(blob, decoder, (y0_, x0_) + region, images=[image])[0]):
                raise SystemExit('ColourRegionDecoder is not decode_colour_region')
        inner = {'nb_streams': d.luma.nb_streams, 'use_graphs': True, 'pad': True}
        with codec.RegionDecoder(variables, False, n, h, w, length, args.coding_tile, region, nb_in_flight=d.luma.nb_in_flight, **inner) as luma_alone, \
                codec.RegionDecoder(variables, False, n, d.hc, d.wc, length, args.coding_tile, d.chroma_region,
                                    nb_in_flight=d.chroma.nb_in_flight, **inner) as chroma_alone:
            planned = [d._plan(requests)[1] for requests in steps]          # the requests of the Y, Cb and Cr steps
            for ticket in (luma_alone.submit(planned[0][0]), chroma_alone.submit(planned[0][1]), chroma_alone.submit(planned[0][2])):
                ticket.result()

            def colour_steps():
                kept = []

                def run():
                    kept.extend(d.submit(requests) for requests in steps)
                    d.drain()
                out = base.timed(run, len(steps))[0]
                kept[-1].result()
                return out

            def inner_steps():
                kept = []

                def run():
                    for planes in planned:
                        kept.extend((luma_alone.submit(planes[0]), chroma_alone.submit(planes[1]), chroma_alone.submit(planes[2])))
                    luma_alone.drain()
                    chroma_alone.drain()
                out = base.timed(run, len(steps))[0]
                for ticket in kept[-3:]:
                    ticket.result()
                return out

            turn = [0]

            def one_region():
                (_, image, y0_, x0_) = steps[turn[0] % len(steps)][0]
                turn[0] += 1
                return base.timed(lambda: container.decode_colour_region(blob, decoder, (y0_, x0_) + region, images=[image]), 1)[0]

            def whole_picture():
                return base.timed(lambda: container.decode_colour_images(blob, decoder), 1)[0]

            measured = blocks_of({'ColourRegionDecoder step ({0} crops)'.format(n): colour_steps,
                                  'its three inner steps alone': inner_steps,
                                  'container.decode_colour_region, one request': one_region,
                                  'container.decode_colour_images, the {0} whole picture(s)'.format(count): whole_picture}, args.blocks)
            for (name, values) in measured.items():
                lines.append({'what': 'step', 'leg': name, 'ms': base.summary(values), 'depth': d.depth,
                              'luma': [d.luma.nb_streams, d.luma.nb_in_flight], 'chroma': [d.chroma.nb_streams, d.chroma.nb_in_flight],
                              'blob_bytes': len(blob), 'chroma_region': list(d.chroma_region)})
    return lines


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--blocks', type=int, default=5)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--crops', type=int, default=8)
    parser.add_argument('--pictures', type=int, default=1)
    parser.add_argument('--size', type=pair, default=(2048, 2048))
    parser.add_argument('--region', type=pair, default=(256, 256))
    parser.add_argument('--coding-tile', type=pair, default=(16, 16))
    parser.add_argument('--bin-widths', nargs='+', type=float, default=[1.0])
    parser.add_argument('--repeat', type=int, default=30)
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'colour_region_decoder.md'))
    args = parser.parse_args()
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for line in kernel_legs(args, device):
        emit(line)
    rgb = colour_profile.pictures(args.pictures, *args.size)
    for bin_width in args.bin_widths:
        variables = bench.synthetic_model(bin_width)
        for line in step_legs(variables, variables[var.BIN_WIDTHS_NAME], rgb, args, device):
            emit(dict(line, bin_width=bin_width))
        torch.cuda.empty_cache()
    write_report(args.output, lines, args)


def write_report(path, lines, args):
    def cell(s):
        return '{0} ({1} .. {2})'.format(s['median'], s['min'], s['max'])

    name = lambda p: '{0} x {1}'.format(*p)
    out = ['# RGB crops out of tile-indexed EAC1 containers: the crop merge and the ColourRegionDecoder step', '',
           'Written by `profiles/colour_region_decoder.py`: {0} crops of {1} per step at random positions out of {2} picture(s) of {3}, coding tile '
           '{4}; {5} hardware queues (GPU_MAX_HW_QUEUES, set by: {6}).'.format(args.crops, name(args.region), args.pictures, name(args.size),
                                                                               name(args.coding_tile), package.HW_QUEUES[0], package.HW_QUEUES[1]), '',
           '## The two merge kernels on as many output bytes, into the same destination', '',
           'Device events, median (min .. max) of {0} launches each, in microseconds; the sibling and the new kernel alternate, twice.'.format(args.repeat),
           '', '| destination | round | launch | microseconds |', '|---|---|---|---|']
    out += ['| {0} | {1} | {2} | {3} |'.format(line['destination'], line['round'], line['leg'], cell(line['microseconds']))
            for line in lines if line['what'] == 'kernel']
    for bin_width in args.bin_widths:
        rows = [line for line in lines if line['what'] == 'step' and line['bin_width'] == bin_width]
        if not rows:
            continue
        out += ['', '## Bin width {0}: the step'.format(bin_width), '',
                '{0} blocks of {1} steps per leg, alternating in one process; ms per step, median (min .. max) of the blocks; the two synchronous '
                'functions are one call per block. Luminance decoder {2} streams and {3} steps in flight, chroma decoder {4} and {5}, graphs; ring '
                'depth {6}; chroma rectangle {7}; the blob has {8} bytes.'.format(args.blocks, args.steps, rows[0]['luma'][0], rows[0]['luma'][1],
                                                                                 rows[0]['chroma'][0], rows[0]['chroma'][1], rows[0]['depth'],
                                                                                 name(rows[0]['chroma_region']), rows[0]['blob_bytes']), '',
                '| leg | ms per step (per call) |', '|---|---|']
        out += ['| {0} | {1} |'.format(line['leg'], cell(line['ms'])) for line in rows]
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
