#!/usr/bin/env python
"""container.py of this tree against container.py of another commit (profiles/container_paths.md): byte identity of the blobs, cross
decode, and wall time per call in alternating blocks, on bench.py's images, model and statistics (24 images of 512 x 768, bin widths
1.0 and 0.05). A block is `--calls` calls of one version, each ending in a device synchronise; its figure is the mean per call. One
JSON line per measurement.

    git show <commit>:autoencoder_based_image_compression_amd/container.py > /tmp/container_parent.py
    python profiles/container_paths.py --parent /tmp/container_parent.py [--blocks 9] [--calls 10]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/container_paths.py --parent /tmp/container_parent.py --trace parent
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/container_paths.py --trace new

--trace: nothing but one EAE1 encode + decode of a (2, 64, 96) batch with the named version, for a kernel trace.
"""
import argparse
import gc
import importlib.util
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
from autoencoder_based_image_compression_amd import container as new  # noqa: E402
from autoencoder_based_image_compression_amd import pipeline  # noqa: E402
from autoencoder_based_image_compression_amd import device as dev  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats  # noqa: E402


def load_parent(path):
    """The other commit's container.py as a module of the package (its relative imports resolve to this tree's modules)."""
    spec = importlib.util.spec_from_file_location('autoencoder_based_image_compression_amd._container_parent', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def summary(values):
    ordered = sorted(values)
    return {'median': round(ordered[(len(ordered) - 1)//2], 4), 'min': round(ordered[0], 4), 'max': round(ordered[-1], 4)}


def first_difference(a, b):
    if a == b:
        return 'equal'
    n = min(len(a), len(b))
    x = numpy.frombuffer(a, dtype=numpy.uint8, count=n)
    y = numpy.frombuffer(b, dtype=numpy.uint8, count=n)
    d = numpy.flatnonzero(x != y)
    return 'first difference at offset {} (lengths {} / {})'.format(int(d[0]) if d.size else n, len(a), len(b))


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0)*1e3, out


def trace(container):
    variables = var.random_variables(1., False, seed=4, bias_std=0.01)
    variables['decoder/weights_6'] = (variables['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    with numpy.load(os.path.join(ROOT, 'tests', 'golden', 'coder_golden.npz')) as g:
        probabilities = g['real_probabilities_1']
    encoder = pipeline.DeviceEncoder(variables, False)
    decoder = pipeline.DeviceDecoder(variables, False)
    images = numpy.random.RandomState(1).randint(16, 236, size=(2, 64, 96)).astype(numpy.uint8)
    bin_widths = numpy.full(128, 0.5, dtype=numpy.float32)
    map_mean = numpy.random.RandomState(2).normal(scale=0.1, size=128).astype(numpy.float32)
    (blob, _) = container.encode_images(images, encoder, bin_widths, map_mean, probabilities, 67)
    reconstruction = container.decode_images(blob, decoder)
    torch.cuda.synchronize()
    print(json.dumps({'blob_bytes': len(blob), 'sum_of_pixels': int(reconstruction.astype(numpy.int64).sum())}), flush=True)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--parent', help='container.py of the commit to compare with')
    parser.add_argument('--blocks', type=int, default=9)
    parser.add_argument('--calls', type=int, default=10)
    parser.add_argument('--trace', choices=['parent', 'new'])
    args = parser.parse_args()
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    if args.trace == 'new':
        return trace(new)
    parent = load_parent(args.parent)
    if args.trace == 'parent':
        return trace(parent)
    (batch, h, w) = (24, 512, 768)
    images = bench.synthetic_images(1000, batch, h, w)
    for bin_width in (1.0, 0.05):
        variables = bench.synthetic_model(bin_width)
        bin_widths = variables[var.BIN_WIDTHS_NAME]
        encoder = pipeline.DeviceEncoder(variables, False, device)
        decoder = pipeline.DeviceDecoder(variables, False, device)
        y0 = encoder(torch.from_numpy(images).to(device))
        map_mean = dev.map_means(y0).cpu().numpy()
        probabilities = lossless_stats.compute_binary_probabilities(y0.cpu().numpy(), bin_widths, map_mean, bench.TRUNCATED_UNARY_LENGTH)
        del y0
        idx = bench.IDX_MAP_EXCEPTION
        versions = {'parent': parent, 'new': new}

        def enc(m, **kw):
            return m.encode_images(images, encoder, bin_widths, map_mean, probabilities, idx, **kw)[0]

        blobs = {name: {'EAE1': enc(m), 'EAT1': enc(m, coding_tile=(8, 12))} for (name, m) in versions.items()}
        identity = {'EAE1 blob, new vs parent': first_difference(blobs['new']['EAE1'], blobs['parent']['EAE1']),
                    'EAT1 blob, new vs parent': first_difference(blobs['new']['EAT1'], blobs['parent']['EAT1'])}
        for kind in ('EAE1', 'EAT1'):
            a = parent.decode_images(blobs['parent'][kind], decoder)
            b = new.decode_images(blobs['parent'][kind], decoder)
            identity['new decode of the parent\'s {} blob vs the parent\'s decode'.format(kind)] = \
                'equal' if numpy.array_equal(a, b) else 'first difference at element {}'.format(int(numpy.flatnonzero(a != b)[0]))
        (_, sa) = parent.decode_symbols(blobs['parent']['EAE1'])
        (_, sb) = new.decode_symbols(blobs['parent']['EAE1'])
        identity['new decode_symbols of the parent\'s EAE1 blob vs the parent\'s'] = 'equal' if torch.equal(sa, sb) and sa.shape == sb.shape else 'different'
        del sa, sb
        print(json.dumps({'what': 'identity', 'bin_width': bin_width, 'blob_bytes': {k: len(v) for (k, v) in blobs['parent'].items()}, **identity}), flush=True)

        measurements = {
            'encode_images EAE1': lambda m: enc(m),
            'decode_images EAE1': lambda m: m.decode_images(blobs['parent']['EAE1'], decoder),
            'encode_images(coding_tile=(8, 12)) + decode_images EAT1': lambda m: m.decode_images(enc(m, coding_tile=(8, 12)), decoder),
        }
        for (what, f) in measurements.items():
            for m in versions.values():
                for _ in range(2):
                    timed(lambda: f(m))
            times = {name: [] for name in versions}
            gc.collect()
            gc.disable()
            try:
                for _ in range(args.blocks):
                    for (name, m) in versions.items():          # alternating
                        times[name].append(sum(timed(lambda: f(m))[0] for _ in range(args.calls))/args.calls)
            finally:
                gc.enable()
            (p, n) = (summary(times['parent']), summary(times['new']))
            bound = p['median'] + (p['max'] - p['min'])
            print(json.dumps({'what': what, 'bin_width': bin_width, 'blocks': args.blocks, 'calls_per_block': args.calls, 'unit': 'ms per call of 24 images', 'parent': p, 'new': n,
                          'bound (parent median + parent spread)': round(bound, 4), 'holds': bool(n['median'] <= bound),
                          'parent_blocks': [round(t, 3) for t in times['parent']], 'new_blocks': [round(t, 3) for t in times['new']]}), flush=True)


if __name__ == '__main__':
    main()
