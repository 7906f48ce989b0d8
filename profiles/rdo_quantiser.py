#!/usr/bin/env python
"""The rate-distortion optimised quantiser, measured (profiles/rdo_quantiser.md). On the GPU, 24 Kodak-sized
synthetic images (bench.py's images and model at bin width 0.05), L = 10.

    python profiles/rdo_quantiser.py [--calls 30] [--blocks 7] [--steps 20] [--hw-queues 16]
      (a) device.latent_quantize_rdo against device.latent_quantize_rows of the same tree on the same latents and outputs (one row
          of bin widths, inverse_gdn_4, symbols, flags, checks), device events around each call, median of `--calls`; at the
          thresholds of lambda = 0.2 bw^2, and with thresholds of zeros
      (b) the step of BatchCodec(emit_container=True, rdo_lambda=...) in `codec.product_mode` against the same call with
          rdo_lambda=None (the parent's code path): `--blocks` blocks of `--steps` pipelined steps each, the two codecs alternating,
          host clock from the first submit to the last result; median over the blocks; then gdn_3 and the quantiser as the launches
          of their own the step gains, device events, against the latent stage they replace
      (c) rate and error for lambda over two decades, with tables fitted on these latents and with the authors' tables
          (tests/golden/coder_golden.npz): the share of the non-zero nearest-rounded symbols lowered, the coder's bits, the squared
          error of the latents and of the images (container.encode_images + decode_images)
One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import sys
import time

import numpy

# as bench.py: the product mode's streams need their hardware queues, asked for before the runtime comes up (--hw-queues)
if '--hw-queues' in sys.argv[1:-1]:
    os.environ['GPU_MAX_HW_QUEUES'] = str(int(sys.argv[sys.argv.index('--hw-queues') + 1]))
else:
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '16')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from autoencoder_based_image_compression_amd import ratecontrol  # noqa: E402

LAMBDA_IN_BINS = (0.02, 0.05, 0.1, 0.2, 0.5, 1., 2.)               # lambda / bw^2: squared bins per bit, two decades
STEP_LAMBDA_IN_BINS = 0.2


def emit(**fields):
    print(json.dumps(fields), flush=True)


def median_event_ms(torch, fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        (start, stop) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return {'median_ms': round(times[(len(times) - 1)//2], 4), 'min_ms': round(times[0], 4), 'max_ms': round(times[-1], 4)}


def block_ms_per_step(torch, submit, steps):
    """Host clock around `steps` pipelined steps, from the first submit to the last result, behind a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tickets = [submit() for _ in range(steps)]
    for ticket in tickets:
        ticket.result()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0)*1e3/steps


def main(calls, blocks, steps):
    import torch
    import bench
    from autoencoder_based_image_compression_amd import codec, container, pipeline
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats
    (n, h, w, length) = (24, 512, 768, 10)
    map_size = (h//16)*(w//16)
    v = bench.synthetic_model(0.05)
    images = bench.synthetic_images(0, n, h, w)
    images_d = torch.from_numpy(images).cuda()
    encoder = pipeline.DeviceEncoder(v, False)
    decoder = pipeline.DeviceDecoder(v, False)
    y = encoder(images_d)
    y_host = y.cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y_host)
    bin_widths = numpy.ascontiguousarray(v[var.BIN_WIDTHS_NAME], dtype=numpy.float32)
    width2 = float(bin_widths[0])**2
    fitted = lossless_stats.compute_binary_probabilities_ladder(y_host, bin_widths[None], map_mean, length)[0]
    with numpy.load(os.path.join(ROOT, 'tests', 'golden', 'coder_golden.npz')) as g:
        authors = numpy.ascontiguousarray(g['real_probabilities_1'], dtype=numpy.float64)
    assert authors.shape == fitted.shape and (bin_widths == bin_widths[0]).all()
    (mean_d, bw_d) = (torch.from_numpy(map_mean).cuda(), torch.from_numpy(bin_widths[None]).cuda())
    point = torch.zeros(n, dtype=torch.int32, device='cuda')
    emit(device=dev.device_info(), gpu_max_hw_queues=os.environ.get('GPU_MAX_HW_QUEUES'), images=n, height=h, width=w, length=length,
         bin_width=float(bin_widths[0]), y_megabytes=round(y.numel()*4/1e6, 1))

    # (a) the kernel against its sibling
    igdn = (decoder.g[4], decoder.v['decoder/beta_4'])
    symbols = torch.empty((n, 128, map_size), dtype=torch.int16, device='cuda')
    flags = torch.zeros((n, 128), dtype=torch.int32, device='cuda')
    checks = torch.zeros(3, dtype=torch.int32, device='cuda')
    step_lambda = STEP_LAMBDA_IN_BINS*width2
    thresholds = torch.from_numpy(ratecontrol.rdo_thresholds(bin_widths[None], fitted[None], step_lambda)).cuda()
    zero_thresholds = torch.zeros_like(thresholds)
    timings = {}
    for round_ in range(2):                                         # the three launches alternate: twice, the second round reported too
        timings['latent_quantize_rows_%d' % round_] = median_event_ms(torch, lambda: dev.latent_quantize_rows(
            y, bw_d, point, mean_d, igdn_out=igdn, want_flags=True, out_symbols=symbols, out_flags=flags, out_checks=checks), calls)
        timings['latent_quantize_rdo_%d' % round_] = median_event_ms(torch, lambda: dev.latent_quantize_rdo(
            y, bw_d, thresholds, point, length, mean_d, igdn_out=igdn, want_flags=True, out_symbols=symbols, out_flags=flags, out_checks=checks), calls)
        timings['latent_quantize_rdo_zero_thresholds_%d' % round_] = median_event_ms(torch, lambda: dev.latent_quantize_rdo(
            y, bw_d, zero_thresholds, point, length, mean_d, igdn_out=igdn, want_flags=True, out_symbols=symbols, out_flags=flags,
            out_checks=checks), calls)
    ratio = timings['latent_quantize_rdo_1']['median_ms']/timings['latent_quantize_rows_1']['median_ms']
    emit(measurement='a', lambda_in_bins=STEP_LAMBDA_IN_BINS, ratio_rdo_to_rows=round(ratio, 3), **timings)

    # (b) the step, the two codecs alternating; then the launches the step gains, alone
    options = codec.product_mode(h, w)
    rdo_codec = codec.BatchCodec(v, False, bin_widths, map_mean, fitted, -1, n, h, w, emit_container=True, rdo_lambda=step_lambda, **options)
    plain_codec = codec.BatchCodec(v, False, bin_widths, map_mean, fitted, -1, n, h, w, emit_container=True, **options)
    submits = {'rdo_lambda': lambda: rdo_codec.submit(images_d), 'rdo_lambda_none': lambda: plain_codec.submit(images_d)}
    for submit in submits.values():
        block_ms_per_step(torch, submit, steps)                                          # warm: captures the graphs
    block_timings = {name: [] for name in submits}
    for _ in range(blocks):
        for (name, submit) in submits.items():
            block_timings[name].append(block_ms_per_step(torch, submit, steps))
    emit(measurement='b', mode=options, lambda_in_bins=STEP_LAMBDA_IN_BINS, blocks=blocks, steps_per_block=steps,
         **{name + '_ms_per_step': {'median': round(float(numpy.median(t)), 4), 'min': round(min(t), 4), 'max': round(max(t), 4)}
            for (name, t) in block_timings.items()})
    rdo_codec.close()
    plain_codec.close()
    y_raw = torch.randn_like(y)
    gdn_in = (encoder.g[3], encoder.v['encoder/beta_3'])
    emit(measurement='b', launch='gdn_3 alone', **median_event_ms(torch, lambda: dev.gdn(y_raw, *gdn_in), calls))
    emit(measurement='b', launch='latent_stage (gdn_3 + quantiser + inverse_gdn_4): what the step without lambda runs',
         **median_event_ms(torch, lambda: dev.latent_stage(y_raw, bw_d[0], mean_d, gdn_in=gdn_in, igdn_out=igdn, want_flags=True, out_symbols=symbols,
                                                           out_flags=flags, out_checks=checks), calls))

    # (c) rate and error over two decades of lambda
    nearest = dev.latent_quantize_rows(y, bw_d, point, mean_d, want_shifted=True)
    nonzero = int((nearest['symbols'] != 0).sum().item())

    def row(table, rdo_lambda):
        arguments = (encoder, bin_widths, map_mean, table, -1)
        (blob, info) = container.encode_images(images, *arguments, rdo_lambda=rdo_lambda)
        decoded = container.decode_images(blob, decoder).astype(numpy.int64)
        out = {'coder_bits': int(info['nb_bits'].astype(numpy.int64).sum()), 'image_sse': int(((decoded - images.astype(numpy.int64))**2).sum())}
        if rdo_lambda is None:
            q = nearest
        else:
            t = torch.from_numpy(ratecontrol.rdo_thresholds(bin_widths[None], table[None], rdo_lambda)).cuda()
            q = dev.latent_quantize_rdo(y, bw_d, t, point, length, mean_d, want_shifted=True)
            out['share_of_nonzero_lowered'] = round(int((q['symbols'] != nearest['symbols']).sum().item())/float(nonzero), 5)
        out['latent_squared_error'] = float(((q['shifted'].double() - y.double())**2).sum().item())
        return out

    for (name, table) in (('fitted on these latents', fitted), ('the authors\' tables', authors)):
        base = row(table, None)
        emit(measurement='c', tables=name, rdo_lambda=None, nonzero_symbols=nonzero, symbols=n*128*map_size, **base)
        for in_bins in LAMBDA_IN_BINS:
            r = row(table, in_bins*width2)
            emit(measurement='c', tables=name, lambda_in_bins=in_bins, rdo_lambda=in_bins*width2,
                 bits_change_percent=round(100.*(r['coder_bits']/base['coder_bits'] - 1.), 2),
                 latent_error_change_percent=round(100.*(r['latent_squared_error']/base['latent_squared_error'] - 1.), 2),
                 image_sse_change_percent=round(100.*(r['image_sse']/base['image_sse'] - 1.), 3), **r)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--calls', type=int, default=30)
    parser.add_argument('--blocks', type=int, default=7)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--hw-queues', type=int, default=None, help='GPU_MAX_HW_QUEUES of this process (default: the environment\'s, else 16)')
    args = parser.parse_args()
    main(args.calls, args.blocks, args.steps)
