#!/usr/bin/env python
"""`codec.BudgetCodec`, measured (profiles/budget_codec.md). On the GPU, 24 Kodak-sized synthetic images
(bench.py's images and model at bin width 0.05), the ladder of profiles/rate_ladder.py: the reference's nine multipliers, L = 10.

    python profiles/budget_codec.py [--calls 30] [--blocks 7] [--steps 20] [--hw-queues 16]
      (a) device.ladder_select and device.latent_quantize_rows alone, device events around each call, median of `--calls`;
          latent_quantize_rows against device.latent_stage with one row of bin widths (no gdn_3, the same inputs and outputs)
      (b) the BudgetCodec step in `codec.product_mode` against BatchCodec(emit_container=True) at the point most images select:
          `--blocks` blocks of `--steps` pipelined steps each, the two codecs alternating, host clock from the first submit to the last
          result; median over the blocks. Then the same 24 images through container.encode_images_to_budget.
      (c) over the twelve budgets of profiles/rate_ladder.md (c): images on a coarser point than encode_images_to_budget chose, and
          images with `promised` and not `fits`
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

MULTIPLIERS = numpy.array([1., 1.25, 1.5, 2., 3., 4., 6., 8., 10.], dtype=numpy.float32)    # collecting_stats_eae_extra.py:44


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
    y = encoder(images_d)
    y_host = y.cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y_host)
    bin_widths_points = (MULTIPLIERS[:, None]*v[var.BIN_WIDTHS_NAME][None, :]).astype(numpy.float32)
    tables = lossless_stats.compute_binary_probabilities_ladder(y_host, bin_widths_points, map_mean, length)
    ladder = ratecontrol.RateLadder(bin_widths_points, tables, map_mean)
    k_points = ladder.nb_points
    (mean_d, bw_d) = (torch.from_numpy(map_mean).cuda(), torch.from_numpy(bin_widths_points).cuda())
    emit(device=dev.device_info(), gpu_max_hw_queues=os.environ.get('GPU_MAX_HW_QUEUES'), images=n, height=h, width=w, length=length,
         k_points=k_points, y_megabytes=round(y.numel()*4/1e6, 1))

    # (a) the two launches alone
    (hist, bypass, _) = dev.ladder_histograms(y, bw_d, mean_d, length)
    upper = ratecontrol.upper_bounds_fixed(hist.cpu().numpy(), bypass.cpu().numpy(), ladder, map_size)
    budget = int(numpy.median(upper[:, k_points//2]))
    budgets_d = torch.full((n,), budget, dtype=torch.int64, device='cuda')
    costs_d = torch.from_numpy(ratecontrol.fixed_costs(ladder).view(numpy.int32)).cuda()
    selected = dev.ladder_select(hist, bypass, costs_d, None, -1, ratecontrol.header_bytes(ladder), map_size, budgets_d, k_points*128)
    points = selected['point'].cpu().numpy()
    most = int(numpy.bincount(points, minlength=k_points).argmax())
    emit(measurement='a', launch='ladder_select', budget_bytes=budget, points=numpy.bincount(points, minlength=k_points).tolist(),
         **median_event_ms(torch, lambda: dev.ladder_select(hist, bypass, costs_d, None, -1, ratecontrol.header_bytes(ladder), map_size,
                                                            budgets_d, k_points*128, out=selected), calls))
    decoder = pipeline.DeviceDecoder(v, False)
    igdn = (decoder.g[4], decoder.v['decoder/beta_4'])
    symbols = torch.empty((n, 128, map_size), dtype=torch.int16, device='cuda')
    flags = torch.zeros((n, 128), dtype=torch.int32, device='cuda')
    checks = torch.zeros(3, dtype=torch.int32, device='cuda')
    rows = median_event_ms(torch, lambda: dev.latent_quantize_rows(y, bw_d, selected['point'], mean_d, igdn_out=igdn, want_flags=True,
                                                                   out_symbols=symbols, out_flags=flags, out_checks=checks), calls)
    one = median_event_ms(torch, lambda: dev.latent_stage(y, bw_d[most], mean_d, gdn_in=None, igdn_out=igdn, want_flags=True,
                                                          out_symbols=symbols, out_flags=flags, out_checks=checks), calls)
    emit(measurement='a', launch='latent_quantize_rows', rows_per_image=rows, latent_stage_one_row_no_gdn3=one)

    # (b) the step, the two codecs alternating
    options = codec.product_mode(h, w)
    budget_codec = codec.BudgetCodec(v, False, ladder, n, h, w, budget_bytes=budget, **options)
    batch_codec = codec.BatchCodec(v, False, bin_widths_points[most], map_mean, tables[most], -1, n, h, w, emit_container=True, **options)
    submits = {'budget_codec': lambda: budget_codec.submit(images_d), 'batch_codec': lambda: batch_codec.submit(images_d)}
    for submit in submits.values():
        block_ms_per_step(torch, submit, steps)                                          # warm: captures the graphs
    timings = {name: [] for name in submits}
    for _ in range(blocks):
        for (name, submit) in submits.items():
            timings[name].append(block_ms_per_step(torch, submit, steps))
    result = budget_codec.submit(images_d).result()
    emit(measurement='b', mode=options, streams_run={'transform': budget_codec.nb_transform_streams, 'coder': budget_codec.nb_in_flight},
         most_selected_point=most, rate_points=numpy.bincount(result['rate_point'], minlength=k_points).tolist(),
         blocks=blocks, steps_per_block=steps,
         **{name + '_ms_per_step': {'median': round(float(numpy.median(t)), 4), 'min': round(min(t), 4), 'max': round(max(t), 4)}
            for (name, t) in timings.items()})
    batch_codec.close()
    container.encode_images_to_budget(images, encoder, ladder, budget)                     # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    container.encode_images_to_budget(images, encoder, ladder, budget)
    torch.cuda.synchronize()
    emit(measurement='b', encode_images_to_budget_ms=round((time.perf_counter() - t0)*1e3, 1), budget_bytes=budget)

    # (c) against the host loop over the twelve budgets of profiles/rate_ladder.md
    sizes = numpy.array([[len(container.encode_images(images[i:i + 1], encoder, bin_widths_points[k], map_mean, tables[k])[0])
                          for k in range(k_points)] for i in range(n)])
    (coarser, finer, promised_not_fitting, not_promised, total) = (0, 0, 0, 0, 0)
    for b in numpy.linspace(sizes.min()*0.9, sizes.max()*1.05, 12).astype(numpy.int64).tolist():
        (_, info) = container.encode_images_to_budget(images, encoder, ladder, b)
        r = budget_codec.submit(images_d, b).result()
        coarser += int((r['rate_point'] > info['rate_point']).sum())
        finer += int((r['rate_point'] < info['rate_point']).sum())
        promised_not_fitting += int((r['promised'] & ~r['fits']).sum())
        not_promised += int((~r['promised']).sum())
        total += n
    emit(measurement='c', budgets=12, images=total, coarser_than_encode_images_to_budget=coarser, finer=finer,
         promised_and_not_fits=promised_not_fitting, not_promised=not_promised)
    budget_codec.close()


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--calls', type=int, default=30)
    parser.add_argument('--blocks', type=int, default=7)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--hw-queues', type=int, default=None, help='GPU_MAX_HW_QUEUES of this process (default: the environment\'s, else 16)')
    args = parser.parse_args()
    main(args.calls, args.blocks, args.steps)
