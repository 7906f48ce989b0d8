#!/usr/bin/env python
"""The rate-control codecs on a ladder with a price, measured (profiles/rdo_ladder.md). On the GPU, 24 Kodak-sized
synthetic images (bench.py's images and model at bin width 0.05), the ladder of profiles/rate_ladder.py: the reference's nine
multipliers, L = 10, tables fitted on these latents; the price is rdo_lambda = 2 bw_k^2 at every point.

    python profiles/rdo_ladder.py [--calls 30] [--blocks 5] [--steps 20] [--hw-queues 16]
      (a) device.ladder_histograms_rdo against device.ladder_histograms of the same tree on the same latents (24 x 32 x 48, K = 9), device
          events around each call, median of `--calls`, the launches alternating, twice; with the ladder's thresholds and with thresholds
          of zeros; then the tiles pair at tiles of 16 and of 8. And what the device says a block may ask for in LDS: what staging the
          table there would need (106 KB at K = 9, L = 10).
      (b) the step of BudgetCodec, TiledBudgetCodec (tiles of 16) and QualityCodec in `codec.product_mode` with the price in the ladder
          against the same codec on the same ladder without: `--blocks` blocks of `--steps` pipelined steps each, the two codecs
          alternating, host clock from the first submit to the last result; median over the blocks.
      (c) what the price buys, at 2 bw^2 and at 0.2 bw^2: over twelve budgets, the images that land on a finer point than without the
          price, and the blob sizes; at a floor per image (the squared error of the middle point without a price, and 1 % above it),
          the mean blob size with and without.
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
LAMBDA_IN_BINS = 2.


def emit(**fields):
    print(json.dumps(fields), flush=True)


def event_ms(torch, fn, calls):
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


def summary(times):
    return {'median': round(float(numpy.median(times)), 4), 'min': round(min(times), 4), 'max': round(max(times), 4)}


def main(calls, blocks, steps):
    import torch
    import bench
    from autoencoder_based_image_compression_amd import codec, pipeline
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats
    (n, h, w, length) = (24, 512, 768, 10)
    v = bench.synthetic_model(0.05)
    images = bench.synthetic_images(0, n, h, w)
    images_d = torch.from_numpy(images).cuda()
    encoder = pipeline.DeviceEncoder(v, False)
    decoder = pipeline.DeviceDecoder(v, False)
    y = encoder(images_d)
    y_host = y.cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y_host)
    bin_widths_points = (MULTIPLIERS[:, None]*v[var.BIN_WIDTHS_NAME][None, :]).astype(numpy.float32)
    tables = lossless_stats.compute_binary_probabilities_ladder(y_host, bin_widths_points, map_mean, length)
    lambdas = LAMBDA_IN_BINS*(bin_widths_points.astype(numpy.float64)**2).mean(axis=1)
    plain = ratecontrol.RateLadder(bin_widths_points, tables, map_mean)
    priced = ratecontrol.RateLadder(bin_widths_points, tables, map_mean, rdo_lambda=lambdas)
    k_points = plain.nb_points
    (mean_d, bw_d) = (torch.from_numpy(map_mean).cuda(), torch.from_numpy(bin_widths_points).cuda())
    thresholds = torch.from_numpy(priced.rdo_thresholds_points).cuda()
    by_magnitude = dev.rdo_thresholds_by_magnitude(thresholds)
    zeros = torch.zeros_like(thresholds)
    properties = torch.cuda.get_device_properties(0)
    emit(device=dev.device_info(), gpu_max_hw_queues=os.environ.get('GPU_MAX_HW_QUEUES'), images=n, height=h, width=w, length=length,
         k_points=k_points, lambda_in_bins=LAMBDA_IN_BINS, y_megabytes=round(y.numel()*4/1e6, 1),
         lds_bytes_a_block_may_ask_for={name: getattr(properties, name) for name in ('shared_memory_per_block', 'shared_memory_per_block_optin',
                                                                                      'shared_memory_per_multiprocessor')
                                        if hasattr(properties, name)},
         lds_bytes_to_stage_the_table=k_points*(length + 3 + min(length, 16))*128*4)

    # (a) the count against its sibling, whole maps and per tile
    plane = y.view(n, h//16, w//16, 128)
    nearest = dev.ladder_histograms(y, bw_d, mean_d, length)
    counted = dev.ladder_histograms_rdo(y, bw_d, thresholds, mean_d, length, by_magnitude=by_magnitude)
    nonzero = (nearest[0].sum(dim=(0, 2)).sum(dim=1) - nearest[0][..., 0].sum(dim=(0, 2))).cpu().numpy()
    lowered_to_zero = (counted[0][..., 0].sum(dim=(0, 2)) - nearest[0][..., 0].sum(dim=(0, 2))).cpu().numpy()
    emit(measurement='a', nonzero_symbols_per_point=nonzero.tolist(), symbols_lowered_to_zero_per_point=lowered_to_zero.tolist(),
         bypass_bits_per_point={'nearest': nearest[1].sum(dim=(0, 2)).tolist(), 'rdo': counted[1].sum(dim=(0, 2)).tolist()})

    def pair(name, out, launch_nearest, launch_rdo):
        timings = {}
        for round_ in range(2):
            timings['nearest_%d' % round_] = event_ms(torch, lambda: launch_nearest(out), calls)
            timings['rdo_%d' % round_] = event_ms(torch, lambda: launch_rdo(out, thresholds), calls)
            timings['rdo_zero_thresholds_%d' % round_] = event_ms(torch, lambda: launch_rdo(out, zeros), calls)
        emit(measurement='a', launch=name, ratio_rdo_to_nearest=round(timings['rdo_1']['median_ms']/timings['nearest_1']['median_ms'], 3),
             **timings)

    zeros_by_magnitude = dev.rdo_thresholds_by_magnitude(zeros)

    def launch_whole_rdo(out, table):
        return dev.ladder_histograms_rdo(y, bw_d, table, mean_d, length, out=out,
                                         by_magnitude=by_magnitude if table is thresholds else zeros_by_magnitude)

    pair('ladder_histograms[_rdo]', tuple(torch.zeros_like(t) for t in nearest),
         lambda out: dev.ladder_histograms(y, bw_d, mean_d, length, out=out), launch_whole_rdo)
    for tile in (16, 8):
        first = dev.ladder_histograms_tiles(plane, bw_d, (tile, tile), mean_d, length)

        def launch_tiles_rdo(out, table, tile=tile):
            return dev.ladder_histograms_rdo_tiles(plane, bw_d, table, (tile, tile), mean_d, length, out=out,
                                                   by_magnitude=by_magnitude if table is thresholds else zeros_by_magnitude)

        pair('ladder_histograms[_rdo]_tiles, tiles of %d' % tile, tuple(torch.zeros_like(t) for t in first),
             lambda out, tile=tile: dev.ladder_histograms_tiles(plane, bw_d, (tile, tile), mean_d, length, out=out), launch_tiles_rdo)
        del first

    # the middle point's bound and squared error without a price: the budget and the floor of (b) and (c)
    map_size = (h//16)*(w//16)
    upper = ratecontrol.upper_bounds_fixed(nearest[0].cpu().numpy(), nearest[1].cpu().numpy(), plain, map_size)
    budget = int(numpy.median(upper[:, k_points//2]))
    floor = numpy.zeros(n, dtype=numpy.int64)
    for i in range(n):
        q = dev.quantize_maps(y[i:i + 1], bw_d[k_points//2], mean_d, want_shifted=True)
        (_, decoded, _) = decoder(q['shifted'])
        floor[i] = int(dev.sse_u8(decoded, images_d[i:i + 1]).item())

    # (b) the steps, a codec with the price against the same codec without, alternating
    options = codec.product_mode(h, w)
    makers = {'BudgetCodec': (lambda ladder: codec.BudgetCodec(v, False, ladder, n, h, w, budget_bytes=budget, **options),
                              lambda c: c.submit(images_d)),
              'TiledBudgetCodec, tiles of 16': (lambda ladder: codec.TiledBudgetCodec(v, False, ladder, n, h, w, (16, 16), budget_bytes=budget,
                                                                                     **options), lambda c: c.submit(images_d)),
              'QualityCodec': (lambda ladder: codec.QualityCodec(v, False, ladder, n, h, w, max_sse=floor, **options), lambda c: c.submit(images_d))}
    kept = {}
    for (name, (make, submit)) in makers.items():
        codecs = {'with_price': make(priced), 'without': make(plain)}
        submits = {key: (lambda c=c: submit(c)) for (key, c) in codecs.items()}
        for s in submits.values():
            block_ms_per_step(torch, s, steps)                                           # warm: captures the graphs
        timings = {key: [] for key in submits}
        for _ in range(blocks):
            for (key, s) in submits.items():
                timings[key].append(block_ms_per_step(torch, s, steps))
        results = {key: s().result() for (key, s) in submits.items()}
        emit(measurement='b', codec=name, mode=options, blocks=blocks, steps_per_block=steps,
             rate_points={key: numpy.bincount(r['rate_point'], minlength=k_points).tolist() for (key, r) in results.items()},
             mean_blob_bytes={key: round(float(r['blob_bytes'].mean()), 1) for (key, r) in results.items()},
             **{key + '_ms_per_step': summary(t) for (key, t) in timings.items()})
        if name == 'TiledBudgetCodec, tiles of 16':
            for c in codecs.values():
                c.close()
        else:
            kept[name] = codecs

    # (c) what the price buys, at the price of (a) and (b) and at a tenth of it
    for c in kept['BudgetCodec'].values():
        c.close()
    kept['QualityCodec']['with_price'].close()
    plain_budget = makers['BudgetCodec'][0](plain)
    plain_quality = kept['QualityCodec']['without']
    budgets = numpy.linspace(upper.min()*0.9, upper.max()*1.05, 12).astype(numpy.int64).tolist()
    for in_bins in (LAMBDA_IN_BINS, LAMBDA_IN_BINS/10.):
        ladder = ratecontrol.RateLadder(bin_widths_points, tables, map_mean,
                                        rdo_lambda=in_bins*(bin_widths_points.astype(numpy.float64)**2).mean(axis=1))
        with makers['BudgetCodec'][0](ladder) as priced_budget:
            (finer, coarser, total, promised_not_fitting) = (0, 0, 0, 0)
            (bytes_with, bytes_without) = ([], [])
            for b in budgets:
                r = priced_budget.submit(images_d, b).result()
                p = plain_budget.submit(images_d, b).result()
                finer += int((r['rate_point'] < p['rate_point']).sum())
                coarser += int((r['rate_point'] > p['rate_point']).sum())
                promised_not_fitting += int((r['promised'] & ~r['fits']).sum())
                total += n
                bytes_with.append(float(r['blob_bytes'].mean()))
                bytes_without.append(float(p['blob_bytes'].mean()))
        emit(measurement='c', lambda_in_bins=in_bins, at='twelve budgets', images=total, on_a_finer_point_with_the_price=finer,
             on_a_coarser_point=coarser, promised_and_not_fits=promised_not_fitting,
             mean_blob_bytes_with=round(float(numpy.mean(bytes_with)), 1), mean_blob_bytes_without=round(float(numpy.mean(bytes_without)), 1))
        # (the model is not a trained one: its squared error barely depends on the symbols, so the floor is also tried 1 % higher)
        with makers['QualityCodec'][0](ladder) as priced_quality:
            for slack in (1., 1.01):
                floors = (floor*slack).astype(numpy.int64)
                r = priced_quality.submit(images_d, max_sse=floors).result()
                p = plain_quality.submit(images_d, max_sse=floors).result()
                emit(measurement='c', lambda_in_bins=in_bins,
                     at='a floor per image: %.2f times the squared error of point %d without a price' % (slack, k_points//2),
                     met={'with_price': int(r['met'].sum()), 'without': int(p['met'].sum())},
                     rate_points={'with_price': numpy.bincount(r['rate_point'], minlength=k_points).tolist(),
                                  'without': numpy.bincount(p['rate_point'], minlength=k_points).tolist()},
                     mean_blob_bytes={'with_price': round(float(r['blob_bytes'].mean()), 1), 'without': round(float(p['blob_bytes'].mean()), 1)},
                     mean_sse={'with_price': round(float(r['sse'].mean()), 1), 'without': round(float(p['sse'].mean()), 1)})
    plain_budget.close()
    plain_quality.close()


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--calls', type=int, default=30)
    parser.add_argument('--blocks', type=int, default=5)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--hw-queues', type=int, default=None, help='GPU_MAX_HW_QUEUES of this process (default: the environment\'s, else 16)')
    args = parser.parse_args()
    main(args.calls, args.blocks, args.steps)
