#!/usr/bin/env python
"""The rate ladder, measured (profiles/rate_ladder.md).

    python profiles/rate_ladder.py --sweep      CPU only: the host coder's arithmetic-coded stream against the cost of its decisions,
                                                the sweep behind ratecontrol.ALLOWANCE_LOW / ALLOWANCE_HIGH / floor_bits
    python profiles/rate_ladder.py [--calls 30] on the GPU, 24 Kodak-sized synthetic images (bench.py's images and model):
      (a) device.ladder_histograms at L = 10, K = 1, 3, 9 against K x (quantize_maps(want_symbols) + symbol_histograms), the route
          stats.compute_binary_probabilities takes today, and against reading y once at the copy rate of DESIGN.md section 11;
          device events around each call, median of `--calls`
      (b) container.encode_images_to_budget at a budget in the middle of the ladder against brute force over the 9 points with
          container.encode_images; attempts per image and upper_bound_misses
      (c) over a sweep of budgets, the share of images whose first attempt was the final choice
One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from autoencoder_based_image_compression_amd import ratecontrol  # noqa: E402
from autoencoder_based_image_compression_amd.kodak.lossless import interface_cython  # noqa: E402

MULTIPLIERS = numpy.array([1., 1.25, 1.5, 2., 3., 4., 6., 8., 10.], dtype=numpy.float32)    # collecting_stats_eae_extra.py:44
COPY_RATE_TBS = 5.93                                                                         # DESIGN.md section 11, tile_copy


def emit(**fields):
    print(json.dumps(fields), flush=True)


# ---- the sweep -------------------------------------------------------------------------------------------------------------------

def clipped_histogram(symbols, length):
    return numpy.bincount(numpy.minimum(numpy.abs(symbols.astype(numpy.int64)), length), minlength=length + 1)


def fitted_table(symbols, length):
    return ratecontrol.probabilities_from_counts(*ratecontrol.decision_counts(clipped_histogram(symbols, length)))


def sweep():
    from autoencoder_based_image_compression_amd import device as dev
    rng = numpy.random.RandomState(0)
    rows = []
    skipped = 0
    for length in (1, 4, 10):
        for size in (1, 2, 24, 96, 384, 1536, 4096, 16384):
            for scale in (0., 0.05, 0.3, 1., 3., 12.):
                for _ in range(3 if size >= 4096 else 6):
                    symbols = numpy.rint(rng.laplace(size=size)*scale).astype(numpy.int16)

                    def fit(factor):
                        return fitted_table(numpy.rint(rng.laplace(size=max(size, 64))*scale*factor).astype(numpy.int16), length)

                    tables = (('matched', fit(1.)), ('mismatched 1.5x', fit(1.5)), ('own', fitted_table(symbols, length)),
                              ('mismatched 0.1x', fit(.1)), ('mismatched 10x', fit(10.)), ('all 0.99', numpy.full(length, 0.99)),
                              ('all 0.01', numpy.full(length, 0.01)), ('all 0.999', numpy.full(length, 0.999)),
                              ('all 0.001', numpy.full(length, 0.001)))
                    (zeros, ones) = ratecontrol.decision_counts(clipped_histogram(symbols, length))
                    exact = int(dev._bypass_bits_of_magnitudes(numpy.abs(symbols.astype(numpy.int64)), length).sum())
                    for (kind, table) in tables:
                        try:
                            (_, bac_bits, _, bypass_bits) = interface_cython.encode_flattened_map(symbols, table)
                        except RuntimeError:             # the stream outgrows the coder's capacity (32 bits per symbol)
                            skipped += 1
                            continue
                        rows.append((kind, size, length, bac_bits, float(ratecontrol.ideal_bits(zeros, ones, table)),
                                     float(ratecontrol.floor_bits(zeros, ones, table)), bypass_bits == exact))
    kinds = numpy.array([r[0] for r in rows])
    sizes = numpy.array([r[1] for r in rows])
    (actual, ideal, floor) = (numpy.array([r[k] for r in rows], dtype=numpy.float64) for k in (3, 4, 5))
    fitted = numpy.isin(kinds, ['matched', 'mismatched 1.5x', 'own'])

    def span(x):
        return [round(float(x.min()), 3), round(float(x.max()), 3)]

    emit(sweep='all', maps=len(rows), skipped_over_capacity=skipped, bypass_formula_exact=bool(all(r[6] for r in rows)),
         actual_minus_ideal=span(actual - ideal), actual_minus_ceil_ideal=span(actual - numpy.ceil(ideal)),
         actual_minus_floor_of_floor_bits=span(actual - numpy.floor(floor)))
    emit(sweep='fitted tables (matched, mismatched 1.5x, own)', maps=int(fitted.sum()), actual_minus_ideal=span((actual - ideal)[fitted]),
         actual_minus_floor_ideal=span((actual - numpy.floor(ideal))[fitted]), actual_minus_ceil_ideal=span((actual - numpy.ceil(ideal))[fitted]))
    for kind in sorted(set(kinds.tolist())):
        m = kinds == kind
        emit(sweep='table', table=kind, maps=int(m.sum()), actual_minus_ideal=span((actual - ideal)[m]),
             actual_minus_floor_of_floor_bits=span((actual - numpy.floor(floor))[m]))
    for size in sorted(set(sizes.tolist())):
        m = sizes == size
        emit(sweep='size', symbols=int(size), fitted_actual_minus_ideal=span((actual - ideal)[m & fitted]),
             all_actual_minus_ideal=span((actual - ideal)[m]), fitted_ideal_minus_floor_bits_max=round(float((ideal - floor)[m & fitted].max()), 3))


# ---- the GPU measurements ----------------------------------------------------------------------------------------------------------

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


def gpu(calls):
    import torch
    import bench
    from autoencoder_based_image_compression_amd import container, pipeline
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats
    (n, h, w, length) = (24, 512, 768, 10)
    v = bench.synthetic_model(0.05)
    images = bench.synthetic_images(0, n, h, w)
    encoder = pipeline.DeviceEncoder(v, False)
    y = encoder(torch.from_numpy(images).cuda())
    y_host = y.cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y_host)
    bin_widths_points = (MULTIPLIERS[:, None]*v[var.BIN_WIDTHS_NAME][None, :]).astype(numpy.float32)
    (mean_d, bw_d) = (torch.from_numpy(map_mean).cuda(), torch.from_numpy(bin_widths_points).cuda())
    emit(device=dev.device_info(), images=n, height=h, width=w, length=length, y_megabytes=round(y.numel()*4/1e6, 1),
         read_y_once_us=round(y.numel()*4/(COPY_RATE_TBS*1e12)*1e6, 2), max_points=dev.ladder_max_points(length))

    # (a) the kernel against the K-pass route; outputs preallocated for both, so that the launches are what is timed
    for k_points in (1, 3, 9):
        out = (torch.zeros((n, k_points, 128, length + 1), dtype=torch.int32, device='cuda'),
               torch.zeros((n, k_points, 128), dtype=torch.int64, device='cuda'), torch.zeros(k_points, dtype=torch.int32, device='cuda'))
        symbols = torch.empty((n, 128, (h//16)*(w//16)), dtype=torch.int16, device='cuda')
        checks = torch.zeros(3, dtype=torch.int32, device='cuda')
        hist = (torch.zeros((n*128, 2*255 + 1), dtype=torch.int32, device='cuda'), torch.zeros(n*128, dtype=torch.int32, device='cuda'))

        def one_pass():
            dev.ladder_histograms(y, bw_d[:k_points], mean_d, length, out=out)

        def k_passes():
            for k in range(k_points):
                q = dev.quantize_maps(y, bw_d[k], mean_d, want_symbols=True, out_symbols=symbols, out_checks=checks)
                dev.symbol_histograms(q['symbols'], 255, out=hist, zero=False)

        emit(measurement='a', k_points=k_points, ladder_histograms=median_event_ms(torch, one_pass, calls),
             quantize_and_histogram_per_point=median_event_ms(torch, k_passes, calls))

    # tables for (b) and (c): one pass, as save_statistics would use it
    tables = lossless_stats.compute_binary_probabilities_ladder(y_host, bin_widths_points, map_mean, length)
    ladder = ratecontrol.RateLadder(bin_widths_points, tables, map_mean)

    # (b) the whole function against brute force
    t0 = time.perf_counter()
    sizes = numpy.array([[len(container.encode_images(images[i:i + 1], encoder, bin_widths_points[k], map_mean, tables[k])[0])
                          for k in range(len(MULTIPLIERS))] for i in range(n)])
    torch.cuda.synchronize()
    brute_ms = (time.perf_counter() - t0)*1e3
    budget = int(numpy.median(sizes[:, len(MULTIPLIERS)//2]))
    container.encode_images_to_budget(images, encoder, ladder, budget)                     # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    (blobs, info) = container.encode_images_to_budget(images, encoder, ladder, budget)
    torch.cuda.synchronize()
    budget_ms = (time.perf_counter() - t0)*1e3
    emit(measurement='b', budget_bytes=budget, sizes_min=sizes.min(axis=0).tolist(), sizes_max=sizes.max(axis=0).tolist(),
         encode_images_to_budget_ms=round(budget_ms, 1), brute_force_9_points_ms=round(brute_ms, 1),
         attempts_per_image=round(float(info['attempts'].mean()), 3), attempts_max=int(info['attempts'].max()),
         upper_bound_misses=int(info['upper_bound_misses']), fits=int(info['fits'].sum()),
         bounds_hold=bool((info['lower_bytes'] <= sizes).all() and (sizes <= info['upper_bytes']).all()),
         upper_minus_lower_bytes_max=int((info['upper_bytes'] - info['lower_bytes']).max()),
         upper_minus_actual_bytes_max=int((info['upper_bytes'] - sizes).max()), actual_minus_lower_bytes_max=int((sizes - info['lower_bytes']).max()))

    # (c) the selection over a sweep of budgets
    (first_final, total, misses) = (0, 0, 0)
    for budget in numpy.linspace(sizes.min()*0.9, sizes.max()*1.05, 12).astype(numpy.int64).tolist():
        (_, info) = container.encode_images_to_budget(images, encoder, ladder, budget)
        first_final += int((info['attempts'] == 1).sum())
        total += n
        misses += int(info['upper_bound_misses'])
    emit(measurement='c', budgets=12, images=total, first_attempt_was_final=first_final, share=round(first_final/total, 4), upper_bound_misses=misses)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--sweep', action='store_true')
    parser.add_argument('--calls', type=int, default=30)
    args = parser.parse_args()
    if args.sweep:
        sweep()
    else:
        gpu(args.calls)
