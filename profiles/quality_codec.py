#!/usr/bin/env python
"""`codec.QualityCodec`, measured (profiles/quality_codec.md). On the GPU, 24 Kodak-sized synthetic images
(bench.py's images and model at bin width 0.05), the ladder of profiles/rate_ladder.py: the reference's nine multipliers, L = 10.

    python profiles/quality_codec.py [--calls 30] [--blocks 7] [--steps 20] [--hw-queues 16]
      (a) device.quality_search alone, device events around each call, median of `--calls`: round 0, a middle round and the last;
          and the launches of one probe (quantiser without symbols, tconv1, tconv2, tconv3 without a uint8 plane) the same way
      (b) the QualityCodec step in `codec.product_mode` against the BudgetCodec step (the parent code path: same images, same ladder,
          every image's budget the bound of the point the search takes): `--blocks` blocks of `--steps` pipelined steps each, the two codecs
          alternating, host clock from the first submit to the last result; median over the blocks. The difference against
          R x (one probe + one round) from (a). Then the same 24 images through container.encode_images_to_quality.
      (c) over ten thresholds -- every image's squared error at point j of the ladder, and one nothing meets --: the points taken,
          `met`, and whether the host loop takes the same points
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
    ladder = ratecontrol.RateLadder(bin_widths_points, tables, map_mean)
    k_points = ladder.nb_points
    nb_rounds = ratecontrol.quality_rounds(k_points)
    (mean_d, bw_d) = (torch.from_numpy(map_mean).cuda(), torch.from_numpy(bin_widths_points).cuda())
    emit(device=dev.device_info(), gpu_max_hw_queues=os.environ.get('GPU_MAX_HW_QUEUES'), images=n, height=h, width=w, length=length,
         k_points=k_points, nb_rounds=nb_rounds)

    # (a) the round alone, and the launches of one probe
    first = torch.zeros(n, dtype=torch.int32, device='cuda')
    max_sse = torch.full((n,), int(ratecontrol.max_sse_for_psnr(32., h*w)), dtype=torch.int64, device='cuda')
    state = torch.zeros((n, 2), dtype=torch.int32, device='cuda')
    probe_acc = torch.zeros(n, dtype=torch.int64, device='cuda')
    point = torch.zeros(n, dtype=torch.int32, device='cuda')
    prob_row = torch.zeros((n, 128), dtype=torch.int32, device='cuda')
    trace_point = torch.zeros((n, nb_rounds), dtype=torch.int32, device='cuda')
    trace_sse = torch.zeros((n, nb_rounds), dtype=torch.int64, device='cuda')
    flags = torch.zeros(n, dtype=torch.int32, device='cuda')
    searches = {}
    for r in (0, 1, nb_rounds):
        searches[r] = median_event_ms(torch, lambda: dev.quality_search(first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags,
                                                            k_points, r, -1, k_points*128), calls)
        emit(measurement='a', launch='quality_search', round=r, **searches[r])
    dev.quality_search(first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags, k_points, 0, -1, k_points*128)
    igdn = (decoder.g[4], decoder.v['decoder/beta_4'])
    d = decoder.v
    latent = torch.empty_like(y)
    ws = dev.conv_workspace(y.device)
    probe = {}
    probe['probe_latent'] = median_event_ms(torch, lambda: dev.latent_quantize_rows(y, bw_d, point, mean_d, igdn_out=igdn, want_symbols=False,
                                                                                    want_checks=False, out_t=latent), calls)
    t1 = dev.tconv5x5s2(latent, decoder.w4, d['decoder/biases_4'], dev.NORM_IGDN, decoder.g[5], d['decoder/beta_5'], workspace=ws)
    probe['probe_tconv1_igdn5'] = median_event_ms(torch, lambda: dev.tconv5x5s2(latent, decoder.w4, d['decoder/biases_4'], dev.NORM_IGDN, decoder.g[5],
                                                                                d['decoder/beta_5'], out=t1, workspace=ws), calls)
    t2 = dev.tconv5x5s2(t1, decoder.w5, d['decoder/biases_5'], dev.NORM_IGDN, decoder.g[6], d['decoder/beta_6'], workspace=ws)
    probe['probe_tconv2_igdn6'] = median_event_ms(torch, lambda: dev.tconv5x5s2(t1, decoder.w5, d['decoder/biases_5'], dev.NORM_IGDN, decoder.g[6],
                                                                                d['decoder/beta_6'], out=t2, workspace=ws), calls)
    probe['probe_tconv3'] = median_event_ms(torch, lambda: dev.tconv9x9s4_luma(t2, decoder.w6, want_f32=False, want_u8=False, ref_u8=images_d,
                                                                              sse=probe_acc), calls)
    one_probe = sum(m['median_ms'] for m in probe.values())
    search_ms = searches[1]['median_ms']
    emit(measurement='a', launch='one probe', one_probe_median_ms=round(one_probe, 4), **probe)
    del t1, t2, latent

    # (b) the step, the two codecs alternating; every image's budget is the bound of the point the search takes for it, so that both
    # codecs quantise, code and synthesise the same points and the difference is the search
    # (the synthetic model is no trained one, its PSNR is a few dB at every point: the thresholds are taken from its own table, every
    # image's squared error at the middle point of the ladder, and said as max_sse)
    table = numpy.stack([dev.sse_u8(decoder(dev.quantize_maps(y, bw_d[k], mean_d, want_shifted=True)['shifted'])[1], images_d).cpu().numpy()
                         for k in range(k_points)], axis=1)
    psnr = 10.*numpy.log10(255.**2*h*w/numpy.maximum(table, 1))
    emit(measurement='table', images_whose_squared_error_never_falls_along_the_ladder=int((numpy.diff(table, axis=1) >= 0).all(axis=1).sum()),
         mean_psnr_per_point=[round(float(p), 3) for p in psnr.mean(axis=0)])
    options = codec.product_mode(h, w)
    target = table[:, k_points//2].copy()
    quality_codec = codec.QualityCodec(v, False, ladder, n, h, w, max_sse=target, **options)
    result = quality_codec.submit(images_d).result()
    budgets = result['upper_bound_bytes'][numpy.arange(n), result['rate_point']]
    budget_codec = codec.BudgetCodec(v, False, ladder, n, h, w, budget_bytes=budgets, **options)
    same_points = bool(numpy.array_equal(budget_codec.submit(images_d).result()['rate_point'], result['rate_point']))
    submits = {'quality_codec': lambda: quality_codec.submit(images_d), 'budget_codec': lambda: budget_codec.submit(images_d)}
    for submit in submits.values():
        block_ms_per_step(torch, submit, steps)                                          # warm: captures the graphs
    timings = {name: [] for name in submits}
    for _ in range(blocks):
        for (name, submit) in submits.items():
            timings[name].append(block_ms_per_step(torch, submit, steps))
    result = quality_codec.submit(images_d).result()
    medians = {name: float(numpy.median(t)) for (name, t) in timings.items()}
    emit(measurement='b', mode=options, streams_run={'transform': quality_codec.nb_transform_streams, 'coder': quality_codec.nb_in_flight},
         max_sse='the squared error at point {0}'.format(k_points//2), rate_points=numpy.bincount(result['rate_point'], minlength=k_points).tolist(),
         met=int(result['met'].sum()), budget_codec_takes_the_same_points=same_points,
         blocks=blocks, steps_per_block=steps, step_difference_ms=round(medians['quality_codec'] - medians['budget_codec'], 4),
         expected_difference_ms=round(nb_rounds*(one_probe + search_ms), 4),
         **{name + '_ms_per_step': {'median': round(medians[name], 4), 'min': round(min(t), 4), 'max': round(max(t), 4)}
            for (name, t) in timings.items()})
    budget_codec.close()
    container.encode_images_to_quality(images, encoder, decoder, ladder, max_sse=target)          # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    (_, info) = container.encode_images_to_quality(images, encoder, decoder, ladder, max_sse=target)
    torch.cuda.synchronize()
    emit(measurement='b', encode_images_to_quality_ms=round((time.perf_counter() - t0)*1e3, 1),
         same_points_as_the_codec=bool(numpy.array_equal(info['rate_point'], result['rate_point'])))

    # (c) a sweep of thresholds: every image's squared error at point j, then one nothing meets
    for j in list(range(k_points)) + [None]:
        thresholds = table[:, j].copy() if j is not None else table.min(axis=1) - 1
        r = quality_codec.submit(images_d, max_sse=thresholds).result()
        (_, info) = container.encode_images_to_quality(images, encoder, decoder, ladder, max_sse=thresholds)
        emit(measurement='c', max_sse_is_the_squared_error_at_point=j, rate_points=numpy.bincount(r['rate_point'], minlength=k_points).tolist(),
             met=int(r['met'].sum()), mean_blob_bytes=int(r['blob_bytes'].mean()),
             probes_match_the_table=bool(numpy.array_equal(r['probe_sse'], numpy.take_along_axis(table, r['probe_points'], axis=1))),
             host_loop_agrees=bool(numpy.array_equal(info['rate_point'], r['rate_point']) and numpy.array_equal(info['probe_sse'], r['probe_sse'])))
    quality_codec.close()


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--calls', type=int, default=30)
    parser.add_argument('--blocks', type=int, default=7)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--hw-queues', type=int, default=None, help='GPU_MAX_HW_QUEUES of this process (default: the environment\'s, else 16)')
    args = parser.parse_args()
    main(args.calls, args.blocks, args.steps)
