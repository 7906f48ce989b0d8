#!/usr/bin/env python
"""`codec.TiledQualityCodec`, measured (profiles/tiled_quality_codec.md). On the GPU, 24 Kodak-sized synthetic
images (bench.py's images and model at bin width 0.05), the ladder of profiles/rate_ladder.py: the reference's nine multipliers,
L = 10; coding tiles of 16 and 8 latents (6 and 24 tiles of the 32 x 48 latent plane).

    python profiles/tiled_quality_codec.py [--calls 30] [--blocks 7] [--steps 20] [--hw-queues 4]
      (a) device.quality_search_tiles alone against device.quality_search, device events around each call, median of `--calls`: round
          0, a middle round and the last, at T = 1, 6, 24 and 96 tiles per image
      (b) per coding tile, the TiledQualityCodec step in `codec.product_mode` against the TiledBudgetCodec step (the parent code path:
          same images, same ladder, every image's budget the bound of the point the search takes) and against the QualityCodec step on
          the same thresholds, hence the same points: `--blocks` blocks of `--steps` pipelined steps each, the three codecs alternating,
          host clock from the first submit to the last result; median over the blocks. Then the same 24 images through
          container.encode_images_to_quality(coding_tile=...).
One JSON line per measurement on stdout.
"""
import argparse
import os
import sys
import time

import numpy

# as bench.py: the product mode's streams need their hardware queues, asked for before the runtime comes up (--hw-queues)
if '--hw-queues' in sys.argv[1:-1]:
    os.environ['GPU_MAX_HW_QUEUES'] = str(int(sys.argv[sys.argv.index('--hw-queues') + 1]))
else:
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '4')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

from quality_codec import MULTIPLIERS, block_ms_per_step, emit, median_event_ms  # noqa: E402

from autoencoder_based_image_compression_amd import ratecontrol  # noqa: E402


def main(calls, blocks, steps):
    import torch
    import bench
    from autoencoder_based_image_compression_amd import codec, container, pipeline
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats
    (n, h, w, length) = (24, 512, 768, 10)
    (h_map, w_map) = (h//16, w//16)
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

    # (a) the round alone: whole maps, then 1, 6, 24 and 96 tiles per image
    first = torch.zeros(n, dtype=torch.int32, device='cuda')
    max_sse = torch.full((n,), int(ratecontrol.max_sse_for_psnr(32., h*w)), dtype=torch.int64, device='cuda')
    state = torch.zeros((n, 2), dtype=torch.int32, device='cuda')
    probe_acc = torch.zeros(n, dtype=torch.int64, device='cuda')
    point = torch.zeros(n, dtype=torch.int32, device='cuda')
    trace_point = torch.zeros((n, nb_rounds), dtype=torch.int32, device='cuda')
    trace_sse = torch.zeros((n, nb_rounds), dtype=torch.int64, device='cuda')
    flags = torch.zeros(n, dtype=torch.int32, device='cuda')
    prob_row = torch.zeros((n, 128), dtype=torch.int32, device='cuda')
    whole = {}
    for r in (0, 1, nb_rounds):
        whole[r] = median_event_ms(torch, lambda: dev.quality_search(first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags,
                                                                     k_points, r, -1, k_points*128), calls)
        emit(measurement='a', launch='quality_search', round=r, **whole[r])
    for tile in (48, 16, 8, 4):
        layout = codec.coding_tile_layout(n, h_map, w_map, (tile, tile))
        nb_tiles = layout['nb_tiles']
        run_entry = torch.from_numpy(layout['run_entry'].astype(numpy.int32)).cuda()
        rows = torch.zeros((n*nb_tiles, 128), dtype=torch.int32, device='cuda')
        for r in (0, 1, nb_rounds):
            m = median_event_ms(torch, lambda: dev.quality_search_tiles(first, max_sse, state, probe_acc, point, rows, trace_point, trace_sse, flags,
                                                                        run_entry, nb_tiles, k_points, r, -1, k_points*128), calls)
            emit(measurement='a', launch='quality_search_tiles', coding_tile=tile, nb_tiles=nb_tiles, words_written=n*nb_tiles*128, round=r,
                 ratio_to_quality_search=round(m['median_ms']/whole[r]['median_ms'], 3), **m)
        rows_right = bool(numpy.array_equal(rows.cpu().numpy().reshape(-1), codec.tile_prob_rows(layout, point.cpu().numpy(), -1, k_points*128)))
        emit(measurement='a', coding_tile=tile, rows_equal_the_host_rule=rows_right)

    # (b) the step; the thresholds are taken from the model's own table (profiles/quality_codec.py says why): every image's squared
    # error at the middle point of the ladder
    table = numpy.stack([dev.sse_u8(decoder(dev.quantize_maps(y, bw_d[k], mean_d, want_shifted=True)['shifted'])[1], images_d).cpu().numpy()
                         for k in range(k_points)], axis=1)
    target = table[:, k_points//2].copy()
    options = codec.product_mode(h, w)
    quality_codec = codec.QualityCodec(v, False, ladder, n, h, w, max_sse=target, **options)
    whole_points = quality_codec.submit(images_d).result()['rate_point']
    for tile in (16, 8):
        coding_tile = (tile, tile)
        tiled_quality = codec.TiledQualityCodec(v, False, ladder, n, h, w, coding_tile, max_sse=target, **options)
        ticket = tiled_quality.submit(images_d)
        result = ticket.result()
        blobs = ticket.image_containers()
        budgets = result['upper_bound_bytes'][numpy.arange(n), result['rate_point']]
        tiled_budget = codec.TiledBudgetCodec(v, False, ladder, n, h, w, coding_tile, budget_bytes=budgets, **options)
        same_points = bool(numpy.array_equal(tiled_budget.submit(images_d).result()['rate_point'], result['rate_point']))
        submits = {'tiled_quality_codec': lambda: tiled_quality.submit(images_d), 'tiled_budget_codec': lambda: tiled_budget.submit(images_d),
                   'quality_codec': lambda: quality_codec.submit(images_d)}
        for submit in submits.values():
            block_ms_per_step(torch, submit, steps)                                      # warm: captures the graphs
        timings = {name: [] for name in submits}
        for _ in range(blocks):
            for (name, submit) in submits.items():
                timings[name].append(block_ms_per_step(torch, submit, steps))
        medians = {name: float(numpy.median(t)) for (name, t) in timings.items()}
        emit(measurement='b', coding_tile=tile, nb_tiles=tiled_quality._tile_layout['nb_tiles'], mode=options,
             streams_run={'transform': tiled_quality.nb_transform_streams, 'coder': tiled_quality.nb_in_flight},
             max_sse='the squared error at point {0}'.format(k_points//2), rate_points=numpy.bincount(result['rate_point'], minlength=k_points).tolist(),
             met=int(result['met'].sum()), tiled_budget_codec_takes_the_same_points=same_points,
             quality_codec_takes_the_same_points=bool(numpy.array_equal(whole_points, result['rate_point'])),
             probes_match_the_table=bool(numpy.array_equal(result['probe_sse'], numpy.take_along_axis(table, result['probe_points'], axis=1))),
             blocks=blocks, steps_per_block=steps, against_tiled_budget_codec_ms=round(medians['tiled_quality_codec'] - medians['tiled_budget_codec'], 4),
             against_quality_codec_ms=round(medians['tiled_quality_codec'] - medians['quality_codec'], 4),
             **{name + '_ms_per_step': {'median': round(medians[name], 4), 'min': round(min(t), 4), 'max': round(max(t), 4)}
                for (name, t) in timings.items()})
        tiled_budget.close()
        tiled_quality.close()
        container.encode_images_to_quality(images, encoder, decoder, ladder, max_sse=target, coding_tile=coding_tile)          # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        (host_blobs, info) = container.encode_images_to_quality(images, encoder, decoder, ladder, max_sse=target, coding_tile=coding_tile)
        torch.cuda.synchronize()
        emit(measurement='b', coding_tile=tile, encode_images_to_quality_ms=round((time.perf_counter() - t0)*1e3, 1),
             same_points_as_the_codec=bool(numpy.array_equal(info['rate_point'], result['rate_point'])),
             same_blobs_as_the_codec=[bytes(b) for b in host_blobs] == [bytes(b) for b in blobs])
    quality_codec.close()


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--calls', type=int, default=30)
    parser.add_argument('--blocks', type=int, default=7)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--hw-queues', type=int, default=None, help='GPU_MAX_HW_QUEUES of this process (default: the environment\'s, else 4)')
    args = parser.parse_args()
    main(args.calls, args.blocks, args.steps)
