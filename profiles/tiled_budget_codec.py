#!/usr/bin/env python
"""`codec.TiledBudgetCodec` and its two launches, measured (profiles/tiled_budget_codec.md). On the GPU, 24
Kodak-sized synthetic images (bench.py's images and model at bin width 0.05), the ladder of profiles/rate_ladder.py: the reference's
nine multipliers, L = 10; coding tiles of 16 and of 8 latents.

    python profiles/tiled_budget_codec.py [--calls 30] [--blocks 7] [--steps 20] [--hw-queues 4] [--out profiles/tiled_budget_codec.md]
    (--hw-queues: GPU_MAX_HW_QUEUES of the process; without it the environment's, else 16. The recorded numbers were taken at 4.)
      (a) device.ladder_histograms_tiles against device.ladder_histograms on the same latents, device events around each call, median
          of `--calls`; the zeroing of the accumulators on its own
      (b) device.ladder_select_tiles alone
      (c) the TiledBudgetCodec step in `codec.product_mode` against BatchCodec(emit_container=True, coding_tile=...) at the point most
          images select, and against BudgetCodec (whole maps) on the same ladder: `--blocks` blocks of `--steps` pipelined steps each,
          the codecs alternating, host clock from the first submit to the last result; median over the blocks
      (d) over the twelve budgets of profiles/rate_ladder.md (c): the gap between the upper bound and the real size, images on a
          coarser point than encode_images_to_budget(coding_tile=...) chose, and images with `promised` and not `fits`
One JSON line per measurement on stdout; `--out` gets the same lines as a document.
"""
import argparse
import json
import os
import sys

import numpy

# as bench.py: the product mode's streams need their hardware queues, asked for before the runtime comes up (--hw-queues)
if '--hw-queues' in sys.argv[1:-1]:
    os.environ['GPU_MAX_HW_QUEUES'] = str(int(sys.argv[sys.argv.index('--hw-queues') + 1]))
else:
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '16')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

from budget_codec import MULTIPLIERS, block_ms_per_step, median_event_ms  # noqa: E402

from autoencoder_based_image_compression_amd import ratecontrol  # noqa: E402

LINES = []


def emit(**fields):
    LINES.append(json.dumps(fields))
    print(LINES[-1], flush=True)


def spread(values):
    return {'median': round(float(numpy.median(values)), 4), 'min': round(min(values), 4), 'max': round(max(values), 4)}


def main(calls, blocks, steps, out):
    import torch
    import bench
    from autoencoder_based_image_compression_amd import codec, container, pipeline
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats
    (n, h, w, length) = (24, 512, 768, 10)
    (h_map, w_map) = (h//16, w//16)
    map_size = h_map*w_map
    v = bench.synthetic_model(0.05)
    images = bench.synthetic_images(0, n, h, w)
    images_d = torch.from_numpy(images).cuda()
    encoder = pipeline.DeviceEncoder(v, False)
    y = encoder(images_d).view(n, h_map, w_map, 128)
    y_host = y.cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y_host)
    bin_widths_points = (MULTIPLIERS[:, None]*v[var.BIN_WIDTHS_NAME][None, :]).astype(numpy.float32)
    tables = lossless_stats.compute_binary_probabilities_ladder(y_host, bin_widths_points, map_mean, length)
    ladder = ratecontrol.RateLadder(bin_widths_points, tables, map_mean)
    k_points = ladder.nb_points
    (mean_d, bw_d) = (torch.from_numpy(map_mean).cuda(), torch.from_numpy(bin_widths_points).cuda())
    costs_d = torch.from_numpy(ratecontrol.fixed_costs(ladder).view(numpy.int32)).cuda()
    emit(device=dev.device_info(), gpu_max_hw_queues=os.environ.get('GPU_MAX_HW_QUEUES'), images=n, height=h, width=w, length=length,
         k_points=k_points, y_megabytes=round(y.numel()*4/1e6, 1))
    whole = dev.ladder_histograms(y, bw_d, mean_d, length)
    whole_ms = median_event_ms(torch, lambda: dev.ladder_histograms(y, bw_d, mean_d, length, out=whole), calls)
    options = codec.product_mode(h, w)
    for side in (16, 8):
        coding_tile = (side, side)
        # (a) the histograms per tile against the whole-map kernel
        out_t = dev.ladder_histograms_tiles(y, bw_d, coding_tile, mean_d, length)
        (hist, bypass) = (out_t[0].clone(), out_t[1].clone())
        assert torch.equal(hist.sum(dim=2), whole[0]//(3 + calls + 1))         # (the whole-map buffers accumulated over the timed calls)
        tiles_ms = median_event_ms(torch, lambda: dev.ladder_histograms_tiles(y, bw_d, coding_tile, mean_d, length, out=out_t), calls)
        accum = torch.zeros(out_t[0].numel() + 2*out_t[1].numel() + k_points, dtype=torch.int32, device='cuda')
        zero_ms = median_event_ms(torch, lambda: accum.zero_(), calls)
        emit(measurement='a', coding_tile=side, nb_tiles=int(hist.shape[2]), accumulator_megabytes=round(accum.numel()*4/1e6, 2),
             ladder_histograms_tiles=tiles_ms, ladder_histograms=whole_ms, ratio=round(tiles_ms['median_ms']/whole_ms['median_ms'], 3),
             zeroing=zero_ms)
        # (b) the selection alone
        header = ratecontrol.header_bytes(ladder, h, w, coding_tile)
        upper = ratecontrol.upper_bounds_fixed_tiles(hist.cpu().numpy(), bypass.cpu().numpy(), ladder, map_size, header)
        budget = int(numpy.median(upper[:, k_points//2]))
        budgets_d = torch.full((n,), budget, dtype=torch.int64, device='cuda')
        layout = codec.coding_tile_layout(n, h_map, w_map, coding_tile)
        images_of = torch.from_numpy(numpy.array([layout['entries'][p][0] for p in layout['payload_entry'].tolist()], dtype=numpy.int32)).cuda()
        selected = dev.ladder_select_tiles(hist, bypass, costs_d, None, -1, header, map_size, budgets_d, images_of, k_points*128)
        assert numpy.array_equal(selected['upper'].cpu().numpy(), upper)
        points = selected['point'].cpu().numpy()
        most = int(numpy.bincount(points, minlength=k_points).argmax())
        emit(measurement='b', coding_tile=side, launch='ladder_select_tiles', budget_bytes=budget,
             points=numpy.bincount(points, minlength=k_points).tolist(),
             **median_event_ms(torch, lambda: dev.ladder_select_tiles(hist, bypass, costs_d, None, -1, header, map_size, budgets_d, images_of,
                                                                      k_points*128, out=selected), calls))
        # (c) the step, the codecs alternating
        tiled_codec = codec.TiledBudgetCodec(v, False, ladder, n, h, w, coding_tile, budget_bytes=budget, **options)
        batch_codec = codec.BatchCodec(v, False, bin_widths_points[most], map_mean, tables[most], -1, n, h, w, emit_container=True,
                                       coding_tile=coding_tile, **options)
        whole_upper = ratecontrol.upper_bounds_fixed((whole[0]//(3 + calls + 1)).cpu().numpy(), (whole[1]//(3 + calls + 1)).cpu().numpy(), ladder, map_size)
        budget_codec = codec.BudgetCodec(v, False, ladder, n, h, w, budget_bytes=int(numpy.median(whole_upper[:, k_points//2])), **options)
        submits = {'tiled_budget_codec': lambda: tiled_codec.submit(images_d), 'batch_codec_tiles': lambda: batch_codec.submit(images_d),
                   'budget_codec_whole_maps': lambda: budget_codec.submit(images_d)}
        for submit in submits.values():
            block_ms_per_step(torch, submit, steps)                                          # warm: captures the graphs
        timings = {name: [] for name in submits}
        for _ in range(blocks):
            for (name, submit) in submits.items():
                timings[name].append(block_ms_per_step(torch, submit, steps))
        result = tiled_codec.submit(images_d).result()
        emit(measurement='c', coding_tile=side, mode=options, most_selected_point=most,
             rate_points=numpy.bincount(result['rate_point'], minlength=k_points).tolist(), blocks=blocks, steps_per_block=steps,
             **{name + '_ms_per_step': spread(t) for (name, t) in timings.items()})
        batch_codec.close()
        budget_codec.close()
        # (d) the bound and the choices against the host loop over the twelve budgets of profiles/rate_ladder.md
        sizes = numpy.array([[len(container.encode_images(images[i:i + 1], encoder, bin_widths_points[k], map_mean, tables[k],
                                                          coding_tile=coding_tile)[0]) for k in range(k_points)] for i in range(n)])
        gap = upper - sizes
        (coarser, finer, promised_not_fitting, not_promised, total) = (0, 0, 0, 0, 0)
        for b in numpy.linspace(sizes.min()*0.9, sizes.max()*1.05, 12).astype(numpy.int64).tolist():
            (_, info) = container.encode_images_to_budget(images, encoder, ladder, b, coding_tile=coding_tile)
            r = tiled_codec.submit(images_d, b).result()
            coarser += int((r['rate_point'] > info['rate_point']).sum())
            finer += int((r['rate_point'] < info['rate_point']).sum())
            promised_not_fitting += int((r['promised'] & ~r['fits']).sum())
            not_promised += int((~r['promised']).sum())
            total += n
        emit(measurement='d', coding_tile=side, streams_per_image=int(hist.shape[2])*128, blob_bytes={'min': int(sizes.min()), 'max': int(sizes.max())},
             upper_minus_real_bytes={'min': int(gap.min()), 'median': int(numpy.median(gap)), 'max': int(gap.max())},
             upper_minus_real_bytes_per_stream=round(float(numpy.median(gap))/(int(hist.shape[2])*128), 3),
             budgets=12, images=total, coarser_than_encode_images_to_budget=coarser, finer=finer, promised_and_not_fits=promised_not_fitting,
             not_promised=not_promised)
        tiled_codec.close()
    if out:
        with open(out, 'w') as f:
            f.write('# `codec.TiledBudgetCodec`, measured\n\n`python profiles/tiled_budget_codec.py --hw-queues {3}` on one MI355X (GPU_MAX_HW_QUEUES = {3}: `product_mode` runs 1 + 2 streams at 4, 3 + 6 at 16; every leg of a comparison shares the process): 24 images of 512 x 768, the nine '
                    'multipliers on bin width 0.05, L = 10, coding tiles of 16 and 8 latents. (a) the histograms per tile against the whole-map '
                    'kernel, device events, median of {0}; (b) the selection alone; (c) alternating blocks of {1} pipelined steps, host clock, '
                    'median of {2} blocks; (d) the bound and the choices over twelve budgets. DESIGN.md section 20 reads them.\n\n```\n'.format(
                        calls, steps, blocks, os.environ.get('GPU_MAX_HW_QUEUES')))
            f.write('\n'.join(LINES) + '\n```\n')


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--calls', type=int, default=30)
    parser.add_argument('--blocks', type=int, default=7)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--hw-queues', type=int, default=None, help='GPU_MAX_HW_QUEUES of this process (default: the environment\'s, else 16)')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tiled_budget_codec.md'))
    args = parser.parse_args()
    main(args.calls, args.blocks, args.steps, args.out)
