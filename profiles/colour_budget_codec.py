#!/usr/bin/env python
"""`codec.ColourBudgetCodec`, measured (profiles/colour_budget_codec.md). On the GPU, 24 RGB pictures of 512 x 768
(bench.py's synthetic images in every channel, its model at bin width 0.05), the ladder of profiles/budget_codec.py: the reference's
nine multipliers, L = 10, tables and map means measured on the luminance planes; Cb and Cr take the same ladder.

    python profiles/colour_budget_codec.py [--calls 30] [--blocks 7] [--steps 20] [--hw-queues 4]
      (a) device.colour_budget_rest alone, device events around each call, median of `--calls`
      (b) in ONE process, in alternating blocks of `--steps` pipelined steps, host clock from the first submit to the drain, median
          (min .. max) of `--blocks` blocks, every codec in `codec.product_mode` of its plane:
            the ColourBudgetCodec step at the default chroma share;
            its three inner `_PlaneBudgetCodec` steps alone -- the same planes and budgets submitted to `luma` and `chroma` directly,
            nothing waiting for anything: no split, no `colour_budget_rest`, no merge, and Y not behind chroma;
            the ColourCodec(emit_container=True) step at the points most pictures take;
          then the same pictures through container.encode_colour_images_to_budget, once warm
      (c) at that budget: the share of the blob's bytes the two chroma planes took
      (d) over twelve budgets from under the coarsest points' bounds to over the finest ones': pictures with `picture_promised` and not
          `picture_fits`, pictures not promised, and pictures that landed elsewhere than encode_colour_images_to_budget put them
One JSON line per measurement on stdout.
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy

# as bench.py: the product mode's streams need their hardware queues, asked for before the runtime comes up (--hw-queues)
if '--hw-queues' in sys.argv[1:-1]:
    os.environ['GPU_MAX_HW_QUEUES'] = str(int(sys.argv[sys.argv.index('--hw-queues') + 1]))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from autoencoder_based_image_compression_amd import ratecontrol  # noqa: E402

MULTIPLIERS = numpy.array([1., 1.25, 1.5, 2., 3., 4., 6., 8., 10.], dtype=numpy.float32)    # collecting_stats_eae_extra.py:44


def emit(**fields):
    print(json.dumps(fields), flush=True)


def summary(values):
    ordered = sorted(values)
    return {'median': round(ordered[(len(ordered) - 1)//2], 4), 'min': round(ordered[0], 4), 'max': round(ordered[-1], 4)}


def median_event_us(torch, fn, calls):
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
        times.append(start.elapsed_time(stop)*1e3)
    return summary(times)


def block_ms_per_step(torch, submit, drain, steps):
    """Host clock around `steps` pipelined steps, from the first submit to the end of the drain, behind a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kept = [submit() for _ in range(steps)]
    drain()
    torch.cuda.synchronize()
    elapsed = (time.perf_counter() - t0)*1e3/steps
    last = kept[-1]
    for ticket in (last if isinstance(last, tuple) else (last,)):
        ticket.result()
    return elapsed


def main(calls, blocks, steps):
    import torch
    import bench
    from autoencoder_based_image_compression_amd import codec, colour, container, pipeline
    from autoencoder_based_image_compression_amd import device as dev
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats
    (n, h, w, length) = (24, 512, 768, 10)
    (hc, wc) = dev.chroma_size(h, w)
    v = bench.synthetic_model(0.05)
    rgb = numpy.ascontiguousarray(numpy.stack([bench.synthetic_images(1000 + channel, n, h, w) for channel in range(3)], axis=3))
    rgb_d = torch.from_numpy(rgb).cuda()
    planes = colour.split_420_numpy(rgb)
    planes_d = [torch.from_numpy(plane).cuda() for plane in planes]
    encoder = pipeline.DeviceEncoder(v, False)
    y_host = encoder(planes_d[0]).cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y_host)
    bin_widths_points = (MULTIPLIERS[:, None]*v[var.BIN_WIDTHS_NAME][None, :]).astype(numpy.float32)
    tables = lossless_stats.compute_binary_probabilities_ladder(y_host, bin_widths_points, map_mean, length)
    del y_host
    ladder = ratecontrol.RateLadder(bin_widths_points, tables, map_mean)
    k_points = ladder.nb_points
    emit(device=dev.device_info(), gpu_max_hw_queues=os.environ.get('GPU_MAX_HW_QUEUES'), pictures=n, height=h, width=w, length=length,
         k_points=k_points)

    options = dict(chroma_options=codec.product_mode(hc, wc), **codec.product_mode(h, w))
    budget_codec = codec.ColourBudgetCodec(v, False, ladder, n, h, w, **options)
    first = budget_codec.submit(rgb_d, codec.QualityCodec.NO_BUDGET).result()
    upper = first['upper_bound_bytes']                                                    # (N, 3, K)
    header = container.COLOUR_HEADER_BYTES
    budget = int(numpy.median(header + upper[:, :, k_points//2].sum(axis=1)))
    r = budget_codec.submit(rgb_d, budget).result()
    most = [int(numpy.bincount(r['rate_point'][:, plane], minlength=k_points).argmax()) for plane in range(3)]

    # (a) the new launch alone, on the blocks of a finished step
    chroma_slots = [budget_codec.chroma._budget_slots[id(slot)] for slot in budget_codec.chroma._slots[:2]]
    budgets_d = torch.full((n,), budget, dtype=torch.int64, device='cuda')
    rest = torch.zeros(n, dtype=torch.int64, device='cuda')
    emit(measurement='a', launch='colour_budget_rest', pictures=n, microseconds=median_event_us(
        torch, lambda: dev.colour_budget_rest(budgets_d, chroma_slots[0].upper, chroma_slots[0].point, chroma_slots[1].upper, chroma_slots[1].point, rest),
        calls))

    # (b) the step against its siblings, alternating
    chroma_point = (bin_widths_points[most[1]], map_mean, tables[most[1]], -1)
    colour_codec = codec.ColourCodec(v, False, bin_widths_points[most[0]], map_mean, tables[most[0]], -1, n, h, w, chroma=chroma_point,
                                     emit_container=True, **options)
    luma_budgets_d = torch.from_numpy(numpy.ascontiguousarray(r['budget_bytes'][:, 0])).cuda()
    chroma_budgets = numpy.ascontiguousarray(r['budget_bytes'][:, 1])

    def inner_alone():
        return (budget_codec.luma.submit(planes_d[0], luma_budgets_d), budget_codec.chroma.submit(planes_d[1], chroma_budgets),
                budget_codec.chroma.submit(planes_d[2], chroma_budgets))

    legs = {'colour_budget_codec': (lambda: budget_codec.submit(rgb_d, budget), budget_codec.drain),
            'three_plane_budget_codecs_alone': (inner_alone, budget_codec.drain),
            'colour_codec_at_most_taken_points': (lambda: colour_codec.submit(rgb_d), colour_codec.drain)}
    for (submit, drain) in legs.values():
        block_ms_per_step(torch, submit, drain, steps)                                    # warm: captures the graphs
    timings = {name: [] for name in legs}
    gc.collect()
    gc.disable()
    try:
        for _ in range(blocks):
            for (name, (submit, drain)) in legs.items():                                  # alternating: every leg sees the same box at the same time
                timings[name].append(block_ms_per_step(torch, submit, drain, steps))
    finally:
        gc.enable()
    emit(measurement='b', budget_bytes=budget, depth=budget_codec.depth, blocks=blocks, steps_per_block=steps, most_taken_points=most,
         luma_streams=[budget_codec.luma.nb_transform_streams, budget_codec.luma.nb_in_flight],
         chroma_streams=[budget_codec.chroma.nb_transform_streams, budget_codec.chroma.nb_in_flight],
         rate_points=[numpy.bincount(r['rate_point'][:, plane], minlength=k_points).tolist() for plane in range(3)],
         **{name + '_ms_per_step': summary(t) for (name, t) in timings.items()})
    colour_codec.close()
    container.encode_colour_images_to_budget(rgb, encoder, ladder, budget)                 # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    (blobs, info) = container.encode_colour_images_to_budget(rgb, encoder, ladder, budget)
    torch.cuda.synchronize()
    emit(measurement='b', encode_colour_images_to_budget_ms=round((time.perf_counter() - t0)*1e3, 1), budget_bytes=budget,
         same_blobs=[bytes(b) for b in budget_codec.submit(rgb_d, budget).image_containers()] == blobs)

    # (c) what chroma took at the default share
    chroma_bytes = r['blob_bytes'][:, 1:].sum(axis=1)
    emit(measurement='c', chroma_share=budget_codec.chroma_share, budget_bytes=budget,
         chroma_share_of_blob_bytes={'mean': round(float((chroma_bytes/r['picture_blob_bytes']).mean()), 4),
                                     'min': round(float((chroma_bytes/r['picture_blob_bytes']).min()), 4),
                                     'max': round(float((chroma_bytes/r['picture_blob_bytes']).max()), 4)},
         chroma_budget_share_of_payload=round(float((2*r['budget_bytes'][:, 1]/(budget - header)).mean()), 4),
         mean_blob_bytes=[round(float(x), 1) for x in r['blob_bytes'].mean(axis=0)], pictures_promised=int(r['picture_promised'].sum()),
         planes_promised=r['promised'].sum(axis=0).tolist())

    # (d) twelve budgets
    low = int((header + upper[:, :, -1].sum(axis=1)).min()*0.9)
    high = int((header + upper[:, :, 0].sum(axis=1)).max()*1.05)
    (promised_not_fitting, not_promised, elsewhere, total) = (0, 0, 0, 0)
    for b in numpy.linspace(low, high, 12).astype(numpy.int64).tolist():
        (_, info) = container.encode_colour_images_to_budget(rgb, encoder, ladder, b)
        r = budget_codec.submit(rgb_d, b).result()
        promised_not_fitting += int((r['picture_promised'] & ~r['picture_fits']).sum())
        not_promised += int((~r['picture_promised']).sum())
        elsewhere += int((r['rate_point'] != info['rate_point']).any(axis=1).sum())
        total += n
    emit(measurement='d', budgets=12, lowest=low, highest=high, pictures=total, promised_and_not_fits=promised_not_fitting, not_promised=not_promised,
         elsewhere_than_encode_colour_images_to_budget=elsewhere)
    budget_codec.close()


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--calls', type=int, default=30)
    parser.add_argument('--blocks', type=int, default=7)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--hw-queues', type=int, default=None, help='GPU_MAX_HW_QUEUES of this process (default: the environment\'s)')
    args = parser.parse_args()
    main(args.calls, args.blocks, args.steps)
