#!/usr/bin/env python
"""`codec.ColourQualityCodec`, measured (profiles/colour_quality_codec.md). On the GPU, 24 RGB pictures of
512 x 768 (bench.py's synthetic images in every channel, its model at bin width 0.05), the ladder of profiles/budget_codec.py: the
reference's nine multipliers, L = 10, tables and map means measured on the luminance planes; Cb and Cr take the same ladder.

    python profiles/colour_quality_codec.py [--calls 30] [--blocks 7] [--steps 20] [--hw-queues 4]
      (a) the probe launch, squared error only (no plane written), on 24 planes coded at 512 x 768, in ONE run, alternating, device
          events around each call, median (min .. max) of `--calls`:
            device.tconv9x9s4_luma             -- the existing entry point, whose kernel is the parent's instruction for instruction:
                                                  the yardstick; measured TWICE, so that its own run-to-run spread stands beside
            device.tconv9x9s4_luma_frame at the real size 512 x 768 (every pixel inside) and at 500 x 750 (masked rows and columns)
      (b) device.colour_quality_rest alone
      (c) in ONE process, in alternating blocks of `--steps` pipelined steps, host clock from the first submit to the drain, median
          (min .. max) of `--blocks` blocks, every codec in `codec.product_mode` of its plane:
            the ColourQualityCodec step at the default chroma share;
            its three inner `_PlaneQualityCodec` steps alone -- the same planes and plane thresholds submitted to `luma` and `chroma`
            directly, nothing waiting for anything: no split, no `colour_quality_rest`, no merge, and Y not behind chroma;
            the ColourBudgetCodec step at budgets built from the bounds of the points the quality step took (how many pictures land
            on those points is reported);
          then the same pictures through container.encode_colour_images_to_quality, once warm
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


def event_us(torch, fn):
    (start, stop) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)*1e3


def alternating_event_us(torch, legs, calls):
    """Every leg once per round, `calls` rounds, behind three warm rounds -> {name: summary}."""
    for _ in range(3):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(calls):
        for (name, fn) in legs.items():
            times[name].append(event_us(torch, fn))
    return {name: summary(t) for (name, t) in times.items()}


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
    decoder = pipeline.DeviceDecoder(v, False)
    y_host = encoder(planes_d[0]).cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y_host)
    bin_widths_points = (MULTIPLIERS[:, None]*v[var.BIN_WIDTHS_NAME][None, :]).astype(numpy.float32)
    tables = lossless_stats.compute_binary_probabilities_ladder(y_host, bin_widths_points, map_mean, length)
    del y_host
    ladder = ratecontrol.RateLadder(bin_widths_points, tables, map_mean)
    k_points = ladder.nb_points
    emit(device=dev.device_info(), gpu_max_hw_queues=os.environ.get('GPU_MAX_HW_QUEUES'), pictures=n, height=h, width=w, length=length,
         k_points=k_points)

    # (a) the probe launch: the input of transpose_conv_3 for 24 planes coded at 512 x 768, the squared error only
    t = torch.randn((n, h//4, w//4, 128), dtype=torch.float32, device='cuda')
    acc = torch.zeros(n, dtype=torch.int64, device='cuda')
    frame = planes_d[0]
    legs = {'tconv9x9s4_luma': lambda: dev.tconv9x9s4_luma(t, decoder.w6, want_f32=False, want_u8=False, ref_u8=frame, sse=acc),
            'tconv9x9s4_luma_frame_512x768': lambda: dev.tconv9x9s4_luma_frame(t, decoder.w6, (h, w), want_f32=False, want_u8=False, ref_u8=frame, sse=acc),
            'tconv9x9s4_luma_again': lambda: dev.tconv9x9s4_luma(t, decoder.w6, want_f32=False, want_u8=False, ref_u8=frame, sse=acc),
            'tconv9x9s4_luma_frame_500x750': lambda: dev.tconv9x9s4_luma_frame(t, decoder.w6, (500, 750), want_f32=False, want_u8=False, ref_u8=frame,
                                                                               sse=acc)}
    emit(measurement='a', planes=n, coded=[h, w], microseconds=alternating_event_us(torch, legs, calls))
    del t

    # (b) the luminance threshold's launch alone
    (m_d, cb_d, cr_d, out_d) = (torch.full((n,), 1 << 40, dtype=torch.int64, device='cuda'), torch.full((n,), 12345, dtype=torch.int64, device='cuda'),
                                torch.full((n,), 54321, dtype=torch.int64).pin_memory(), torch.zeros(n, dtype=torch.int64, device='cuda'))
    emit(measurement='b', launch='colour_quality_rest', pictures=n,
         microseconds=alternating_event_us(torch, {'colour_quality_rest': lambda: dev.colour_quality_rest(m_d, cb_d, cr_d, out_d)}, calls))

    # (c) the step against its siblings, alternating
    options = dict(chroma_options=codec.product_mode(hc, wc), **codec.product_mode(h, w))
    quality_codec = codec.ColourQualityCodec(v, False, ladder, n, h, w, **options)
    finest = quality_codec.submit(rgb_d, max_sse=0).result()
    coarsest = quality_codec.submit(rgb_d, max_sse=1 << 62).result()
    thresholds = numpy.sqrt(finest['picture_sse'].astype(numpy.float64)*coarsest['picture_sse'].astype(numpy.float64)).astype(numpy.int64)
    r = quality_codec.submit(rgb_d, max_sse=thresholds).result()
    rows = numpy.arange(n)
    budgets = container.COLOUR_HEADER_BYTES + sum(r['upper_bound_bytes'][rows, plane, r['rate_point'][:, plane]] for plane in range(3))
    budget_codec = codec.ColourBudgetCodec(v, False, ladder, n, h, w, **options)
    on_the_same_points = int((budget_codec.submit(rgb_d, budgets).result()['rate_point'] == r['rate_point']).all(axis=1).sum())
    luma_thresholds_d = torch.from_numpy(numpy.ascontiguousarray(r['max_sse'][:, 0])).cuda()
    chroma_thresholds = numpy.ascontiguousarray(r['max_sse'][:, 1])

    def inner_alone():
        return (quality_codec.luma.submit(planes_d[0], max_sse=luma_thresholds_d), quality_codec.chroma.submit(planes_d[1], max_sse=chroma_thresholds),
                quality_codec.chroma.submit(planes_d[2], max_sse=chroma_thresholds))

    legs = {'colour_quality_codec': (lambda: quality_codec.submit(rgb_d, max_sse=thresholds), quality_codec.drain),
            'three_plane_quality_codecs_alone': (inner_alone, quality_codec.drain),
            'colour_budget_codec': (lambda: budget_codec.submit(rgb_d, budgets), budget_codec.drain)}
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
    emit(measurement='c', depth=quality_codec.depth, blocks=blocks, steps_per_block=steps, rounds=quality_codec.luma.nb_rounds,
         luma_streams=[quality_codec.luma.nb_transform_streams, quality_codec.luma.nb_in_flight],
         chroma_streams=[quality_codec.chroma.nb_transform_streams, quality_codec.chroma.nb_in_flight],
         rate_points=[numpy.bincount(r['rate_point'][:, plane], minlength=k_points).tolist() for plane in range(3)],
         pictures_met=int(r['picture_met'].sum()), planes_met=r['met'].sum(axis=0).tolist(),
         budget_codec_pictures_on_the_same_points=on_the_same_points,
         **{name + '_ms_per_step': summary(t) for (name, t) in timings.items()})
    budget_codec.close()
    container.encode_colour_images_to_quality(rgb, encoder, decoder, ladder, max_sse=thresholds)      # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    (blobs, info) = container.encode_colour_images_to_quality(rgb, encoder, decoder, ladder, max_sse=thresholds)
    torch.cuda.synchronize()
    emit(measurement='c', encode_colour_images_to_quality_ms=round((time.perf_counter() - t0)*1e3, 1),
         same_blobs=[bytes(b) for b in quality_codec.submit(rgb_d, max_sse=thresholds).image_containers()] == [bytes(b) for b in blobs],
         same_points=bool((info['rate_point'] == r['rate_point']).all()))
    quality_codec.close()


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--calls', type=int, default=30)
    parser.add_argument('--blocks', type=int, default=7)
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--hw-queues', type=int, default=None, help='GPU_MAX_HW_QUEUES of this process (default: the environment\'s)')
    args = parser.parse_args()
    main(args.calls, args.blocks, args.steps)
