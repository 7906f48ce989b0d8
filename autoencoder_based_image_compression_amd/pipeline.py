"""Device-resident analysis / synthesis transforms: the arithmetic behind `sess.run(entropy_ae.node_y)` and
`sess.run(isolated_decoder.node_reconstruction)` of the reference (kodak_tensorflow/eae/batching.py:96-99, 49-52).

`DeviceEncoder` / `DeviceDecoder` keep the variables of one trained model in HBM (7 MB) and chain the kernels of
include/eae_hip.h on torch's current stream; activations never leave the device. Both are the hot path of
`bench.py` and the engine under the reference-shaped classes in `kodak/eae/graph/`.
"""
import numbers

import numpy
import torch

from . import device as dev
from .kodak.eae.graph import constants as csts
from .kodak.eae.graph import variables as var


def _to_device(array, device):
    return torch.from_numpy(numpy.ascontiguousarray(array, dtype=numpy.float32)).to(device)


# Latents before / after a tile that the receptive field of its interior reaches, in both axes.
# Encoder: latent t reads input rows 16t-14 ... 16t+42. Decoder: pixels of latents t0 ... t0+T-1 read latents t0-2 ... t0+T.
ENCODER_HALO = (1, 2)
DECODER_HALO = (2, 1)


def _axis_plan(size, tile, before, after):
    """One axis of `tile_plan`: window length, and (window origin, interior origin in the window, interior origin, extent) per tile."""
    window = min(tile + before + after, size)
    spans = []
    for t0 in range(0, size, tile):
        start = min(max(t0 - before, 0), size - window)
        spans.append((start, t0 - start, t0, min(tile, size - t0)))
    return window, spans


def tile_plan(n, h, w, tile, before, after):
    """The windows of a tiled encode / decode of n images of h x w latents with interiors of tile = (th, tw) latents.

    Every window has the shape (min(th + before + after, h), min(tw + before + after, w)) and lies inside its image; where a
    window edge lies inside the image, `before` / `after` latents of halo stand between it and the interior. Returns
    (plan, window shape): plan is int32 [n_windows][9], one row per window -- image, window origin (row, col), interior origin in
    the window (row, col), interior origin in the image (row, col), interior extent (rows, cols) -- images, then tile rows, then
    tile columns (include/eae_hip.h, eae_hip_tile_copy)."""
    (window_h, rows) = _axis_plan(h, tile[0], before, after)
    (window_w, cols) = _axis_plan(w, tile[1], before, after)
    plan = numpy.array([(i, r[0], c[0], r[1], c[1], r[2], c[2], r[3], c[3]) for i in range(n) for r in rows for c in cols],
                       dtype=numpy.int32).reshape(-1, dev.TILE_PLAN_COLS)
    return plan, (window_h, window_w)


def _tile_arguments(tile, tiles_per_launch):
    def positive(x):
        return isinstance(x, numbers.Integral) and not isinstance(x, bool) and x >= 1
    if not isinstance(tile, (tuple, list)) or len(tile) != 2 or not all(positive(t) for t in tile):
        raise ValueError('`tile` must be a pair of positive integers (latent rows, latent columns).')
    if not positive(tiles_per_launch):
        raise ValueError('`tiles_per_launch` must be a positive integer.')
    return (int(tile[0]), int(tile[1])), int(tiles_per_launch)


def _cached_plan(cache, n, h, w, tile, halo, device):
    """tile_plan and its device copy, kept per shape: building and uploading the plan is host work in front of the first launch."""
    key = (n, h, w, tile, tuple(halo), str(device))
    if key not in cache:
        if len(cache) >= 8:
            cache.clear()
        (plan, shape) = tile_plan(n, h, w, tile, *halo)
        cache[key] = (plan, shape, torch.from_numpy(plan).to(device))
    return cache[key]


def _groups(plan, plan_device, per_launch):
    """(host rows, device rows, count) of every group of at most `per_launch` windows."""
    for g0 in range(0, plan.shape[0], per_launch):
        g1 = min(g0 + per_launch, plan.shape[0])
        yield plan[g0:g1], plan_device[g0:g1], g1 - g0


class DeviceEncoder(object):
    """components.encoder (kodak_tensorflow/eae/graph/components.py:86-142) on the GPU."""

    def __init__(self, variables, are_bin_widths_learned, device='cuda'):
        names = var.ENCODER_NAMES + (() if are_bin_widths_learned else var.ENCODER_NAMES_FIXED_BW)
        var.check_variables(variables, names)
        self.are_bin_widths_learned = are_bin_widths_learned
        self.device = torch.device(device)
        self.v = {name: _to_device(variables[name], self.device) for name in names}
        # kernel-side layouts, packed once on the device (include/eae_hip.h "packed" channel order)
        self.w1 = dev.pack_conv9x9s4_weights(self.v['encoder/weights_1'])
        self.w2 = dev.pack_conv_weights(self.v['encoder/weights_2'])
        self.w3 = dev.pack_conv_weights(self.v['encoder/weights_3'])
        self.g = {i: dev.pack_gamma(self.v['encoder/gamma_{}'.format(i)]) for i in ((1, 2) if are_bin_widths_learned else (1, 2, 3))}
        self.tile_halo = ENCODER_HALO        # (before, after) of a tiled call's windows
        self._plans = {}
        # the same variables behind the library's whole-path entry point (include/eae_hip.h: eae_hip_encode), built on first use:
        # the per-layer layouts above are what codec.BatchCodec chains itself (it fuses gdn_3 into the latent stage and times
        # every launch) and a codec that is never called image by image should not pay for a second copy of the weights
        self._model = None
        self._model_variables = {name: variables[name] for name in names}

    @property
    def model(self):
        if self._model is None:
            with torch.cuda.device(self.device if self.device.index is not None else torch.cuda.current_device()):
                self._model = dev.Model(self._model_variables, self.are_bin_widths_learned)
            self._model_variables = None
        return self._model

    def check(self):
        """Waits for the calls issued so far and raises if one of them left tiles unfinished (device.Model.check)."""
        if self._model is not None:
            self._model.check(wait=True)

    def __call__(self, luminances_uint8, out=None, tile=None, tiles_per_launch=16):
        """uint8 [N,H,W] or [N,H,W,1] (device) -> float32 latents [N,H/16,W/16,128] (device); `out`: tensor to write them into.
        tile=(th, tw): encode through windows whose interiors are th x tw latents, `tiles_per_launch` windows per eae_hip_encode
        call -- same bits as tile=None, for any image size, with memory bounded by one group of windows beyond the full planes."""
        if tile is not None:
            (tile, tiles_per_launch) = _tile_arguments(tile, tiles_per_launch)
        if luminances_uint8.dtype != torch.uint8:
            raise TypeError('`luminances_uint8.dtype` is not equal to `torch.uint8`.')
        (h_in, w_in) = (luminances_uint8.shape[1], luminances_uint8.shape[2])
        if h_in % csts.STRIDE_PROD != 0:
            raise ValueError('The height of the input images is not divisible by the product of the three strides.')
        if w_in % csts.STRIDE_PROD != 0:
            raise ValueError('The width of the input images is not divisible by the product of the three strides.')
        if luminances_uint8.dim() == 4:
            luminances_uint8 = luminances_uint8[:, :, :, 0]
        if tile is None:
            return self.model.encode(luminances_uint8.contiguous(), out=out)
        return self._encode_tiled(luminances_uint8.contiguous(), out, tile, tiles_per_launch)

    def _encode_tiled(self, images, out, tile, per_launch):
        model = self.model
        if images.device != model.device:
            raise dev.HipError('images on {0} but the model lives on {1}'.format(images.device, model.device))
        (n, h, w) = (images.shape[0], images.shape[1]//csts.STRIDE_PROD, images.shape[2]//csts.STRIDE_PROD)
        latents = out if out is not None else torch.empty((n, h, w, dev.NB_MAPS), dtype=torch.float32, device=images.device)
        if latents.dtype != torch.float32 or tuple(latents.shape) != (n, h, w, dev.NB_MAPS):
            raise dev.HipError('`out` must be float32 of shape (N, H/16, W/16, 128)')
        if not latents.is_contiguous() or latents.device != model.device:
            raise dev.HipError('`out` must be a contiguous tensor on {0}'.format(model.device))
        (plan, (wh, ww), plan_device) = _cached_plan(self._plans, n, h, w, tile, self.tile_halo, images.device)
        g = min(per_launch, plan.shape[0])
        windows = torch.empty((g, 16*wh, 16*ww), dtype=torch.uint8, device=images.device)
        window_latents = torch.empty((g, wh, ww, dev.NB_MAPS), dtype=torch.float32, device=images.device)
        for (rows, rows_device, count) in _groups(plan, plan_device, per_launch):
            dev.tile_copy(images, windows[:count], rows_device, rows, 16, True)
            model.encode(windows[:count], out=window_latents[:count])
            dev.tile_copy(latents, window_latents[:count], rows_device, rows, 1, False)
        return latents


class DeviceDecoder(object):
    """components.decoder (components.py:11-84) + tls.cast_bt601 (batching.py:53) on the GPU."""

    def __init__(self, variables, are_bin_widths_learned, device='cuda'):
        names = var.DECODER_NAMES + (() if are_bin_widths_learned else var.DECODER_NAMES_FIXED_BW)
        var.check_variables(variables, names)
        self.are_bin_widths_learned = are_bin_widths_learned
        self.device = torch.device(device)
        self.v = {name: _to_device(variables[name], self.device) for name in names}
        # kernel-side weight layouts, packed once on the device
        self.w4 = dev.pack_tconv_weights(self.v['decoder/weights_4'])
        self.w5 = dev.pack_tconv_weights(self.v['decoder/weights_5'])
        self.w6 = dev.pack_tconv9x9s4_weights(self.v['decoder/weights_6'])
        self.g = {i: dev.pack_gamma(self.v['decoder/gamma_{}'.format(i)]) for i in ((5, 6) if are_bin_widths_learned else (4, 5, 6))}
        self.tile_halo = DECODER_HALO        # (before, after) of a tiled call's windows
        self._plans = {}
        self._model = None           # eae_hip_decode, built on first use (see DeviceEncoder)
        self._model_variables = {name: variables[name] for name in names}

    @property
    def model(self):
        if self._model is None:
            with torch.cuda.device(self.device if self.device.index is not None else torch.cuda.current_device()):
                self._model = dev.Model(self._model_variables, self.are_bin_widths_learned)
            self._model_variables = None
        return self._model

    def check(self):
        if self._model is not None:
            self._model.check(wait=True)

    def __call__(self, quantized_y, want_float=False, want_uint8=True, reference_uint8=None, sse=None, out_uint8=None, tile=None,
                 tiles_per_launch=16):
        """float32 [N,h,w,128] (device) -> (float32 [N,16h,16w] or None, uint8 [N,16h,16w] or None, sse or None).
        tile=(th, tw): decode through windows whose interiors are th x tw latents (see DeviceEncoder.__call__): same results."""
        if tile is None:
            return self.model.decode(quantized_y.contiguous(), want_f32=want_float, want_u8=want_uint8, ref_u8=reference_uint8, sse=sse,
                                     out_u8=out_uint8)
        (tile, tiles_per_launch) = _tile_arguments(tile, tiles_per_launch)
        return self._decode_tiled(quantized_y.contiguous(), want_float, want_uint8, reference_uint8, sse, out_uint8, tile,
                                  tiles_per_launch)

    def _decode_tiled(self, y, want_float, want_uint8, reference, sse, out_u8, tile, per_launch):
        model = self.model
        (n, h, w, _) = y.shape
        d = y.device
        if d != model.device:
            raise dev.HipError('latents on {0} but the model lives on {1}'.format(d, model.device))
        if out_u8 is not None and (out_u8.dtype != torch.uint8 or out_u8.numel() != n*16*h*16*w):
            raise dev.HipError('`out_u8` must hold N x 16h x 16w uint8 elements')
        if out_u8 is not None and (not out_u8.is_contiguous() or out_u8.device != model.device):
            raise dev.HipError('`out_u8` must be a contiguous tensor on {0}'.format(model.device))
        out_f32 = torch.empty((n, 16*h, 16*w), dtype=torch.float32, device=d) if want_float else None
        if out_u8 is None and want_uint8:
            out_u8 = torch.empty((n, 16*h, 16*w), dtype=torch.uint8, device=d)
        if reference is not None and sse is None:
            sse = torch.zeros(n, dtype=torch.int64, device=d)
        image = out_u8.view(n, 16*h, 16*w) if out_u8 is not None else None
        ref = reference.reshape(n, 16*h, 16*w) if reference is not None else None
        need_u8 = image is not None or ref is not None
        (plan, (wh, ww), plan_device) = _cached_plan(self._plans, n, h, w, tile, self.tile_halo, d)
        g = min(per_launch, plan.shape[0])
        windows = torch.empty((g, wh, ww, dev.NB_MAPS), dtype=torch.float32, device=d)
        windows_u8 = torch.empty((g, 16*wh, 16*ww), dtype=torch.uint8, device=d) if need_u8 else None
        for (rows, rows_device, count) in _groups(plan, plan_device, per_launch):
            dev.tile_copy(y, windows[:count], rows_device, rows, 1, True)
            (rec_f32, _, _) = model.decode(windows[:count], want_f32=want_float, want_u8=need_u8,
                                           out_u8=windows_u8[:count] if need_u8 else None)
            if want_float:
                dev.tile_copy(out_f32, rec_f32, rows_device, rows, 16, False)
            if need_u8:
                dev.tile_stitch_u8(windows_u8[:count], rows_device, rows, image=image, ref_u8=ref, sse=sse)
        return out_f32, out_u8, sse


# Algorithmic work per INPUT pixel of each launch, fixed-bin-width model.
# MACs: conv1 648 + GDN1 1024; conv2 6400 + GDN2 256; conv3 1600 + GDN3 64; IGDN4 64; tconv1 1600 + IGDN5 256;
# tconv2 6400 + IGDN6 1024; tconv3 648.
FLOP_PER_PIXEL = {
    'conv1_gdn1': 2*(648 + 1024),
    'conv2_gdn2': 2*(6400 + 256),
    'conv3_gdn3': 2*(1600 + 64),
    'igdn4': 2*64,
    'tconv1_igdn5': 2*(1600 + 256),
    'tconv2_igdn6': 2*(6400 + 1024),
    'tconv3': 2*648,
}
FLOP_PER_PIXEL_TOTAL = sum(FLOP_PER_PIXEL.values())   # 39,968
