"""Device-resident ops: torch tensors (used only as HBM buffers + streams) -> include/eae_hip.h entry points.

Every function launches asynchronously on torch's current stream and returns device tensors. There is no CPU
fallback: a missing libeae_hip.so or a non-CUDA tensor raises.
"""
import torch

from . import _native

NORM_NONE, NORM_GDN, NORM_IGDN = 0, 1, 2
NB_MAPS = 128


class HipError(RuntimeError):
    pass


def _check(status, what):
    if status != 0:
        raise HipError('{0} failed with status {1}'.format(what, status))


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream(on=None):
    """hipStream_t of torch's current stream on the current device (every launch of this module goes there). `on`: the
    launch's main tensor -- it must live on the current device (a kernel launched on another device's stream with foreign
    pointers faults or silently serialises): select the device with `torch.cuda.device(...)` / `set_device` first."""
    current = torch.cuda.current_device()
    if on is not None and on.device.index != current:
        raise HipError('tensor on {0} but the current device is cuda:{1}: wrap the call in `with torch.cuda.device({0!r})`'.format(
            on.device, current))
    if _raw_stream is not None:                      # one C call instead of building a torch.cuda.Stream object per launch
        return _raw_stream(current)
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise HipError('expected a device tensor')
    if not t.is_contiguous():
        raise HipError('expected a contiguous tensor')
    return t.data_ptr()


def device_info():
    import ctypes
    name = ctypes.create_string_buffer(128)
    cus = ctypes.c_int(0)
    mhz = ctypes.c_int(0)
    mem = ctypes.c_int64(0)
    _check(_native.hip().eae_hip_device_info(name, 128, ctypes.byref(cus), ctypes.byref(mhz), ctypes.byref(mem)), 'device_info')
    return {'name': name.value.decode(), 'compute_units': cus.value, 'clock_mhz': mhz.value, 'hbm_bytes': mem.value}


def partition_info():
    """{'compute_units', 'xcds', 'whole_device'} of the current logical device (include/eae_hip.h: eae_hip_partition_info)."""
    import ctypes
    (cus, xcds, whole) = (ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0))
    _check(_native.hip().eae_hip_partition_info(ctypes.byref(cus), ctypes.byref(xcds), ctypes.byref(whole)), 'partition_info')
    return {'compute_units': cus.value, 'xcds': xcds.value, 'whole_device': bool(whole.value)}


class Model(object):
    """eae_hip_model (include/eae_hip.h, whole-path entry points): the variables of one trained entropy autoencoder resident
    on the current device in the kernels' layouts. `variables`: dict of numpy arrays keyed by the TensorFlow variable names
    (kodak/eae/graph/variables.py); encoder-only and decoder-only dicts are accepted."""

    _FIELDS = ('weights_1', 'biases_1', 'gamma_1', 'beta_1', 'weights_2', 'biases_2', 'gamma_2', 'beta_2', 'weights_3', 'biases_3',
               'gamma_3', 'beta_3', 'gamma_4', 'beta_4', 'weights_4', 'biases_4', 'gamma_5', 'beta_5', 'weights_5', 'biases_5',
               'gamma_6', 'beta_6', 'weights_6')

    def __init__(self, variables, are_bin_widths_learned):
        import ctypes
        import numpy
        self.are_bin_widths_learned = bool(are_bin_widths_learned)
        self.device = torch.device('cuda', torch.cuda.current_device())
        pointers = (ctypes.c_void_p*len(self._FIELDS))()
        keep = []
        for (i, field) in enumerate(self._FIELDS):
            name = ('encoder/' if int(field[-1]) <= 3 else 'decoder/') + field
            if name in variables and not (self.are_bin_widths_learned and field in ('gamma_3', 'beta_3', 'gamma_4', 'beta_4')):
                array = numpy.ascontiguousarray(variables[name], dtype=numpy.float32)
                keep.append(array)
                pointers[i] = array.ctypes.data
        handle = ctypes.c_void_p()
        _check(_native.hip().eae_hip_model_create(ctypes.cast(pointers, ctypes.c_void_p), 1 if self.are_bin_widths_learned else 0,
                                                  ctypes.byref(handle)), 'eae_hip_model_create')
        self._handle = handle
        # the failure word of a call sits behind the conv workspace at the head of its scratch block (eae_hip_transform_status);
        # calls are asynchronous, so the word is published to pinned memory behind each call and looked at later (`check`)
        self._status_offset = (int(_native.hip().eae_hip_conv_workspace_bytes()) + 255)//256*256
        self._pending = []          # (event, pinned word) of calls nobody has looked at yet
        self._free_words = []

    def _track(self, scratch):
        word = scratch[self._status_offset:self._status_offset + 4].view(torch.int32)
        pinned = self._free_words.pop() if self._free_words else torch.zeros(1, dtype=torch.int32).pin_memory()
        publish_to_host(word, pinned)
        event = torch.cuda.Event()
        event.record()
        self._pending.append((event, pinned))

    def check(self, wait=False):
        """Raises `SplitHandOffTimeout` if an encode / decode call that has completed (wait=True: any call issued so far) left
        tiles unfinished (include/eae_hip.h: eae_hip_conv_workspace_collect) -- its outputs are then invalid. Every encode /
        decode looks at the completed calls first; the reference-shaped `sess.run` nodes wait, right after their device -> host copy."""
        (still, failed) = ([], 0)
        for (event, pinned) in self._pending:
            if wait:
                event.synchronize()
            if event.query():
                failed += int(pinned[0])
                self._free_words.append(pinned)
            else:
                still.append((event, pinned))
        self._pending = still
        if failed:
            raise SplitHandOffTimeout('{} tiles of a cut conv launch were not handed over (eae_hip_transform_status): the outputs '
                                      'of that call are invalid'.format(failed))

    def close(self):
        if getattr(self, '_handle', None):
            _native.hip().eae_hip_model_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, images_u8, out=None):
        """uint8 [N,H,W] (device) -> latents f32 [N,H/16,W/16,128]: `sess.run(node_y)` of eae/batching.py:96-99 in one call.
        out: a contiguous float32 tensor of that shape to write into (e.g. a mini-batch's slice of the whole set's latents)."""
        if images_u8.dtype != torch.uint8:
            raise TypeError('`images_u8.dtype` is not `torch.uint8`.')
        (n, h, wd) = images_u8.shape[:3]
        nbytes = int(_native.hip().eae_hip_encode_scratch_bytes(n, h, wd))
        if nbytes == 0:
            raise ValueError('The image size is not divisible by the product of the three strides.')
        if images_u8.device != self.device:
            raise HipError('images on {0} but the model lives on {1}'.format(images_u8.device, self.device))
        self.check()
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=images_u8.device)
        latents = out if out is not None else torch.empty((n, h//16, wd//16, NB_MAPS), dtype=torch.float32, device=images_u8.device)
        if latents.dtype != torch.float32 or tuple(latents.shape) != (n, h//16, wd//16, NB_MAPS):
            raise HipError('`out` must be float32 of shape (N, H/16, W/16, 128)')
        if not latents.is_contiguous() or latents.device != self.device:
            # the kernels get a raw pointer and write N x h x w x 128 floats flat behind it
            raise HipError('`out` must be a contiguous tensor on {0} (got {1}, {2})'.format(
                self.device, 'contiguous' if latents.is_contiguous() else 'non-contiguous', latents.device))
        _check(_native.hip().eae_hip_encode(self._handle, _p(images_u8), n, h, wd, _p(latents), _p(scratch), nbytes, _stream(images_u8)),
               'eae_hip_encode')
        self._track(scratch)
        return latents

    def decode(self, quantized_latents, want_f32=False, want_u8=True, ref_u8=None, sse=None, out_u8=None):
        """f32 [N,h,w,128] (device) -> (f32 [N,16h,16w] or None, uint8 or None, sse or None): `sess.run(node_reconstruction)` +
        `tls.cast_bt601` of eae/batching.py:49-53 (+ the squared error of tls.psnr_2d) in one call. out_u8: a contiguous uint8
        tensor of N x 16h x 16w elements to write the reconstruction into."""
        (n, h, wd, c) = quantized_latents.shape
        d = quantized_latents.device
        if d != self.device:
            raise HipError('latents on {0} but the model lives on {1}'.format(d, self.device))
        self.check()
        nbytes = int(_native.hip().eae_hip_decode_scratch_bytes(n, h, wd))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=d)
        out_f32 = torch.empty((n, 16*h, 16*wd), dtype=torch.float32, device=d) if want_f32 else None
        if out_u8 is not None and (out_u8.dtype != torch.uint8 or out_u8.numel() != n*16*h*16*wd):
            raise HipError('`out_u8` must hold N x 16h x 16w uint8 elements')
        if out_u8 is not None and (not out_u8.is_contiguous() or out_u8.device != self.device):
            raise HipError('`out_u8` must be a contiguous tensor on {0} (got {1}, {2})'.format(
                self.device, 'contiguous' if out_u8.is_contiguous() else 'non-contiguous', out_u8.device))
        if out_u8 is None:
            out_u8 = torch.empty((n, 16*h, 16*wd), dtype=torch.uint8, device=d) if want_u8 else None
        if ref_u8 is not None and sse is None:
            sse = torch.zeros(n, dtype=torch.int64, device=d)
        _check(_native.hip().eae_hip_decode(self._handle, _p(quantized_latents), n, h, wd, _p(out_f32), _p(out_u8), _p(ref_u8), _p(sse),
                                            _p(scratch), nbytes, _stream(quantized_latents)), 'eae_hip_decode')
        self._track(scratch)
        return out_f32, out_u8, sse

    def decode_scratch(self, n, h, wd):
        """A scratch block `decode_into` can use for latents f32 [n, h, wd, 128], and the view of its failure word (int32 [1]: tiles a
        cut conv launch left unfinished; zeroed by every call, final behind it)."""
        scratch = torch.empty(int(_native.hip().eae_hip_decode_scratch_bytes(n, h, wd)), dtype=torch.uint8, device=self.device)
        return scratch, scratch[self._status_offset:self._status_offset + 4].view(torch.int32)

    def decode_into(self, quantized_latents, out_u8, scratch):
        """`decode(...)` for a caller that owns every buffer (codec.BatchDecoder: one per slot, inside a captured step): nothing is
        allocated, no event is recorded and nothing is tracked -- the caller publishes the scratch block's failure word
        (`decode_scratch`) and looks at it itself."""
        (n, h, wd, c) = quantized_latents.shape
        if out_u8.dtype != torch.uint8 or out_u8.numel() != n*16*h*16*wd or c != NB_MAPS:
            raise HipError('`out_u8` must hold N x 16h x 16w uint8 elements')
        _check(_native.hip().eae_hip_decode(self._handle, _p(quantized_latents), n, h, wd, None, _p(out_u8), None, None, _p(scratch),
                                            scratch.numel(), _stream(quantized_latents)), 'eae_hip_decode')


def conv9x9s4_u8(x_u8, w_packed, bias, gamma_packed=None, beta=None, out=None):
    """conv_1 + bias_add (+ gdn_1). x_u8: uint8 [N,H,W] or [N,H,W,1] -> f32 [N,H/4,W/4,128].
    w_packed from `pack_conv9x9s4_weights`, gamma_packed from `pack_gamma`."""
    if x_u8.dtype != torch.uint8:
        raise TypeError('`x_u8.dtype` is not `torch.uint8`.')
    (n, h, wd) = x_u8.shape[:3]
    if out is None:
        out = torch.empty((n, h//4, wd//4, NB_MAPS), dtype=torch.float32, device=x_u8.device)
    _check(_native.hip().eae_hip_conv9x9s4_u8(_p(x_u8), _p(w_packed), _p(bias), _p(gamma_packed), _p(beta), _p(out), n, h, wd, _stream(x_u8)),
           'eae_hip_conv9x9s4_u8')
    return out


def conv_workspace(device):
    """Zeroed scratch that lets conv5x5s2 / tconv5x5s2 cut the last tiles of a launch (include/eae_hip.h): every launch leaves
    it zeroed, so one allocation serves any number of launches that cannot overlap each other (one per stream / batch slot).
    Whoever passes one to a launch owns its error word: `conv_workspace_collect` behind the launches, and a look at the word
    before their outputs are trusted (codec.BatchCodec does both per batch)."""
    return torch.zeros(int(_native.hip().eae_hip_conv_workspace_bytes())//4, dtype=torch.int32, device=device)


class SplitHandOffTimeout(HipError):
    """A cut conv launch left tiles unfinished (include/eae_hip.h: eae_hip_conv_workspace_collect): its outputs are invalid."""


def conv_workspace_collect(workspace, error_word):
    """Stream-ordered: adds the number of tiles the launches on `workspace` left unfinished since the last collect to
    `error_word` (int32 device tensor of one element, or a pinned host one) and restores the all-zero workspace."""
    if error_word.numel() != 1 or error_word.element_size() != 4:
        raise HipError('`error_word` must be one 32-bit word')
    word = error_word.data_ptr() if not error_word.is_cuda else _p(error_word)
    _check(_native.hip().eae_hip_conv_workspace_collect(_p(workspace), word, _stream(workspace)), 'eae_hip_conv_workspace_collect')


GEMM_PLAN_FIELDS = ('family', 'waves', 'nt', 'packed', 'cut', 'k', 'grid', 'block', 'norm_pass', 'latent_fused', 'items')
GEMM_PLAN_FAMILIES = {0: None, 1: 'lds', 2: 'wave', 3: 'split'}


def last_gemm_plan():
    """What the last conv GEMM launch of the calling thread launched, as its launcher recorded it (include/eae_hip.h:
    eae_hip_debug_last_gemm_plan): a dict of GEMM_PLAN_FIELDS, 'family' as one of 'lds' / 'wave' / 'split' (None: no launch yet).
    Test build only: the product library has no such entry point."""
    import ctypes
    lib = _native.hip()
    if not hasattr(lib, 'eae_hip_debug_last_gemm_plan'):
        raise HipError('eae_hip_debug_last_gemm_plan is a test hook: it lives in lib/libeae_hip_test.so only (EAE_HIP_LIB=test)')
    words = (ctypes.c_int32*len(GEMM_PLAN_FIELDS))()
    written = lib.eae_hip_debug_last_gemm_plan(words, len(words))
    if written != len(words):
        raise HipError('eae_hip_debug_last_gemm_plan wrote {0} of {1} words'.format(written, len(words)))
    plan = dict(zip(GEMM_PLAN_FIELDS, (int(w) for w in words)))
    plan['family'] = GEMM_PLAN_FAMILIES[plan['family']]
    return plan


def conv5x5s2(x, w_packed, bias, norm=NORM_NONE, gamma_packed=None, beta=None, out=None, workspace=None):
    """conv_2 / conv_3 + bias_add (+ gdn). workspace: a `conv_workspace` (the launch may cut its last tiles: same bits, no
    partly empty last round; the caller collects its error word, see `conv_workspace_collect`); None / False -> the entry
    point without a workspace (whole tiles only, nothing to collect)."""
    (n, h, wd, c) = x.shape
    if out is None:
        out = torch.empty((n, h//2, wd//2, NB_MAPS), dtype=torch.float32, device=x.device)
    if workspace is None or workspace is False:
        _check(_native.hip().eae_hip_conv5x5s2(_p(x), _p(w_packed), _p(bias), norm, _p(gamma_packed), _p(beta), _p(out), n, h, wd, _stream(x)),
               'eae_hip_conv5x5s2')
        return out
    _check(_native.hip().eae_hip_conv5x5s2_ws(_p(x), _p(w_packed), _p(bias), norm, _p(gamma_packed), _p(beta), _p(out), n, h, wd,
                                                  _p(workspace), _stream(x)), 'eae_hip_conv5x5s2_ws')
    return out


def gdn(x, gamma_packed, beta, inverse=False, out=None):
    if out is None:
        out = torch.empty_like(x)
    rows = x.numel()//NB_MAPS
    _check(_native.hip().eae_hip_gdn(_p(x), _p(gamma_packed), _p(beta), 1 if inverse else 0, _p(out), rows, _stream(x)), 'eae_hip_gdn')
    return out


def tconv5x5s2(x, w_packed, bias, norm=NORM_NONE, gamma_packed=None, beta=None, out=None, workspace=None):
    """transpose_conv_1 / _2 + bias_add (+ inverse gdn); `workspace` as in conv5x5s2."""
    (n, h, wd, c) = x.shape
    if out is None:
        out = torch.empty((n, 2*h, 2*wd, NB_MAPS), dtype=torch.float32, device=x.device)
    if workspace is None or workspace is False:
        _check(_native.hip().eae_hip_tconv5x5s2(_p(x), _p(w_packed), _p(bias), norm, _p(gamma_packed), _p(beta), _p(out), n, h, wd, _stream(x)),
               'eae_hip_tconv5x5s2')
        return out
    _check(_native.hip().eae_hip_tconv5x5s2_ws(_p(x), _p(w_packed), _p(bias), norm, _p(gamma_packed), _p(beta), _p(out), n, h, wd,
                                                   _p(workspace), _stream(x)), 'eae_hip_tconv5x5s2_ws')
    return out


def tconv9x9s4_luma(x, w_phase, want_f32=False, want_u8=True, ref_u8=None, sse=None):
    """transpose_conv_3 (+ cast_bt601, + squared error vs ref_u8). Returns (f32 or None, u8 or None, sse or None)."""
    (n, h, wd, c) = x.shape
    out_f32 = torch.empty((n, 4*h, 4*wd), dtype=torch.float32, device=x.device) if want_f32 else None
    out_u8 = torch.empty((n, 4*h, 4*wd), dtype=torch.uint8, device=x.device) if want_u8 else None
    if ref_u8 is not None and sse is None:
        sse = torch.zeros(n, dtype=torch.int64, device=x.device)
    _check(_native.hip().eae_hip_tconv9x9s4_luma(_p(x), _p(w_phase), _p(out_f32), _p(out_u8), _p(ref_u8), _p(sse), n, h, wd, _stream(x)),
           'eae_hip_tconv9x9s4_luma')
    return out_f32, out_u8, sse


def tconv9x9s4_luma_frame(x, w_phase, image_size, want_f32=False, want_u8=True, ref_u8=None, sse=None):
    """`tconv9x9s4_luma` whose squared error is over the REAL pixels of padded planes: image_size = (real_h,
    real_w), anywhere in [1, 4h] x [1, 4w]; ref_u8 is the CODED frame [N, 4h, 4w] (`frame_pad_u8`'s output), of which the bytes outside
    the real rectangle never reach the sum; the outputs requested are of the whole coded plane, bit for bit `tconv9x9s4_luma`'s.
    sse[i] is added into. Returns (f32 or None, u8 or None, sse or None)."""
    (n, h, wd, c) = x.shape
    (real_h, real_w) = (int(image_size[0]), int(image_size[1]))
    if ref_u8 is not None and (ref_u8.dtype != torch.uint8 or tuple(ref_u8.shape) != (n, 4*h, 4*wd) or not ref_u8.is_contiguous()):
        raise HipError('ref_u8 must be the coded frame: uint8 [N, 4h, 4w], contiguous')
    out_f32 = torch.empty((n, 4*h, 4*wd), dtype=torch.float32, device=x.device) if want_f32 else None
    out_u8 = torch.empty((n, 4*h, 4*wd), dtype=torch.uint8, device=x.device) if want_u8 else None
    if ref_u8 is not None and sse is None:
        sse = torch.zeros(n, dtype=torch.int64, device=x.device)
    _check(_native.hip().eae_hip_tconv9x9s4_luma_frame(_p(x), _p(w_phase), _p(out_f32), _p(out_u8), _p(ref_u8), _p(sse), n, h, wd, real_h,
                                                       real_w, _stream(x)), 'eae_hip_tconv9x9s4_luma_frame')
    return out_f32, out_u8, sse


def pack_conv_weights(w_hwio):
    """HWIO [k,k,128,128] -> kernel layout [k*k,128,packed out] (include/eae_hip.h)."""
    (k, k2, ci, co) = w_hwio.shape
    out = torch.empty((k*k2, ci, co), dtype=torch.float32, device=w_hwio.device)
    _check(_native.hip().eae_hip_pack_conv_weights(_p(w_hwio), _p(out), k*k2, _stream()), 'eae_hip_pack_conv_weights')
    return out


def pack_conv9x9s4_weights(w_tf):
    """conv_1 filter [9,9,1,128] -> kernel layout [82, packed out] (row 81 is zero)."""
    out = torch.empty((82, NB_MAPS), dtype=torch.float32, device=w_tf.device)
    _check(_native.hip().eae_hip_pack_conv9x9s4_weights(_p(w_tf), _p(out), _stream()), 'eae_hip_pack_conv9x9s4_weights')
    return out


def pack_tconv_weights(w_tf):
    """TF conv2d_transpose filter [k,k,out,in] -> kernel layout [k*k,in,packed out]."""
    (k, k2, co, ci) = w_tf.shape
    out = torch.empty((k*k2, ci, co), dtype=torch.float32, device=w_tf.device)
    _check(_native.hip().eae_hip_pack_tconv_weights(_p(w_tf), _p(out), k*k2, _stream()), 'eae_hip_pack_tconv_weights')
    return out


def pack_gamma(gamma):
    """gamma [128,128] -> [128, packed c]."""
    out = torch.empty_like(gamma)
    _check(_native.hip().eae_hip_pack_gamma(_p(gamma), _p(out), _stream()), 'eae_hip_pack_gamma')
    return out


def packed_channel_order():
    """numpy index array `perm` with packed[..., perm[c]] = plain[..., c] (c -> (c % 32)*4 + c//32)."""
    import numpy
    c = numpy.arange(NB_MAPS)
    return (c % 32)*4 + c//32


def pack_tconv9x9s4_weights(w_tf):
    """[9,9,1,128] -> [9,128,16]."""
    out = torch.empty((9, NB_MAPS, 16), dtype=torch.float32, device=w_tf.device)
    _check(_native.hip().eae_hip_pack_tconv9x9s4_weights(_p(w_tf), _p(out), _stream()), 'eae_hip_pack_tconv9x9s4_weights')
    return out


def quantize_maps(y, bin_widths, map_mean=None, want_cq=False, want_shifted=False, want_symbols=False, want_flags=False,
                  out_symbols=None, out_flags=None, out_checks=None):
    """One pass over y [N,h,w,C] (or [N,hw,C]); see include/eae_hip.h. Returns a dict of the requested device tensors.

    `checks` (int32 [3]) always comes back: [0] int16 range violations, [1] "quantization was omitted" count,
    [2] "lossless compression altered the data" count. `out_symbols`: a preallocated int16 [N, C, hw] buffer to write
    the planar symbols into (a caller that hands them to another stream keeps them out of the caching allocator).
    """
    n = y.shape[0]
    c = y.shape[-1]
    hw = y.numel()//(n*c)
    d = y.device
    cq = torch.empty_like(y) if want_cq else None
    shifted = torch.empty_like(y) if want_shifted else None
    symbols = (out_symbols if out_symbols is not None else torch.empty((n, c, hw), dtype=torch.int16, device=d)) if want_symbols else None
    if symbols is not None and (symbols.dtype != torch.int16 or symbols.numel() != n*c*hw):
        raise TypeError('`out_symbols` must be an int16 tensor of N x C x hw elements.')
    # out_flags / out_checks: preallocated int32 buffers ALREADY ZEROED by the caller (the kernel only sets / adds)
    flags = (out_flags if out_flags is not None else torch.zeros((n, c), dtype=torch.int32, device=d)) if want_flags else None
    checks = out_checks if out_checks is not None else torch.zeros(3, dtype=torch.int32, device=d)
    _check(_native.hip().eae_hip_quantize_maps(_p(y), _p(map_mean), _p(bin_widths), _p(cq), _p(shifted), _p(symbols), _p(flags),
                                               _p(checks), n, hw, c, _stream(y)), 'eae_hip_quantize_maps')
    return {'cq': cq, 'shifted': shifted, 'symbols': symbols, 'nonzero_flags': flags, 'checks': checks}


def latent_stage(x, bin_widths, map_mean=None, gdn_in=None, igdn_out=None, want_y=False, want_shifted=False, want_symbols=True,
                 want_flags=False, out_symbols=None, out_flags=None, out_checks=None):
    """conv_3 output x [N,h,w,128] (bias added, not normalised) -> gdn_3 -> quantiser -> (+mean) inverse_gdn_4, one kernel.
    gdn_in / igdn_out: (gamma_packed, beta) pairs or None. Returns a dict like quantize_maps plus 'y' and 't' (the input of
    transpose_conv_1). out_* buffers: preallocated, flags / checks already zeroed (see quantize_maps)."""
    n = x.shape[0]
    c = x.shape[-1]
    hw = x.numel()//(n*c)
    d = x.device
    y = torch.empty_like(x) if want_y else None
    shifted = torch.empty_like(x) if want_shifted else None
    t = torch.empty_like(x) if igdn_out is not None else None
    symbols = (out_symbols if out_symbols is not None else torch.empty((n, c, hw), dtype=torch.int16, device=d)) if want_symbols else None
    flags = (out_flags if out_flags is not None else torch.zeros((n, c), dtype=torch.int32, device=d)) if want_flags else None
    checks = out_checks if out_checks is not None else torch.zeros(3, dtype=torch.int32, device=d)
    (g_in, b_in) = gdn_in if gdn_in is not None else (None, None)
    (g_out, b_out) = igdn_out if igdn_out is not None else (None, None)
    _check(_native.hip().eae_hip_latent_stage(_p(x), _p(g_in), _p(b_in), _p(map_mean), _p(bin_widths), _p(g_out), _p(b_out), _p(y),
                                              _p(shifted), _p(t), _p(symbols), _p(flags), _p(checks), n, hw, _stream(x)),
           'eae_hip_latent_stage')
    return {'y': y, 'shifted': shifted, 't': t, 'symbols': symbols, 'nonzero_flags': flags, 'checks': checks}


def conv5x5s2_latent(x, w_packed, bias, bin_widths, map_mean=None, gdn_in=None, igdn_out=None, want_y=False, want_shifted=False,
                     want_flags=False, out_symbols=None, out_flags=None, out_checks=None, workspace=None):
    """conv_3 + bias followed by `latent_stage` in one launch (include/eae_hip.h: eae_hip_conv5x5s2_latent): x is the gdn_2
    output [N,h,w,128]; returns latent_stage's dict ('t' for the fixed-bin-width model, 'shifted' for the learned one is the
    synthesis transform's input). Same bits as conv5x5s2(..., NORM_NONE) + latent_stage."""
    (n, h, wd, c) = x.shape
    d = x.device
    hw = (h//2)*(wd//2)
    fixed = gdn_in is not None
    if fixed != (igdn_out is not None):
        raise ValueError('`gdn_in` and `igdn_out` go together (the fixed-bin-width model has both, the learned one neither).')
    shape = (n, h//2, wd//2, c)
    y = torch.empty(shape, dtype=torch.float32, device=d) if want_y else None
    shifted = torch.empty(shape, dtype=torch.float32, device=d) if (want_shifted or not fixed) else None
    t = torch.empty(shape, dtype=torch.float32, device=d) if fixed else None
    symbols = out_symbols if out_symbols is not None else torch.empty((n, c, hw), dtype=torch.int16, device=d)
    flags = (out_flags if out_flags is not None else torch.zeros((n, c), dtype=torch.int32, device=d)) if want_flags else None
    checks = out_checks if out_checks is not None else torch.zeros(3, dtype=torch.int32, device=d)
    (g_in, b_in) = gdn_in if fixed else (None, None)
    (g_out, b_out) = igdn_out if fixed else (None, None)
    if workspace is None:
        workspace = False          # never cut without a workspace whose owner collects its error word
    _check(_native.hip().eae_hip_conv5x5s2_latent(_p(x), _p(w_packed), _p(bias), _p(g_in), _p(b_in), _p(map_mean), _p(bin_widths), _p(g_out),
                                                  _p(b_out), _p(y), _p(shifted), _p(t), _p(symbols), _p(flags), _p(checks), n, h, wd,
                                                  _p(workspace) if workspace is not False else None, _stream(x)),
           'eae_hip_conv5x5s2_latent')
    return {'y': y, 'shifted': shifted, 't': t, 'symbols': symbols, 'nonzero_flags': flags, 'checks': checks}


def map_means(y):
    """float32 per-map means over every other axis of y [..., C]: `numpy.mean(y, axis=(0, 1, 2))` of lossless/stats.py:306 bit
    for bit (float32 accumulator per map, rows ascending, then / float32(rows))."""
    c = y.shape[-1]
    rows = y.numel()//c
    means = torch.empty(c, dtype=torch.float32, device=y.device)
    _check(_native.hip().eae_hip_map_means(_p(y), _p(means), rows, c, _stream(y)), 'eae_hip_map_means')
    return means


def map_minmax(y):
    """Per-map minimum and maximum over every other axis of y [..., C]: float32 [2, C]."""
    c = y.shape[-1]
    out = torch.empty((2, c), dtype=torch.float32, device=y.device)
    keys = torch.empty(2*c, dtype=torch.int32, device=y.device)
    _check(_native.hip().eae_hip_map_minmax(_p(y), _p(out), _p(keys), y.numel()//c, c, _stream()), 'eae_hip_map_minmax')
    return out


def floor_histograms(y, radius):
    """Per-map histogram of floor(y) for y [..., C]: (hist int32 [C, 2*radius+1] with bin floor(y)+radius, overflow int32 [C])."""
    c = y.shape[-1]
    hist = torch.zeros((c, 2*radius + 1), dtype=torch.int32, device=y.device)
    overflow = torch.zeros(c, dtype=torch.int32, device=y.device)
    _check(_native.hip().eae_hip_floor_histograms(_p(y), _p(hist), radius, _p(overflow), y.numel()//c, c, _stream()),
           'eae_hip_floor_histograms')
    return hist, overflow


def nonzero_flags(x):
    """x [N, ..., C] -> int32 [N, C], 1 where map (n, c) has a non-zero element."""
    n = x.shape[0]
    c = x.shape[-1]
    flags = torch.zeros((n, c), dtype=torch.int32, device=x.device)
    _check(_native.hip().eae_hip_nonzero_flags(_p(x), _p(flags), n, x.numel()//(n*c), c, _stream()), 'eae_hip_nonzero_flags')
    return flags


def cast_int16(x):
    """int16(round_half_even(x)) and the count of out-of-range elements (int32 [1])."""
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    range_error = torch.zeros(1, dtype=torch.int32, device=x.device)
    _check(_native.hip().eae_hip_cast_int16(_p(x), _p(out), x.numel(), _p(range_error), _stream()), 'eae_hip_cast_int16')
    return out, range_error


def symbol_histograms(symbols_planar, radius, out=None, first_map=0, map_step=1, zero=True):
    """symbols [..., map_size] int16 -> (hist int32 [n_maps, 2*radius+1], overflow int32 [n_maps]); `out` = that pair,
    preallocated (zeroed here unless zero=False: the kernel accumulates). first_map / map_step: only every map_step-th
    map starting at first_map (e.g. the exception map of every image of a batch)."""
    map_size = symbols_planar.shape[-1]
    n_maps = (symbols_planar.numel()//map_size - first_map + map_step - 1)//map_step
    if out is None:
        hist = torch.zeros((n_maps, 2*radius + 1), dtype=torch.int32, device=symbols_planar.device)
        overflow = torch.zeros(n_maps, dtype=torch.int32, device=symbols_planar.device)
    else:
        (hist, overflow) = out
        if zero:
            hist.zero_()
            overflow.zero_()
    _check(_native.hip().eae_hip_symbol_histograms_strided(_p(symbols_planar), _p(hist), radius, _p(overflow), n_maps, map_size,
                                                           first_map, map_step, _stream(symbols_planar)), 'eae_hip_symbol_histograms_strided')
    return hist, overflow


def ladder_max_points(length):
    """The most rate points one `eae_hip_ladder_histograms` launch takes at truncated unary length `length`; 0 when none fits."""
    return int(_native.hip().eae_hip_ladder_max_points(int(length)))


def _bypass_bits_of_magnitudes(magnitudes, length):
    """Bits |symbol| = magnitudes (int64 array) leaves in the bypass stream (include/eae_hip.h, rate ladder): the sign of a non-zero
    symbol, and 2 floor(log2(|s| - L + 1)) + 1 bits of suffix from L on."""
    import numpy
    suffix = numpy.maximum(magnitudes - length + 1, 1)
    nb_bits = numpy.frexp(suffix.astype(numpy.float64))[1].astype(numpy.int64) - 1       # floor(log2(.)), exact below 2^53
    return (magnitudes != 0).astype(numpy.int64) + numpy.where(magnitudes >= length, 2*nb_bits + 1, 0)


def _wrapped_magnitudes(y, bin_widths, map_mean, rdo=None):
    """|symbol| of y [N, ..., 128] at a rate point whose int16 symbols have wrapped, recounted on the host with the quantiser's float32
    expressions (numpy divides and rounds as the kernels do) -> numpy (magnitudes int64 [N, hw, 128], 0 where the symbol does not fit
    int16; good bool [N, hw, 128]: where it does). rdo: None, or (thresholds float32 [128, 16], length) of the rate-distortion
    optimised quantiser (ratecontrol.rdo_quantize_numpy)."""
    import numpy
    host = y.reshape(y.shape[0], -1, y.shape[-1]).cpu().numpy()
    bw = bin_widths.cpu().numpy()
    centered = host - (map_mean.cpu().numpy() if map_mean is not None else numpy.float32(0.))
    with numpy.errstate(all='ignore'):
        if rdo is None:
            r = numpy.rint(centered/bw)
        else:
            from . import ratecontrol
            r = ratecontrol.rdo_quantize_numpy(centered, bw, None, rdo[0].cpu().numpy(), rdo[1])
        rs = numpy.abs(numpy.rint(bw*r/bw))
        good = rs < numpy.float32(32768.)
    return numpy.where(good, rs, 0.).astype(numpy.int64), good


def _point_symbols(y, bin_widths, map_mean, rdo):
    """The quantiser pass of `_ladder_point_by_passes` and `_ladder_point_tiles_by_passes`: `quantize_maps`, or with rdo =
    (thresholds float32 [128, 16], length) `latent_quantize_rdo` at that one point."""
    if rdo is None:
        return quantize_maps(y, bin_widths, map_mean, want_symbols=True)
    return latent_quantize_rdo(y, bin_widths.reshape(1, -1), rdo[0].reshape(1, NB_MAPS, 16).contiguous(),
                               torch.zeros(y.shape[0], dtype=torch.int32, device=y.device), rdo[1], map_mean, want_symbols=True)


def _ladder_point_by_passes(y, bin_widths, map_mean, length, rdo=None):
    """One rate point by the route `stats.compute_binary_probabilities` takes: `quantize_maps`, `symbol_histograms`, a fold on the
    host -> numpy (hist int64 [N, 128, L + 1], bypass bits int64 [N, 128], range errors). A point with range errors, whose int16
    symbols have wrapped, is recounted on the host with the quantiser's float32 expressions (`_wrapped_magnitudes`), so that the
    arrays are `eae_hip_ladder_histograms`' in every case."""
    import numpy
    (n, c) = (y.shape[0], y.shape[-1])
    q = _point_symbols(y, bin_widths, map_mean, rdo)
    range_errors = int(q['checks'][0].item())
    if range_errors:
        (magnitudes, good) = _wrapped_magnitudes(y, bin_widths, map_mean, rdo)
        hist = numpy.zeros((n, c, length + 1), dtype=numpy.int64)
        for b in range(length + 1):
            hist[:, :, b] = (good & ((magnitudes == b) if b < length else (magnitudes >= length))).sum(axis=1)
        return hist, (_bypass_bits_of_magnitudes(magnitudes, length)*good).sum(axis=1), range_errors
    radius = 1024
    (full, overflow) = symbol_histograms(q['symbols'], radius)
    if int(overflow.sum().item()) != 0:
        radius = 32768
        full = torch.cat([symbol_histograms(q['symbols'][i], radius)[0] for i in range(n)])      # 32 MB of bins per image
    full = full.cpu().numpy().astype(numpy.int64).reshape(n, c, 2*radius + 1)
    by_magnitude = full[:, :, radius:].copy()
    by_magnitude[:, :, 1:] += full[:, :, :radius][:, :, ::-1]
    hist = numpy.concatenate([by_magnitude[:, :, :length], by_magnitude[:, :, length:].sum(axis=2, keepdims=True)], axis=2)
    bits = (by_magnitude*_bypass_bits_of_magnitudes(numpy.arange(radius + 1, dtype=numpy.int64), length)).sum(axis=2)
    return hist, bits, 0


def _ladder_point_tiles_by_passes(y, bin_widths, map_mean, length, tiles, rdo=None):
    """One rate point of `ladder_histograms_tiles` without its kernel: the symbols of `quantize_maps` folded per tile on the host ->
    numpy (hist int64 [N, T, 128, L + 1], bypass bits int64 [N, T, 128], range errors). A point with range errors, whose int16
    symbols have wrapped, is counted from the quantiser's float32 expressions instead (`_wrapped_magnitudes`). y [N, h, w, 128];
    tiles: the rows of `container.coding_tile_grid`."""
    import numpy
    (n, h, w, c) = y.shape
    nb_tiles = tiles.shape[0]
    q = _point_symbols(y, bin_widths, map_mean, rdo)
    range_errors = int(q['checks'][0].item())
    if range_errors:
        (magnitudes, good) = _wrapped_magnitudes(y, bin_widths, map_mean, rdo)
    else:
        magnitudes = numpy.abs(q['symbols'].cpu().numpy().astype(numpy.int64)).transpose(0, 2, 1)          # [N, hw, 128]
        good = numpy.ones(magnitudes.shape, dtype=bool)
    (good, magnitudes) = (good.reshape(n, h, w, c), magnitudes.reshape(n, h, w, c))
    clipped = numpy.minimum(magnitudes, length)
    bits = _bypass_bits_of_magnitudes(magnitudes, length)*good
    hist = numpy.zeros((n, nb_tiles, c, length + 1), dtype=numpy.int64)
    bypass = numpy.zeros((n, nb_tiles, c), dtype=numpy.int64)
    for (t, (r0, c0, rows, cols, _)) in enumerate(tiles.tolist()):
        window = (slice(None), slice(r0, r0 + rows), slice(c0, c0 + cols))
        for b in range(length + 1):
            hist[:, t, :, b] = (good[window] & (clipped[window] == b)).sum(axis=(1, 2))
        bypass[:, t] = bits[window].sum(axis=(1, 2))
    return hist, bypass, range_errors


def _ladder_points_checked(bin_widths_points, map_mean, length):
    """The argument checks `ladder_histograms` and `ladder_histograms_tiles` share, behind their own of y."""
    if bin_widths_points.dtype != torch.float32 or bin_widths_points.dim() != 2 or bin_widths_points.shape[1] != NB_MAPS:
        raise HipError('bin_widths_points must be float32 [K, 128]')
    if map_mean is not None and (map_mean.dtype != torch.float32 or map_mean.numel() != NB_MAPS):
        raise HipError('map_mean must be float32 of 128 elements')
    if length < 1 or length > 255:
        raise ValueError('The truncated unary length does not belong to [1, 255].')


def _ladder_accumulate(y, bin_widths_points, length, out, group, launch, point_by_passes):
    """What `ladder_histograms` (group = ()) and `ladder_histograms_tiles` (group = (T,)) do alike once their arguments are checked:
    the counts are [N, K] + group + [128, ...]. launch(k0, k1, hist, bypass_bits, range_errors): the native call for the points
    [k0, k1) of the ladder; point_by_passes(k): point k folded on the host, as `_ladder_point_by_passes`."""
    (n, c, d) = (y.shape[0], y.shape[-1], y.device)
    k_points = bin_widths_points.shape[0]
    if k_points < 1:
        raise ValueError('A ladder has at least one rate point.')

    def buffers(points, errors=None):
        return (torch.zeros((n, points) + group + (c, length + 1), dtype=torch.int32, device=d),
                torch.zeros((n, points) + group + (c,), dtype=torch.int64, device=d),
                torch.zeros(points, dtype=torch.int32, device=d) if errors is None else errors)

    if out is None:
        out = buffers(k_points)
    (hist, bypass_bits, range_errors) = out
    if (hist.dtype, bypass_bits.dtype, range_errors.dtype) != (torch.int32, torch.int64, torch.int32) \
            or tuple(hist.shape) != (n, k_points) + group + (c, length + 1) or tuple(bypass_bits.shape) != (n, k_points) + group + (c,) \
            or tuple(range_errors.shape) != (k_points,):
        raise HipError('`out` must be (int32 [N, K, {0}128, L + 1], int64 [N, K, {0}128], int32 [K])'.format('T, ' if group else ''))
    most = ladder_max_points(length)
    if most == 0:
        for k in range(k_points):
            (hist_k, bits_k, errors_k) = point_by_passes(k)
            hist[:, k] += torch.from_numpy(hist_k).to(d).to(torch.int32)
            bypass_bits[:, k] += torch.from_numpy(bits_k).to(d)
            range_errors[k] += errors_k
        return out
    whole = k_points <= most
    for k0 in range(0, k_points, most):
        k1 = min(k0 + most, k_points)
        # a launch writes [N][its points][...]: a part of a longer ladder gets buffers of its own, added into the whole afterwards
        part = out if whole else buffers(k1 - k0, range_errors[k0:k1])
        launch(k0, k1, *part)
        if not whole:
            hist[:, k0:k1] += part[0]
            bypass_bits[:, k0:k1] += part[1]
    return out


def ladder_histograms(y, bin_widths_points, map_mean=None, length=10, out=None):
    """One pass over y [N, h, w, 128] (or [N, hw, 128]) for the K rate points bin_widths_points float32 [K, 128] (include/eae_hip.h,
    rate ladder) -> (hist int32 [N, K, 128, L + 1]: |symbol| clipped at L = length; bypass_bits int64 [N, K, 128]: the exact length
    of every map's bypass stream; range_errors int32 [K]: elements whose symbol does not fit int16, counted nowhere else).
    A ladder longer than `ladder_max_points(length)` takes several launches. At a length for which not one point fits a launch
    (large L) every point goes the route of `stats.compute_binary_probabilities` instead -- `quantize_maps`, `symbol_histograms`, a
    fold on the host -- and the same arrays come back. out: that triple, preallocated, to ACCUMULATE into (the kernel adds)."""
    n = y.shape[0]
    c = y.shape[-1]
    hw = y.numel()//(n*c)
    length = int(length)
    if c != NB_MAPS or y.dtype != torch.float32:
        raise HipError('y must be float32 [N, ..., 128]')
    _ladder_points_checked(bin_widths_points, map_mean, length)

    def launch(k0, k1, hist, bypass_bits, range_errors):
        _check(_native.hip().eae_hip_ladder_histograms(_p(y), _p(map_mean), _p(bin_widths_points[k0:k1]), k1 - k0, length, _p(hist),
                                                       _p(bypass_bits), _p(range_errors), n, hw, _stream(y)), 'eae_hip_ladder_histograms')

    return _ladder_accumulate(y, bin_widths_points, length, out, (), launch,
                              lambda k: _ladder_point_by_passes(y, bin_widths_points[k].contiguous(), map_mean, length))


def ladder_histograms_tiles(y, bin_widths_points, coding_tile, map_mean=None, length=10, out=None):
    """`ladder_histograms` per coding tile (include/eae_hip.h: eae_hip_ladder_histograms_tiles). y float32
    [N, h, w, 128]; coding_tile=(th, tw) latents, clamped to the plane as `container.encode_images` clamps it; the T tiles are those
    of `container.coding_tile_grid(h, w, coding_tile)`, row-major -> (hist int32 [N, K, T, 128, L + 1], bypass_bits int64
    [N, K, T, 128], range_errors int32 [K]). Summed over T they are `ladder_histograms`' on the same input.
    A ladder longer than `ladder_max_points(length)` takes several launches; at a length for which not one point fits a launch the
    same arrays are folded on the host from `quantize_maps` symbols. out: that triple, preallocated, to ACCUMULATE into."""
    if y.dim() != 4 or y.shape[-1] != NB_MAPS or y.dtype != torch.float32:
        raise HipError('y must be float32 [N, h, w, 128]')
    (n, h, w, _) = y.shape
    length = int(length)
    _ladder_points_checked(bin_widths_points, map_mean, length)
    from . import container                       # (it imports this module; both are loaded by the time anything is called)
    (th, tw) = container._positive_pair(coding_tile, '`coding_tile`')
    (th, tw) = (min(th, h), min(tw, w))
    (tiles, _) = container.coding_tile_grid(h, w, (th, tw))

    def launch(k0, k1, hist, bypass_bits, range_errors):
        _check(_native.hip().eae_hip_ladder_histograms_tiles(_p(y), _p(map_mean), _p(bin_widths_points[k0:k1]), k1 - k0, length, _p(hist),
                                                             _p(bypass_bits), _p(range_errors), n, h, w, th, tw, _stream(y)),
               'eae_hip_ladder_histograms_tiles')

    return _ladder_accumulate(y, bin_widths_points, length, out, (tiles.shape[0],), launch,
                              lambda k: _ladder_point_tiles_by_passes(y, bin_widths_points[k].contiguous(), map_mean, length, tiles))


def rdo_thresholds_by_magnitude(thresholds_points):
    """thresholds_points float32 [K, 128, 16] (ratecontrol.rdo_thresholds) -> the copy [K, 16, 128] `eae_hip_ladder_histograms_rdo`
    reads (include/eae_hip.h): a codec makes it once and hands it to `ladder_histograms_rdo` with every call."""
    if thresholds_points.dtype != torch.float32 or thresholds_points.dim() != 3 or tuple(thresholds_points.shape[1:]) != (NB_MAPS, 16):
        raise HipError('thresholds_points must be float32 [K, 128, 16]')
    return thresholds_points.transpose(1, 2).contiguous()


def _ladder_thresholds_checked(bin_widths_points, thresholds_points, by_magnitude):
    """The checks of the two tables of `ladder_histograms_rdo` and `ladder_histograms_rdo_tiles` -> the table by magnitude."""
    k_points = bin_widths_points.shape[0]
    if thresholds_points.dtype != torch.float32 or tuple(thresholds_points.shape) != (k_points, NB_MAPS, 16):
        raise HipError('thresholds_points must be float32 [K, 128, 16]')
    if by_magnitude is None:
        return rdo_thresholds_by_magnitude(thresholds_points)
    if by_magnitude.dtype != torch.float32 or tuple(by_magnitude.shape) != (k_points, 16, NB_MAPS) or not by_magnitude.is_contiguous():
        raise HipError('by_magnitude must be a contiguous float32 [K, 16, 128]')
    return by_magnitude


def ladder_histograms_rdo(y, bin_widths_points, thresholds_points, map_mean=None, length=10, out=None, by_magnitude=None):
    """`ladder_histograms` of the symbols the rate-distortion optimised quantiser chooses (include/eae_hip.h:
    eae_hip_ladder_histograms_rdo; the rule is ratecontrol.rdo_quantize_numpy): thresholds_points float32
    [K, 128, 16] (ratecontrol.rdo_thresholds of the K points). Point k of the result counts the symbols `latent_quantize_rdo` writes
    with point == k; thresholds of zeros give `ladder_histograms`' words. by_magnitude: `rdo_thresholds_by_magnitude(
    thresholds_points)`, made once by a caller that launches every step (None: made here, a transposition per call). Everything
    else, `out` and the routes of a long ladder and of a large L included, as `ladder_histograms`."""
    n = y.shape[0]
    c = y.shape[-1]
    hw = y.numel()//(n*c)
    length = int(length)
    if c != NB_MAPS or y.dtype != torch.float32:
        raise HipError('y must be float32 [N, ..., 128]')
    _ladder_points_checked(bin_widths_points, map_mean, length)
    by_magnitude = _ladder_thresholds_checked(bin_widths_points, thresholds_points, by_magnitude)

    def launch(k0, k1, hist, bypass_bits, range_errors):
        _check(_native.hip().eae_hip_ladder_histograms_rdo(_p(y), _p(map_mean), _p(bin_widths_points[k0:k1]), _p(by_magnitude[k0:k1]),
                                                           k1 - k0, length, _p(hist), _p(bypass_bits), _p(range_errors), n, hw,
                                                           _stream(y)), 'eae_hip_ladder_histograms_rdo')

    return _ladder_accumulate(y, bin_widths_points, length, out, (), launch,
                              lambda k: _ladder_point_by_passes(y, bin_widths_points[k].contiguous(), map_mean, length,
                                                                (thresholds_points[k], length)))


def ladder_histograms_rdo_tiles(y, bin_widths_points, thresholds_points, coding_tile, map_mean=None, length=10, out=None,
                                by_magnitude=None):
    """`ladder_histograms_rdo` per coding tile, as `ladder_histograms_tiles` is `ladder_histograms`' (include/eae_hip.h:
    eae_hip_ladder_histograms_rdo_tiles). y float32 [N, h, w, 128] -> (hist int32 [N, K, T, 128, L + 1], bypass_bits int64
    [N, K, T, 128], range_errors int32 [K]); summed over T they are `ladder_histograms_rdo`'s on the same input."""
    if y.dim() != 4 or y.shape[-1] != NB_MAPS or y.dtype != torch.float32:
        raise HipError('y must be float32 [N, h, w, 128]')
    (n, h, w, _) = y.shape
    length = int(length)
    _ladder_points_checked(bin_widths_points, map_mean, length)
    by_magnitude = _ladder_thresholds_checked(bin_widths_points, thresholds_points, by_magnitude)
    from . import container
    (th, tw) = container._positive_pair(coding_tile, '`coding_tile`')
    (th, tw) = (min(th, h), min(tw, w))
    (tiles, _) = container.coding_tile_grid(h, w, (th, tw))

    def launch(k0, k1, hist, bypass_bits, range_errors):
        _check(_native.hip().eae_hip_ladder_histograms_rdo_tiles(_p(y), _p(map_mean), _p(bin_widths_points[k0:k1]), _p(by_magnitude[k0:k1]),
                                                                 k1 - k0, length, _p(hist), _p(bypass_bits), _p(range_errors), n, h, w, th,
                                                                 tw, _stream(y)), 'eae_hip_ladder_histograms_rdo_tiles')

    return _ladder_accumulate(y, bin_widths_points, length, out, (tiles.shape[0],), launch,
                              lambda k: _ladder_point_tiles_by_passes(y, bin_widths_points[k].contiguous(), map_mean, length, tiles,
                                                                      (thresholds_points[k], length)))


def _ladder_select_checked(hist, bypass_bits, fixed_costs, log2_tables, map_size, budgets, tiled):
    """The argument checks `ladder_select` and `ladder_select_tiles` (tiled: counts per coding tile) share -> the shape of hist."""
    group_names = 'T, ' if tiled else ''
    if hist.dim() != (5 if tiled else 4) or hist.shape[-2] != NB_MAPS or hist.dtype != torch.int32:
        raise HipError('hist must be int32 [N, K, {0}128, L + 1]'.format(group_names))
    (n, k_points, length) = (hist.shape[0], hist.shape[1], hist.shape[-1] - 1)
    if bypass_bits.dtype != torch.int64 or tuple(bypass_bits.shape) != tuple(hist.shape[:-1]):
        raise HipError('bypass_bits must be int64 [N, K, {0}128]'.format(group_names))
    if fixed_costs.element_size() != 4 or fixed_costs.is_floating_point() or fixed_costs.numel() != k_points*NB_MAPS*length*2:
        raise HipError('fixed_costs must hold K x 128 x L x 2 32-bit words')
    if log2_tables is not None and (log2_tables.element_size() != 4 or log2_tables.is_floating_point()
                                    or log2_tables.numel() != 2*(map_size + 1)):
        raise HipError('log2_tables must hold 2 x (map_size + 1) 32-bit words')
    if budgets.dtype != torch.int64 or budgets.numel() != n:
        raise HipError('budgets must be int64 [N]')
    return tuple(hist.shape)


def _ladder_select_out(out, n, k_points, rows, d):
    """`out` of `ladder_select` and `ladder_select_tiles`, made where it is None and checked: `rows` rows of 128 in 'prob_row'."""
    if out is None:
        out = {'point': torch.empty(n, dtype=torch.int32, device=d), 'prob_row': torch.empty((rows, NB_MAPS), dtype=torch.int32, device=d),
               'upper': torch.empty((n, k_points), dtype=torch.int64, device=d), 'flags': torch.empty(n, dtype=torch.int32, device=d)}
    for (name, dtype, count) in (('point', torch.int32, n), ('prob_row', torch.int32, rows*NB_MAPS), ('upper', torch.int64, n*k_points),
                                 ('flags', torch.int32, n)):
        if out[name].dtype != dtype or out[name].numel() != count:
            raise HipError('`out[{0!r}]` must hold {1} elements of {2}'.format(name, count, dtype))
    return out


def ladder_select_tiles(hist, bypass_bits, fixed_costs, log2_tables, idx_map_exception, header_bytes, map_size, budgets, entry_image,
                        exception_row_base, out=None):
    """`ladder_select` for single-image EAT1 blobs (include/eae_hip.h: eae_hip_ladder_select_tiles; the host rule is
    ratecontrol.upper_bounds_fixed_tiles + valid_points on the counts summed over the tiles + select_by_upper_bound). hist int32
    [N, K, T, 128, L + 1] and bypass_bits int64 [N, K, T, 128] as `ladder_histograms_tiles` leaves them; map_size: symbols of a WHOLE
    map; header_bytes: ratecontrol.header_bytes(ladder, height, width, coding_tile); entry_image int32 [entries] on the device: the
    image of every (image, tile) entry in the order the coder takes them (`codec.coding_tile_layout`'s run order). The other
    arguments as `ladder_select`. -> dict: 'point' int32 [N], 'prob_row' int32 [entries, 128], 'upper' int64 [N, K], 'flags' int32
    [N]. out: that dict, preallocated; every element is written."""
    map_size = int(map_size)
    (n, k_points, nb_tiles, _, nb) = _ladder_select_checked(hist, bypass_bits, fixed_costs, log2_tables, map_size, budgets, True)
    if entry_image.dtype != torch.int32 or entry_image.dim() != 1 or entry_image.numel() < 1:
        raise HipError('entry_image must be int32 [entries]')
    entries = entry_image.numel()
    out = _ladder_select_out(out, n, k_points, entries, hist.device)
    _check(_native.hip().eae_hip_ladder_select_tiles(_p(hist), _p(bypass_bits), _p(fixed_costs), _p(log2_tables), k_points, nb - 1,
                                                     int(idx_map_exception), int(header_bytes), map_size, nb_tiles, _p(budgets),
                                                     _p(entry_image), entries, int(exception_row_base), _p(out['point']),
                                                     _p(out['prob_row']), _p(out['upper']), _p(out['flags']), n, _stream(hist)),
           'eae_hip_ladder_select_tiles')
    return out


def ladder_select(hist, bypass_bits, fixed_costs, log2_tables, idx_map_exception, header_bytes, map_size, budgets, exception_row_base,
                  out=None):
    """The rate point of every image for its byte budget, on the device (include/eae_hip.h: eae_hip_ladder_select; the host rule is
    ratecontrol.upper_bounds_fixed + valid_points + select_by_upper_bound). hist int32 [N, K, 128, L + 1] and bypass_bits int64
    [N, K, 128] as `ladder_histograms` leaves them; fixed_costs int32/uint32 [K, 128, L, 2] (ratecontrol.fixed_costs) and log2_tables
    [2, map_size + 1] (ratecontrol.log2_tables; None without an exception map), as device tensors of 32-bit words; budgets int64 [N]
    on the device. -> dict: 'point' int32 [N], 'prob_row' int32 [N, 128], 'upper' int64 [N, K], 'flags' int32 [N] (bit 0 promised,
    bit 1 no valid point). out: that dict, preallocated; every element is written."""
    map_size = int(map_size)
    (n, k_points, _, nb) = _ladder_select_checked(hist, bypass_bits, fixed_costs, log2_tables, map_size, budgets, False)
    out = _ladder_select_out(out, n, k_points, n, hist.device)
    _check(_native.hip().eae_hip_ladder_select(_p(hist), _p(bypass_bits), _p(fixed_costs), _p(log2_tables), k_points, nb - 1,
                                               int(idx_map_exception), int(header_bytes), map_size, _p(budgets), int(exception_row_base),
                                               _p(out['point']), _p(out['prob_row']), _p(out['upper']), _p(out['flags']), n,
                                               _stream(hist)), 'eae_hip_ladder_select')
    return out


def _quality_search_checked(first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags, k_points, rows, more=()):
    """The tensor table `quality_search` and `quality_search_tiles` share -> (N, R). rows: of 128 in `prob_row`; more: (name, tensor,
    dtype, elements) entries behind it."""
    n = first.numel()
    nb_rounds = int(k_points).bit_length()
    for (name, t, dtype, count) in (('first', first, torch.int32, n), ('max_sse', max_sse, torch.int64, n), ('state', state, torch.int32, 2*n),
                                    ('probe_acc', probe_acc, torch.int64, n), ('point', point, torch.int32, n),
                                    ('prob_row', prob_row, torch.int32, rows*NB_MAPS), ('trace_point', trace_point, torch.int32, n*nb_rounds),
                                    ('trace_sse', trace_sse, torch.int64, n*nb_rounds), ('flags', flags, torch.int32, n)) + tuple(more):
        if t.dtype != dtype or t.numel() != count:
            raise HipError('`{0}` must hold {1} elements of {2}'.format(name, count, dtype))
    return n, nb_rounds


def quality_search(first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags, k_points, round, idx_map_exception,
                   exception_row_base):
    """One round of the bisection for a PSNR floor per image, on the device (include/eae_hip.h: eae_hip_quality_search; the host rule
    is ratecontrol.select_by_quality). All tensors are preallocated device memory: first int32 [N], max_sse int64 [N], state int32
    [N, 2], probe_acc int64 [N] (what `tconv9x9s4_luma` adds the probe's squared errors into), point int32 [N], prob_row int32
    [N, 128], trace_point int32 [N, R], trace_sse int64 [N, R], flags int32 [N], R = ratecontrol.quality_rounds(k_points). round:
    0..R, the only argument that differs between the R + 1 calls of a step."""
    (n, nb_rounds) = _quality_search_checked(first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags, k_points,
                                             first.numel())
    _check(_native.hip().eae_hip_quality_search(_p(first), _p(max_sse), _p(state), _p(probe_acc), _p(point), _p(prob_row), _p(trace_point),
                                                _p(trace_sse), _p(flags), int(k_points), nb_rounds, int(round), int(idx_map_exception),
                                                int(exception_row_base), n, _stream(first)), 'eae_hip_quality_search')


def quality_search_tiles(first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags, run_entry, nb_tiles, k_points,
                         round, idx_map_exception, exception_row_base):
    """`quality_search` for a step in coding tiles (include/eae_hip.h: eae_hip_quality_search_tiles; the rows are
    `codec.tile_prob_rows`). run_entry int32 [N * nb_tiles] on the device: `codec.coding_tile_layout`'s 'run_entry'; prob_row int32
    [N * nb_tiles, 128], written in that layout's run order. Everything else as `quality_search`."""
    nb_tiles = int(nb_tiles)
    (n, nb_rounds) = _quality_search_checked(first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags, k_points,
                                             first.numel()*nb_tiles, [('run_entry', run_entry, torch.int32, first.numel()*nb_tiles)])
    _check(_native.hip().eae_hip_quality_search_tiles(_p(first), _p(max_sse), _p(state), _p(probe_acc), _p(point), _p(prob_row),
                                                      _p(trace_point), _p(trace_sse), _p(flags), _p(run_entry), nb_tiles, int(k_points),
                                                      nb_rounds, int(round), int(idx_map_exception), int(exception_row_base), n,
                                                      _stream(first)), 'eae_hip_quality_search_tiles')


def _quantize_rows_checked(y, bin_widths_points, point, map_mean, igdn_out, want_shifted, want_symbols, want_flags, out_symbols, out_flags,
                           out_checks, want_checks=True, out_shifted=None, out_t=None, thresholds_points=None):
    """The input checks and the outputs of `latent_quantize_rows` and `latent_quantize_rdo` (thresholds_points: the latter's table).
    Returns (n, hw, the dict both return)."""
    n = y.shape[0]
    c = y.shape[-1]
    hw = y.numel()//(n*c)
    d = y.device
    if c != NB_MAPS or y.dtype != torch.float32:
        raise HipError('y must be float32 [N, ..., 128]')
    if bin_widths_points.dtype != torch.float32 or bin_widths_points.dim() != 2 or bin_widths_points.shape[1] != NB_MAPS:
        raise HipError('bin_widths_points must be float32 [K, 128]')
    if thresholds_points is not None and (thresholds_points.dtype != torch.float32 or
                                          tuple(thresholds_points.shape) != (bin_widths_points.shape[0], NB_MAPS, 16)):
        raise HipError('thresholds_points must be float32 [K, 128, 16]')
    if point.dtype != torch.int32 or point.numel() != n:
        raise HipError('point must be int32 [N]')
    if map_mean is not None and (map_mean.dtype != torch.float32 or map_mean.numel() != NB_MAPS):
        raise HipError('map_mean must be float32 of 128 elements')
    for (name, out) in (('out_shifted', out_shifted), ('out_t', out_t)):
        if out is not None and (out.dtype != torch.float32 or out.numel() != y.numel()):
            raise HipError('`{0}` must be a float32 tensor of the size of y'.format(name))
    shifted = (out_shifted if out_shifted is not None else torch.empty_like(y)) if want_shifted else None
    t = (out_t if out_t is not None else torch.empty_like(y)) if igdn_out is not None else None
    symbols = (out_symbols if out_symbols is not None else torch.empty((n, c, hw), dtype=torch.int16, device=d)) if want_symbols else None
    if symbols is not None and (symbols.dtype != torch.int16 or symbols.numel() != n*c*hw):
        raise TypeError('`out_symbols` must be an int16 tensor of N x C x hw elements.')
    flags = (out_flags if out_flags is not None else torch.zeros((n, c), dtype=torch.int32, device=d)) if want_flags else None
    if flags is not None and flags.numel() != n*c:
        raise HipError('`out_flags` must hold N x 128 words')
    checks = (out_checks if out_checks is not None else torch.zeros(3, dtype=torch.int32, device=d)) if want_checks else None
    if checks is not None and checks.numel() < 3:
        raise HipError('`out_checks` must hold three words')
    return n, hw, {'shifted': shifted, 't': t, 'symbols': symbols, 'nonzero_flags': flags, 'checks': checks}


def latent_quantize_rows(y, bin_widths_points, point, map_mean=None, igdn_out=None, want_shifted=False, want_symbols=True,
                         want_flags=False, out_symbols=None, out_flags=None, out_checks=None, want_checks=True, out_shifted=None,
                         out_t=None):
    """The quantiser half of `latent_stage` with one row of bin widths per image (include/eae_hip.h: eae_hip_latent_quantize_rows):
    y [N, h, w, 128] (or [N, hw, 128]) are the latents after gdn_3, image i is quantised with bin_widths_points[point[i]] (float32
    [K, 128]; point int32 [N] on the device, clamped to [0, K)). Returns `latent_stage`'s dict without 'y'; image i's part equals
    `latent_stage(y[i:i + 1], bin_widths_points[point[i]], map_mean, gdn_in=None, igdn_out=igdn_out)` bit for bit. out_* buffers:
    preallocated, flags / checks already zeroed (see quantize_maps). want_checks=False: no check is counted ('checks': None).
    out_shifted / out_t: preallocated float32 outputs of y's size (a probe of `codec.QualityCodec` owns its latent buffer)."""
    (n, hw, out) = _quantize_rows_checked(y, bin_widths_points, point, map_mean, igdn_out, want_shifted, want_symbols, want_flags, out_symbols,
                                          out_flags, out_checks, want_checks, out_shifted, out_t)
    (g_out, b_out) = igdn_out if igdn_out is not None else (None, None)
    _check(_native.hip().eae_hip_latent_quantize_rows(_p(y), _p(map_mean), _p(bin_widths_points), _p(point), bin_widths_points.shape[0],
                                                      _p(g_out), _p(b_out), _p(out['shifted']), _p(out['t']), _p(out['symbols']),
                                                      _p(out['nonzero_flags']), _p(out['checks']), n, hw, _stream(y)),
           'eae_hip_latent_quantize_rows')
    return out


def latent_quantize_rdo(y, bin_widths_points, thresholds_points, point, truncated_unary_length, map_mean=None, igdn_out=None,
                        want_shifted=False, want_symbols=True, want_flags=False, out_symbols=None, out_flags=None, out_checks=None,
                        want_checks=True, out_shifted=None, out_t=None):
    """`latent_quantize_rows` with the rate-distortion optimised choice of every symbol (include/eae_hip.h:
    eae_hip_latent_quantize_rdo; the rule is ratecontrol.rdo_quantize_numpy): thresholds_points float32
    [K, 128, 16] (ratecontrol.rdo_thresholds), image i takes row point[i] of it as of bin_widths_points. A latent whose nearest
    symbol has magnitude a in [1, min(L, 16)] is coded one step nearer zero when 2 (|x| - a) + 1 < thresholds[k, c, a - 1].
    Returns `latent_quantize_rows`' dict; with thresholds of zeros, its bits. want_checks, out_shifted, out_t: as there."""
    (n, hw, out) = _quantize_rows_checked(y, bin_widths_points, point, map_mean, igdn_out, want_shifted, want_symbols, want_flags, out_symbols,
                                          out_flags, out_checks, want_checks, out_shifted, out_t, thresholds_points=thresholds_points)
    (g_out, b_out) = igdn_out if igdn_out is not None else (None, None)
    _check(_native.hip().eae_hip_latent_quantize_rdo(_p(y), _p(map_mean), _p(bin_widths_points), _p(thresholds_points), _p(point),
                                                     bin_widths_points.shape[0], int(truncated_unary_length), _p(g_out), _p(b_out),
                                                     _p(out['shifted']), _p(out['t']), _p(out['symbols']), _p(out['nonzero_flags']),
                                                     _p(out['checks']), n, hw, _stream(y)), 'eae_hip_latent_quantize_rdo')
    return out


def cast_bt601(x):
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _check(_native.hip().eae_hip_cast_bt601(_p(x), _p(out), x.numel(), _stream()), 'eae_hip_cast_bt601')
    return out


def rgb_to_ycbcr(rgb_uint8, want_ycbcr=True, want_luma=False):
    """uint8 [..., 3] RGB -> (ycbcr uint8 [..., 3] or None, luma uint8 [...] or None), ITU-R BT.601 (tools.py:1019-1083)."""
    count = rgb_uint8.numel()//3
    ycbcr = torch.empty_like(rgb_uint8) if want_ycbcr else None
    luma = torch.empty(rgb_uint8.shape[:-1], dtype=torch.uint8, device=rgb_uint8.device) if want_luma else None
    _check(_native.hip().eae_hip_rgb_to_ycbcr(_p(rgb_uint8), _p(ycbcr), _p(luma), count, _stream()), 'eae_hip_rgb_to_ycbcr')
    return ycbcr, luma


def sse_u8(a, b):
    """Per-image sum of squared differences of two uint8 stacks [N, ...] -> int64 [N]."""
    n = a.shape[0]
    sse = torch.zeros(n, dtype=torch.int64, device=a.device)
    _check(_native.hip().eae_hip_sse_u8(_p(a), _p(b), _p(sse), n, a.numel()//n, _stream()), 'eae_hip_sse_u8')
    return sse


# ---- tiled encode / decode (include/eae_hip.h, "tiled encode / decode"; the plan comes from pipeline.tile_plan) ----------

TILE_PLAN_COLS = 9


def _plan_pointers(plan_device, plan_host):
    """(device pointer, host pointer, rows) of one plan slice; both copies must hold the same int32 rows."""
    if plan_host.dtype.name != 'int32' or plan_host.ndim != 2 or plan_host.shape[1] != TILE_PLAN_COLS or not plan_host.flags.c_contiguous:
        raise HipError('the host plan must be a C-contiguous int32 array of {} columns'.format(TILE_PLAN_COLS))
    if plan_device.dtype != torch.int32 or tuple(plan_device.shape) != plan_host.shape:
        raise HipError('the device plan must be int32 of the host plan\'s shape')
    return _p(plan_device), plan_host.ctypes.data, plan_host.shape[0]


def tile_copy(plane, windows, plan_device, plan_host, unit, to_windows):
    """Rectangles between a full plane [N, h*unit, w*unit, ...] and a batch of windows [G, wh*unit, ww*unit, ...] of the same
    element type: to_windows=True gathers every whole window, False stitches every interior into the plane. h, w, wh, ww in
    latents; one plan row per window (G rows)."""
    if plane.dtype != windows.dtype:
        raise HipError('plane and windows must have the same dtype')
    (n, hp, wp) = plane.shape[:3]
    (g, hw_, ww_) = windows.shape[:3]
    if hp % unit or wp % unit or hw_ % unit or ww_ % unit:
        raise HipError('plane and window sides must be multiples of `unit`')
    elem_bytes = plane.element_size()*(plane[0, 0, 0].numel() if plane.dim() > 3 else 1)
    if windows.element_size()*(windows[0, 0, 0].numel() if windows.dim() > 3 else 1) != elem_bytes:
        raise HipError('plane and windows must have the same element size')
    (plan_p, host_p, rows) = _plan_pointers(plan_device, plan_host)
    if rows != g:
        raise HipError('one plan row per window')
    _check(_native.hip().eae_hip_tile_copy(_p(plane), n, hp//unit, wp//unit, _p(windows), hw_//unit, ww_//unit, unit, elem_bytes, plan_p,
                                           host_p, rows, 1 if to_windows else 0, _stream(plane)), 'eae_hip_tile_copy')


def tile_stitch_u8(windows, plan_device, plan_host, image=None, ref_u8=None, sse=None):
    """uint8 reconstruction windows [G, 16wh, 16ww] -> their interiors into image [N, 16h, 16w] (optional) and, with ref_u8, the
    squared error of exactly those pixels added into sse int64 [N] (zeroed here when not given). Returns sse or None."""
    plane = image if image is not None else ref_u8
    if plane is None:
        raise HipError('tile_stitch_u8 needs an image or a reference')
    (n, hp, wp) = plane.shape[:3]
    (g, hw_, ww_) = windows.shape[:3]
    if ref_u8 is not None and sse is None:
        sse = torch.zeros(n, dtype=torch.int64, device=plane.device)
    if image is not None and ref_u8 is not None and image.shape != ref_u8.shape:
        raise HipError('image and reference must have the same shape')
    (plan_p, host_p, rows) = _plan_pointers(plan_device, plan_host)
    if rows != g or hp % 16 or wp % 16 or hw_ % 16 or ww_ % 16:
        raise HipError('one plan row per window, sides multiples of 16')
    _check(_native.hip().eae_hip_tile_stitch_u8(_p(windows), hw_//16, ww_//16, _p(image), _p(ref_u8), _p(sse), n, hp//16, wp//16,
                                                plan_p, host_p, rows, _stream(windows)), 'eae_hip_tile_stitch_u8')
    return sse


# ---- coding tiles of the EAT1 container (include/eae_hip.h, "coding tiles"; the plan comes from container.py) ---------------

TILE_SYMBOLS_PLAN_COLS = 6


def _symbols_plan_pointers(plan_device, plan_host):
    """(device pointer, host pointer, rows) of a coding-tile plan; both copies must hold the same int64 rows."""
    if plan_host.dtype.name != 'int64' or plan_host.ndim != 2 or plan_host.shape[1] != TILE_SYMBOLS_PLAN_COLS or not plan_host.flags.c_contiguous:
        raise HipError('the host plan must be a C-contiguous int64 array of {} columns'.format(TILE_SYMBOLS_PLAN_COLS))
    if plan_device.dtype != torch.int64 or tuple(plan_device.shape) != plan_host.shape:
        raise HipError('the device plan must be int64 of the host plan\'s shape')
    return _p(plan_device), plan_host.ctypes.data, plan_host.shape[0]


def tile_symbols_gather(symbols_planar, tiles, plan_device, plan_host, h, w):
    """int16 symbols [N, 128, h*w] -> the tile-major runs of the plan's coding tiles in `tiles` (int16, 1-D). One plan row per
    tile: image, origin (row, col), extent (rows, cols), offset of the tile's map 0 in `tiles`."""
    if symbols_planar.dtype != torch.int16 or tiles.dtype != torch.int16 or tiles.dim() != 1:
        raise HipError('symbols and tiles must be int16, tiles one-dimensional')
    (n, c, hw) = symbols_planar.shape
    if c != NB_MAPS or hw != h*w:
        raise HipError('symbols must be [N, 128, h*w]')
    (plan_p, host_p, rows) = _symbols_plan_pointers(plan_device, plan_host)
    _check(_native.hip().eae_hip_tile_symbols_gather(_p(symbols_planar), n, h, w, _p(tiles), tiles.numel(), plan_p, host_p, rows,
                                                     _stream(symbols_planar)), 'eae_hip_tile_symbols_gather')


def tile_symbols_dequantize(tiles, plan_device, plan_host, bin_widths, map_mean, out):
    """Tile-major int16 runs -> float32 out [N, hs, ws, 128] = bin_widths[c] * symbol + map_mean[c] (dequantize_maps' arithmetic)
    for every pixel of the plan's tiles inside `out`. Plan rows as tile_symbols_gather's, with image and origin in `out`."""
    if tiles.dtype != torch.int16 or tiles.dim() != 1:
        raise HipError('tiles must be one-dimensional int16')
    if out.dtype != torch.float32 or out.dim() != 4 or out.shape[3] != NB_MAPS:
        raise HipError('out must be float32 [N, hs, ws, 128]')
    if bin_widths.dtype != torch.float32 or bin_widths.numel() != NB_MAPS or (map_mean is not None and (map_mean.dtype != torch.float32 or map_mean.numel() != NB_MAPS)):
        raise HipError('bin widths and map means must be float32 of 128 elements')
    (plan_p, host_p, rows) = _symbols_plan_pointers(plan_device, plan_host)
    (n, hs, ws) = out.shape[:3]
    _check(_native.hip().eae_hip_tile_symbols_dequantize(_p(tiles), tiles.numel(), plan_p, host_p, rows, _p(bin_widths), _p(map_mean),
                                                         _p(out), n, hs, ws, _stream(tiles)), 'eae_hip_tile_symbols_dequantize')
    return out


def tile_symbols_dequantize_rows(tiles, plan_device, plan_host, bin_widths_rows, map_mean_rows, out):
    """`tile_symbols_dequantize` with one row of bin widths and one row of means (or None) per image of `out`, float32 [N, 128] each:
    a tile takes the rows of its plan row's image. Bit for bit `tile_symbols_dequantize` called image by image with that image's rows."""
    if tiles.dtype != torch.int16 or tiles.dim() != 1:
        raise HipError('tiles must be one-dimensional int16')
    if out.dtype != torch.float32 or out.dim() != 4 or out.shape[3] != NB_MAPS:
        raise HipError('out must be float32 [N, hs, ws, 128]')
    (n, hs, ws) = out.shape[:3]
    for rows in (bin_widths_rows,) if map_mean_rows is None else (bin_widths_rows, map_mean_rows):
        if rows.dtype != torch.float32 or rows.numel() != n*NB_MAPS or not rows.is_contiguous():
            raise HipError('bin widths and map means must be contiguous float32 of 128 elements per image of out')
    (plan_p, host_p, nb_rows) = _symbols_plan_pointers(plan_device, plan_host)
    _check(_native.hip().eae_hip_tile_symbols_dequantize_rows(_p(tiles), tiles.numel(), plan_p, host_p, nb_rows, _p(bin_widths_rows),
                                                              _p(map_mean_rows), _p(out), n, hs, ws, _stream(tiles)),
           'eae_hip_tile_symbols_dequantize_rows')
    return out


TILE_SYMBOLS_SLOT_COLS = 3


def tile_symbols_dequantize_placed(tiles, slots_device, slots_host, placement, bin_widths_rows, map_mean_rows, out):
    """`tile_symbols_dequantize_rows` with the plan in two halves (include/eae_hip.h): `slots_device` / `slots_host`, int64
    [n_slots, 3], the same rows on the device and on the host -- extent (rows, cols) and element offset of every slot in `tiles`,
    checked before the launch --, and `placement`, int32 [n_slots, 4] on the device -- image, origin row, origin col of every slot in
    `out`, one unused word --, which only the kernel reads: a slot whose image is outside `out` is skipped, an origin may be anything.
    No argument depends on a step's placement, so the launch can be captured."""
    if tiles.dtype != torch.int16 or tiles.dim() != 1:
        raise HipError('tiles must be one-dimensional int16')
    if out.dtype != torch.float32 or out.dim() != 4 or out.shape[3] != NB_MAPS:
        raise HipError('out must be float32 [N, hs, ws, 128]')
    (n, hs, ws) = out.shape[:3]
    for rows in (bin_widths_rows,) if map_mean_rows is None else (bin_widths_rows, map_mean_rows):
        if rows.dtype != torch.float32 or rows.numel() != n*NB_MAPS or not rows.is_contiguous():
            raise HipError('bin widths and map means must be contiguous float32 of 128 elements per image of out')
    if slots_host.dtype.name != 'int64' or slots_host.ndim != 2 or slots_host.shape[1] != TILE_SYMBOLS_SLOT_COLS or not slots_host.flags.c_contiguous:
        raise HipError('the host slots must be a C-contiguous int64 array of {} columns'.format(TILE_SYMBOLS_SLOT_COLS))
    if slots_device.dtype != torch.int64 or tuple(slots_device.shape) != slots_host.shape:
        raise HipError('the device slots must be int64 of the host slots\' shape')
    if placement.dtype != torch.int32 or placement.numel() != 4*slots_host.shape[0]:
        raise HipError('the placement must hold four int32 words per slot')
    _check(_native.hip().eae_hip_tile_symbols_dequantize_placed(_p(tiles), tiles.numel(), _p(slots_device), slots_host.ctypes.data,
                                                                slots_host.shape[0], _p(placement), _p(bin_widths_rows), _p(map_mean_rows),
                                                                _p(out), n, hs, ws, _stream(tiles)), 'eae_hip_tile_symbols_dequantize_placed')
    return out


# ---- lossless coder on the device (include/eae_hip.h, "lossless coder on the device") ---------------------------------

CODER_ROUNDTRIP, CODER_ENCODE_ONLY, CODER_ROUNDTRIP_VERIFY = 0, 1, 2


class CoderStreams(object):
    """Per-map streams of one batch, resident in HBM, in the layout of eae_coder_encode_maps (include/eae_coder.h):
    map m owns `streams[m]` (stride bytes): BAC bytes at +0, bypass bytes at +stride/2."""

    def __init__(self, n_maps, map_size, truncated_unary_length, device, results=None):
        self.n_maps = n_maps
        self.map_size = map_size
        self.truncated_unary_length = truncated_unary_length
        self.stride = coder_stream_stride_bytes(map_size, truncated_unary_length)
        self.streams = torch.empty((n_maps, self.stride), dtype=torch.uint8, device=device)
        # one allocation so that a caller can fetch all four per-map results with a single device -> host copy
        self.results = results if results is not None else torch.zeros((4, n_maps), dtype=torch.int32, device=device)
        # (its four rows are what the launches read and write: a block of columns of a wider results block will do)
        if self.results.shape != (4, n_maps) or self.results.dtype != torch.int32 or self.results.stride(1) != 1:
            raise TypeError('`results` must be an int32 tensor of shape (4, n_maps) with contiguous rows.')
        (self.bac_bits, self.bypass_bits, self.status, self.stage) = self.results.unbind(0)

    def nb_bits(self):
        return self.bac_bits + self.bypass_bits


def coder_compress_maps(symbols_planar, probabilities, prob_row, truncated_unary_length, mode=CODER_ROUNDTRIP_VERIFY,
                        out=None, lanes_per_wave=0):
    """symbols [..., map_size] int16 (device), probabilities [rows, L] float64 (device), prob_row int32 [n_maps] or None
    -> (CoderStreams, reconstruction or None). Asynchronous: per-map errors are in `streams.status`."""
    map_size = symbols_planar.shape[-1]
    n_maps = symbols_planar.numel()//map_size
    if symbols_planar.dtype != torch.int16 or probabilities.dtype != torch.float64:
        raise TypeError('`symbols_planar` must be int16 and `probabilities` float64.')
    if out is None:
        out = CoderStreams(n_maps, map_size, truncated_unary_length, symbols_planar.device)
    reconstruction = torch.empty_like(symbols_planar) if mode == CODER_ROUNDTRIP else None
    _check(_native.hip().eae_hip_coder_compress_maps(n_maps, map_size, _p(symbols_planar), _p(reconstruction) if reconstruction is not None else None,
                                                     truncated_unary_length, _p(probabilities), _p(prob_row) if prob_row is not None else None,
                                                     _p(out.streams), out.stride, _p(out.bac_bits), _p(out.bypass_bits), _p(out.status),
                                                     _p(out.stage), mode, lanes_per_wave, _stream(symbols_planar)), 'eae_hip_coder_compress_maps')
    return out, reconstruction


def coder_decode_maps(streams, probabilities, prob_row, lanes_per_wave=0):
    """CoderStreams -> int16 [n_maps, map_size] (device); maps with prob_row < 0 are left untouched (zeros)."""
    out = torch.zeros((streams.n_maps, streams.map_size), dtype=torch.int16, device=streams.streams.device)
    _check(_native.hip().eae_hip_coder_decode_maps(streams.n_maps, streams.map_size, _p(out), streams.truncated_unary_length,
                                                   _p(probabilities), _p(prob_row) if prob_row is not None else None,
                                                   _p(streams.streams), streams.stride, _p(streams.bac_bits), _p(streams.bypass_bits),
                                                   _p(streams.status), _p(streams.stage), lanes_per_wave, _stream()),
           'eae_hip_coder_decode_maps')
    return out


def coder_verify_maps(streams, expected_symbols, probabilities, prob_row, lanes_per_wave=0):
    """Decodes every map of `streams` and compares with `expected_symbols` on the device; failures land in
    `streams.status` (6 = roundtrip mismatch)."""
    if expected_symbols.dtype != torch.int16 or expected_symbols.numel() != streams.n_maps*streams.map_size:
        raise TypeError('`expected_symbols` must hold n_maps x map_size int16 symbols.')
    _check(_native.hip().eae_hip_coder_verify_maps(streams.n_maps, streams.map_size, _p(expected_symbols), streams.truncated_unary_length,
                                                   _p(probabilities), _p(prob_row), _p(streams.streams), streams.stride,
                                                   _p(streams.bac_bits), _p(streams.bypass_bits), _p(streams.status), _p(streams.stage),
                                                   lanes_per_wave, _stream()), 'eae_hip_coder_verify_maps')


def publish_to_host(src_device, dst_pinned):
    """Stream-ordered copy of a small device tensor into a pinned host tensor of the same byte size, done by a kernel
    (never blocks the calling thread). Synchronise an event recorded after it before reading `dst_pinned`."""
    nbytes = src_device.numel()*src_device.element_size()
    if not dst_pinned.is_pinned() or dst_pinned.numel()*dst_pinned.element_size() != nbytes or not dst_pinned.is_contiguous():
        raise HipError('expected a contiguous pinned host tensor of the same size')
    _check(_native.hip().eae_hip_publish_to_host(_p(src_device), dst_pinned.data_ptr(), nbytes, _stream()), 'eae_hip_publish_to_host')


def publish_sequence(counter_device, word_pinned):
    """Stream-ordered: increments `counter_device` (int32 device tensor of one element) and leaves the new value in `word_pinned`
    (int32 pinned host tensor of one element), behind everything the current stream has done so far (include/eae_hip.h)."""
    if counter_device.numel() != 1 or counter_device.element_size() != 4 or word_pinned.numel() != 1 or word_pinned.element_size() != 4:
        raise HipError('expected two 32-bit words')
    if not word_pinned.is_pinned():
        raise HipError('expected a pinned host word')
    _check(_native.hip().eae_hip_publish_sequence(_p(counter_device), word_pinned.data_ptr(), _stream(counter_device)), 'eae_hip_publish_sequence')


def publish_step(src_device, dst_pinned, clear_from, tickets_device, counter_device, word_pinned, conv_ws=None, error_word=None):
    """One launch for the end of a step's side (include/eae_hip.h: eae_hip_publish_step): [`conv_workspace_collect(conv_ws,
    error_word)`] -> `publish_to_host(src_device, dst_pinned)` -> `src_device` zeroed from element `clear_from` on (its accumulators,
    for the step that uses it next) -> `publish_sequence(counter_device, word_pinned)`. `tickets_device`: a zeroed int32 on the device."""
    nbytes = src_device.numel()*src_device.element_size()
    if not dst_pinned.is_pinned() or dst_pinned.numel()*dst_pinned.element_size() != nbytes or not dst_pinned.is_contiguous() or not word_pinned.is_pinned():
        raise HipError('expected contiguous pinned host tensors, the first of the size of the source')
    if any(t.numel() != 1 or t.element_size() != 4 for t in (tickets_device, counter_device, word_pinned)):
        raise HipError('expected three 32-bit words')
    _check(_native.hip().eae_hip_publish_step(_p(src_device), dst_pinned.data_ptr(), nbytes, int(clear_from)*src_device.element_size(),
                                              _p(conv_ws), _p(error_word), _p(tickets_device), _p(counter_device),
                                              word_pinned.data_ptr(), _stream(src_device)), 'eae_hip_publish_step')


def coder_stream_stride_bytes(map_size, truncated_unary_length):
    """Bytes of one map's stream region (`CoderStreams.stride`): arithmetic-coded bytes at +0, bypass bytes at half of it."""
    return int(_native.hip().eae_hip_coder_stream_stride_bytes(map_size, truncated_unary_length))


def coder_workspace_bytes(n_maps, map_size, truncated_unary_length):
    return int(_native.hip().eae_hip_coder_workspace_bytes(n_maps, map_size, truncated_unary_length))


def coder_workspace(n_maps, map_size, truncated_unary_length, device):
    """Scratch for coder_encode_batch / coder_decode_batch (one per batch in flight)."""
    return torch.empty(coder_workspace_bytes(n_maps, map_size, truncated_unary_length), dtype=torch.uint8, device=device)


def coder_encode_batch(symbols_planar, probabilities, prob_row, truncated_unary_length, out=None, workspace=None):
    """The 64-maps-per-wavefront encoder (include/eae_hip.h). Same results as coder_compress_maps(mode=CODER_ENCODE_ONLY)."""
    map_size = symbols_planar.shape[-1]
    n_maps = symbols_planar.numel()//map_size
    if symbols_planar.dtype != torch.int16 or probabilities.dtype != torch.float64:
        raise TypeError('`symbols_planar` must be int16 and `probabilities` float64.')
    if out is None:
        out = CoderStreams(n_maps, map_size, truncated_unary_length, symbols_planar.device)
    if workspace is None:
        workspace = coder_workspace(n_maps, map_size, truncated_unary_length, symbols_planar.device)
    _check(_native.hip().eae_hip_coder_encode_batch(n_maps, map_size, _p(symbols_planar), truncated_unary_length, _p(probabilities),
                                                    _p(prob_row), _p(out.streams), out.stride, _p(out.bac_bits), _p(out.bypass_bits),
                                                    _p(out.status), _p(out.stage), _p(workspace), workspace.numel(), _stream(symbols_planar)),
           'eae_hip_coder_encode_batch')
    return out


def coder_decode_batch(streams, probabilities, prob_row, expected=None, workspace=None, out=None):
    """The 64-maps-per-wavefront decoder. expected=None: returns the decoded symbols [n_maps, map_size] (skipped maps
    zero), in `out` when given (int16, n_maps x map_size contiguous elements; skipped maps are left as they are there).
    With `expected`: decodes into the workspace and compares on the device; failures land in `streams.status`.
    With a workspace (`coder_workspace`; always there with `expected`) the serial core leaves one prefix byte per symbol there
    and a data-parallel pass adds signs and suffixes (csrc/hip/coder_simd.hip); without, the general kernel decodes every
    map. Same results."""
    device = streams.streams.device
    if expected is None and out is not None:
        if out.dtype != torch.int16 or out.numel() != streams.n_maps*streams.map_size:
            raise TypeError('`out` must hold n_maps x map_size int16 symbols.')
    elif expected is None:
        out = torch.zeros((streams.n_maps, streams.map_size), dtype=torch.int16, device=device)
    else:
        out = None
        if expected.dtype != torch.int16 or expected.numel() != streams.n_maps*streams.map_size:
            raise TypeError('`expected` must hold n_maps x map_size int16 symbols.')
        if workspace is None:
            workspace = coder_workspace(streams.n_maps, streams.map_size, streams.truncated_unary_length, device)
    _check(_native.hip().eae_hip_coder_decode_batch(streams.n_maps, streams.map_size, _p(out), _p(expected), streams.truncated_unary_length,
                                                    _p(probabilities), _p(prob_row), _p(streams.streams), streams.stride,
                                                    _p(streams.bac_bits), _p(streams.bypass_bits), _p(streams.status), _p(streams.stage),
                                                    _p(workspace), workspace.numel() if workspace is not None else 0, _stream(streams.streams)),
           'eae_hip_coder_decode_batch')
    return out


class ExperimentalCoderMissing(HipError):
    """The library in use was built without -DEAE_EXPERIMENTAL_CODER (the product library always is: include/eae_hip.h)."""


def _experimental_coder():
    lib = _native.hip()
    if not hasattr(lib, 'eae_hip_coder_roundtrip_trailing'):
        raise ExperimentalCoderMissing(
            'the chunked / fused coder round trips are experimental and not part of lib/libeae_hip.so (both measured slower than '
            'encode_batch + decode_batch: DESIGN.md section 5); they live in lib/libeae_hip_test.so (EAE_HIP_LIB=test, or '
            '`make -C csrc EXTRA_HIPFLAGS=-DEAE_EXPERIMENTAL_CODER`)')
    return lib


def coder_trailing_workspace(n_maps, map_size, truncated_unary_length, device):
    """Scratch for coder_roundtrip_trailing (one per batch in flight). Experimental build only."""
    nbytes = int(_experimental_coder().eae_hip_coder_trailing_workspace_bytes(n_maps, map_size, truncated_unary_length))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def coder_roundtrip_trailing(symbols_planar, probabilities, prob_row, truncated_unary_length, chunks=4, out=None, workspace=None):
    """Encode every map, decode it back, compare (coder_encode_batch + coder_decode_batch(expected=symbols)) with the serial
    chains cut into `chunks` launches so that emit pass and decoder trail the encoder core (include/eae_hip.h: for one or two
    images). Same streams, bit counts, statuses and stages. Returns the CoderStreams. Experimental build only."""
    map_size = symbols_planar.shape[-1]
    n_maps = symbols_planar.numel()//map_size
    if symbols_planar.dtype != torch.int16 or probabilities.dtype != torch.float64:
        raise TypeError('`symbols_planar` must be int16 and `probabilities` float64.')
    if out is None:
        out = CoderStreams(n_maps, map_size, truncated_unary_length, symbols_planar.device)
    if workspace is None:
        workspace = coder_trailing_workspace(n_maps, map_size, truncated_unary_length, symbols_planar.device)
    _check(_experimental_coder().eae_hip_coder_roundtrip_trailing(n_maps, map_size, _p(symbols_planar), truncated_unary_length, _p(probabilities),
                                                          _p(prob_row), _p(out.streams), out.stride, _p(out.bac_bits), _p(out.bypass_bits),
                                                          _p(out.status), _p(out.stage), _p(workspace), workspace.numel(), int(chunks),
                                                          _stream(symbols_planar)), 'eae_hip_coder_roundtrip_trailing')
    return out


def coder_roundtrip_fused(symbols_planar, probabilities, prob_row, truncated_unary_length, out=None, workspace=None):
    """Encode every map, decode it back, compare, with the three serial stages of a group of 64 maps as three wavefronts of one
    workgroup handing records and stream words to each other through LDS (include/eae_hip.h: eae_hip_coder_roundtrip_fused). Same
    streams, bit counts, statuses and stages as coder_encode_batch + coder_decode_batch(expected=symbols). Returns the CoderStreams.
    Experimental build only."""
    map_size = symbols_planar.shape[-1]
    n_maps = symbols_planar.numel()//map_size
    if symbols_planar.dtype != torch.int16 or probabilities.dtype != torch.float64:
        raise TypeError('`symbols_planar` must be int16 and `probabilities` float64.')
    if out is None:
        out = CoderStreams(n_maps, map_size, truncated_unary_length, symbols_planar.device)
    if workspace is None:
        workspace = coder_trailing_workspace(n_maps, map_size, truncated_unary_length, symbols_planar.device)
    _check(_experimental_coder().eae_hip_coder_roundtrip_fused(n_maps, map_size, _p(symbols_planar), truncated_unary_length, _p(probabilities),
                                                       _p(prob_row), _p(out.streams), out.stride, _p(out.bac_bits), _p(out.bypass_bits),
                                                       _p(out.status), _p(out.stage), _p(workspace), workspace.numel(), _stream(symbols_planar)),
           'eae_hip_coder_roundtrip_fused')
    return out


def coder_pack_streams(streams, offsets, payload_bytes, payload=None):
    """Gathers the valid stream bytes of every map into one uint8 device tensor; `offsets` int64 [n_maps, 2] (device).
    payload: a uint8 device tensor of at least `payload_bytes` bytes to write into (several batches can share one)."""
    if payload is None:
        payload = torch.zeros(max(int(payload_bytes), 1), dtype=torch.uint8, device=streams.streams.device)
    elif payload.dtype != torch.uint8 or payload.numel() < int(payload_bytes):
        raise HipError('`payload` must be uint8 of at least payload_bytes bytes')
    _check(_native.hip().eae_hip_coder_pack_streams(streams.n_maps, _p(streams.streams), streams.stride, _p(streams.bac_bits),
                                                    _p(streams.bypass_bits), _p(offsets), _p(payload), _stream()),
           'eae_hip_coder_pack_streams')
    return payload


def coder_unpack_streams(payload, offsets, bac_bits, bypass_bits, map_size, truncated_unary_length):
    """The inverse: a CoderStreams whose regions hold the bytes of `payload` (bit counts int32 [n_maps], device)."""
    n_maps = bac_bits.numel()
    streams = CoderStreams(n_maps, map_size, truncated_unary_length, payload.device)
    streams.bac_bits.copy_(bac_bits)
    streams.bypass_bits.copy_(bypass_bits)
    _check(_native.hip().eae_hip_coder_unpack_streams(n_maps, _p(payload), _p(offsets), _p(streams.bac_bits), _p(streams.bypass_bits),
                                                      _p(streams.streams), streams.stride, _stream()), 'eae_hip_coder_unpack_streams')
    return streams


def coder_unpack_into(streams, payload, offsets):
    """`coder_unpack_streams` into an existing CoderStreams whose bit counts are already on the device (`offsets` int64 [n_maps, 2])."""
    if payload.dtype != torch.uint8 or offsets.dtype != torch.int64 or offsets.numel() != 2*streams.n_maps:
        raise HipError('`payload` must be uint8 and `offsets` hold 2 n_maps int64 words')
    _check(_native.hip().eae_hip_coder_unpack_streams(streams.n_maps, _p(payload), _p(offsets), _p(streams.bac_bits), _p(streams.bypass_bits),
                                                      _p(streams.streams), streams.stride, _stream(payload)), 'eae_hip_coder_unpack_streams')


def dequantize_maps(symbols_planar, bin_widths, map_mean=None, want_cq=False, want_shifted=True):
    """int16 symbols [N, 128, hw] -> float32 [N, hw, 128]: bw * symbol (and + map_mean), the arrays quantize_maps produced."""
    (n, c, hw) = symbols_planar.shape
    cq = torch.empty((n, hw, c), dtype=torch.float32, device=symbols_planar.device) if want_cq else None
    shifted = torch.empty((n, hw, c), dtype=torch.float32, device=symbols_planar.device) if want_shifted else None
    _check(_native.hip().eae_hip_dequantize_maps(_p(symbols_planar), _p(bin_widths), _p(map_mean), _p(cq), _p(shifted), n, hw, c, _stream(symbols_planar)),
           'eae_hip_dequantize_maps')
    return {'cq': cq, 'shifted': shifted}


# ---- containers from the pipelined codec (include/eae_hip.h, csrc/hip/codec_container.hip) -----------------------------------
# No argument of these five depends on a result of the step, so they can be captured into the coder's hipGraph.

def coder_index_streams(streams, maps_per_image, capacity_bytes, offsets=None, index=None):
    """Byte offsets of every stream piece of `streams` (CoderStreams) in the payload, and the index words, from the bit counts on
    the device: -> (offsets int64 [n_maps, 2], index int64 [2 + n_maps/maps_per_image]: total bytes, 1 when the total exceeds
    `capacity_bytes`, then the bytes of every image). `offsets` / `index`: preallocated outputs. Only the bit counts are read:
    of `streams`, n_maps, stride, bac_bits and bypass_bits are used."""
    n_maps = streams.n_maps
    device = streams.bac_bits.device
    if maps_per_image < 1 or n_maps % maps_per_image != 0:
        raise HipError('`n_maps` is not a multiple of `maps_per_image`')
    if offsets is None:
        offsets = torch.empty((n_maps, 2), dtype=torch.int64, device=device)
    if index is None:
        index = torch.empty(2 + n_maps//maps_per_image, dtype=torch.int64, device=device)
    if offsets.dtype != torch.int64 or offsets.numel() != 2*n_maps or index.dtype != torch.int64 or index.numel() != 2 + n_maps//maps_per_image:
        raise HipError('`offsets` must hold 2 n_maps and `index` 2 + n_maps/maps_per_image int64 words')
    _check(_native.hip().eae_hip_coder_index_streams(n_maps, maps_per_image, _p(streams.bac_bits), _p(streams.bypass_bits),
                                                     int(streams.stride), int(capacity_bytes), _p(offsets),
                                                     _p(index), _stream(streams.bac_bits)), 'eae_hip_coder_index_streams')
    return offsets, index


def coder_index_tiles(bac_bits, bypass_bits, entry_table, maps_per_entry, entries_per_image, capacity_bytes, offsets=None, index=None):
    """`coder_index_streams` for a step coded in coding tiles (include/eae_hip.h: eae_hip_coder_index_tiles). bac_bits / bypass_bits
    int32 [n_streams] in run order (the entries -- (image, tile) pairs of `maps_per_entry` maps -- of one shape class side by side);
    entry_table int64 [n_entries, 2] on the device, one row per entry in payload order: its run-order index and half the stream
    stride of its class. -> (offsets int64 [n_streams, 2] in run order: where every piece lies in the payload, index int64
    [2 + n_entries/entries_per_image]: total bytes, overflow flag, bytes per image)."""
    n_streams = bac_bits.numel()
    if maps_per_entry < 1 or entries_per_image < 1 or n_streams % (maps_per_entry*entries_per_image) != 0:
        raise HipError('`n_streams` is not a multiple of `maps_per_entry*entries_per_image`')
    n_entries = n_streams//maps_per_entry
    if bypass_bits.numel() != n_streams or bac_bits.element_size() != 4 or bypass_bits.element_size() != 4:
        raise HipError('`bac_bits` and `bypass_bits` must hold n_streams 32-bit words each')
    if entry_table.dtype != torch.int64 or entry_table.numel() != 2*n_entries or not entry_table.is_contiguous():
        raise HipError('`entry_table` must be contiguous int64 [n_entries, 2]')
    device = bac_bits.device
    if offsets is None:
        offsets = torch.empty((n_streams, 2), dtype=torch.int64, device=device)
    if index is None:
        index = torch.empty(2 + n_entries//entries_per_image, dtype=torch.int64, device=device)
    if offsets.dtype != torch.int64 or offsets.numel() != 2*n_streams or index.dtype != torch.int64 or index.numel() != 2 + n_entries//entries_per_image:
        raise HipError('`offsets` must hold 2 n_streams and `index` 2 + n_entries/entries_per_image int64 words')
    _check(_native.hip().eae_hip_coder_index_tiles(n_streams, int(maps_per_entry), int(entries_per_image), _p(bac_bits), _p(bypass_bits),
                                                   _p(entry_table), int(capacity_bytes), _p(offsets), _p(index), _stream(bac_bits)),
           'eae_hip_coder_index_tiles')
    return offsets, index


def coder_pack_indexed(streams, offsets, index, payload):
    """`coder_pack_streams` into `payload` (uint8, the capacity `index` was formed against) with the offsets and the overflow flag
    of `coder_index_streams`: nothing is copied when the flag is set."""
    if payload.dtype != torch.uint8 or offsets.numel() != 2*streams.n_maps:
        raise HipError('`payload` must be uint8 and `offsets` hold 2 n_maps words')
    _check(_native.hip().eae_hip_coder_pack_indexed(streams.n_maps, _p(streams.streams), streams.stride, _p(streams.bac_bits),
                                                    _p(streams.bypass_bits), _p(offsets), _p(index), _p(payload), _stream(payload)),
           'eae_hip_coder_pack_indexed')
    return payload


def publish_prefix(src_device, dst_pinned, nbytes_device):
    """Stream-ordered copy, by a kernel, of the first `nbytes_device[0]` bytes (an int64 device word; at most the buffers' size) of
    `src_device` into the pinned host tensor `dst_pinned`, rounded up to 16 bytes; the rest of `dst_pinned` is not written. Both
    uint8, of one size, a multiple of 16."""
    capacity = src_device.numel()*src_device.element_size()
    if not dst_pinned.is_pinned() or dst_pinned.numel()*dst_pinned.element_size() != capacity or not dst_pinned.is_contiguous() or capacity % 16:
        raise HipError('expected a contiguous pinned host tensor of the same size, a multiple of 16 bytes')
    if nbytes_device.numel() != 1 or nbytes_device.element_size() != 8:
        raise HipError('expected one 64-bit word')
    _check(_native.hip().eae_hip_publish_prefix(_p(src_device), dst_pinned.data_ptr(), capacity, _p(nbytes_device), _stream(src_device)),
           'eae_hip_publish_prefix')


def exception_rows(hist, overflow, map_size, truncated_unary_length, out=None):
    """`symbol_histograms` of exception maps (hist int32 [n, 2*radius+1], overflow int32 [n]) -> their probability rows, float64
    [n, L] on the device, bit-equal to container._exception_rows (include/eae_hip.h). Needs radius >= L. `out`: preallocated."""
    (n, width) = hist.shape
    if hist.dtype != torch.int32 or overflow.dtype != torch.int32 or overflow.numel() != n or width % 2 != 1:
        raise HipError('expected int32 histograms [n, 2*radius + 1] and int32 overflow counts [n]')
    if out is None:
        out = torch.empty((n, truncated_unary_length), dtype=torch.float64, device=hist.device)
    if out.dtype != torch.float64 or out.numel() != n*truncated_unary_length:
        raise HipError('`out` must hold n x L float64')
    _check(_native.hip().eae_hip_exception_rows(n, _p(hist), _p(overflow), (width - 1)//2, int(map_size), int(truncated_unary_length),
                                                _p(out), _stream(hist)), 'eae_hip_exception_rows')
    return out


# ---- the pipelined decoder's own launches (include/eae_hip.h, csrc/hip/codec_decode.hip) --------------------------------------

def fetch_prefix(src_pinned, dst_device, nbytes_device):
    """Stream-ordered copy, by a kernel, of the first `nbytes_device[0]` bytes (an int64 device word; at most the buffers' size) of
    the pinned host tensor `src_pinned` into `dst_device`, rounded up to 16 bytes; the rest of `dst_device` is not written. Both
    uint8-sized alike, a multiple of 16 bytes. The mirror of `publish_prefix`."""
    capacity = dst_device.numel()*dst_device.element_size()
    if not src_pinned.is_pinned() or src_pinned.numel()*src_pinned.element_size() != capacity or not src_pinned.is_contiguous() or capacity % 16:
        raise HipError('expected a contiguous pinned host tensor of the same size, a multiple of 16 bytes')
    if nbytes_device.numel() != 1 or nbytes_device.element_size() != 8:
        raise HipError('expected one 64-bit word')
    _check(_native.hip().eae_hip_fetch_prefix(src_pinned.data_ptr(), _p(dst_device), capacity, _p(nbytes_device), _stream(dst_device)),
           'eae_hip_fetch_prefix')


def dequantize_maps_rows(symbols_planar, bin_widths_rows, map_mean_rows=None, want_cq=False, want_shifted=True, out_cq=None, out_shifted=None):
    """`dequantize_maps` with one row of bin widths and means per image: int16 symbols [N, 128, hw], float32 rows [N, 128] ->
    float32 [N, hw, 128], bit-identical to `dequantize_maps` image by image. `out_cq` / `out_shifted`: preallocated outputs."""
    (n, c, hw) = symbols_planar.shape
    device = symbols_planar.device
    if symbols_planar.dtype != torch.int16 or bin_widths_rows.dtype != torch.float32 or bin_widths_rows.numel() != n*c:
        raise HipError('expected int16 symbols [N, 128, hw] and float32 bin widths [N, 128]')
    if map_mean_rows is not None and (map_mean_rows.dtype != torch.float32 or map_mean_rows.numel() != n*c):
        raise HipError('expected float32 means [N, 128]')
    for out in (out_cq, out_shifted):
        if out is not None and (out.dtype != torch.float32 or out.numel() != n*hw*c):
            raise HipError('an output must hold N x hw x 128 float32')
    cq = out_cq if out_cq is not None else (torch.empty((n, hw, c), dtype=torch.float32, device=device) if want_cq else None)
    shifted = out_shifted if out_shifted is not None else (torch.empty((n, hw, c), dtype=torch.float32, device=device) if want_shifted else None)
    _check(_native.hip().eae_hip_dequantize_maps_rows(_p(symbols_planar), _p(bin_widths_rows), _p(map_mean_rows), _p(cq), _p(shifted), n, hw, c,
                                                      _stream(symbols_planar)), 'eae_hip_dequantize_maps_rows')
    return {'cq': cq, 'shifted': shifted}


def publish_crops(planes, origins, dst, crop_h, crop_w):
    """Stream-ordered, by a kernel: the crop_h x crop_w rectangle at `origins[i]` (int32 [N, 2] on the device: row, col; clamped
    into the plane by the kernel) of every plane of `planes` (uint8 [N, H, W], device) into `dst` as [N, crop_h, crop_w], flat: a
    contiguous uint8 tensor, pinned host or device memory, 16-byte aligned, a multiple of 16 bytes and at least N*crop_h*crop_w
    rounded up to 16. Whole 16-byte words are stored; the pad of the last one is zero, nothing behind it is written."""
    if planes.dtype != torch.uint8 or planes.dim() != 3:
        raise HipError('planes must be uint8 [N, H, W]')
    (n, h, w) = planes.shape
    if origins.dtype != torch.int32 or origins.numel() != 2*n:
        raise HipError('origins must hold two int32 words per plane')
    if dst.dtype != torch.uint8 or not dst.is_contiguous() or not (dst.is_cuda or dst.is_pinned()):
        raise HipError('dst must be a contiguous uint8 tensor in device or pinned host memory')
    _check(_native.hip().eae_hip_publish_crops(_p(planes), n, h, w, _p(origins), int(crop_h), int(crop_w), dst.data_ptr(), dst.numel(),
                                               _stream(planes)), 'eae_hip_publish_crops')


# ---- images of any height and width (include/eae_hip.h, csrc/hip/frame.hip) ------------------------------

def coded_size(height, width):
    """The size an image of height x width (any positive integers) is coded at: both sides rounded up to multiples of 16."""
    return (-(-int(height)//16)*16, -(-int(width)//16)*16)


def frame_pad_u8(images, out=None):
    """uint8 [N, h, w], contiguous, in device or pinned host memory -> uint8 [N, H, W] (device) with (H, W) = coded_size(h, w), the
    image extended by edge replication: numpy.pad(x, ((0, 0), (0, H - h), (0, W - w)), mode='edge'). One launch; `out`: the
    preallocated result (a graph's static input)."""
    if images.dtype != torch.uint8 or images.dim() != 3 or not images.is_contiguous() or not (images.is_cuda or images.is_pinned()):
        raise HipError('images must be a contiguous uint8 [N, h, w] tensor in device or pinned host memory')
    (n, h, w) = images.shape
    (coded_h, coded_w) = coded_size(h, w)
    if out is None:
        device = images.device if images.is_cuda else torch.device('cuda', torch.cuda.current_device())
        out = torch.empty((n, coded_h, coded_w), dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, coded_h, coded_w):
        raise HipError('`out` must be uint8 [N, H, W] of the coded size')
    _check(_native.hip().eae_hip_frame_pad_u8(images.data_ptr(), _p(out), n, h, w, coded_h, coded_w, _stream(out)), 'eae_hip_frame_pad_u8')
    return out


def frame_sse_u8(reconstruction, reference, out=None):
    """Squared error per image over the real pixels: reconstruction uint8 [N, H, W] at the coded size, reference uint8 [N, h, w] ->
    int64 [N], sum over y < h, x < w of (reference - reconstruction)^2. `out`: int64 [N] to ADD into (the caller zeroes it)."""
    if reconstruction.dtype != torch.uint8 or reference.dtype != torch.uint8 or reconstruction.dim() != 3 or reference.dim() != 3:
        raise HipError('expected uint8 [N, H, W] and uint8 [N, h, w]')
    (n, h, w) = reference.shape
    if tuple(reconstruction.shape) != (n,) + coded_size(h, w):
        raise HipError('the reconstruction does not have the coded size of the reference')
    if out is None:
        out = torch.zeros(n, dtype=torch.int64, device=reconstruction.device)
    if out.dtype != torch.int64 or out.numel() != n:
        raise HipError('`out` must hold one int64 per image')
    _check(_native.hip().eae_hip_frame_sse_u8(_p(reconstruction), _p(reference), _p(out), n, h, w, reconstruction.shape[1],
                                              reconstruction.shape[2], _stream(reconstruction)), 'eae_hip_frame_sse_u8')
    return out


# ---- colour images, 4:2:0 (include/eae_hip.h, csrc/hip/colour.hip; colour.py states both in numpy) --------

def chroma_size(height, width):
    """The size of the Cb and Cr planes of a height x width picture: both sides halved, rounded up."""
    return ((int(height) + 1)//2, (int(width) + 1)//2)


def _colour_device(*tensors):
    for t in tensors:
        if t is not None and t.is_cuda:
            return t.device
    return torch.device('cuda', torch.cuda.current_device())


def colour_split_420(rgb, out=None):
    """uint8 [N, h, w, 3], contiguous, in device or pinned host memory -> (y [N, h, w], cb [N, hc, wc], cr [N, hc, wc]), uint8 on the
    device, (hc, wc) = chroma_size(h, w): `colour.split_420_numpy`, bit for bit. One launch; `out`: the three preallocated planes."""
    if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[3] != 3 or not rgb.is_contiguous() or not (rgb.is_cuda or rgb.is_pinned()):
        raise HipError('rgb must be a contiguous uint8 [N, h, w, 3] tensor in device or pinned host memory')
    (n, h, w, _) = rgb.shape
    (hc, wc) = chroma_size(h, w)
    if out is None:
        device = _colour_device(rgb)
        out = (torch.empty((n, h, w), dtype=torch.uint8, device=device), torch.empty((n, hc, wc), dtype=torch.uint8, device=device),
               torch.empty((n, hc, wc), dtype=torch.uint8, device=device))
    (y, cb, cr) = out
    if any(t.dtype != torch.uint8 for t in out) or tuple(y.shape) != (n, h, w) or tuple(cb.shape) != (n, hc, wc) or tuple(cr.shape) != (n, hc, wc):
        raise HipError('`out` must be uint8 (y [N, h, w], cb [N, hc, wc], cr [N, hc, wc])')
    _check(_native.hip().eae_hip_colour_split_420(rgb.data_ptr(), _p(y), _p(cb), _p(cr), n, h, w, _stream(y)), 'eae_hip_colour_split_420')
    return (y, cb, cr)


def _plane_pitch(t):
    """(rows, columns) of the contiguous [N, rows, columns] planes `t` is, or is the top-left view of (what `BatchCodec(pad=True)`
    hands out as a reconstruction: `planes[:, :h, :w]`)."""
    (image, row, column) = t.stride()
    if column != 1 or row < t.shape[2] or image % row != 0 or image//row < t.shape[1]:
        raise HipError('expected contiguous planes [N, rows, columns] or their top-left view [:, :h, :w]')
    return (image//row, row)


def colour_merge_420(y, cb, cr, size, out=None, reference=None, sse=None):
    """Planes -> RGB: `colour.merge_420_numpy` of the top-left h x w of y and hc x wc of cb and cr, bit for bit, with size = (h, w).
    y uint8 [N, H, W], cb and cr uint8 [N, Hc, Wc], on the device, H >= h, W >= w, Hc >= hc, Wc >= wc: dense planes, or the coded
    planes a codec keeps (contiguous, or their top-left view), whose padding is never read. Returns (rgb, sse):
    rgb uint8 [N, h, w, 3] on the device; `out`: a preallocated one, in device or pinned host memory; out=False: no picture is written
    (then `reference` is needed) and rgb is None.
    reference: uint8 [N, h, w, 3] on the device: sse int64 [N] receives the squared error per image over its 3 h w samples; `sse`: int64
    [N] on the device to ADD into (the caller zeroes it). Without a reference sse is None. One launch."""
    planes = (y, cb, cr)
    if any(t.dtype != torch.uint8 or t.dim() != 3 or not t.is_cuda for t in planes):
        raise HipError('y, cb and cr must be uint8 [N, rows, columns] tensors on the device')
    (h, w) = (int(size[0]), int(size[1]))
    (hc, wc) = chroma_size(h, w)
    n = y.shape[0]
    (coded_h, coded_w) = _plane_pitch(y)
    (chroma_h, chroma_w) = _plane_pitch(cb)
    if h < 1 or w < 1 or y.shape[1] < h or y.shape[2] < w or cb.shape[1] < hc or cb.shape[2] < wc or cb.shape[0] != n or cr.shape != cb.shape \
            or _plane_pitch(cr) != (chroma_h, chroma_w):
        raise HipError('the planes do not hold {0} x {1} pictures: y [N, >= h, >= w], cb and cr alike [N, >= hc, >= wc]'.format(h, w))
    if out is False:
        out = None
        if reference is None:
            raise HipError('neither a picture nor a squared error was asked for')
    else:
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=y.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or not out.is_contiguous() or not (out.is_cuda or out.is_pinned()):
            raise HipError('`out` must be a contiguous uint8 [N, h, w, 3] tensor in device or pinned host memory')
    if reference is None:
        if sse is not None:
            raise HipError('`sse` comes with a `reference`')
    else:
        if reference.dtype != torch.uint8 or tuple(reference.shape) != (n, h, w, 3) or not reference.is_cuda:
            raise HipError('`reference` must be a uint8 [N, h, w, 3] tensor on the device')
        if sse is None:
            sse = torch.zeros(n, dtype=torch.int64, device=y.device)
        if sse.dtype != torch.int64 or sse.numel() != n:
            raise HipError('`sse` must hold one int64 per image')
    _check(_native.hip().eae_hip_colour_merge_420(y.data_ptr(), cb.data_ptr(), cr.data_ptr(), None if out is None else out.data_ptr(), _p(reference), _p(sse), n, h, w,
                                                  coded_h, coded_w, chroma_h, chroma_w, _stream(y)), 'eae_hip_colour_merge_420')
    return (out, sse)


def colour_words_bytes(nb_images, height, width):
    """The bytes `colour_merge_420_words` needs of its `out` for that many pictures: 3 h w each, rounded up to whole 16-byte words."""
    return -(-int(nb_images)*int(height)*int(width)*3//16)*16


def colour_merge_420_words(y, cb, cr, size, out):
    """`colour_merge_420`'s picture of the same planes (same checks, same top-left rule), written in whole aligned 16-byte words
    (DESIGN.md section 27): `out` is a contiguous uint8 tensor in device or pinned host memory, 16-byte aligned, flat or [N, h, w, 3]
    over a buffer of a multiple of 16 bytes that is at least `colour_words_bytes(N, h, w)` (the bytes of the tensor itself, or, for
    a view, of its storage behind its first byte). The first N h w 3 bytes are the pictures, the pad of the last word is zero and
    nothing behind that word is written. One launch. Returns `out`."""
    planes = (y, cb, cr)
    if any(t.dtype != torch.uint8 or t.dim() != 3 or not t.is_cuda for t in planes):
        raise HipError('y, cb and cr must be uint8 [N, rows, columns] tensors on the device')
    (h, w) = (int(size[0]), int(size[1]))
    (hc, wc) = chroma_size(h, w)
    n = y.shape[0]
    (coded_h, coded_w) = _plane_pitch(y)
    (chroma_h, chroma_w) = _plane_pitch(cb)
    if h < 1 or w < 1 or y.shape[1] < h or y.shape[2] < w or cb.shape[1] < hc or cb.shape[2] < wc or cb.shape[0] != n or cr.shape != cb.shape \
            or _plane_pitch(cr) != (chroma_h, chroma_w):
        raise HipError('the planes do not hold {0} x {1} pictures: y [N, >= h, >= w], cb and cr alike [N, >= hc, >= wc]'.format(h, w))
    if out.dtype != torch.uint8 or not out.is_contiguous() or not (out.is_cuda or out.is_pinned()) \
            or (out.dim() != 1 and tuple(out.shape) != (n, h, w, 3)):
        raise HipError('`out` must be a contiguous uint8 tensor, flat or [N, h, w, 3], in device or pinned host memory')
    # the bytes the launch may write: the tensor's own, or, for a [N, h, w, 3] view of a longer buffer, what its storage holds behind it
    room = out.numel()
    if out.dim() != 1:
        room = out.untyped_storage().nbytes() - out.storage_offset()
        room -= room % 16
    _check(_native.hip().eae_hip_colour_merge_420_words(y.data_ptr(), cb.data_ptr(), cr.data_ptr(), out.data_ptr(), room, n, h, w,
                                                        coded_h, coded_w, chroma_h, chroma_w, _stream(y)), 'eae_hip_colour_merge_420_words')
    return out


def chroma_region_size(size, region):
    """(rch, rcw): the size of the chroma rectangle `colour.chroma_region` gives a crop of region = (rh, rw) pixels out of a picture
    of size = (h, w), wherever the crop lies: half the region and three samples, at most the chroma plane."""
    (hc, wc) = chroma_size(*size)
    return (min(hc, int(region[0])//2 + 3), min(wc, int(region[1])//2 + 3))


def colour_merge_420_crops(y, cb, cr, image_size, origins, out):
    """Crops of planes -> crops of RGB pictures: `colour.merge_420_region_numpy`, bit for bit. y uint8
    [N, rh, rw], cb and cr uint8 [N, rch, rcw] with (rch, rcw) = `chroma_region_size(image_size, (rh, rw))`, contiguous, on the
    device: crop k the pixels at origins[k] = (y0, x0) of a picture of image_size = (h, w), its chroma crops the rectangle
    `colour.chroma_region` names, whose origin the kernel derives itself. origins: int32 [N, 2], contiguous, on the device or in pinned
    host memory; the kernel reads it, so a launch's arguments do not depend on the placement. Every crop must lie inside the picture
    (0 <= y0 <= h - rh, 0 <= x0 <= w - rw): the caller's to ensure, nothing here reads `origins`.
    `out` as `colour_merge_420_words`': a contiguous uint8 tensor in device or pinned host memory, 16-byte aligned, flat or
    [N, rh, rw, 3] over a buffer of a multiple of 16 bytes that is at least `colour_words_bytes(N, rh, rw)`; the first N rh rw 3
    bytes are the crops, the pad of the last word is zero and nothing behind that word is written. One launch. Returns `out`."""
    planes = (y, cb, cr)
    if any(t.dtype != torch.uint8 or t.dim() != 3 or not t.is_cuda or not t.is_contiguous() for t in planes):
        raise HipError('y, cb and cr must be contiguous uint8 [N, rows, columns] tensors on the device')
    (h, w) = (int(image_size[0]), int(image_size[1]))
    (n, rh, rw) = y.shape
    if h < 1 or w < 1 or n < 1 or not (1 <= rh <= h and 1 <= rw <= w):
        raise HipError('the crops [N, {0}, {1}] are empty or larger than the {2} x {3} picture'.format(rh, rw, h, w))
    (rch, rcw) = chroma_region_size((h, w), (rh, rw))
    if tuple(cb.shape) != (n, rch, rcw) or cr.shape != cb.shape:
        raise HipError('cb and cr must be [N, {0}, {1}]: the chroma rectangle of a {2} x {3} crop of a {4} x {5} picture'.format(
            rch, rcw, rh, rw, h, w))
    if origins.dtype != torch.int32 or tuple(origins.shape) != (n, 2) or not origins.is_contiguous() or not (origins.is_cuda or origins.is_pinned()):
        raise HipError('origins must be a contiguous int32 [N, 2] tensor in device or pinned host memory')
    if out.dtype != torch.uint8 or not out.is_contiguous() or not (out.is_cuda or out.is_pinned()) \
            or (out.dim() != 1 and tuple(out.shape) != (n, rh, rw, 3)):
        raise HipError('`out` must be a contiguous uint8 tensor, flat or [N, rh, rw, 3], in device or pinned host memory')
    room = out.numel()
    if out.dim() != 1:
        room = out.untyped_storage().nbytes() - out.storage_offset()
        room -= room % 16
    _check(_native.hip().eae_hip_colour_merge_420_crops(y.data_ptr(), cb.data_ptr(), cr.data_ptr(), origins.data_ptr(), out.data_ptr(), room,
                                                        n, h, w, rh, rw, rch, rcw, _stream(y)), 'eae_hip_colour_merge_420_crops')
    return out


def colour_budget_rest(budgets, upper_cb, point_cb, upper_cr, point_cr, out):
    """The byte budget of the luminance plane of N colour pictures from what their chroma planes took:
    `ratecontrol.colour_luma_budgets`, element for element, without a visit to the host. budgets int64 [N]: the budget of every
    picture's single-picture EAC1 blob; upper_cb, upper_cr int64 [N, K]: the upper bounds of the chroma planes at every point (byte
    counts, never negative); point_cb, point_cr int32 [N]: the points they took; out int64 [N]. All contiguous, in device or pinned
    host memory. out[i] = max(P - upper_cb[i, point_cb[i]] - upper_cr[i, point_cr[i]], 0) with P = max(budgets[i] - 48, 0), the 48
    `container`'s colour header; a picture with a point outside [0, K) gets 0. One launch on the current stream. Returns `out`."""
    from . import container                       # (it imports this module; both are loaded by the time anything is called)
    wide = (budgets, upper_cb, upper_cr, out)
    points = (point_cb, point_cr)
    if any(t.dtype != torch.int64 for t in wide) or any(t.dtype != torch.int32 for t in points):
        raise HipError('budgets, upper_cb, upper_cr and out must be int64, point_cb and point_cr int32')
    if any(not t.is_contiguous() or not (t.is_cuda or t.is_pinned()) for t in wide + points):
        raise HipError('every argument must be contiguous, in device or pinned host memory')
    if upper_cb.dim() != 2 or upper_cb.shape[0] < 1 or upper_cb.shape[1] < 1 or upper_cr.shape != upper_cb.shape:
        raise HipError('upper_cb and upper_cr must be alike [N, K] with N, K >= 1')
    (n, k_points) = upper_cb.shape
    if any(tuple(t.shape) != (n,) for t in (budgets, point_cb, point_cr, out)):
        raise HipError('budgets, point_cb, point_cr and out must be [N]')
    _check(_native.hip().eae_hip_colour_budget_rest(budgets.data_ptr(), upper_cb.data_ptr(), point_cb.data_ptr(), upper_cr.data_ptr(),
                                                    point_cr.data_ptr(), out.data_ptr(), n, k_points, container.COLOUR_HEADER_BYTES,
                                                    _stream(next((t for t in wide + points if t.is_cuda), None))), 'eae_hip_colour_budget_rest')
    return out


def colour_quality_rest(max_sse, sse_cb, sse_cr, out):
    """The squared-error threshold of the luminance plane of N colour pictures from what their chroma planes spent (DESIGN.md section
    30): `ratecontrol.colour_luma_max_sse`, element for element, without a visit to the host. max_sse int64 [N]: the threshold of
    every picture over all samples of its 4:2:0 form, up to 2^62; sse_cb, sse_cr int64 [N]: the squared errors of the points the
    chroma planes took, never negative; out int64 [N]. All contiguous, in device or pinned host memory. out[i] = max(max_sse[i] -
    sse_cb[i] - sse_cr[i], 0). One launch on the current stream. Returns `out`."""
    every = (max_sse, sse_cb, sse_cr, out)
    if any(t.dtype != torch.int64 for t in every):
        raise HipError('max_sse, sse_cb, sse_cr and out must be int64')
    if any(not t.is_contiguous() or not (t.is_cuda or t.is_pinned()) for t in every):
        raise HipError('every argument must be contiguous, in device or pinned host memory')
    if max_sse.dim() != 1 or max_sse.shape[0] < 1 or any(t.shape != max_sse.shape for t in every):
        raise HipError('max_sse, sse_cb, sse_cr and out must be alike [N] with N >= 1')
    _check(_native.hip().eae_hip_colour_quality_rest(max_sse.data_ptr(), sse_cb.data_ptr(), sse_cr.data_ptr(), out.data_ptr(), max_sse.shape[0],
                                                     _stream(next((t for t in every if t.is_cuda), None))), 'eae_hip_colour_quality_rest')
    return out


# ---- SVHN float64 path (include/eae_hip.h, "SVHN path") -------------------------------------------------------------

def svhn_dense(x, w, b, leaky_relu):
    """act(x . w + b) in float64; x [n,k], w [k,m], b [m] or [1,m]."""
    (n, k) = x.shape
    m = w.shape[1]
    out = torch.empty((n, m), dtype=torch.float64, device=x.device)
    _check(_native.hip().eae_hip_svhn_dense_f64(_p(x), _p(w), _p(b), _p(out), n, k, m, 1 if leaky_relu else 0, _stream()),
           'eae_hip_svhn_dense_f64')
    return out


def svhn_preprocess(images_u8, mean, std_training):
    (n, d) = images_u8.shape
    out = torch.empty((n, d), dtype=torch.float64, device=images_u8.device)
    _check(_native.hip().eae_hip_svhn_preprocess(_p(images_u8), _p(mean), float(std_training), _p(out), n, d, _stream()),
           'eae_hip_svhn_preprocess')
    return out


def svhn_quantize(y, bin_width, want_q=True, want_symbols=False):
    q = torch.empty_like(y) if want_q else None
    symbols = torch.empty(y.shape, dtype=torch.int32, device=y.device) if want_symbols else None
    checks = torch.zeros(2, dtype=torch.int32, device=y.device)
    _check(_native.hip().eae_hip_svhn_quantize_f64(_p(y), float(bin_width), _p(q), _p(symbols), _p(checks), y.numel(), _stream()),
           'eae_hip_svhn_quantize_f64')
    return q, symbols, checks


def svhn_symbol_histogram(symbols):
    """Exact histogram of int32 symbols from their minimum to their maximum: (hist int64 numpy, minimum)."""
    minmax = torch.tensor([2147483647, -2147483648], dtype=torch.int32, device=symbols.device)
    _check(_native.hip().eae_hip_svhn_symbol_range(_p(symbols), symbols.numel(), _p(minmax), _stream()), 'eae_hip_svhn_symbol_range')
    (lo, hi) = minmax.cpu().tolist()
    nb = hi - lo + 1
    hist = torch.zeros(nb, dtype=torch.int32, device=symbols.device)
    overflow = torch.zeros(1, dtype=torch.int32, device=symbols.device)
    _check(_native.hip().eae_hip_svhn_symbol_histogram(_p(symbols), symbols.numel(), lo, nb, _p(hist), _p(overflow), _stream()),
           'eae_hip_svhn_symbol_histogram')
    if int(overflow.item()) != 0:
        raise HipError('symbol outside [min, max]')
    return hist.cpu().numpy().astype('int64'), lo


def svhn_postprocess(reconstruction, std_training, mean, ref_u8=None):
    (n, d) = reconstruction.shape
    out = torch.empty((n, d), dtype=torch.uint8, device=reconstruction.device)
    sse = torch.zeros(n, dtype=torch.int64, device=reconstruction.device) if ref_u8 is not None else None
    _check(_native.hip().eae_hip_svhn_postprocess(_p(reconstruction), float(std_training), _p(mean), _p(out), _p(ref_u8), _p(sse),
                                                  n, d, _stream()), 'eae_hip_svhn_postprocess')
    return out, sse
