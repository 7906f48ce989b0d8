"""A self-describing container for the coded latent variables and a standalone decoder.

The reference never serialises: `compress_lossless` (kodak_tensorflow/lossless/c++/source/compression.cpp:27-64) builds
the two bitstreams of a map, counts their bits, decodes them again and throws them away, and the decoder side of
`fix_gamma` (reconstructing_eae_kodak.py:192-207) restarts from the float array the encoder side still holds. Here the
streams produced by the device coder are packed into one blob that carries everything but the network weights, and
`decode_images` rebuilds the images from the blob alone: unpack -> arithmetic decode -> symbol * bin width + map mean
(the inverse of lossless/compression.py:142 and reconstructing_eae_kodak.py:178) -> synthesis transform -> BT.601 cast.
The reconstruction is bit-identical to the in-memory path's (tests/test_container.py).

Layout (little endian):
    magic 'EAE1' | version u16 | flags u16 (bit 0: learned bin widths) | nb_images u32 | height u32 | width u32 |
    nb_maps u16 | L u8 | crop u8 | idx_map_exception i32
    bin_widths f32[nb_maps] | map_mean f32[nb_maps] | binary_probabilities f64[nb_maps][L]
    exception_probabilities f64[nb_images][L]              (only when idx_map_exception >= 0)
    bit counts u32[nb_images * nb_maps][2]                 (arithmetic-coded stream, bypass stream)
    payload: for every image, every map: arithmetic-coded bytes, then bypass bytes (each rounded up to a byte)

The exception map. The reference does not code it: it charges ceil(h*w*entropy) bits for it (compression.py:68-75), the
cost of an ideal adaptive coder. A decodable file has to carry it, so it goes through the same UEG0 + arithmetic coder
with a probability row measured on that very map (stats.py:181-195 applied to its histogram), stored per image.

The tile-indexed format EAT1 (`encode_images(..., coding_tile=(th, tw))`). The latent plane of every
map is cut into a plain grid of coding tiles of th x tw latents (edge tiles smaller; `coding_tile_grid`), and every (image,
tile, map) is coded as its own pair of streams, the symbols of the tile in raster order. The probabilities are static, so a
tile's stream costs its share of the whole map's bits plus its own termination and byte padding. The exception map keeps one
probability row per image, measured on the whole map. Layout (little endian):
    magic 'EAT1' | version u16 (= 1) | flags u16 | nb_images u32 | height u32 | width u32 | nb_maps u16 | L u8 | crop u8 |
    idx_map_exception i32 | coding_tile_h u16 | coding_tile_w u16                       (tile sides in latents)
    bin_widths f32[nb_maps] | map_mean f32[nb_maps] | binary_probabilities f64[nb_maps][L]
    exception_probabilities f64[nb_images][L]              (only when idx_map_exception >= 0)
    bit counts u32[nb_images][nb_tiles][nb_maps][2]        (arithmetic-coded stream, bypass stream)
    payload: for every image, every tile (row-major), every map: arithmetic-coded bytes, then bypass bytes (each rounded up
    to a byte)
The streams of one (image, tile) are contiguous, so a region of the image needs one byte range per (image, tile) it touches
(`region_plan`), and `decode_region` reads only those from a file. With one tile per map the payload is EAE1's, byte for byte.

One path serves both formats: EAE1 is the case coding tile = (h, w), one tile per map. `_fixed_header` checks the fixed part of
either magic and `_read_arrays` reads what follows (`read_header`, `fetch_region`); `_pack_header` writes it; `_encode_entries` codes
and `_decode_entries` decodes groups of (image, tile) entries. An EAE1 blob is one group of whole maps, coded where the quantiser
left the symbols.

Images of any height and width. The transforms take sides that are multiples of 16, so an h x w image is
coded at (H, W) = (h, w) rounded up to multiples of 16. `height` / `width` of both headers are that CODED size: latent planes, tile
grids, header length, capacities and byte ranges all derive from them as before. Byte 23 of both fixed headers, `crop`, holds what a
decoder cuts off: (H - h) << 4 | (W - w), two nibbles 0..15 (any value is valid: H, W >= 16). It was a reserved byte, written as 0
and never read: crop == 0 is that blob, byte for byte, and there is no new version. `read_header` gives the real size as
'image_height' / 'image_width'. How the encoder fills the H x W plane outside the image is its own business -- `encode_images(...,
pad=True)` replicates the last row and column (device.frame_pad_u8) -- since a decoder only crops: `decode_images` returns h x w,
and the regions of `decode_region` / `fetch_region` / `region_plan` are in real-image coordinates, inside h x w.

Colour pictures: EAC1 wraps the blobs of the three planes of 4:2:0 pictures (colour.py: Y at h x w, Cb and Cr
at ceil(h/2) x ceil(w/2)), little endian like the others:
    magic 'EAC1' | version u16 (= 1) | flags u16 (= 0) | nb_images u32 | image_height u32 | image_width u32 |
    subsampling u8 (= 1: 4:2:0; every other value is reserved and refused) | reserved u8[3] (= 0) | plane_bytes u64[3]    (48 bytes)
    Y blob | Cb blob | Cr blob
Each plane blob is byte for byte what `encode_images(plane, ..., pad=True)` writes -- EAE1 or EAT1 with its own `crop` byte, rate
point and tables --, so every decoder above reads a plane of a colour file unchanged (`split_colour_blob`). `read_header` and
`decode_images` raise on an EAC1 blob as on any unknown magic: `read_colour_header`, `decode_colour_images` read it.
"""
import math
import numbers
import struct

import numpy
import torch

from . import colour as colour_rules
from . import device as dev
from . import pipeline
from .kodak.eae.graph import constants as csts
from .kodak.lossless import interface_cython
from .kodak.lossless import stats as lossless_stats
from .kodak.tools import tools as tls

MAGIC = b'EAE1'
VERSION = 1
_HEADER = struct.Struct('<4sHHIIIHBBi')
TILE_MAGIC = b'EAT1'
TILE_VERSION = 1
_TILE_HEADER = struct.Struct('<4sHHIIIHBBiHH')
TILES_PER_CALL = 64            # (image, tile) entries the coder takes per group by default: bounds its streams and workspace


def _exception_rows(symbols_planar, idx_map_exception, truncated_unary_length):
    """One probability row per image for its exception map, from the map's own histogram (stats.py:181-195, :56-66)."""
    nb_images = symbols_planar.shape[0]
    (hist, radius) = tls._symbol_histograms(symbols_planar[:, idx_map_exception:idx_map_exception + 1].contiguous())
    rows = numpy.zeros((nb_images, truncated_unary_length), dtype=numpy.float64)
    for i in range(nb_images):
        hist_abs = hist[i, radius:].copy()
        hist_abs[1:] += hist[i, :radius][::-1]
        (zeros, ones) = lossless_stats._decisions_from_hist(hist_abs, truncated_unary_length)
        total = (zeros + ones).astype(numpy.float64)
        with numpy.errstate(invalid='ignore', divide='ignore'):
            p = zeros.astype(numpy.float64)/total
        p[numpy.isnan(p)] = 0.5
        p[p == 0.] = 0.01
        p[p == 1.] = 0.99
        rows[i] = p
    return rows


def stream_capacity_bits(map_size, truncated_unary_length):
    """Bits a stream of the coder can hold at most: map_size * max(32, L) rounded up to a byte, the reference's own capacity
    (compression.cpp:24, Bitstream.cpp:3-11); the coder writes into a region of at least that many bytes + 16 per stream
    (eae_hip_coder_stream_stride_bytes / 2). Pure arithmetic -- the header check does not need the GPU library."""
    return (map_size*max(32, truncated_unary_length) + 7)//8*8


def _raise_for_statuses(results):
    bad = numpy.flatnonzero(results[2])
    if bad.size:
        interface_cython.raise_for_status(int(results[2, bad[0]]), int(results[3, bad[0]]))


def _fields(are_bin_widths_learned, nb_images, height, width, idx_map_exception, bin_widths, map_mean, binary_probabilities,
            exception_rows, coding_tile=None, image_size=None):
    """The header of a blob to write, under `read_header`'s keys (no 'bits', no 'payload_offset'); EAT1 with a coding tile.
    height, width: the coded size; image_size: None, or the real (h, w) it is the coded size of (module docstring: `crop`)."""
    (image_height, image_width) = (height, width) if image_size is None else _image_size(image_size, height, width)
    fields = {'nb_images': nb_images, 'height': height, 'width': width, 'image_height': image_height, 'image_width': image_width,
              'nb_maps': binary_probabilities.shape[0],
              'truncated_unary_length': binary_probabilities.shape[1], 'idx_map_exception': idx_map_exception,
              'are_bin_widths_learned': bool(are_bin_widths_learned), 'bin_widths': bin_widths, 'map_mean': map_mean,
              'binary_probabilities': binary_probabilities, 'exception_probabilities': exception_rows}
    if coding_tile is not None:
        fields.update({'format': 'EAT1', 'coding_tile': coding_tile})
    return fields


def coded_size(height, width):
    """The size an image of height x width is coded at: both sides rounded up to multiples of 16 (module docstring)."""
    return dev.coded_size(height, width)


def _image_size(image_size, height, width):
    """A real size (h, w) to write into a header of coded size height x width."""
    image_size = _positive_pair(image_size, '`image_size`')
    if coded_size(*image_size) != (height, width):
        raise ValueError('{} x {} is not the coded size of a {} x {} image.'.format(height, width, *image_size))
    return image_size


def _pack_header(fields, bits):
    """Everything in front of the payload (module docstring), as bytes: what `read_header` parses. bits uint32, in payload order."""
    crop = (fields['height'] - fields['image_height']) << 4 | (fields['width'] - fields['image_width'])
    common = (1 if fields['are_bin_widths_learned'] else 0, fields['nb_images'], fields['height'], fields['width'], fields['nb_maps'],
              fields['truncated_unary_length'], crop, fields['idx_map_exception'])
    if fields.get('format') == 'EAT1':
        head = _TILE_HEADER.pack(TILE_MAGIC, TILE_VERSION, *(common + tuple(fields['coding_tile'])))
    else:
        head = _HEADER.pack(MAGIC, VERSION, *common)
    return b''.join([head, fields['bin_widths'].tobytes(), fields['map_mean'].tobytes(), fields['binary_probabilities'].tobytes(),
                     fields['exception_probabilities'].tobytes(), bits.tobytes()])


def _clamped_coding_tile(coding_tile, height, width):
    """A coding tile to write: a pair of positive integers, clamped to the latent plane of a height x width image; its sides must fit
    the header's 16 bits."""
    coding_tile = _positive_pair(coding_tile, '`coding_tile`')
    coding_tile = (min(coding_tile[0], height//csts.STRIDE_PROD), min(coding_tile[1], width//csts.STRIDE_PROD))
    if max(coding_tile) > 0xFFFF:
        raise ValueError('A coding tile side does not fit the container (65535 latents at most).')
    return coding_tile


def assemble_blob(are_bin_widths_learned, nb_images, height, width, idx_map_exception, bin_widths, map_mean, binary_probabilities,
                  exception_rows, bits, payload, coding_tile=None, image_size=None):
    """The EAE1 blob (module docstring) from its parts -> (blob bytes, header bytes). bin_widths / map_mean float32 [nb_maps],
    binary_probabilities float64 [nb_maps, L], exception_rows float64 [nb_images, L] ([0, L] without an exception map), bits
    uint32 [nb_images*nb_maps, 2], payload bytes-like. What a `codec.Ticket` builds its containers with from the pinned blocks of
    its step; `encode_images` packs the same header.
    coding_tile=(th, tw) latents (clamped to the latent plane as `encode_images` clamps it): the EAT1 blob instead; bits uint32
    [nb_images*nb_tiles*nb_maps, 2] in payload order (image -> tile, row-major -> map).
    height, width: the CODED size; image_size=(h, w): the real size it is the coded size of, written as the header's `crop` byte
    (None: the coded size, crop 0)."""
    (nb_maps, truncated_unary_length) = binary_probabilities.shape
    nb_rows = nb_images if idx_map_exception >= 0 else 0
    nb_tiles = 1
    if coding_tile is not None:
        coding_tile = _clamped_coding_tile(coding_tile, height, width)
        nb_tiles = _nb_tiles(height//csts.STRIDE_PROD, width//csts.STRIDE_PROD, coding_tile)
    if bin_widths.dtype != numpy.float32 or map_mean.dtype != numpy.float32 or bin_widths.shape != (nb_maps,) or map_mean.shape != (nb_maps,):
        raise ValueError('`bin_widths` and `map_mean` must be float32 with one element per map.')
    if binary_probabilities.dtype != numpy.float64 or exception_rows.dtype != numpy.float64 or bits.dtype != numpy.uint32:
        raise ValueError('The probabilities must be float64 and the bit counts uint32.')
    if exception_rows.shape != (nb_rows, truncated_unary_length) or bits.shape != (nb_images*nb_tiles*nb_maps, 2):
        raise ValueError('The exception rows or the bit counts do not have the shape the header announces.')
    if len(payload) != int(_entry_bytes(bits.reshape(nb_images*nb_tiles, nb_maps, 2)).sum()):
        raise ValueError('The payload size does not match the bit counts.')
    header = _pack_header(_fields(are_bin_widths_learned, nb_images, height, width, idx_map_exception, bin_widths, map_mean,
                                  binary_probabilities, exception_rows, coding_tile, image_size), bits)
    return (header + bytes(payload), len(header))


def assemble_image_blobs(are_bin_widths_learned, nb_images, height, width, idx_map_exception, bin_widths, map_mean, binary_probabilities,
                         exception_rows, bits, payload, coding_tile=None, image_size=None):
    """The parts of a batch's blob (`assemble_blob`) -> one single-image blob per image: the payload is image-major, so an image's
    blob is its slice of the bit counts, of the exception rows and of the payload behind a header of its own."""
    nb_maps = binary_probabilities.shape[0]
    per_image = bits.shape[0]//nb_images          # nb_maps, times the tiles of an image with a coding tile (`assemble_blob` checks it)
    image_bytes = _entry_bytes(bits.reshape(nb_images, per_image//nb_maps, nb_maps, 2)).sum(axis=1)
    stops = numpy.cumsum(image_bytes)
    view = memoryview(payload)
    blobs = []
    for i in range(nb_images):
        rows = exception_rows[i:i + 1] if idx_map_exception >= 0 else exception_rows
        blobs.append(assemble_blob(are_bin_widths_learned, 1, height, width, idx_map_exception, bin_widths, map_mean, binary_probabilities,
                                   rows, bits[i*per_image:(i + 1)*per_image], view[int(stops[i] - image_bytes[i]):int(stops[i])],
                                   coding_tile, image_size)[0])
    return blobs


def encode_images(luminances_uint8, encoder, bin_widths_test, map_mean, binary_probabilities, idx_map_exception=-1, tile=None,
                  coding_tile=None, tiles_per_call=TILES_PER_CALL, rdo_lambda=None, pad=False):
    """uint8 (N, H, W) or (N, H, W, 1) luminance images -> (blob bytes, info dict).

    encoder: pipeline.DeviceEncoder of the model; bin_widths_test float32 (128,) (the trained bin widths times the
    multiplier of the rate point); map_mean float32 (128,); binary_probabilities float64 (128, L) (stats.py:13-68).
    info: 'nb_bits' uint32 (N, 128) (arithmetic-coded + bypass bits of every map), 'payload_bytes', 'header_bytes'.
    tile=(th, tw): run the analysis transform through windows (pipeline.DeviceEncoder.__call__): the latents, hence the blob
    bytes, are those of tile=None, and images beyond the untiled path's size limit can be written.
    coding_tile=(th, tw) latents: write the tile-indexed format EAT1 (module docstring) instead of EAE1. The coder runs on groups
    of `tiles_per_call` (image, tile) pairs, so its streams and workspace are bounded by one group whatever the image size.
    info then also holds 'tile_bits' uint32 (N, nb_tiles, 128, 2). EAE1 is one tile per map, coded as one group.
    rdo_lambda: None, or a non-negative float in squared latent units per bit: the symbols are chosen by the rate-distortion
    optimised quantiser (device.latent_quantize_rdo with ratecontrol.rdo_thresholds of this rate point)
    instead of by nearest rounding. The blob is an ordinary one, every decoder reads it; the exception map's row is measured on the
    symbols chosen. 0.0 gives the bytes of None.
    pad=True: images of any height and width (N, h, w). They are extended on the device to the coded size (module docstring) by
    edge replication (device.frame_pad_u8) in front of the encoder, so everything above works unchanged behind it, and the real
    size goes into the header's `crop` byte: the blob is that of the numpy-edge-padded images but for byte 23, and `decode_images`
    returns (N, h, w). With sides that are multiples of 16 already the bytes are those of pad=False. Without `pad` such sizes go
    on raising.
    """
    images = numpy.ascontiguousarray(luminances_uint8)
    if images.dtype != numpy.uint8:
        raise TypeError('`luminances_uint8.dtype` is not equal to `numpy.uint8`.')
    if images.ndim == 4:
        images = images[:, :, :, 0]
    (nb_images, height, width) = images.shape
    probabilities = numpy.ascontiguousarray(binary_probabilities, dtype=numpy.float64)
    (nb_maps, truncated_unary_length) = probabilities.shape
    if truncated_unary_length < 1 or truncated_unary_length > 255:
        raise ValueError('The truncated unary length does not belong to [1, 255].')
    bin_widths = numpy.ascontiguousarray(bin_widths_test, dtype=numpy.float32)
    mean = numpy.ascontiguousarray(map_mean, dtype=numpy.float32)
    if bin_widths.shape != (nb_maps,) or mean.shape != (nb_maps,):
        raise ValueError('`bin_widths_test` and `map_mean` must have one element per map.')
    if coding_tile is not None:
        coding_tile = _positive_pair(coding_tile, '`coding_tile`')
        tiles_per_call = _positive_int(tiles_per_call, '`tiles_per_call`')
    device = encoder.device
    thresholds = None
    if rdo_lambda is not None:
        from . import ratecontrol
        thresholds = ratecontrol.rdo_thresholds(bin_widths[None], probabilities[None], rdo_lambda, idx_map_exception)
    image_size = None
    luminances = torch.from_numpy(images).to(device)
    if pad:
        if nb_images < 1 or height < 1 or width < 1:
            raise ValueError('`luminances_uint8` holds no pixel.')
        image_size = (height, width)
        (height, width) = coded_size(height, width)
        luminances = dev.frame_pad_u8(luminances)
    y = encoder(luminances, tile=tile)
    if thresholds is None:
        q = dev.quantize_maps(y, torch.from_numpy(bin_widths).to(device), torch.from_numpy(mean).to(device), want_symbols=True)
    else:
        q = dev.latent_quantize_rdo(y, torch.from_numpy(bin_widths[None]).to(device), torch.from_numpy(thresholds).to(device),
                                    torch.zeros(nb_images, dtype=torch.int32, device=device), truncated_unary_length,
                                    torch.from_numpy(mean).to(device), want_symbols=True)
    if int(q['checks'][0].item()) != 0:
        raise AssertionError('The rounded array elements cannot be represented as 16-bit signed integers.')
    symbols = q['symbols']                                              # [N, 128, map_size] int16, stays in HBM
    exception_rows = numpy.zeros((0, truncated_unary_length), dtype=numpy.float64)
    if 0 <= idx_map_exception < nb_maps:
        exception_rows = _exception_rows(symbols, idx_map_exception, truncated_unary_length)
    else:
        idx_map_exception = -1
    if coding_tile is not None:
        coding_tile = _clamped_coding_tile(coding_tile, height, width)
    fields = _fields(encoder.are_bin_widths_learned, nb_images, height, width, idx_map_exception, bin_widths, mean, probabilities,
                     exception_rows, coding_tile, image_size)
    return _encode_entries(symbols, fields, nb_images if coding_tile is None else tiles_per_call)


def _require_multiples(height, width, what):
    """The entry points that do not pad ("what is refused") say so."""
    if height % csts.STRIDE_PROD != 0 or width % csts.STRIDE_PROD != 0:
        raise ValueError('{} does not pad: {} x {} images are not multiples of {} (`encode_images(..., pad=True)` and '
                         '`codec.BatchCodec(..., pad=True)` take any size).'.format(what, height, width, csts.STRIDE_PROD))


class _LadderOnDevice(object):
    """What `encode_images_to_budget` and `encode_images_to_quality` launch at the points of a ladder: the one pass of counts and the
    quantiser at a point. A ladder with a price (`ratecontrol.RateLadder(..., rdo_lambda=...)`) takes the
    rate-distortion optimised siblings of both, so that the symbols counted, probed and coded are the same."""

    def __init__(self, ladder, device):
        self.length = ladder.truncated_unary_length
        self.mean = torch.from_numpy(ladder.map_mean).to(device)
        self.bin_widths_points = torch.from_numpy(ladder.bin_widths_points).to(device)
        self.thresholds_points = None
        if ladder.rdo_thresholds_points is not None:
            self.thresholds_points = torch.from_numpy(ladder.rdo_thresholds_points).to(device)

    def histograms(self, y, coding_tile=None):
        """(hist, bypass_bits) as numpy: `device.ladder_histograms[_rdo]`, with coding_tile `device.ladder_histograms[_rdo]_tiles` of
        the plane y [N, h, w, 128]."""
        if self.thresholds_points is None:
            counts = (dev.ladder_histograms(y, self.bin_widths_points, self.mean, self.length) if coding_tile is None else
                      dev.ladder_histograms_tiles(y, self.bin_widths_points, coding_tile, self.mean, self.length))
        else:
            counts = (dev.ladder_histograms_rdo(y, self.bin_widths_points, self.thresholds_points, self.mean, self.length)
                      if coding_tile is None else
                      dev.ladder_histograms_rdo_tiles(y, self.bin_widths_points, self.thresholds_points, coding_tile, self.mean, self.length))
        return counts[0].cpu().numpy(), counts[1].cpu().numpy()

    def quantize(self, y, k, **wanted):
        """`device.quantize_maps(y, bin widths of point k, mean, **wanted)`, or `device.latent_quantize_rdo` at point k."""
        if self.thresholds_points is None:
            return dev.quantize_maps(y, self.bin_widths_points[k], self.mean, **wanted)
        point = torch.full((y.shape[0],), int(k), dtype=torch.int32, device=y.device)
        return dev.latent_quantize_rdo(y, self.bin_widths_points, self.thresholds_points, point, self.length, self.mean, **wanted)


def encode_images_to_budget(luminances_uint8, encoder, ladder, budget_bytes, tile=None, coding_tile=None):
    """uint8 (N, H, W) or (N, H, W, 1) luminance images -> (blobs, info): every image compressed into at most `budget_bytes` bytes
    (a scalar, or one value per image) at the first rate point of `ladder` (ratecontrol.RateLadder, finest first) at which it fits.

    One analysis transform and one pass over the latents (device.ladder_histograms) bound the size of every image at every point
    (ratecontrol.blob_byte_bounds); ratecontrol.select_rate_points then walks the ladder per image, skips the points whose lower
    bound exceeds the budget and codes the others -- `quantize_maps` and the coding stage of `encode_images`, one image at a time --
    until one fits. An image no point fits is coded at the last valid point of the ladder and reported in info['fits'].
    blobs: one single-image EAE1 blob per image, byte for byte `encode_images(images[i:i + 1], encoder, bin_widths_k, map_mean,
    table_k, idx_map_exception)[0]` for its point k: `decode_images` and `codec.BatchDecoder.submit(blobs)` read them unchanged.
    info: 'rate_point' int64 (N,); 'lower_bytes', 'upper_bytes' int64 (N, K); 'blob_bytes' int64 (N,); 'attempts' int64 (N,): the
    points coded for the image; 'fits' bool (N,); 'upper_bound_misses': points whose upper bound was within the budget and whose
    blob was not (expected 0: the allowances of ratecontrol.py are measured, not proven).
    An image whose symbols leave int16 at every point raises the AssertionError of `encode_images`.
    tile=(th, tw): as in `encode_images`.
    coding_tile=(th, tw) latents: single-image EAT1 blobs instead, byte for byte `encode_images(..., coding_tile=coding_tile)[0]` at
    the image's point. A tile's termination and byte padding need counts per tile: the one pass is
    `device.ladder_histograms_tiles`, the bounds those of `ratecontrol.blob_byte_bounds(..., coding_tile)`.
    A ladder with a price (`ratecontrol.RateLadder(..., rdo_lambda=...)`): the counts, hence the bounds, and the
    symbols coded are those of the rate-distortion optimised quantiser (`device.ladder_histograms_rdo[_tiles]`,
    `device.latent_quantize_rdo`); the blobs are `encode_images(..., rdo_lambda=ladder.rdo_lambdas[k])`'s.
    Not in this function: codec.BatchCodec, which takes one rate point per codec (codec.BudgetCodec chooses one per image inside
    the step, on the upper bound alone: DESIGN.md section 19)."""
    from . import ratecontrol
    images = numpy.ascontiguousarray(luminances_uint8)
    if images.dtype != numpy.uint8:
        raise TypeError('`luminances_uint8.dtype` is not equal to `numpy.uint8`.')
    if images.ndim == 4:
        images = images[:, :, :, 0]
    if not isinstance(ladder, ratecontrol.RateLadder):
        raise TypeError('`ladder` is not a `ratecontrol.RateLadder`.')
    (nb_images, height, width) = images.shape
    _require_multiples(height, width, '`encode_images_to_budget`')
    budgets = numpy.asarray(budget_bytes)
    if budgets.ndim > 1 or (budgets.ndim == 1 and budgets.shape[0] != nb_images) or budgets.dtype.kind not in 'iuf':
        raise ValueError('`budget_bytes` must be a number or one number per image.')
    length = ladder.truncated_unary_length
    device = encoder.device
    y = encoder(torch.from_numpy(images).to(device), tile=tile)
    points = _LadderOnDevice(ladder, device)
    map_size = (height//csts.STRIDE_PROD)*(width//csts.STRIDE_PROD)
    if coding_tile is None:
        (hist, bypass_bits) = points.histograms(y)
        (lower, upper) = ratecontrol.blob_byte_bounds(hist, bypass_bits, ladder, height, width)
        valid = ratecontrol.valid_points(hist, map_size)
    else:
        coding_tile = _clamped_coding_tile(coding_tile, height, width)
        plane = y.view(nb_images, height//csts.STRIDE_PROD, width//csts.STRIDE_PROD, -1)
        (hist, bypass_bits) = points.histograms(plane, coding_tile)
        (lower, upper) = ratecontrol.blob_byte_bounds(hist, bypass_bits, ladder, height, width, coding_tile)
        valid = ratecontrol.valid_points(hist.astype(numpy.int64).sum(axis=2), map_size)
    coded = {}

    def size_of(i, k):
        q = points.quantize(y[i:i + 1], k, want_symbols=True)
        if int(q['checks'][0].item()) != 0:         # `valid` says it cannot happen: the same symbols were counted
            raise AssertionError('The rounded array elements cannot be represented as 16-bit signed integers.')
        e = ladder.idx_map_exception
        rows = _exception_rows(q['symbols'], e, length) if e >= 0 else numpy.zeros((0, length), dtype=numpy.float64)
        fields = _fields(encoder.are_bin_widths_learned, 1, height, width, e, ladder.bin_widths_points[k], ladder.map_mean,
                         ladder.binary_probabilities_points[k], rows, coding_tile)
        coded[(i, k)] = _encode_entries(q['symbols'], fields, 1 if coding_tile is None else TILES_PER_CALL)[0]
        return len(coded[(i, k)])

    info = ratecontrol.select_rate_points(lower, upper, valid, budgets, size_of)
    info.update({'lower_bytes': lower, 'upper_bytes': upper})
    return [coded[(i, int(info['rate_point'][i]))] for i in range(nb_images)], info


def encode_images_to_quality(luminances_uint8, encoder, decoder, ladder, target_psnr=None, max_sse=None, budget_bytes=None, coding_tile=None):
    """uint8 (N, H, W) or (N, H, W, 1) luminance images -> (blobs, info): every image at the COARSEST rate point of `ladder`
    (ratecontrol.RateLadder, finest first) that keeps its PSNR at `target_psnr` dB or better -- its squared error against the input
    within `max_sse`; give one of the two, a scalar or one value per image. The synchronous sibling of `encode_images_to_budget`
    and the host loop `codec.QualityCodec` runs on the device.

    One analysis transform; then per image the bisection of ratecontrol.select_by_quality, a point's squared error found by
    quantising at it, decoding with `decoder` (pipeline.DeviceDecoder of the model) and `device.sse_u8`; only the point taken is
    coded. budget_bytes (a scalar or one value per image): the search starts at the point `ratecontrol.select_by_upper_bound` takes
    for the budget on `ratecontrol.upper_bounds_fixed`, the rule of `codec.BudgetCodec`, and goes to the coarsest; None: at the first
    point whose symbols fit int16. The squared error is assumed not to decrease along the ladder (select_by_quality).
    blobs: one single-image EAE1 blob per image, byte for byte `encode_images(images[i:i + 1], encoder, bin_widths_k, map_mean,
    table_k, idx_map_exception)[0]` for its point k.
    info: 'rate_point' int64 (N,), 'met' bool (N,), 'probe_points' and 'probe_sse' int64 (N, R) (select_by_quality's), 'max_sse'
    int64 (N,), 'first_point' int64 (N,), 'blob_bytes' int64 (N,), 'upper_bound_bytes' int64 (N, K).
    coding_tile=(th, tw) latents: single-image EAT1 blobs instead, byte for byte `encode_images(..., coding_tile=coding_tile)[0]` at
    the image's point, and the host loop of `codec.TiledQualityCodec`. The search is the same -- a point's
    squared error does not depend on the coding tile --; the budget's point comes from the counts per tile
    (`device.ladder_histograms_tiles`) and `ratecontrol.upper_bounds_fixed_tiles`, the rule of `codec.TiledBudgetCodec`.
    A ladder with a price (`ratecontrol.RateLadder(..., rdo_lambda=...)`): counts, probes and blobs are those of the rate-distortion
    optimised quantiser, as in `encode_images_to_budget`."""
    from . import ratecontrol
    images = numpy.ascontiguousarray(luminances_uint8)
    if images.dtype != numpy.uint8:
        raise TypeError('`luminances_uint8.dtype` is not equal to `numpy.uint8`.')
    if images.ndim == 4:
        images = images[:, :, :, 0]
    if not isinstance(ladder, ratecontrol.RateLadder):
        raise TypeError('`ladder` is not a `ratecontrol.RateLadder`.')
    (nb_images, height, width) = images.shape
    _require_multiples(height, width, '`encode_images_to_quality`')
    if (target_psnr is None) == (max_sse is None):
        raise ValueError('give `target_psnr` or `max_sse`, one of the two.')
    if target_psnr is not None:
        max_sse = ratecontrol.max_sse_for_psnr(numpy.asarray(target_psnr, dtype=numpy.float64), height*width)
    thresholds = numpy.asarray(max_sse)
    if thresholds.dtype.kind not in 'iu' or thresholds.ndim > 1 or (thresholds.ndim == 1 and thresholds.shape[0] != nb_images):
        raise ValueError('`target_psnr` / `max_sse` must be a scalar or one value per image (`max_sse` an integer).')
    thresholds = numpy.ascontiguousarray(numpy.broadcast_to(thresholds.astype(numpy.int64), (nb_images,)))
    (nb_points, length) = (ladder.nb_points, ladder.truncated_unary_length)
    device = encoder.device
    references = torch.from_numpy(images).to(device)
    y = encoder(references)
    points = _LadderOnDevice(ladder, device)
    map_size = (height//csts.STRIDE_PROD)*(width//csts.STRIDE_PROD)
    if coding_tile is None:
        (hist, bypass_bits) = points.histograms(y)
        upper = ratecontrol.upper_bounds_fixed(hist, bypass_bits, ladder, map_size)
        valid = ratecontrol.valid_points(hist, map_size)
    else:
        coding_tile = _clamped_coding_tile(coding_tile, height, width)
        plane = y.view(nb_images, height//csts.STRIDE_PROD, width//csts.STRIDE_PROD, -1)
        (hist, bypass_bits) = points.histograms(plane, coding_tile)
        upper = ratecontrol.upper_bounds_fixed_tiles(hist, bypass_bits, ladder, map_size,
                                                     ratecontrol.header_bytes(ladder, height, width, coding_tile))
        valid = ratecontrol.valid_points(hist.astype(numpy.int64).sum(axis=2), map_size)
    budgets = 1 << 62 if budget_bytes is None else budget_bytes
    (first, _) = ratecontrol.select_by_upper_bound(upper, valid, budgets)

    rounds = ratecontrol.quality_rounds(nb_points)
    info = {'rate_point': numpy.zeros(nb_images, dtype=numpy.int64), 'met': numpy.zeros(nb_images, dtype=bool),
            'probe_points': numpy.zeros((nb_images, rounds), dtype=numpy.int64), 'probe_sse': numpy.zeros((nb_images, rounds), dtype=numpy.int64),
            'max_sse': thresholds, 'first_point': first, 'blob_bytes': numpy.zeros(nb_images, dtype=numpy.int64), 'upper_bound_bytes': upper}
    e = ladder.idx_map_exception
    blobs = []
    for i in range(nb_images):
        known = {}

        def sse_of(k):
            if k not in known:
                q = points.quantize(y[i:i + 1], k, want_shifted=True)
                (_, decoded, _) = decoder(q['shifted'])
                known[k] = int(dev.sse_u8(decoded, references[i:i + 1]).item())
            return known[k]

        (k, info['met'][i], info['probe_points'][i], info['probe_sse'][i]) = ratecontrol.bisect_by_quality(sse_of, nb_points, int(first[i]),
                                                                                                           int(thresholds[i]))
        info['rate_point'][i] = k
        # the coding stage of `encode_images` on the latents at hand (as `encode_images_to_budget` codes a point)
        q = points.quantize(y[i:i + 1], k, want_symbols=True)
        if int(q['checks'][0].item()) != 0:
            raise AssertionError('The rounded array elements cannot be represented as 16-bit signed integers.')
        rows = _exception_rows(q['symbols'], e, length) if e >= 0 else numpy.zeros((0, length), dtype=numpy.float64)
        fields = _fields(encoder.are_bin_widths_learned, 1, height, width, e, ladder.bin_widths_points[k], ladder.map_mean,
                         ladder.binary_probabilities_points[k], rows, coding_tile)
        blobs.append(_encode_entries(q['symbols'], fields, 1 if coding_tile is None else TILES_PER_CALL)[0])
        info['blob_bytes'][i] = len(blobs[i])
    return blobs, info


def _fixed_header(fixed, total_length):
    """Checks the fixed part of the header of either format (`fixed`: the first bytes of the blob or file, `total_length`: the length
    of all of it) -> (fields, bytes of the fixed part, bytes of the whole header). Everything that sizes a read or an allocation is
    checked here, the whole header's length against `total_length` before any array behind the fixed part is read."""
    tiled = bytes(fixed[:4]) == TILE_MAGIC
    layout = _TILE_HEADER if tiled else _HEADER
    if len(fixed) < layout.size:
        raise ValueError('The container is truncated.')
    (magic, version, flags, nb_images, height, width, nb_maps, length, crop, idx_map_exception, *coding_tile) = layout.unpack_from(fixed, 0)
    if magic != (TILE_MAGIC if tiled else MAGIC):
        raise ValueError('The container does not start with the magic bytes.')
    if version != (TILE_VERSION if tiled else VERSION):
        raise ValueError('The container version {} is not supported.'.format(version))
    # sizes first: they dimension device buffers (a crafted header must not get that far)
    if nb_maps != csts.NB_MAPS_3:
        raise ValueError('The container does not hold {} maps per image.'.format(csts.NB_MAPS_3))
    if length < 1:
        raise ValueError('The truncated unary length does not belong to [1, 255].')
    if nb_images < 1 or height < 1 or width < 1 or height % csts.STRIDE_PROD != 0 or width % csts.STRIDE_PROD != 0:
        raise ValueError('The image sizes in the container are not positive multiples of {}.'.format(csts.STRIDE_PROD))
    if not -1 <= idx_map_exception < nb_maps:
        raise ValueError('The index of the exception map in the container is out of range.')
    # the real size: the coded one less the two nibbles of `crop` (module docstring); every value is valid, the sides are 16 at least
    fields = {'nb_images': nb_images, 'height': height, 'width': width, 'image_height': height - (crop >> 4),
              'image_width': width - (crop & 15), 'nb_maps': nb_maps, 'truncated_unary_length': length,
              'idx_map_exception': idx_map_exception, 'are_bin_widths_learned': bool(flags & 1)}
    if tiled:
        if min(coding_tile) < 1:
            raise ValueError('The coding tile sizes in the container are not positive.')
        fields.update({'format': 'EAT1', 'coding_tile': tuple(coding_tile)})
    nb_tiles = _nb_tiles(height//csts.STRIDE_PROD, width//csts.STRIDE_PROD, _coding_tile(fields))
    nb_rows = nb_images if idx_map_exception >= 0 else 0
    header_length = layout.size + 8*nb_maps + 8*nb_maps*length + 8*nb_rows*length + 8*nb_images*nb_tiles*nb_maps
    if header_length > total_length:
        raise ValueError('The container is truncated.')
    return fields, layout.size, header_length


def _read_arrays(fields, pos, blob, total_length):
    """The arrays behind the fixed part (`pos`: its size), which `blob` holds whole, into `fields` -> the header `read_header`
    returns. No bit count may exceed the capacity of its stream, and the counts must add up to `total_length`."""
    (nb_images, nb_maps, length) = (fields['nb_images'], fields['nb_maps'], fields['truncated_unary_length'])
    (h, w) = (fields['height']//csts.STRIDE_PROD, fields['width']//csts.STRIDE_PROD)
    (tiles, _) = coding_tile_grid(h, w, _coding_tile(fields))
    nb_rows = nb_images if fields['idx_map_exception'] >= 0 else 0
    header = dict(fields)

    def take(dtype, *shape):
        nonlocal pos
        out = numpy.frombuffer(blob, dtype=dtype, count=math.prod(shape), offset=pos).copy().reshape(shape)
        pos += out.nbytes
        return out

    header['bin_widths'] = take(numpy.float32, nb_maps)
    header['map_mean'] = take(numpy.float32, nb_maps)
    header['binary_probabilities'] = take(numpy.float64, nb_maps, length)
    header['exception_probabilities'] = take(numpy.float64, nb_rows, length)
    header['bits'] = take(numpy.uint32, nb_images, len(tiles), nb_maps, 2)
    header['payload_offset'] = pos
    # a stream can never be longer than the region the coder gives a map of its tile's size (compression.cpp:24): an inflated count
    # would make the unpacking write past it
    capacity = numpy.array([stream_capacity_bits(int(r*c), length) for (r, c) in tiles[:, 2:4].tolist()], dtype=numpy.int64)
    if (header['bits'].max(axis=(0, 2, 3)).astype(numpy.int64) > capacity).any():
        raise ValueError('A bit count of the header exceeds the capacity of a stream.')
    if pos + int(_entry_bytes(header['bits']).sum()) != total_length:
        raise ValueError('The payload size does not match the bit counts of the header.')
    if 'format' not in fields:
        header['bits'] = header['bits'].reshape(nb_images*nb_maps, 2)
    return header


def read_header(blob):
    """Parses everything in front of the payload. Raises ValueError on a malformed or truncated blob. 'bits' is uint32
    [nb_images*nb_maps, 2] for EAE1; an EAT1 blob gives the same keys, with 'bits' uint32 [nb_images, nb_tiles, nb_maps, 2], plus
    'format' ('EAT1') and 'coding_tile' (th, tw). 'height' / 'width' are the coded size, 'image_height' / 'image_width' the real one
    (module docstring: `crop`)."""
    (fields, pos, _) = _fixed_header(blob, len(blob))
    return _read_arrays(fields, pos, blob, len(blob))


def decode_symbols(blob, device='cuda'):
    """blob -> (header, int16 symbols [N, 128, map_size] on the device), arithmetic decoding only."""
    header = read_header(blob)
    if header.get('format') == 'EAT1':
        raise ValueError('An EAT1 container codes tiles, not whole maps: use decode_tile_symbols.')
    (entries, chunks) = _all_entries(header, blob)
    buffers = []

    def consume(group, decoded, offsets, tiles):
        buffers.append(decoded)

    # one group of whole maps: its buffer is [N, 128, map_size]
    _decode_entries(header, entries, chunks, torch.device(device), len(entries), consume)
    return (header, buffers[0].view(header['nb_images'], header['nb_maps'], -1))


def _require_kind(header, decoder):
    if header['are_bin_widths_learned'] != decoder.are_bin_widths_learned:
        raise ValueError('The container was written by the other kind of model (learned / fixed bin widths).')


def decode_images(blob, decoder, tile=None, tiles_per_call=TILES_PER_CALL):
    """blob + pipeline.DeviceDecoder of the model -> uint8 (N, H, W) reconstructions (BT.601 range, tools.py:61-93), of the real
    size the header's `crop` byte gives: the top-left h x w of the coded planes.
    tile=(th, tw): run the synthesis transform through windows (pipeline.DeviceDecoder.__call__): same reconstruction.
    EAT1 blobs are decoded in groups of `tiles_per_call` coding tiles, scattered and dequantised into the latent plane; the whole
    maps of an EAE1 blob are one group, dequantised by `dequantize_maps`."""
    if bytes(blob[:4]) == TILE_MAGIC:
        header = read_header(blob)
        return decode_region(blob, decoder, (0, 0, header['image_height'], header['image_width']), tile=tile, tiles_per_call=tiles_per_call)
    (header, symbols) = decode_symbols(blob, decoder.device)
    _require_kind(header, decoder)
    device = decoder.device
    shifted = dev.dequantize_maps(symbols, torch.from_numpy(header['bin_widths']).to(device),
                                  torch.from_numpy(header['map_mean']).to(device))['shifted']
    (h_map, w_map) = (header['height']//csts.STRIDE_PROD, header['width']//csts.STRIDE_PROD)
    (_, reconstruction_uint8, _) = decoder(shifted.view(header['nb_images'], h_map, w_map, header['nb_maps']), tile=tile)
    if (header['image_height'], header['image_width']) != (header['height'], header['width']):
        reconstruction_uint8 = reconstruction_uint8[:, :header['image_height'], :header['image_width']]
    return reconstruction_uint8.cpu().numpy()


# ---- coding tiles, regions and groups of (image, tile) entries: both formats -------------------------------------------------

def _positive_int(x, what):
    if not isinstance(x, numbers.Integral) or isinstance(x, bool) or x < 1:
        raise ValueError('{} must be a positive integer.'.format(what))
    return int(x)


def _positive_pair(x, what):
    if not isinstance(x, (tuple, list)) or len(x) != 2:
        raise ValueError('{} must be a pair of positive integers.'.format(what))
    return (_positive_int(x[0], what), _positive_int(x[1], what))


def _nb_tiles(h, w, coding_tile):
    return (-(-h//coding_tile[0]))*(-(-w//coding_tile[1]))


def coding_tile_grid(h, w, coding_tile):
    """The coding tiles of an h x w latent plane: (tiles, classes). tiles int64 [nb_tiles, 5], row-major: origin row, origin col,
    rows, cols, shape class; classes: the distinct (rows, cols), at most 4 (interior, last row, last column, corner)."""
    (th, tw) = _positive_pair(coding_tile, '`coding_tile`')
    (h, w) = (_positive_int(h, '`h`'), _positive_int(w, '`w`'))
    rows = [(r0, min(th, h - r0)) for r0 in range(0, h, th)]
    cols = [(c0, min(tw, w - c0)) for c0 in range(0, w, tw)]
    classes = []
    for shape in ((rows[0][1], cols[0][1]), (rows[-1][1], cols[0][1]), (rows[0][1], cols[-1][1]), (rows[-1][1], cols[-1][1])):
        if shape not in classes:
            classes.append(shape)
    tiles = numpy.empty((len(rows)*len(cols), 5), dtype=numpy.int64)
    k = 0
    for (r0, nr) in rows:
        for (c0, nc) in cols:
            tiles[k] = (r0, c0, nr, nc, classes.index((nr, nc)))
            k += 1
    return tiles, classes


def _coding_tile(fields):
    """The coding tile of either format: an EAE1 blob is one tile per map."""
    if fields.get('format') == 'EAT1':
        return fields['coding_tile']
    return (fields['height']//csts.STRIDE_PROD, fields['width']//csts.STRIDE_PROD)


def _tile_layout(header):
    """(coding tile, bits [N, nb_tiles, 128, 2]) of either format."""
    return _coding_tile(header), header['bits'].reshape(header['nb_images'], -1, header['nb_maps'], 2)


def _entry_bytes(bits):
    """bits [..., 128, 2] -> payload bytes of every (image, tile): its streams rounded up to bytes."""
    return ((bits.astype(numpy.int64) + 7)//8).sum(axis=(-1, -2))


def _stream_offsets(bits):
    """bits [E, 128, 2] of entries laid out one after the other -> byte offset of every stream, int64 [E, 128, 2]."""
    nbytes = (bits.astype(numpy.int64) + 7)//8
    return (numpy.cumsum(nbytes.reshape(-1)) - nbytes.reshape(-1)).reshape(nbytes.shape)


def region_plan(header, region, images=None):
    """What decoding the pixel rectangle region = (y0, x0, height, width) of `images` (indices, default all) needs.

    The region's latents, extended by pipeline.DECODER_HALO and clamped to the image, are the sub-plane whose synthesis gives
    the region's pixels exactly. Returns a dict: 'sub_plane' (row0, row1, col0, col1) in latents,
    'images', 'tiles' (indices of the coding tiles that intersect the sub-plane, row-major), 'entries' [(image, tile)],
    'ranges' [(start, stop)] byte range of every entry in the blob, 'crop' (y, x, height, width) of the region in the
    sub-plane's reconstruction, and 'header_bytes'. An EAE1 header is one tile per map. The region is in the coordinates of the real
    image and lies inside it ('image_height' x 'image_width', module docstring: `crop`)."""
    (nb_images, height, width) = (header['nb_images'], header['height'], header['width'])
    (image_height, image_width) = (header.get('image_height', height), header.get('image_width', width))
    if not isinstance(region, (tuple, list)) or len(region) != 4:
        raise ValueError('`region` must be (y0, x0, height, width).')
    for x in region:
        if not isinstance(x, numbers.Integral) or isinstance(x, bool):
            raise ValueError('`region` must be (y0, x0, height, width) in integers.')
    (y0, x0, rh, rw) = (int(x) for x in region)
    if rh < 1 or rw < 1 or y0 < 0 or x0 < 0 or y0 + rh > image_height or x0 + rw > image_width:
        raise ValueError('The region {} is empty or leaves the {} x {} image.'.format(tuple(region), image_height, image_width))
    if images is None:
        images = list(range(nb_images))
    else:
        images = [int(i) for i in images]
        if not images or len(set(images)) != len(images) or min(images) < 0 or max(images) >= nb_images:
            raise ValueError('`images` must be distinct indices of images of the container.')
    (h, w) = (height//csts.STRIDE_PROD, width//csts.STRIDE_PROD)
    (before, after) = pipeline.DECODER_HALO
    (r0, r1) = (max(y0//16 - before, 0), min(-(-(y0 + rh)//16) + after, h))
    (c0, c1) = (max(x0//16 - before, 0), min(-(-(x0 + rw)//16) + after, w))
    ((th, tw), bits) = _tile_layout(header)
    tiles_per_row = -(-w//tw)
    tiles = [i*tiles_per_row + j for i in range(r0//th, (r1 - 1)//th + 1) for j in range(c0//tw, (c1 - 1)//tw + 1)]
    nbytes = _entry_bytes(bits).reshape(-1)
    starts = header['payload_offset'] + numpy.cumsum(nbytes) - nbytes
    nb_tiles = bits.shape[1]
    entries = [(i, t) for i in images for t in tiles]
    ranges = [(int(starts[i*nb_tiles + t]), int(starts[i*nb_tiles + t] + nbytes[i*nb_tiles + t])) for (i, t) in entries]
    return {'sub_plane': (r0, r1, c0, c1), 'images': images, 'tiles': tiles, 'entries': entries, 'ranges': ranges,
            'crop': (y0 - 16*r0, x0 - 16*c0, rh, rw), 'header_bytes': header['payload_offset']}


def _read_at(f, start, count):
    f.seek(start)
    data = f.read(count)
    if len(data) != count:
        raise ValueError('The container is truncated.')
    return data


def _source_header(source):
    """The header of a container given as a bytes-like blob or as a seekable binary file object -> (header, blob): `blob` is a
    memoryview of the whole container when it is in memory -- a bytes-like source, or an EAE1 file, which is read whole: its maps are
    coded whole --, else None: of an EAT1 file only the fixed header, then the rest of the header, have been read."""
    if not hasattr(source, 'read'):
        blob = memoryview(source).cast('B')
        total = len(blob)
        (fields, pos, _) = _fixed_header(blob, total)
        return _read_arrays(fields, pos, blob, total), blob
    source.seek(0, 2)
    total = source.tell()
    fixed = _read_at(source, 0, min(_TILE_HEADER.size, total))
    (fields, pos, header_length) = _fixed_header(fixed, total)
    whole = 'format' not in fields
    blob = memoryview(fixed + _read_at(source, len(fixed), (total if whole else header_length) - len(fixed)))
    return _read_arrays(fields, pos, blob, total), (blob if whole else None)


def _read_ranges(source, blob, ranges):
    """One bytes-like chunk per byte range (start, stop) of a container: slices of `blob` when it is in memory (`_source_header`),
    else read from the file `source`, runs of adjacent ranges in one read."""
    if blob is not None:
        return [blob[a:b] for (a, b) in ranges]
    chunks = [None]*len(ranges)
    order = sorted(range(len(chunks)), key=lambda k: ranges[k])
    k = 0
    while k < len(order):                       # runs of adjacent ranges in one read
        run = [order[k]]
        while k + len(run) < len(order) and ranges[order[k + len(run)]][0] == ranges[run[-1]][1]:
            run.append(order[k + len(run)])
        start = ranges[run[0]][0]
        data = memoryview(_read_at(source, start, ranges[run[-1]][1] - start))
        for e in run:
            (a, b) = ranges[e]
            chunks[e] = data[a - start:b - start]
        k += len(run)
    return chunks


def fetch_region(source, region, images=None):
    """Host side of decode_region: (header, region_plan, one bytes-like chunk per plan entry). `source`: a bytes-like blob, or a
    seekable binary file object, from which only the fixed header, then the rest of the header, then the plan's byte ranges
    (adjacent ranges in one read) are read. An EAE1 file is read whole: its maps are coded whole."""
    (header, blob) = _source_header(source)
    plan = region_plan(header, region, images)
    return header, plan, _read_ranges(source, blob, plan['ranges'])


def _group_layout(entries, tiles, classes):
    """Device layout of a group of (image, tile) entries: the entries of one shape class side by side, so that the coder codes
    every class as one batch of maps of one size. -> (runs [(class, entry positions, first element)], element offset of every
    entry's map 0, elements of the buffer). Class runs start on 256-byte boundaries."""
    by_class = {}
    for (k, (_, t)) in enumerate(entries):
        by_class.setdefault(int(tiles[t, 4]), []).append(k)
    (runs, offsets, pos) = ([], numpy.zeros(len(entries), dtype=numpy.int64), 0)
    for cls in sorted(by_class):
        ks = by_class[cls]
        size = classes[cls][0]*classes[cls][1]
        runs.append((cls, ks, pos))
        offsets[ks] = pos + numpy.arange(len(ks), dtype=numpy.int64)*(dev.NB_MAPS*size)
        pos = (pos + len(ks)*dev.NB_MAPS*size + 127)//128*128
    return runs, offsets, max(pos, 128)


def _prob_rows(entries, ks, idx_map_exception):
    rows = numpy.tile(numpy.arange(dev.NB_MAPS, dtype=numpy.int32), len(ks)).reshape(len(ks), dev.NB_MAPS)
    if idx_map_exception >= 0:
        rows[:, idx_map_exception] = dev.NB_MAPS + numpy.array([entries[k][0] for k in ks], dtype=numpy.int32)
    return rows.reshape(-1)


def _symbols_plan(entries, tiles, offsets, image_index=None, origin=(0, 0)):
    """Plan rows (device.TILE_SYMBOLS_PLAN_COLS) of a group: image (or its index in the output), origin relative to `origin`,
    extent, offset in the group buffer."""
    plan = numpy.empty((len(entries), dev.TILE_SYMBOLS_PLAN_COLS), dtype=numpy.int64)
    for (k, (i, t)) in enumerate(entries):
        plan[k] = (i if image_index is None else image_index[i], tiles[t, 0] - origin[0], tiles[t, 1] - origin[1], tiles[t, 2],
                   tiles[t, 3], offsets[k])
    return plan


class _Workspace(object):
    """One coder workspace per call, grown to the largest class batch of a group (the batches run one after the other)."""

    def __init__(self, device, length):
        (self.device, self.length, self.tensor) = (device, length, None)

    def get(self, n_maps, map_size):
        need = dev.coder_workspace_bytes(n_maps, map_size, self.length)
        if self.tensor is None or self.tensor.numel() < need:
            self.tensor = None
            self.tensor = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.tensor


def _encode_entries(symbols, fields, per_call):
    """The coding stage of encode_images: symbols [N, 128, h*w] (device) + the header to write (`_fields`) -> (blob, info). Per
    group of `per_call` (image, tile) entries in payload order: one gather launch, one coder batch per shape class, one pack launch
    per class into the group's payload. Whole maps (one tile per map) are the group's layout as they stand: no gather, no copy."""
    (nb_images, nb_maps, _) = symbols.shape
    (h, w) = (fields['height']//csts.STRIDE_PROD, fields['width']//csts.STRIDE_PROD)
    (tiles, classes) = coding_tile_grid(h, w, _coding_tile(fields))
    nb_tiles = tiles.shape[0]
    length = fields['truncated_unary_length']
    device = symbols.device
    table = numpy.concatenate([fields['binary_probabilities'], fields['exception_probabilities']])
    table_device = torch.from_numpy(table).to(device)
    workspace = _Workspace(device, length)
    bits = numpy.zeros((nb_images, nb_tiles, nb_maps, 2), dtype=numpy.uint32)
    all_entries = [(i, t) for i in range(nb_images) for t in range(nb_tiles)]
    pieces = []
    for g0 in range(0, len(all_entries), per_call):
        entries = all_entries[g0:g0 + per_call]
        (runs, offsets, total) = _group_layout(entries, tiles, classes)
        if nb_tiles == 1:
            gathered = symbols[entries[0][0]:entries[-1][0] + 1].view(-1)
        else:
            plan = _symbols_plan(entries, tiles, offsets)
            gathered = torch.empty(total, dtype=torch.int16, device=device)
            dev.tile_symbols_gather(symbols, gathered, torch.from_numpy(plan).to(device), plan, h, w)
        coded = []
        for (cls, ks, start) in runs:
            size = classes[cls][0]*classes[cls][1]
            n_maps = len(ks)*nb_maps
            prob_row = torch.from_numpy(_prob_rows(entries, ks, fields['idx_map_exception'])).to(device)
            coded.append(dev.coder_encode_batch(gathered[start:start + n_maps*size].view(n_maps, size), table_device, prob_row, length,
                                                workspace=workspace.get(n_maps, size)))
        group_bits = numpy.zeros((len(entries), nb_maps, 2), dtype=numpy.uint32)
        for ((_, ks, _), streams) in zip(runs, coded):
            results = streams.results.cpu().numpy()
            _raise_for_statuses(results)
            group_bits[ks] = numpy.stack([results[0], results[1]], axis=1).reshape(len(ks), nb_maps, 2)
        stream_offsets = _stream_offsets(group_bits)
        group_bytes = int(_entry_bytes(group_bits).sum())
        payload = None                              # the first pack allocates it
        for ((_, ks, _), streams) in zip(runs, coded):
            payload = dev.coder_pack_streams(streams, torch.from_numpy(stream_offsets[ks].reshape(-1, 2)).to(device), group_bytes,
                                             payload=payload)
        pieces.append(payload[:group_bytes].cpu().numpy().tobytes())
        for (k, (i, t)) in enumerate(entries):
            bits[i, t] = group_bits[k]
        del gathered, coded, streams, payload       # before the next group allocates its own
    header = _pack_header(fields, bits)
    payload = b''.join(pieces)
    info = {'nb_bits': (bits[..., 0].astype(numpy.int64) + bits[..., 1]).sum(axis=1).astype(numpy.uint32), 'payload_bytes': len(payload),
            'header_bytes': len(header)}
    if 'format' in fields:
        info['tile_bits'] = bits
    return header + payload, info


def _decode_entries(header, entries, chunks, device, per_call, consume):
    """Entropy-decodes (image, tile) entries whose payload bytes are `chunks`, in groups of `per_call`: one upload, then per shape
    class one unpack and one coder batch into the group's tile-major buffer. consume(entries, buffer, offsets, tiles) gets every
    group (offsets: element offset of every entry's map 0). Raises the coder's error after the group that met it."""
    (h, w) = (header['height']//csts.STRIDE_PROD, header['width']//csts.STRIDE_PROD)
    (coding_tile, bits) = _tile_layout(header)
    (tiles, classes) = coding_tile_grid(h, w, coding_tile)
    length = header['truncated_unary_length']
    table = numpy.concatenate([header['binary_probabilities'], header['exception_probabilities']])
    table_device = torch.from_numpy(table).to(device)
    workspace = _Workspace(device, length)
    nb_maps = header['nb_maps']
    for g0 in range(0, len(entries), per_call):
        group = entries[g0:g0 + per_call]
        group_bits = numpy.stack([bits[i, t] for (i, t) in group])
        stream_offsets = _stream_offsets(group_bits)
        sizes = _entry_bytes(group_bits)
        payload = numpy.zeros(int(sizes.sum()) + 8, dtype=numpy.uint8)
        pos = 0
        for (k, chunk) in enumerate(chunks[g0:g0 + per_call]):
            if len(chunk) != sizes[k]:
                raise ValueError('A payload range does not match the bit counts of the header.')
            payload[pos:pos + sizes[k]] = numpy.frombuffer(chunk, dtype=numpy.uint8)
            pos += int(sizes[k])
        payload_device = torch.from_numpy(payload).to(device)
        (runs, offsets, total) = _group_layout(group, tiles, classes)
        decoded = torch.empty(total, dtype=torch.int16, device=device)
        results = []
        for (cls, ks, start) in runs:
            size = classes[cls][0]*classes[cls][1]
            n_maps = len(ks)*nb_maps
            run_bits = group_bits[ks].reshape(-1, 2)
            streams = dev.coder_unpack_streams(payload_device, torch.from_numpy(stream_offsets[ks].reshape(-1, 2)).to(device),
                                               torch.from_numpy(run_bits[:, 0].astype(numpy.int32)).to(device),
                                               torch.from_numpy(run_bits[:, 1].astype(numpy.int32)).to(device), size, length)
            prob_row = torch.from_numpy(_prob_rows(group, ks, header['idx_map_exception'])).to(device)
            dev.coder_decode_batch(streams, table_device, prob_row, workspace=workspace.get(n_maps, size),
                                   out=decoded[start:start + n_maps*size].view(n_maps, size))
            results.append(streams.results)
        consume(group, decoded, offsets, tiles)
        for r in results:
            _raise_for_statuses(r.cpu().numpy())
        del payload_device, decoded, streams, results


def _all_entries(header, blob):
    """Every (image, tile) entry of a blob in payload order, and its payload bytes: (entries, chunks) for _decode_entries."""
    # the whole real image: its sub-plane is the whole latent plane (the coded size is the real one rounded up to the next 16)
    plan = region_plan(header, (0, 0, header.get('image_height', header['height']), header.get('image_width', header['width'])))
    view = memoryview(blob).cast('B')
    return plan['entries'], [view[a:b] for (a, b) in plan['ranges']]


def decode_tile_symbols(blob, device='cuda', tiles_per_call=TILES_PER_CALL):
    """An EAT1 (or EAE1) blob -> (header, symbols): symbols[i][t] = int16 [128, rows, cols] (device) of image i, coding tile t
    (row-major; an EAE1 blob has one tile per map), arithmetic decoding only."""
    header = read_header(blob)
    (entries, chunks) = _all_entries(header, blob)
    out = [[None]*(len(entries)//header['nb_images']) for _ in range(header['nb_images'])]

    def consume(group, decoded, offsets, tiles):
        for (k, (i, t)) in enumerate(group):
            (rows, cols) = (int(tiles[t, 2]), int(tiles[t, 3]))
            start = int(offsets[k])
            out[i][t] = decoded[start:start + dev.NB_MAPS*rows*cols].view(dev.NB_MAPS, rows, cols)

    _decode_entries(header, entries, chunks, torch.device(device), _positive_int(tiles_per_call, '`tiles_per_call`'), consume)
    return header, out


def decode_region(source, decoder, region, images=None, tile=None, tiles_per_call=TILES_PER_CALL):
    """The pixels region = (y0, x0, height, width) of `images` (indices, default all) -> uint8 [N_sel, height, width], equal to
    decode_images(...)[images, y0:y0 + height, x0:x0 + width]. `source`: a bytes-like blob or a seekable binary file object, of
    which only the header and the byte ranges region_plan names are read (fetch_region). Only the coding tiles that meet the
    region's sub-plane are entropy-decoded (for an EAE1 source: the whole maps), and only the sub-plane is synthesised.
    tile=(th, tw): synthesise the sub-plane through windows (pipeline.DeviceDecoder.__call__)."""
    tiles_per_call = _positive_int(tiles_per_call, '`tiles_per_call`')
    return _decode_fetched(*fetch_region(source, region, images), decoder, tile, tiles_per_call)


def _decode_fetched(header, plan, chunks, decoder, tile=None, tiles_per_call=TILES_PER_CALL):
    """The device side of decode_region, of what fetch_region returned."""
    _require_kind(header, decoder)
    device = decoder.device
    (r0, r1, c0, c1) = plan['sub_plane']
    shifted = torch.empty((len(plan['images']), r1 - r0, c1 - c0, header['nb_maps']), dtype=torch.float32, device=device)
    bin_widths = torch.from_numpy(header['bin_widths']).to(device)
    map_mean = torch.from_numpy(header['map_mean']).to(device)
    image_index = {i: k for (k, i) in enumerate(plan['images'])}

    def consume(group, decoded, offsets, tiles):
        rows = _symbols_plan(group, tiles, offsets, image_index, (r0, c0))
        dev.tile_symbols_dequantize(decoded, torch.from_numpy(rows).to(device), rows, bin_widths, map_mean, shifted)

    _decode_entries(header, plan['entries'], chunks, device, tiles_per_call, consume)
    (_, reconstruction, _) = decoder(shifted, tile=tile)
    (y, x, rh, rw) = plan['crop']
    return reconstruction[:, y:y + rh, x:x + rw].cpu().numpy()


# ---- colour pictures: EAC1, three plane blobs behind one header (module docstring) -------------------------------

COLOUR_MAGIC = b'EAC1'
COLOUR_VERSION = 1
SUBSAMPLING_420 = 1            # the only value written and read; the others are reserved for 4:4:4 / 4:2:2 and refused
_COLOUR_HEADER = struct.Struct('<4sHHIIIB3s3Q')
COLOUR_HEADER_BYTES = _COLOUR_HEADER.size          # 48: what a picture's byte budget pays in front of its plane blobs (ratecontrol.py)
_PLANE_NAMES = ('y', 'cb', 'cr')


def _plane_sizes(image_size):
    (h, w) = image_size
    chroma = colour_rules.chroma_size(h, w)
    return ((h, w), chroma, chroma)


def _check_planes(nb_images, image_size, plane_blobs):
    """Every plane blob must be an EAE1 / EAT1 blob of `nb_images` images (None: of the luminance blob's count) of its plane's real
    size -> the image count. Only the fixed part of each header is looked at: `decode_images` checks the rest when it reads a plane."""
    for (name, size, blob) in zip(_PLANE_NAMES, _plane_sizes(image_size), plane_blobs):
        (fields, _, _) = _fixed_header(blob, len(blob))
        if nb_images is None:
            nb_images = fields['nb_images']
        if fields['nb_images'] != nb_images:
            raise ValueError('The {0} plane holds {1} images, not {2}.'.format(name, fields['nb_images'], nb_images))
        if (fields['image_height'], fields['image_width']) != size:
            raise ValueError('The {0} plane of a {1} x {2} picture is {3} x {4}, not {5} x {6}.'.format(
                name, image_size[0], image_size[1], size[0], size[1], fields['image_height'], fields['image_width']))
    return nb_images


def assemble_colour_blob(image_size, y_blob, cb_blob, cr_blob):
    """The EAC1 blob (module docstring) of pictures of image_size = (h, w) from the blobs of their three planes, each what
    `encode_images(plane, ..., pad=True)` writes. Raises ValueError when the planes' image counts differ or their real sizes are not
    (h, w), (hc, wc), (hc, wc)."""
    image_size = _positive_pair(image_size, '`image_size`')
    blobs = tuple(bytes(blob) for blob in (y_blob, cb_blob, cr_blob))
    nb_images = _check_planes(None, image_size, blobs)
    head = _COLOUR_HEADER.pack(COLOUR_MAGIC, COLOUR_VERSION, 0, nb_images, image_size[0], image_size[1], SUBSAMPLING_420, b'\0\0\0',
                               *(len(blob) for blob in blobs))
    return head + b''.join(blobs)


def read_colour_header(blob):
    """The 48 bytes in front of the plane blobs of an EAC1 blob -> {'nb_images', 'image_height', 'image_width', 'subsampling',
    'plane_bytes' (three), 'plane_offsets' (three)}. Raises ValueError on anything but a whole, well-formed EAC1 header whose three
    lengths add up to the blob's."""
    return _colour_header(blob, len(blob))


def _colour_header(blob, total_length):
    """`read_colour_header` of a container of `total_length` bytes of which `blob` holds the first 48 at least."""
    if len(blob) < _COLOUR_HEADER.size:
        raise ValueError('The colour container is truncated.')
    (magic, version, flags, nb_images, height, width, subsampling, reserved, *plane_bytes) = _COLOUR_HEADER.unpack_from(blob, 0)
    if magic != COLOUR_MAGIC:
        raise ValueError('The colour container does not start with the magic bytes.')
    if version != COLOUR_VERSION:
        raise ValueError('The colour container version {} is not supported.'.format(version))
    if flags != 0 or reserved != b'\0\0\0':
        raise ValueError('A reserved field of the colour container is not zero.')
    if subsampling != SUBSAMPLING_420:
        raise ValueError('The chroma subsampling {} is not supported: only 4:2:0 (1) is.'.format(subsampling))
    if nb_images < 1 or height < 1 or width < 1:
        raise ValueError('The colour container holds no pixel.')
    if min(plane_bytes) < 1 or _COLOUR_HEADER.size + sum(plane_bytes) != total_length:
        raise ValueError('The plane lengths of the colour container do not add up to its length.')
    offsets = (_COLOUR_HEADER.size, _COLOUR_HEADER.size + plane_bytes[0], _COLOUR_HEADER.size + plane_bytes[0] + plane_bytes[1])
    return {'nb_images': nb_images, 'image_height': height, 'image_width': width, 'subsampling': subsampling,
            'plane_bytes': tuple(plane_bytes), 'plane_offsets': offsets}


def split_colour_blob(blob):
    """EAC1 blob -> (header, y_blob, cb_blob, cr_blob): `read_colour_header`, and the three plane blobs, each an ordinary EAE1 / EAT1
    blob every decoder of this module reads. Raises ValueError when a plane does not belong to the header (image count, real size)."""
    header = read_colour_header(blob)
    view = memoryview(blob)
    planes = tuple(bytes(view[start:start + count]) for (start, count) in zip(header['plane_offsets'], header['plane_bytes']))
    _check_planes(header['nb_images'], (header['image_height'], header['image_width']), planes)
    return (header,) + planes


def encode_colour_images(rgb_uint8, encoder, bin_widths_test, map_mean, binary_probabilities, idx_map_exception=-1, chroma=None,
                         coding_tile=None, rdo_lambda=None, tile=None):
    """uint8 (N, h, w, 3) RGB pictures of any height and width -> (EAC1 blob bytes, info dict).

    The picture is split on the device into Y, Cb and Cr, 4:2:0 (device.colour_split_420: `colour.split_420_numpy`), and each plane
    goes through `encode_images(plane, encoder, ..., pad=True)`: the three plane blobs inside the EAC1 are those, byte for byte.
    encoder, bin_widths_test, map_mean, binary_probabilities, idx_map_exception: `encode_images`'s, for the luminance plane.
    chroma: None (Cb and Cr take the luminance arguments) or (bin_widths_test, map_mean, binary_probabilities, idx_map_exception)
    for Cb and Cr: a rate point of their own, through the same model.
    coding_tile, rdo_lambda, tile: passed on to the three `encode_images` calls.
    info: 'y', 'cb', 'cr': the planes' infos; 'plane_bytes': their blobs' lengths."""
    rgb = numpy.ascontiguousarray(rgb_uint8)
    if rgb.dtype != numpy.uint8:
        raise TypeError('`rgb_uint8.dtype` is not equal to `numpy.uint8`.')
    if rgb.ndim != 4 or rgb.shape[3] != 3 or 0 in rgb.shape:
        raise ValueError('`rgb_uint8` must be (N, h, w, 3) and hold a pixel.')
    luma_point = (bin_widths_test, map_mean, binary_probabilities, idx_map_exception)
    chroma_point = luma_point if chroma is None else tuple(chroma)
    if len(chroma_point) != 4:
        raise ValueError('`chroma` must be (bin_widths_test, map_mean, binary_probabilities, idx_map_exception).')
    more = {'tile': tile, 'rdo_lambda': rdo_lambda, 'pad': True}
    if coding_tile is not None:
        more['coding_tile'] = coding_tile
    planes = dev.colour_split_420(torch.from_numpy(rgb).to(encoder.device))
    blobs = []
    info = {}
    for (name, plane, point) in zip(_PLANE_NAMES, planes, (luma_point, chroma_point, chroma_point)):
        (blob, info[name]) = encode_images(plane.cpu().numpy(), encoder, *point, **more)
        blobs.append(blob)
    info['plane_bytes'] = tuple(len(blob) for blob in blobs)
    return (assemble_colour_blob(rgb.shape[1:3], *blobs), info)


def encode_colour_images_to_budget(rgb_uint8, encoder, ladder, budget_bytes, chroma_ladder=None, chroma_share=0.25):
    """uint8 (N, h, w, 3) RGB pictures of any height and width -> (blobs, info): every picture as a single-picture EAC1 blob of at
    most `budget_bytes` bytes (a scalar, or one value per picture) where the bounds promise it. The synchronous sibling of
    `codec.ColourBudgetCodec` and the statement of its rule (ratecontrol.py, "the rule of `codec.ColourBudgetCodec`"; DESIGN.md section
    29): a point is taken on `ratecontrol.upper_bounds_fixed` alone, as `codec.BudgetCodec` takes it, and nothing is coded to find out
    -- this is not `encode_images_to_budget`'s trial-coding loop.

    The pictures are split 4:2:0 on the device (device.colour_split_420); every plane is padded (device.frame_pad_u8) and gets one
    analysis transform and one pass of counts at the K points of its ladder -- `ladder` for Y, `chroma_ladder` (None: `ladder`) for
    Cb and Cr, both of the same K. Cb and Cr take `select_by_upper_bound`'s point for `ratecontrol.colour_chroma_budgets(budget_bytes,
    chroma_share)`, Y the point for `ratecontrol.colour_luma_budgets`: the payload less the bounds of the points chroma took. Every
    plane is then coded with `encode_images(plane[i:i + 1], ..., pad=True)` at its point (`rdo_lambda=ladder.rdo_lambdas[k]` for a
    ladder with a price) and the three blobs are assembled with `assemble_colour_blob`: `decode_colour_images` and
    `codec.ColourDecoder` read the blobs unchanged.
    info: 'rate_point' int64 (N, 3) in the order Y, Cb, Cr; 'upper_bound_bytes' int64 (N, 3, K); 'plane_budget_bytes' int64 (N, 3);
    'valid_points' bool (N, 3, K): the points whose symbols fit int16; 'plane_promised' bool (N, 3); 'plane_blob_bytes' int64 (N, 3);
    'budget_bytes', 'blob_bytes' int64 (N,); 'promised' bool (N,): all
    three planes' bounds are within their budgets, and then 48 + the three bounds <= budget; 'fits' bool (N,): the blob is."""
    from . import ratecontrol
    rgb = numpy.ascontiguousarray(rgb_uint8)
    if rgb.dtype != numpy.uint8:
        raise TypeError('`rgb_uint8.dtype` is not equal to `numpy.uint8`.')
    if rgb.ndim != 4 or rgb.shape[3] != 3 or 0 in rgb.shape:
        raise ValueError('`rgb_uint8` must be (N, h, w, 3) and hold a pixel.')
    chroma_ladder = ladder if chroma_ladder is None else chroma_ladder
    if not isinstance(ladder, ratecontrol.RateLadder) or not isinstance(chroma_ladder, ratecontrol.RateLadder):
        raise TypeError('`ladder` and `chroma_ladder` must be `ratecontrol.RateLadder`s.')
    if chroma_ladder.nb_points != ladder.nb_points:
        raise ValueError('`ladder` and `chroma_ladder` hold {0} and {1} rate points: the same number is needed.'.format(
            ladder.nb_points, chroma_ladder.nb_points))
    nb_images = rgb.shape[0]
    budgets = numpy.asarray(budget_bytes)
    if budgets.ndim > 1 or (budgets.ndim == 1 and budgets.shape[0] != nb_images) or budgets.dtype.kind not in 'iuf':
        raise ValueError('`budget_bytes` must be a number or one number per picture.')
    budgets = numpy.ascontiguousarray(numpy.broadcast_to(budgets.astype(numpy.int64), (nb_images,)))
    chroma_budgets = ratecontrol.colour_chroma_budgets(budgets, chroma_share)
    device = encoder.device
    planes = dev.colour_split_420(torch.from_numpy(rgb).to(device))
    ladders = (ladder, chroma_ladder, chroma_ladder)

    def bounds(plane, plane_ladder):
        padded = dev.frame_pad_u8(plane)
        map_size = (padded.shape[1]//csts.STRIDE_PROD)*(padded.shape[2]//csts.STRIDE_PROD)
        (hist, bypass_bits) = _LadderOnDevice(plane_ladder, device).histograms(encoder(padded))
        return ratecontrol.upper_bounds_fixed(hist, bypass_bits, plane_ladder, map_size), ratecontrol.valid_points(hist, map_size)

    (upper_y, valid_y) = bounds(planes[0], ladder)
    (upper_cb, valid_cb) = bounds(planes[1], chroma_ladder)
    (upper_cr, valid_cr) = bounds(planes[2], chroma_ladder)
    (point_cb, promised_cb) = ratecontrol.select_by_upper_bound(upper_cb, valid_cb, chroma_budgets)
    (point_cr, promised_cr) = ratecontrol.select_by_upper_bound(upper_cr, valid_cr, chroma_budgets)
    luma_budgets = ratecontrol.colour_luma_budgets(budgets, upper_cb, point_cb, upper_cr, point_cr)
    (point_y, promised_y) = ratecontrol.select_by_upper_bound(upper_y, valid_y, luma_budgets)
    info = {'rate_point': numpy.stack([point_y, point_cb, point_cr], axis=1),
            'upper_bound_bytes': numpy.stack([upper_y, upper_cb, upper_cr], axis=1),
            'plane_budget_bytes': numpy.stack([luma_budgets, chroma_budgets, chroma_budgets], axis=1),
            'valid_points': numpy.stack([valid_y, valid_cb, valid_cr], axis=1),
            'plane_promised': numpy.stack([promised_y, promised_cb, promised_cr], axis=1),
            'plane_blob_bytes': numpy.zeros((nb_images, 3), dtype=numpy.int64), 'budget_bytes': budgets}
    host_planes = [plane.cpu().numpy() for plane in planes]
    blobs = []
    for i in range(nb_images):
        plane_blobs = []
        for (which, (plane, plane_ladder)) in enumerate(zip(host_planes, ladders)):
            k = int(info['rate_point'][i, which])
            more = {} if plane_ladder.rdo_lambdas is None else {'rdo_lambda': plane_ladder.rdo_lambdas[k]}
            plane_blobs.append(encode_images(plane[i:i + 1], encoder, plane_ladder.bin_widths_points[k], plane_ladder.map_mean,
                                             plane_ladder.binary_probabilities_points[k], plane_ladder.idx_map_exception, pad=True, **more)[0])
            info['plane_blob_bytes'][i, which] = len(plane_blobs[which])
        blobs.append(assemble_colour_blob(rgb.shape[1:3], *plane_blobs))
    info['blob_bytes'] = numpy.array([len(blob) for blob in blobs], dtype=numpy.int64)
    info['promised'] = info['plane_promised'].all(axis=1)
    info['fits'] = info['blob_bytes'] <= budgets
    return blobs, info


def encode_colour_images_to_quality(rgb_uint8, encoder, decoder, ladder, target_psnr=None, max_sse=None, chroma_ladder=None,
                                    chroma_share=1./3.):
    """uint8 (N, h, w, 3) RGB pictures of any height and width -> (blobs, info): every picture as a single-picture EAC1 blob, as small
    as the ladders allow while its PSNR over all S = h w + 2 hc wc samples of its 4:2:0 form is `target_psnr` dB or better -- its
    squared error sse_Y + sse_Cb + sse_Cr against the split input within `max_sse`; give one of the two, a scalar or one value per
    picture. The synchronous sibling of `codec.ColourQualityCodec` and the statement of its rule (ratecontrol.py, "the rule of
    `codec.ColourQualityCodec`").

    The pictures are split 4:2:0 on the device (device.colour_split_420); every plane is padded (device.frame_pad_u8) and gets one
    analysis transform and one pass of counts at the K points of its ladder -- `ladder` for Y, `chroma_ladder` (None: `ladder`) for
    Cb and Cr, both of the same K --, from which its search starts at the first point whose symbols fit int16. A probe quantises the
    padded plane at its point, decodes it with `decoder` and takes the squared error over the REAL samples (`device.frame_sse_u8`
    against the real plane). Cb and Cr run `ratecontrol.bisect_by_quality` for `ratecontrol.colour_chroma_max_sse(max_sse,
    chroma_share)`, Y for `ratecontrol.colour_luma_max_sse`: the threshold less the real squared errors of the points chroma took.
    Every plane is then coded with `encode_images(plane[i:i + 1], ..., pad=True)` at its point (`rdo_lambda=ladder.rdo_lambdas[k]` for
    a ladder with a price) and the three blobs are assembled with `assemble_colour_blob`: `decode_colour_images` and
    `codec.ColourDecoder` read the blobs unchanged. The squared error of a plane is assumed not to decrease along its ladder
    (`ratecontrol.select_by_quality`); the default share is a starting value nobody has measured on a trained model.
    info: 'rate_point', 'first_point', 'sse', 'plane_max_sse', 'plane_blob_bytes' int64 (N, 3) in the order Y, Cb, Cr;
    'plane_met' bool (N, 3); 'probe_points', 'probe_sse' int64 (N, 3, R); 'max_sse', 'picture_sse', 'blob_bytes' int64 (N,); 'met'
    bool (N,): picture_sse <= max_sse."""
    from . import ratecontrol
    rgb = numpy.ascontiguousarray(rgb_uint8)
    if rgb.dtype != numpy.uint8:
        raise TypeError('`rgb_uint8.dtype` is not equal to `numpy.uint8`.')
    if rgb.ndim != 4 or rgb.shape[3] != 3 or 0 in rgb.shape:
        raise ValueError('`rgb_uint8` must be (N, h, w, 3) and hold a pixel.')
    chroma_ladder = ladder if chroma_ladder is None else chroma_ladder
    if not isinstance(ladder, ratecontrol.RateLadder) or not isinstance(chroma_ladder, ratecontrol.RateLadder):
        raise TypeError('`ladder` and `chroma_ladder` must be `ratecontrol.RateLadder`s.')
    if chroma_ladder.nb_points != ladder.nb_points:
        raise ValueError('`ladder` and `chroma_ladder` hold {0} and {1} rate points: the same number is needed.'.format(
            ladder.nb_points, chroma_ladder.nb_points))
    if (target_psnr is None) == (max_sse is None):
        raise ValueError('give `target_psnr` or `max_sse`, one of the two.')
    (nb_images, height, width) = rgb.shape[:3]
    if target_psnr is not None:
        targets = numpy.asarray(target_psnr, dtype=numpy.float64)
        if targets.ndim > 1 or (targets.ndim == 1 and targets.shape[0] != nb_images):
            raise ValueError('`target_psnr` must be a number or one number per picture.')
        max_sse = ratecontrol.max_sse_for_psnr(targets, ratecontrol.colour_nb_samples(height, width))
    if numpy.ndim(max_sse) > 1 or (numpy.ndim(max_sse) == 1 and numpy.shape(max_sse)[0] != nb_images):
        raise ValueError('`max_sse` must be an integer or one integer per picture.')
    thresholds = numpy.ascontiguousarray(numpy.broadcast_to(ratecontrol._colour_max_sse(max_sse), (nb_images,)))
    chroma_thresholds = ratecontrol.colour_chroma_max_sse(thresholds, chroma_share)
    device = encoder.device
    planes = dev.colour_split_420(torch.from_numpy(rgb).to(device))
    (nb_points, rounds) = (ladder.nb_points, ratecontrol.quality_rounds(ladder.nb_points))

    def search(plane, plane_ladder, plane_thresholds):
        """One plane of every picture -> (point, met, probe_points, probe_sse, first, sse of the point taken)."""
        padded = dev.frame_pad_u8(plane)
        map_size = (padded.shape[1]//csts.STRIDE_PROD)*(padded.shape[2]//csts.STRIDE_PROD)
        y = encoder(padded)
        points = _LadderOnDevice(plane_ladder, device)
        (hist, bypass_bits) = points.histograms(y)
        upper = ratecontrol.upper_bounds_fixed(hist, bypass_bits, plane_ladder, map_size)
        (first, _) = ratecontrol.select_by_upper_bound(upper, ratecontrol.valid_points(hist, map_size), 1 << 62)
        found = (numpy.zeros(nb_images, dtype=numpy.int64), numpy.zeros(nb_images, dtype=bool), numpy.zeros((nb_images, rounds), dtype=numpy.int64),
                 numpy.zeros((nb_images, rounds), dtype=numpy.int64), first, numpy.zeros(nb_images, dtype=numpy.int64))
        for i in range(nb_images):
            known = {}

            def sse_of(k):
                if k not in known:
                    q = points.quantize(y[i:i + 1], k, want_shifted=True)
                    (_, decoded, _) = decoder(q['shifted'])
                    known[k] = int(dev.frame_sse_u8(decoded, plane[i:i + 1]).item())
                return known[k]

            (found[0][i], found[1][i], found[2][i], found[3][i]) = ratecontrol.bisect_by_quality(sse_of, nb_points, int(first[i]),
                                                                                                 int(plane_thresholds[i]))
            found[5][i] = sse_of(int(found[0][i]))
        return found

    of_cb = search(planes[1], chroma_ladder, chroma_thresholds)
    of_cr = search(planes[2], chroma_ladder, chroma_thresholds)
    luma_thresholds = ratecontrol.colour_luma_max_sse(thresholds, of_cb[5], of_cr[5])
    of_y = search(planes[0], ladder, luma_thresholds)
    every = (of_y, of_cb, of_cr)
    info = {key: numpy.stack([found[at] for found in every], axis=1)
            for (at, key) in enumerate(('rate_point', 'plane_met', 'probe_points', 'probe_sse', 'first_point', 'sse'))}
    info.update({'plane_max_sse': numpy.stack([luma_thresholds, chroma_thresholds, chroma_thresholds], axis=1), 'max_sse': thresholds,
                 'plane_blob_bytes': numpy.zeros((nb_images, 3), dtype=numpy.int64)})
    host_planes = [plane.cpu().numpy() for plane in planes]
    blobs = []
    for i in range(nb_images):
        plane_blobs = []
        for (which, (plane, plane_ladder)) in enumerate(zip(host_planes, (ladder, chroma_ladder, chroma_ladder))):
            k = int(info['rate_point'][i, which])
            more = {} if plane_ladder.rdo_lambdas is None else {'rdo_lambda': plane_ladder.rdo_lambdas[k]}
            plane_blobs.append(encode_images(plane[i:i + 1], encoder, plane_ladder.bin_widths_points[k], plane_ladder.map_mean,
                                             plane_ladder.binary_probabilities_points[k], plane_ladder.idx_map_exception, pad=True, **more)[0])
            info['plane_blob_bytes'][i, which] = len(plane_blobs[which])
        blobs.append(assemble_colour_blob(rgb.shape[1:3], *plane_blobs))
    info['blob_bytes'] = numpy.array([len(blob) for blob in blobs], dtype=numpy.int64)
    info['picture_sse'] = info['sse'].sum(axis=1)
    info['met'] = info['picture_sse'] <= thresholds
    return blobs, info


def decode_colour_images(blob, decoder, tile=None):
    """EAC1 blob + pipeline.DeviceDecoder of the model -> uint8 (N, h, w, 3) RGB: `decode_images` of each plane, merged on the device
    (device.colour_merge_420: `colour.merge_420_numpy` of the three reconstructions)."""
    (header, *plane_blobs) = split_colour_blob(blob)
    planes = [torch.from_numpy(decode_images(plane_blob, decoder, tile=tile)).to(decoder.device) for plane_blob in plane_blobs]
    (rgb, _) = dev.colour_merge_420(*planes, (header['image_height'], header['image_width']))
    return rgb.cpu().numpy()


# ---- crops of colour pictures ---------------------------------------------------------------------------------

class _FileRange(object):
    """The bytes [start, start + length) of a seekable binary file as a read-only seekable file of their own: what `_source_header`,
    `_read_ranges` and `codec.RegionSource` need of a file, so that a plane blob inside an EAC1 file is read in place."""

    def __init__(self, f, start, length):
        (self._file, self._start, self._length, self._pos) = (f, int(start), int(length), 0)

    def seek(self, offset, whence=0):
        pos = int(offset) + (0 if whence == 0 else (self._pos if whence == 1 else self._length))
        if whence not in (0, 1, 2) or pos < 0:
            raise ValueError('A seek in front of the range, or of an unknown kind.')
        self._pos = pos
        return pos

    def tell(self):
        return self._pos

    def read(self, count=-1):
        left = max(self._length - self._pos, 0)
        count = left if count is None or count < 0 else min(int(count), left)
        self._file.seek(self._start + self._pos)
        data = self._file.read(count)
        self._pos += len(data)
        return data


def colour_source(source):
    """An EAC1 container given as a bytes-like blob or as a seekable binary file object -> (`read_colour_header`'s header, the three
    plane sources Y, Cb, Cr), each a source `fetch_region`, `decode_region` and `codec.RegionSource` take: a memoryview of the plane's
    bytes, or a view of its byte range of the file. Of a file only the 48 bytes of the header are read here."""
    if not hasattr(source, 'read'):
        blob = memoryview(source).cast('B')
        header = _colour_header(blob, len(blob))
        return header, tuple(blob[start:start + count] for (start, count) in zip(header['plane_offsets'], header['plane_bytes']))
    source.seek(0, 2)
    total = source.tell()
    header = _colour_header(_read_at(source, 0, min(_COLOUR_HEADER.size, total)), total)
    return header, tuple(_FileRange(source, start, count) for (start, count) in zip(header['plane_offsets'], header['plane_bytes']))


def check_colour_planes(header, plane_headers):
    """`_check_planes` on parsed plane headers: every plane of an EAC1 container holds the header's image count at its plane's real
    size. Raises ValueError."""
    sizes = _plane_sizes((header['image_height'], header['image_width']))
    for (name, size, fields) in zip(_PLANE_NAMES, sizes, plane_headers):
        if fields['nb_images'] != header['nb_images']:
            raise ValueError('The {0} plane holds {1} images, not {2}.'.format(name, fields['nb_images'], header['nb_images']))
        if (fields['image_height'], fields['image_width']) != size:
            raise ValueError('The {0} plane of a {1} x {2} picture is {3} x {4}, not {5} x {6}.'.format(
                name, header['image_height'], header['image_width'], size[0], size[1], fields['image_height'], fields['image_width']))


def decode_colour_region(source, decoder, region, images=None, tile=None):
    """The pixels region = (y0, x0, height, width) of the pictures `images` (indices, default all) of an EAC1 container -> uint8
    [N_sel, height, width, 3] RGB, equal to decode_colour_images(blob, decoder)[images, y0:y0 + height, x0:x0 + width].
    `source`: a bytes-like EAC1 blob, or a seekable binary file object, of which only the 48-byte header, the three plane headers
    and the byte ranges the three `region_plan`s name are read (an EAE1 plane, whose maps are coded whole, is read whole).
    `decode_region` on Y at `region` and on Cb and Cr at `colour.chroma_region`'s rectangle, then one
    `device.colour_merge_420_crops` launch (`colour.merge_420_region_numpy`). Raises ValueError for a region that is empty or leaves
    the picture. tile: as `decode_region`'s."""
    (header, planes) = colour_source(source)
    (h, w) = (header['image_height'], header['image_width'])
    if not isinstance(region, (tuple, list)) or len(region) != 4 or \
            any(not isinstance(x, numbers.Integral) or isinstance(x, bool) for x in region):
        raise ValueError('`region` must be (y0, x0, height, width) in integers.')
    (y0, x0, rh, rw) = (int(x) for x in region)
    ((rch, rcw), (cy0, cx0)) = colour_rules.chroma_region(h, w, (rh, rw), y0, x0)
    chroma = (cy0, cx0, rch, rcw)
    # everything is read and checked before anything is decoded
    fetched = [fetch_region(plane, where, images) for (plane, where) in zip(planes, ((y0, x0, rh, rw), chroma, chroma))]
    check_colour_planes(header, [plane_header for (plane_header, _, _) in fetched])
    crops = [torch.from_numpy(numpy.ascontiguousarray(_decode_fetched(*plane, decoder, tile))).to(decoder.device) for plane in fetched]
    n = crops[0].shape[0]
    origins = torch.tensor([[y0, x0]]*n, dtype=torch.int32, device=decoder.device)
    out = torch.empty(dev.colour_words_bytes(n, rh, rw), dtype=torch.uint8, device=decoder.device)
    dev.colour_merge_420_crops(*crops, (h, w), origins, out)
    return out[:n*rh*rw*3].view(n, rh, rw, 3).cpu().numpy()
