"""Inputs and the host-side reference of tests/test_gpu_unary_lengths.py (a plain helper module: import it, no fixture lives here).

The truncated unary length L is the number of columns of the probability table. It sizes the coder's decision capacity, stream
stride and LDS, chooses between the 64-maps-per-wavefront kernels (L <= 32) and the general one, and moves every offset behind the
table in the resident codecs' slots and step heads. This module fixes the lengths, the bin width of each, and a reference that
depends on NO kernel under test: numpy for the quantiser, the histograms, the probability rows and the squared error, and the host
coder (`eae_coder_encode_maps`, itself pinned to the compiled reference at random L by tests/test_oracle_coder.py) for the streams.
Everything here is numpy and the host library: it needs no GPU. The latents it starts from are `pipeline.DeviceEncoder`'s, which
other modules pin bit for bit to the oracle; the caller brings them.
"""
import numpy

NB_MAPS = 128
BATCH = 3
# 1: one context, every non-zero symbol escapes; 2 / 3: even and odd parity of every 8*L-byte row of the table; 31 / 32 / 33: the
# last two lengths of the 64-maps-per-wavefront kernels and the first of the general kernel; 255: the top of the accepted range
LENGTHS = (1, 2, 3, 31, 32, 33, 255)
# one bin width per length, chosen so that both sides of the prefix / suffix split are populated (`populations`)
BIN_WIDTH = {1: 1.0, 2: 1.0, 3: 0.05, 31: 0.05, 32: 0.05, 33: 0.05, 255: 0.005}
WHOLE_SHAPE = (64, 96)            # latents 4 x 6: the whole-map paths
TILED_SHAPE = (176, 208)          # latents 11 x 13 in tiles of (4, 4): four shape classes (tests/test_gpu_region_decoder.py)
CODING_TILE = (4, 4)
EXCEPTION_MAPS = (67, -1)
HIST_RADIUS = 2047                # `codec.BatchCodec`'s default
# the shares of symbols a case must have on each side of the split: the Exp-Golomb route, and a prefix that stops early
MIN_SHARE_ESCAPED = 0.05
MIN_SHARE_INSIDE = 0.03


def host_encode_maps(planar, probs, prob_row):
    from autoencoder_based_image_compression_amd import _native
    lib = _native.coder()
    (n, size) = planar.shape
    L = probs.shape[1]
    stride = int(_native.hip().eae_hip_coder_stream_stride_bytes(size, L))
    streams = numpy.zeros((n, stride), dtype=numpy.uint8)
    (bac, byp) = (numpy.zeros(n, dtype=numpy.uint32), numpy.zeros(n, dtype=numpy.uint32))
    (status, stage) = (numpy.zeros(n, dtype=numpy.int32), numpy.zeros(n, dtype=numpy.int32))
    pp = numpy.ascontiguousarray(probs, dtype=numpy.float64)
    rows = numpy.ascontiguousarray(prob_row, dtype=numpy.int32)
    planar = numpy.ascontiguousarray(planar)
    lib.eae_coder_encode_maps(n, size, _native.ptr(planar, _native.c_i16p), L, _native.ptr(pp, _native.c_f64p),
                              _native.ptr(rows, _native.c_i32p), _native.ptr(streams, _native.c_u8p), stride,
                              _native.ptr(bac, _native.c_u32p), _native.ptr(byp, _native.c_u32p),
                              _native.ptr(status, _native.c_i32p), _native.ptr(stage, _native.c_i32p), 4)
    assert not status.any()
    return streams, stride, bac, byp


def variables():
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    v = var.random_variables(1., False, seed=4, bias_std=0.01)
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    return v


def map_mean():
    return numpy.random.RandomState(96).normal(scale=0.1, size=NB_MAPS).astype(numpy.float32)


def bin_widths(length):
    return numpy.full(NB_MAPS, BIN_WIDTH[length], dtype=numpy.float32)


def quantise(latents, widths, mean):
    """The quantiser restated in numpy, float32 throughout: latents float32 [N, h, w, 128] -> int16 symbols [N, 128, h, w]."""
    assert latents.dtype == numpy.float32 and widths.dtype == numpy.float32 and mean.dtype == numpy.float32
    centered_quantised = widths*numpy.rint((latents - mean)/widths)
    symbols = numpy.rint(centered_quantised/widths)
    assert symbols.dtype == numpy.float32 and numpy.abs(symbols).max() < 32767
    return numpy.ascontiguousarray(symbols.astype(numpy.int16).transpose(0, 3, 1, 2))


def dequantise(symbols, widths, mean):
    """int16 symbols [N, 128, h, w] -> float32 [N, h, w, 128]: bin width * float32(symbol), then + mean, each rounded to float32."""
    return numpy.ascontiguousarray(widths*symbols.transpose(0, 2, 3, 1).astype(numpy.float32) + mean)


def fitted_table(symbol_sets, length):
    """The probability table of a case, fitted to its own symbols (all images of all sets): per map the histogram of min(|s|, L),
    then `ratecontrol.decision_counts` and `probabilities_from_counts`. An INPUT of the case, not a reference: a random table
    overflows 50 to 70 of 384 streams at L >= 31 already on the host."""
    from autoencoder_based_image_compression_amd import ratecontrol
    hist = numpy.zeros((NB_MAPS, length + 1), dtype=numpy.int64)
    for symbols in symbol_sets:
        clipped = numpy.minimum(numpy.abs(symbols.astype(numpy.int64)), length)
        for m in range(NB_MAPS):
            hist[m] += numpy.bincount(clipped[:, m].reshape(-1), minlength=length + 1)
    table = ratecontrol.probabilities_from_counts(*ratecontrol.decision_counts(hist))
    assert table.shape == (NB_MAPS, length) and table.dtype == numpy.float64 and ((table > 0.) & (table < 1.)).all()
    return table


def populations(symbol_sets, length):
    """(share of symbols with |s| >= L, share with 0 < |s| < L) over all images of all sets."""
    magnitudes = numpy.concatenate([numpy.abs(symbols.astype(numpy.int64)).reshape(-1) for symbols in symbol_sets])
    return float((magnitudes >= length).mean()), float(((magnitudes > 0) & (magnitudes < length)).mean())


def exception_rows(symbols, idx_map_exception, length, radius=HIST_RADIUS):
    """One probability row per image for its exception map: the numpy `_rows_reference` of tests/test_gpu_codec_container.py on the
    numpy histogram of the whole map over [-radius, radius] and the count of the symbols beyond it. float64 [N, L]; [0, L] without
    an exception map."""
    from test_gpu_codec_container import _rows_reference
    if idx_map_exception < 0:
        return numpy.zeros((0, length), dtype=numpy.float64)
    radius = max(int(radius), length)
    maps = symbols[:, idx_map_exception].reshape(symbols.shape[0], -1).astype(numpy.int64)
    inside = numpy.abs(maps) <= radius
    hist = numpy.stack([numpy.bincount(row[keep] + radius, minlength=2*radius + 1) for (row, keep) in zip(maps, inside)])
    overflow = (~inside).sum(axis=1)
    return _rows_reference(hist, overflow, maps.shape[1], length)


def exception_bits(symbols, idx_map_exception):
    """What the reference charges for the exception map of every image: ceil(map size * entropy of its symbols), int64 [N]."""
    out = numpy.zeros(symbols.shape[0], dtype=numpy.int64)
    if idx_map_exception < 0:
        return out
    for (i, row) in enumerate(symbols[:, idx_map_exception].reshape(symbols.shape[0], -1).astype(numpy.int64)):
        counts = numpy.bincount(row - row.min())
        frequency = counts[counts != 0].astype(numpy.float64)/row.size
        out[i] = int(numpy.ceil(row.size*-numpy.sum(frequency*numpy.log2(frequency))))
    return out


def tile_grid(h, w, coding_tile):
    """[(r0, c0, rows, cols)] of the plain grid of coding tiles, row-major, edge tiles smaller; None: one tile, the whole map."""
    if coding_tile is None:
        return [(0, 0, h, w)]
    (th, tw) = coding_tile
    return [(r0, c0, min(th, h - r0), min(tw, w - c0)) for r0 in range(0, h, th) for c0 in range(0, w, tw)]


def host_reference(symbols, table, idx_map_exception, coding_tile):
    """The host coder on every (image, tile)'s symbols, sliced by numpy, in the container's payload order (image -> tile, row-major
    -> map -> arithmetic-coded bytes, bypass bytes). The exception map is coded with its image's own row, measured on the whole map.
    -> {'bits' uint32 [N, tiles, 128, 2], 'payload' bytes, 'image_payloads' [bytes], 'tile_payloads' {(image, tile): bytes},
    'exception_rows' float64 [N or 0, L]}. `host_encode_maps` asserts status 0 for every map."""
    (n, nb_maps, h, w) = symbols.shape
    length = table.shape[1]
    rows = exception_rows(symbols, idx_map_exception, length)
    full_table = numpy.concatenate([table, rows])
    tiles = tile_grid(h, w, coding_tile)
    bits = numpy.zeros((n, len(tiles), nb_maps, 2), dtype=numpy.uint32)
    (image_payloads, tile_payloads) = ([], {})
    for i in range(n):
        prob_row = numpy.arange(nb_maps, dtype=numpy.int32)
        if idx_map_exception >= 0:
            prob_row[idx_map_exception] = nb_maps + i
        pieces = []
        for (t, (r0, c0, nr, nc)) in enumerate(tiles):
            planar = symbols[i, :, r0:r0 + nr, c0:c0 + nc].reshape(nb_maps, nr*nc)
            (streams, stride, bac, byp) = host_encode_maps(planar, full_table, prob_row)
            (bits[i, t, :, 0], bits[i, t, :, 1]) = (bac, byp)
            # map by map, the bytes of the arithmetic-coded stream (from 0 on), then those of the bypass stream (from stride/2 on)
            column = numpy.arange(stride, dtype=numpy.int64)[None, :]
            (nbac, nbyp) = ((bac.astype(numpy.int64)[:, None] + 7)//8, (byp.astype(numpy.int64)[:, None] + 7)//8)
            assert int(nbac.max()) <= stride//2 and int(nbyp.max()) <= stride//2
            tile_payloads[(i, t)] = streams[(column < nbac) | ((column >= stride//2) & (column < stride//2 + nbyp))].tobytes()
            pieces.append(tile_payloads[(i, t)])
        image_payloads.append(b''.join(pieces))
    return {'bits': bits, 'payload': b''.join(image_payloads), 'image_payloads': image_payloads, 'tile_payloads': tile_payloads,
            'exception_rows': rows}


def coder_bits(bits, idx_map_exception):
    """What a ticket reports as 'coder_bits': both streams of every tile and map of an image but its exception map. int64 [N]."""
    per_map = bits.astype(numpy.int64).sum(axis=3)
    if idx_map_exception >= 0:
        per_map[:, :, idx_map_exception] = 0
    return per_map.sum(axis=(1, 2))


def dead_maps(symbols):
    """Maps of every image all of whose symbols are zero. int64 [N]."""
    return (~(symbols != 0).any(axis=(2, 3))).sum(axis=1).astype(numpy.int64)


def squared_errors(images, reconstruction):
    difference = images.astype(numpy.int64) - reconstruction.astype(numpy.int64)
    return (difference*difference).sum(axis=(1, 2))


def check_blob(blob, reference, images, length, widths, mean, table, idx_map_exception, coding_tile, learned=False):
    """A blob against the host reference: every field `read_header` gives equals the inputs and the host coder's counts, and the
    payload is the host streams one behind the other, byte for byte."""
    from autoencoder_based_image_compression_amd import container
    header = container.read_header(blob)
    (n, height, width) = images.shape
    assert blob[:4] == (b'EAE1' if coding_tile is None else b'EAT1')
    assert (header['nb_images'], header['height'], header['width'], header['nb_maps']) == (n, height, width, NB_MAPS)
    assert header['truncated_unary_length'] == length and header['idx_map_exception'] == idx_map_exception
    assert header['are_bin_widths_learned'] == learned
    assert header.get('coding_tile') == coding_tile
    assert header['bin_widths'].tobytes() == widths.tobytes() and header['map_mean'].tobytes() == mean.tobytes()
    assert header['binary_probabilities'].shape == (NB_MAPS, length) and header['binary_probabilities'].tobytes() == table.tobytes()
    assert header['exception_probabilities'].shape == reference['exception_rows'].shape
    assert header['exception_probabilities'].tobytes() == reference['exception_rows'].tobytes()
    bits = reference['bits'] if coding_tile is not None else reference['bits'].reshape(-1, 2)
    assert header['bits'].shape == bits.shape and numpy.array_equal(header['bits'], bits)
    assert blob[header['payload_offset']:] == reference['payload']
    return header
