"""Colour pictures as three planes, 4:2:0: the rules, in numpy. No GPU is needed here.

An RGB picture of h x w becomes a luminance plane Y of h x w and two chrominance planes Cb, Cr of hc x wc = ceil(h/2) x ceil(w/2);
each plane is then coded through the luminance autoencoder like any luminance image (`container.encode_colour_images`,
`codec.ColourCodec`). The device kernels (`device.colour_split_420`, `device.colour_merge_420`; csrc/hip/colour.hip) are held
against the functions of this module bit for bit.

Forward, `split_420_numpy`: per pixel, (Y, Cb, Cr) is `kodak.tools.tools.rgb_to_ycbcr` -- ITU-R BT.601 in float64, the terms
added left to right, clipped to [0, 255], rounded by `numpy.round`. The full-resolution Cb and Cr planes are extended to even
sides by edge replication and every chroma sample is (a + b + c + d + 2) >> 2 over its 2 x 2 block. No clamp is applied to chroma:
values up to 240 go into the chroma codec, while the synthesis side's `cast_bt601` returns 235 at most -- a limit of the model's
cast, which this layer does not hide.

Inverse, `merge_420_numpy`, in integers only: chroma is upsampled centre-sited, weights 3:1 in both directions, the neighbours
clamped at the real chroma size; then the 8-bit integer BT.601 inverse with an arithmetic (flooring) shift.
"""
import numpy


def chroma_size(height, width):
    """The size of the Cb and Cr planes of a height x width picture."""
    return ((int(height) + 1)//2, (int(width) + 1)//2)


def _checked_rgb(rgb, what):
    rgb = numpy.asarray(rgb)
    if rgb.dtype != numpy.uint8:
        raise TypeError('`{}.dtype` is not equal to `numpy.uint8`.'.format(what))
    if rgb.ndim != 4 or rgb.shape[3] != 3 or 0 in rgb.shape:
        raise ValueError('`{}` must be (N, h, w, 3) and hold a pixel.'.format(what))
    return rgb


def ycbcr_numpy(rgb):
    """uint8 (..., 3) RGB -> uint8 (..., 3) YCbCr: `kodak.tools.tools.rgb_to_ycbcr` on any leading shape, on the host."""
    (r, g, b) = (rgb[..., k].astype(numpy.float64) for k in range(3))
    y = 16. + (65.481/255.)*r + (128.553/255.)*g + (24.966/255.)*b
    cb = 128. - (37.797/255.)*r - (74.203/255.)*g + (112./255.)*b
    cr = 128. + (112./255.)*r - (93.786/255.)*g - (18.214/255.)*b
    return numpy.round(numpy.stack((y, cb, cr), axis=-1).clip(min=0., max=255.)).astype(numpy.uint8)


def split_420_numpy(rgb):
    """uint8 (N, h, w, 3) -> (y (N, h, w), cb (N, hc, wc), cr (N, hc, wc)), all uint8 (module docstring)."""
    rgb = _checked_rgb(rgb, 'rgb')
    (_, h, w, _) = rgb.shape
    ycbcr = ycbcr_numpy(rgb)
    chroma = numpy.pad(ycbcr[..., 1:], ((0, 0), (0, h % 2), (0, w % 2), (0, 0)), mode='edge').astype(numpy.int32)
    means = (chroma[:, 0::2, 0::2] + chroma[:, 0::2, 1::2] + chroma[:, 1::2, 0::2] + chroma[:, 1::2, 1::2] + 2) >> 2
    means = means.astype(numpy.uint8)
    return (numpy.ascontiguousarray(ycbcr[..., 0]), numpy.ascontiguousarray(means[..., 0]), numpy.ascontiguousarray(means[..., 1]))


def _upsampled(plane, h, w):
    """uint8 (N, hc, wc) -> int32 (N, h, w): centre-sited, 3:1 both ways, neighbours clamped at the plane's own size."""
    (hc, wc) = plane.shape[1:]
    p = plane.astype(numpy.int32)
    (r, c) = (numpy.arange(h), numpy.arange(w))
    (i, j) = (r >> 1, c >> 1)
    i2 = numpy.clip(i + numpy.where(r & 1, 1, -1), 0, hc - 1)
    j2 = numpy.clip(j + numpy.where(c & 1, 1, -1), 0, wc - 1)
    (i, i2, j, j2) = (i[:, None], i2[:, None], j[None, :], j2[None, :])
    return (9*p[:, i, j] + 3*p[:, i, j2] + 3*p[:, i2, j] + p[:, i2, j2] + 8) >> 4


def merge_420_numpy(y, cb, cr):
    """uint8 y (N, h, w), cb and cr (N, hc, wc) -> uint8 (N, h, w, 3) RGB, in integers only (module docstring)."""
    (y, cb, cr) = (numpy.asarray(plane) for plane in (y, cb, cr))
    if y.dtype != numpy.uint8 or cb.dtype != numpy.uint8 or cr.dtype != numpy.uint8:
        raise TypeError('The planes must be `numpy.uint8`.')
    if y.ndim != 3 or 0 in y.shape:
        raise ValueError('`y` must be (N, h, w) and hold a pixel.')
    (n, h, w) = y.shape
    if cb.shape != (n,) + chroma_size(h, w) or cr.shape != cb.shape:
        raise ValueError('`cb` and `cr` must be (N, ceil(h/2), ceil(w/2)).')
    scaled = 298*(y.astype(numpy.int32) - 16)
    u = _upsampled(cb, h, w) - 128
    v = _upsampled(cr, h, w) - 128
    rgb = numpy.stack(((scaled + 409*v + 128) >> 8, (scaled - 100*u - 208*v + 128) >> 8, (scaled + 516*u + 128) >> 8), axis=-1)
    return numpy.clip(rgb, 0, 255).astype(numpy.uint8)


def chroma_region(h, w, region, y0, x0):
    """((rch, rcw), (cy0, cx0)): the chroma rectangle the crop of region = (rh, rw) pixels at pixel (y0, x0) of an h x w picture needs
    (DESIGN.md section 28). Its SIZE depends on the region and the picture alone -- half the region, the sample a crop that starts at
    an odd pixel shares with its neighbour, and one sample on either side for the 3:1 neighbours, at most the plane --, so a resident
    decoder is built for it; its origin is one sample in front of the crop's first, clamped into the plane. Every sample
    `merge_420_numpy` reads for the crop's pixels, the clamped neighbours included, lies inside."""
    (rh, rw) = (int(region[0]), int(region[1]))
    (y0, x0) = (int(y0), int(x0))
    if rh < 1 or rw < 1 or y0 < 0 or x0 < 0 or y0 + rh > h or x0 + rw > w:
        raise ValueError('The region {0} is empty or leaves the {1} x {2} picture.'.format((y0, x0, rh, rw), h, w))
    (hc, wc) = chroma_size(h, w)
    (rch, rcw) = (min(hc, rh//2 + 3), min(wc, rw//2 + 3))
    return ((rch, rcw), (min(max((y0 >> 1) - 1, 0), hc - rch), min(max((x0 >> 1) - 1, 0), wc - rcw)))


def merge_420_region_numpy(y_crop, cb_crop, cr_crop, image_size, origins):
    """uint8 y_crop (n, rh, rw), cb_crop and cr_crop (n, rch, rcw), origins int (n, 2) -> uint8 (n, rh, rw, 3): crop k is the pixels
    [y0, y0 + rh) x [x0, x0 + rw), (y0, x0) = origins[k], of an image_size = (h, w) picture, its chroma crops the rectangle
    `chroma_region` names. The samples, the parity of the weights and the clamp of the neighbours are those of the pixel's position
    in the PICTURE (`merge_420_numpy`); every chroma index is then shifted by the crop's chroma origin. Equal to
    `merge_420_numpy(full planes)[k, y0:y0 + rh, x0:x0 + rw]` for crops cut out of full planes."""
    (y_crop, cb_crop, cr_crop) = (numpy.asarray(plane) for plane in (y_crop, cb_crop, cr_crop))
    if y_crop.dtype != numpy.uint8 or cb_crop.dtype != numpy.uint8 or cr_crop.dtype != numpy.uint8:
        raise TypeError('The planes must be `numpy.uint8`.')
    if y_crop.ndim != 3 or 0 in y_crop.shape:
        raise ValueError('`y_crop` must be (n, rh, rw) and hold a pixel.')
    (n, rh, rw) = y_crop.shape
    (h, w) = (int(image_size[0]), int(image_size[1]))
    (hc, wc) = chroma_size(h, w)
    origins = numpy.asarray(origins)
    if origins.shape != (n, 2) or origins.dtype.kind not in 'iu':
        raise ValueError('`origins` must be (n, 2) in integers.')
    out = numpy.empty((n, rh, rw, 3), dtype=numpy.uint8)
    for k in range(n):
        (y0, x0) = (int(origins[k, 0]), int(origins[k, 1]))
        ((rch, rcw), (cy0, cx0)) = chroma_region(h, w, (rh, rw), y0, x0)
        if cb_crop.shape != (n, rch, rcw) or cr_crop.shape != cb_crop.shape:
            raise ValueError('`cb_crop` and `cr_crop` must be (n, {0}, {1}): `chroma_region`.'.format(rch, rcw))
        (r, c) = (y0 + numpy.arange(rh), x0 + numpy.arange(rw))
        (i, j) = (r >> 1, c >> 1)
        i2 = numpy.clip(i + numpy.where(r & 1, 1, -1), 0, hc - 1)
        j2 = numpy.clip(j + numpy.where(c & 1, 1, -1), 0, wc - 1)
        (i, i2, j, j2) = ((i - cy0)[:, None], (i2 - cy0)[:, None], (j - cx0)[None, :], (j2 - cx0)[None, :])
        scaled = 298*(y_crop[k].astype(numpy.int32) - 16)
        (u, v) = ((9*p[i, j] + 3*p[i, j2] + 3*p[i2, j] + p[i2, j2] + 8 >> 4) - 128
                  for p in (cb_crop[k].astype(numpy.int32), cr_crop[k].astype(numpy.int32)))
        rgb = numpy.stack(((scaled + 409*v + 128) >> 8, (scaled - 100*u - 208*v + 128) >> 8, (scaled + 516*u + 128) >> 8), axis=-1)
        out[k] = numpy.clip(rgb, 0, 255)
    return out


def sse_rgb_numpy(rgb, rec):
    """int64 (N,): the exact squared error of every picture over its 3 h w samples."""
    rgb = _checked_rgb(rgb, 'rgb')
    rec = _checked_rgb(rec, 'rec')
    if rgb.shape != rec.shape:
        raise ValueError('`rgb` and `rec` do not have the same shape.')
    difference = rgb.astype(numpy.int64) - rec.astype(numpy.int64)
    return (difference*difference).sum(axis=(1, 2, 3))


def psnr_from_sse(sse, nb_samples):
    """10 log10(255^2 nb_samples / sse) in float64 (inf where sse is 0)."""
    sse = numpy.asarray(sse, dtype=numpy.float64)
    with numpy.errstate(divide='ignore'):
        return 10.*numpy.log10(255.**2*float(nb_samples)/sse)
