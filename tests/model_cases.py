"""Model parameters shaped like a TRAINED model's, shared by the CPU tests of the oracle (tests/test_oracle_transforms.py), the
checkpoint round trip (tests/test_tf_checkpoint.py) and the GPU parity tests of every normalisation path
(tests/test_gpu_trained_like.py).

`variables.random_variables` is the reference's INITIALISATION: every `gamma` is symmetric (0.5*(U + U.T), tfutils.py:445-478)
and every `beta` is 1. Training keeps neither: `gamma` is a free 128 x 128 variable used as `matmul(x**2, gamma)`
(tfutils.py:393-397, 505-509), i.e. d[c] = sum_k x[k]^2 * gamma[k][c], and `beta` becomes one number per channel. With symmetric
`gamma` and constant `beta` a kernel, packer or oracle that reads gamma[c][k], or beta in the kernels' packed channel order, gives
the same result; with the parameters made here it does not. Everything is derived from seeds; nothing needs the reference."""
import numpy

from autoencoder_based_image_compression_amd.kodak.eae.graph import constants as csts
from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var


def trained_like_variables(bin_width_init, are_bin_widths_learned, seed, bias_std=0.01):
    """`random_variables` with every `gamma` and `beta` replaced:
    gamma = the symmetric initialisation x a per-row factor U[0.1, 4] x an elementwise factor U[0.5, 2], about 5 % of the entries
    then at the reference's lower clip `MIN_GAMMA_BETA` (2e-5) and the whole matrix floored there: float32, strictly positive,
    strongly asymmetric; beta ~ U[0.25, 4] per channel with every 17th channel at `MIN_GAMMA_BETA`. All of it stays inside the
    range in which `gdn_tile` (csrc/hip/common.h) takes its short square root and division, as a real model's parameters do."""
    v = var.random_variables(bin_width_init, are_bin_widths_learned, seed=seed, bias_std=bias_std)
    rng = numpy.random.RandomState(0 if seed is None else seed + 100003)       # a stream of its own: the rest stays as random_variables gives it
    floor = numpy.float32(csts.MIN_GAMMA_BETA)
    for name in sorted(v):
        leaf = name.split('/')[1]
        if leaf.startswith('gamma_'):
            g = v[name].astype(numpy.float64)*rng.uniform(0.1, 4., size=(128, 1))*rng.uniform(0.5, 2., size=(128, 128))
            g[rng.uniform(size=(128, 128)) < 0.05] = floor
            v[name] = numpy.maximum(g.astype(numpy.float32), floor)
        elif leaf.startswith('beta_'):
            b = rng.uniform(0.25, 4., size=128).astype(numpy.float32)
            b[::17] = floor
            v[name] = b
    return v


def asymmetry(gamma):
    """Median of |g - g.T| / (g + g.T): 0 for a symmetric matrix."""
    g = gamma.astype(numpy.float64)
    return float(numpy.median(numpy.abs(g - g.T)/(g + g.T)))


def gdn_float64(x, gamma, beta, inverse=False):
    """The definition (tfutils.py:393-397, 505-509) in float64: x / sqrt(matmul(x**2, gamma) + beta), or x * sqrt(...)."""
    x = numpy.asarray(x, dtype=numpy.float64)
    s = numpy.sqrt(numpy.matmul(x**2, numpy.asarray(gamma, dtype=numpy.float64)) + numpy.asarray(beta, dtype=numpy.float64))
    return x*s if inverse else x/s


def packed_channel_order():
    """perm with packed[..., perm[c]] = plain[..., c] (csrc/hip/common.h: packed_channel)."""
    c = numpy.arange(128)
    return (c % 32)*4 + c//32


# ---- the wrong indexings that symmetric gamma and constant beta cannot see ----------------------------------------------------
def gamma_transposed(gamma):
    return numpy.ascontiguousarray(gamma.T)


def beta_rolled(beta):
    return numpy.roll(beta, 1)


def beta_in_packed_order(beta):
    """What a kernel reads that indexes the natural-order `beta` with a packed channel number."""
    return numpy.ascontiguousarray(beta[packed_channel_order()])


def fraction_beyond(a, b, rel=1e-3):
    """Fraction of the elements at which `a` differs from `b` by more than rel*|b|."""
    return float(numpy.mean(numpy.abs(a - b) > rel*numpy.abs(b)))


def quantize(y, bin_widths, map_mean):
    """numpy restatement of the quantiser (reconstructing_eae_kodak.py:178-192 + tools.py:927-929 + compression.py:142; the one
    of tests/test_gpu_kernels.py::test_quantize_maps_and_histograms) in float32: y [N,h,w,128] -> dict with 'cq', 'shifted',
    'symbols' (int16, planar [N,128,h*w]), 'nonzero_flags' ([N,128], 1 where a map has a non-zero symbol) and the three 'checks'."""
    shape = y.shape[:3]
    mean = numpy.tile(map_mean.astype(numpy.float32), shape + (1,))
    tiled = numpy.tile(bin_widths.astype(numpy.float32).reshape(1, 1, 1, 128), shape + (1,))
    centered = y - mean
    cq = tiled*numpy.round(centered/tiled)
    rounded = numpy.round(cq/tiled)
    sym = rounded.astype(numpy.int16)
    checks = [int((~(numpy.abs(rounded) < numpy.float32(32768.))).sum()),
              int((~(numpy.abs(cq.astype(numpy.float64) - centered.astype(numpy.float64)) < 1.5e-10)).sum()),
              int((~(sym.astype(numpy.float32)*tiled == centered)).sum())]
    return {'cq': cq, 'shifted': cq + mean, 'symbols': numpy.ascontiguousarray(sym.reshape(shape[0], -1, 128).transpose(0, 2, 1)),
            'nonzero_flags': (cq != 0).any(axis=(1, 2)).astype(numpy.int32), 'checks': checks}
