// colour.hip -- colour images, 4:2:0: the two launches that stand between an RGB picture and the three planes
// the luminance codecs take (colour.py states both in numpy; tests/test_gpu_colour_kernels.py holds the kernels to it bit for bit).
//   eae_hip_colour_split_420: rgb u8 [n][h][w][3] (device or pinned host memory, any byte address) -> y u8 [n][h][w] and cb, cr u8
//     [n][hc][wc], hc = ceil(h / 2), wc = ceil(w / 2): BT.601 in float64 per pixel (bt601.h), chroma the rounded mean of its 2 x 2 block,
//     the block completed by edge replication at an odd side.
//   eae_hip_colour_merge_420: y u8 [n][H][W], cb, cr u8 [n][Hc][Wc], of which the top-left h x w / hc x wc are read -> rgb u8
//     [n][h][w][3] and / or sse[i] += the squared error against a reference picture: chroma upsampled 3:1 centre-sited with the
//     neighbours clamped at the real chroma size, then the integer BT.601 inverse.
// In both a lane owns one chroma sample, i.e. a 2 x 2 block of pixels: 12 bytes of the picture, six contiguous ones in each of two
// rows, so a wave covers 384 contiguous bytes of a row. A block lies inside one image (blocks_per_image blocks of 256 samples each):
// the image index is a division of the block index, the offset of the image 64 bits wide, everything inside an image 32 bits. The
// grids are one chroma sample per lane, whatever the size, with ONE exception: a merge that takes the squared error ends every block
// in an atomic on its image's word, so an image then gets MERGE_SSE_BLOCKS_PER_IMAGE blocks at most, which loop over its samples
// (384 atomics per word for a 512 x 768 picture took 98 us against 26 us for the same launch without the error).
#include "bt601.h"
#include "byte_runs.h"
#include "common.h"

namespace {

struct ColourShape {
    uint32_t n, h, w, hc, wc;          // pictures, their real size, the real size of their chroma planes
    uint32_t H, W, Hc, Wc;             // merge: the strides of the planes read (the coded sizes); split: h, w, hc, wc
    uint32_t blocks_per_image;
};

// The two pixels at p .. p + 5, inside [begin, end): (r0 | g0 << 8 | b0 << 16, r1 | g1 << 8 | b1 << 16)
__device__ __forceinline__ void load_two_pixels(const uint8_t* begin, const uint8_t* end, const uint8_t* p, uint32_t& p0, uint32_t& p1) {
    const uint32_t lo = load_run4(begin, end, p), hi = load_run4(begin, end, p + 2);      // bytes 0..3 and 2..5
    p0 = lo & 0xFFFFFFu;
    p1 = (lo >> 24) | ((hi >> 16) << 8);
}
__device__ __forceinline__ uint32_t load_pixel(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

// `count` (1 or 2) bytes to q, the low byte first; one 16-bit store where the address allows it
__device__ __forceinline__ void store_bytes2(uint8_t* q, uint32_t v, bool two) {
    if (two && (((uintptr_t)q) & 1u) == 0) {
        *reinterpret_cast<uint16_t*>(q) = (uint16_t)v;
    } else {
        q[0] = (uint8_t)v;
        if (two) q[1] = (uint8_t)(v >> 8);
    }
}

__global__ __launch_bounds__(256) void colour_split_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ y, uint8_t* __restrict__ cb,
                                                           uint8_t* __restrict__ cr, ColourShape s) {
    const uint32_t img = blockIdx.x / s.blocks_per_image, part = blockIdx.x - img * s.blocks_per_image;
    const uint32_t sample = part * 256u + threadIdx.x;
    if (sample >= s.hc * s.wc) return;
    const uint32_t i = sample / s.wc, j = sample - i * s.wc;
    const uint8_t* end = rgb + (uint64_t)s.n * s.h * s.w * 3u;
    const uint8_t* image = rgb + (uint64_t)img * s.h * s.w * 3u;
    uint8_t* luma = y + (uint64_t)img * s.h * s.w;
    const bool two_columns = 2u * j + 1u < s.w, two_rows = 2u * i + 1u < s.h;
    uint32_t sum_cb = 0, sum_cr = 0;
#pragma unroll
    for (uint32_t dy = 0; dy < 2; ++dy) {
        if (dy == 1 && !two_rows) {                     // the last row repeats downwards
            sum_cb *= 2u, sum_cr *= 2u;
            break;
        }
        const uint32_t at = (2u * i + dy) * s.w + 2u * j;
        const uint8_t* p = image + (uint64_t)at * 3u;
        uint32_t p0, p1;
        if (two_columns) {
            load_two_pixels(rgb, end, p, p0, p1);
        } else {                                        // the last column repeats to the right
            p0 = p1 = load_pixel(p);
        }
        const double r0 = (double)(p0 & 255u), g0 = (double)((p0 >> 8) & 255u), b0 = (double)(p0 >> 16);
        uint32_t y2 = bt601_y(r0, g0, b0), cb1 = bt601_cb(r0, g0, b0), cr1 = bt601_cr(r0, g0, b0);
        sum_cb += cb1, sum_cr += cr1;
        if (two_columns) {
            const double r1 = (double)(p1 & 255u), g1 = (double)((p1 >> 8) & 255u), b1 = (double)(p1 >> 16);
            y2 |= (uint32_t)bt601_y(r1, g1, b1) << 8;
            cb1 = bt601_cb(r1, g1, b1), cr1 = bt601_cr(r1, g1, b1);
        }
        sum_cb += cb1, sum_cr += cr1;
        store_bytes2(luma + at, y2, two_columns);
    }
    const uint64_t out = (uint64_t)img * s.hc * s.wc + sample;
    cb[out] = (uint8_t)((sum_cb + 2u) >> 2);
    cr[out] = (uint8_t)((sum_cr + 2u) >> 2);
}

// One chroma plane around sample (i, j): the four upsampled values of its 2 x 2 block, c[dy][dx]
__device__ __forceinline__ void upsample_block(const uint8_t* __restrict__ plane, uint32_t stride, const uint32_t (&rows)[3],
                                               const uint32_t (&columns)[3], int (&c)[2][2]) {
    int left[3], right[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint8_t* line = plane + rows[k] * stride;
        const int centre = 3 * (int)line[columns[1]];
        left[k] = centre + (int)line[columns[0]];
        right[k] = centre + (int)line[columns[2]];
    }
    c[0][0] = (3 * left[1] + left[0] + 8) >> 4;
    c[0][1] = (3 * right[1] + right[0] + 8) >> 4;
    c[1][0] = (3 * left[1] + left[2] + 8) >> 4;
    c[1][1] = (3 * right[1] + right[2] + 8) >> 4;
}

__device__ __forceinline__ uint32_t clip_u8(int x) { return (uint32_t)(x < 0 ? 0 : (x > 255 ? 255 : x)); }

// r | g << 8 | b << 16 of one pixel; `>>` on the signed sums is an arithmetic shift (v_ashrrev_i32): a floor, as numpy's
__device__ __forceinline__ uint32_t bt601_inverse(int luma, int cb_value, int cr_value) {
    const int scaled = 298 * (luma - 16), u = cb_value - 128, v = cr_value - 128;
    return clip_u8((scaled + 409 * v + 128) >> 8) | (clip_u8((scaled - 100 * u - 208 * v + 128) >> 8) << 8) |
           (clip_u8((scaled + 516 * u + 128) >> 8) << 16);
}

__device__ __forceinline__ uint32_t squared_error(uint32_t a, uint32_t b) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int d = (int)((a >> (8 * k)) & 255u) - (int)((b >> (8 * k)) & 255u);
        sum += (uint32_t)(d * d);
    }
    return sum;
}

constexpr int MERGE_SSE_BLOCKS_PER_IMAGE = 64;
__global__ __launch_bounds__(256) void colour_merge_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb,
                                                           const uint8_t* __restrict__ cr, uint8_t* __restrict__ rgb_out,
                                                           const uint8_t* __restrict__ ref, unsigned long long* __restrict__ sse,
                                                           ColourShape s) {
    const uint32_t img = blockIdx.x / s.blocks_per_image, part = blockIdx.x - img * s.blocks_per_image;
    unsigned long long error = 0;
    // one trip when the grid is not capped; with `sse` a block goes on through the image in steps of the image's blocks
    for (uint64_t at_sample = (uint64_t)part * 256u + threadIdx.x; at_sample < (uint64_t)s.hc * s.wc; at_sample += (uint64_t)s.blocks_per_image * 256u) {
        const uint32_t sample = (uint32_t)at_sample;
        const uint32_t i = sample / s.wc, j = sample - i * s.wc;
        // the neighbours, clamped at the real chroma size: never the padding of a coded plane
        const uint32_t rows[3] = {i > 0u ? i - 1u : 0u, i, i + 1u < s.hc ? i + 1u : s.hc - 1u};
        const uint32_t columns[3] = {j > 0u ? j - 1u : 0u, j, j + 1u < s.wc ? j + 1u : s.wc - 1u};
        const uint64_t chroma_image = (uint64_t)img * s.Hc * s.Wc;
        int c_b[2][2], c_r[2][2];
        upsample_block(cb + chroma_image, s.Wc, rows, columns, c_b);
        upsample_block(cr + chroma_image, s.Wc, rows, columns, c_r);
        const uint8_t* luma = y + (uint64_t)img * s.H * s.W;
        const uint64_t picture = (uint64_t)img * s.h * s.w * 3u;
        const uint8_t* ref_end = ref + (uint64_t)s.n * s.h * s.w * 3u;
        const bool two_columns = 2u * j + 1u < s.w;
#pragma unroll
        for (uint32_t dy = 0; dy < 2; ++dy) {
            if (2u * i + dy >= s.h) break;
            const uint8_t* line = luma + (2u * i + dy) * s.W + 2u * j;
            const uint32_t at = ((2u * i + dy) * s.w + 2u * j) * 3u;
            const uint32_t p0 = bt601_inverse((int)line[0], c_b[dy][0], c_r[dy][0]);
            const uint32_t p1 = two_columns ? bt601_inverse((int)line[1], c_b[dy][1], c_r[dy][1]) : 0u;
            if (rgb_out) {
                uint8_t* q = rgb_out + picture + at;
                // six bytes (three at the odd last column): 16-bit stores where the address is even
                store_bytes2(q, p0, true);
                if (two_columns) {
                    store_bytes2(q + 2, (p0 >> 16) | (p1 << 8), true);
                    store_bytes2(q + 4, p1 >> 8, true);
                } else {
                    q[2] = (uint8_t)(p0 >> 16);
                }
            }
            if (ref) {
                const uint8_t* q = ref + picture + at;
                if (two_columns) {
                    uint32_t r0, r1;
                    load_two_pixels(ref, ref_end, q, r0, r1);
                    error += squared_error(p0, r0) + squared_error(p1, r1);
                } else {
                    error += squared_error(p0, load_pixel(q));
                }
            }
        }
    }
    if (!sse) return;                                   // uniform: a kernel argument
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) error += __shfl_down(error, off, 64);
    __shared__ unsigned long long red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = error;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sse[img], red[0] + red[1] + red[2] + red[3]);
}

// Fills `s` and returns true when n pictures of h x w, read or written through planes of the given strides, can be launched:
// everything inside one image is addressed with 32 bits, and the grid is n * blocks_per_image blocks.
bool colour_shape(int n, int h, int w, int H, int W, int Hc, int Wc, ColourShape& s) {
    if (n <= 0 || h <= 0 || w <= 0) return false;
    const int64_t hc = ((int64_t)h + 1) / 2, wc = ((int64_t)w + 1) / 2;
    if (H < h || W < w || (int64_t)Hc < hc || (int64_t)Wc < wc) return false;
    if ((uint64_t)h * (uint64_t)w * 3u > 0xFFFFFFFFull || (uint64_t)H * (uint64_t)W > 0xFFFFFFFFull ||
        (uint64_t)Hc * (uint64_t)Wc > 0xFFFFFFFFull)
        return false;
    const uint64_t blocks_per_image = ((uint64_t)hc * (uint64_t)wc + 255u) / 256u;
    if ((uint64_t)n * blocks_per_image > 0x7FFFFFFFull) return false;
    s.n = (uint32_t)n, s.h = (uint32_t)h, s.w = (uint32_t)w, s.hc = (uint32_t)hc, s.wc = (uint32_t)wc;
    s.H = (uint32_t)H, s.W = (uint32_t)W, s.Hc = (uint32_t)Hc, s.Wc = (uint32_t)Wc;
    s.blocks_per_image = (uint32_t)blocks_per_image;
    return true;
}

}  // namespace

extern "C" int eae_hip_colour_split_420(const uint8_t* rgb, uint8_t* y, uint8_t* cb, uint8_t* cr, int n, int h, int w, void* stream) {
    ColourShape s;
    if (!rgb || !y || !cb || !cr || n <= 0 || h <= 0 || w <= 0) return EAE_HIP_BAD_ARGUMENT;
    if (!colour_shape(n, h, w, h, w, (int)(((int64_t)h + 1) / 2), (int)(((int64_t)w + 1) / 2), s)) return EAE_HIP_BAD_ARGUMENT;
    hipLaunchKernelGGL(colour_split_kernel, dim3(s.n * s.blocks_per_image), dim3(256), 0, (hipStream_t)stream, rgb, y, cb, cr, s);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_colour_merge_420(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint8_t* rgb_out, const uint8_t* ref_rgb,
                                        uint64_t* sse, int n, int h, int w, int H, int W, int Hc, int Wc, void* stream) {
    ColourShape s;
    if (!y || !cb || !cr || (!rgb_out && !ref_rgb) || (ref_rgb == nullptr) != (sse == nullptr)) return EAE_HIP_BAD_ARGUMENT;
    if ((((uintptr_t)sse) & 7u) || !colour_shape(n, h, w, H, W, Hc, Wc, s)) return EAE_HIP_BAD_ARGUMENT;      // 64-bit atomics
    // every block ends in one atomic on its image's word, and atomics on one word serialise: with `sse` an image gets 64 blocks at most
    if (sse && s.blocks_per_image > (uint32_t)MERGE_SSE_BLOCKS_PER_IMAGE) s.blocks_per_image = MERGE_SSE_BLOCKS_PER_IMAGE;
    hipLaunchKernelGGL(colour_merge_kernel, dim3(s.n * s.blocks_per_image), dim3(256), 0, (hipStream_t)stream, y, cb, cr, rgb_out, ref_rgb,
                       reinterpret_cast<unsigned long long*>(sse), s);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
