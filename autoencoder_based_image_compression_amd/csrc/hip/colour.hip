// colour.hip -- colour images, 4:2:0: the two launches that stand between an RGB picture and the three planes
// the luminance codecs take (colour.py states both in numpy; tests/test_gpu_colour_kernels.py holds the kernels to it bit for bit).
//   eae_hip_colour_split_420: rgb u8 [n][h][w][3] (device or pinned host memory, any byte address) -> y u8 [n][h][w] and cb, cr u8
//     [n][hc][wc], hc = ceil(h / 2), wc = ceil(w / 2): BT.601 in float64 per pixel (bt601.h), chroma the rounded mean of its 2 x 2 block,
//     the block completed by edge replication at an odd side.
//   eae_hip_colour_merge_420: y u8 [n][H][W], cb, cr u8 [n][Hc][Wc], of which the top-left h x w / hc x wc are read -> rgb u8
//     [n][h][w][3] and / or sse[i] += the squared error against a reference picture: chroma upsampled 3:1 centre-sited with the
//     neighbours clamped at the real chroma size, then the integer BT.601 inverse.
//   eae_hip_colour_merge_420_words: the same picture in whole aligned 16-byte words, for the resident decoder (further down).
//   eae_hip_colour_budget_rest: the byte budget of a picture's luminance plane from what its chroma planes took (at
//     the end of the file): no pixel work, one lane per picture.
//   eae_hip_colour_quality_rest: the squared-error threshold of a picture's luminance plane from what its chroma planes spent (DESIGN.md
//     section 30; behind it): the same shape of launch.
// In the first two a lane owns one chroma sample, i.e. a 2 x 2 block of pixels: 12 bytes of the picture, six contiguous ones in each of two
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

// ---- the merge in whole words ----------------------------------------------------------------------------------
// The batch's output [n][h][w][3] is one flat run of bytes, cut into aligned 16-byte words. A lane owns 16 consecutive flat pixels: 48
// bytes, three words; a block 768 consecutive words, which it stages in LDS so that every store instruction of a wave writes 1 KB of
// consecutive words (lane t stores words t, t + 256 and t + 512 of the block). A lane finds (picture, row, column) of its first pixel
// by division. When its 16 pixels lie in one row -- every lane of a picture whose width is a multiple of 16, all but the one or two
// lanes around each row end otherwise -- it takes them in runs of four (`load_run4`, bounded by the ROW: nothing outside the top-left
// h x w / hc x wc of a plane is loaded) and writes its three words into LDS whole. A lane whose pixels cross a row end, a picture end
// or the end of the batch goes pixel by pixel with carries and writes bytes into LDS; pixels past n * h * w are zero bytes.
constexpr uint32_t WORDS_LANE_PIXELS = 16, WORDS_PER_BLOCK = 768;

// Four bytes of one row of a plane, at columns first .. first + 3 clamped to [0, width): a run where all four exist
__device__ __forceinline__ uint32_t clamped_run4(const uint8_t* line, uint32_t width, int first) {
    if (first >= 0 && (uint32_t)first + 4u <= width) return load_run4(line, line + width, line + first);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int column = first + k;
        v |= (uint32_t)line[column < 0 ? 0 : ((uint32_t)column < width ? (uint32_t)column : width - 1u)] << (8 * k);
    }
    return v;
}

__device__ __forceinline__ int window_byte(const uint32_t (&window)[3], int index) { return (int)((window[index >> 2] >> (8 * (index & 3))) & 255u); }

// One chroma plane over the 16 pixels of row r that start at column c: `near` is chroma row r >> 1, `far` its clamped neighbour, both
// as the 12 bytes at chroma columns (c >> 1) - 1 .. (c >> 1) + 10, clamped. Position m = 0 .. 16 counts pixels from the even column
// c & ~1: its sample is byte 1 + (m >> 1) of the window, the neighbour the byte in front (m even) or behind (m odd). value[m] is the
// upsampled chroma of that pixel; the pixels of the lane are positions (c & 1) .. (c & 1) + 15.
__device__ __forceinline__ void upsample_row16(const uint32_t (&near)[3], const uint32_t (&far)[3], int (&value)[17]) {
#pragma unroll
    for (int m = 0; m < 17; ++m) {
        const int sample = 1 + (m >> 1), neighbour = (m & 1) ? sample + 1 : sample - 1;
        const int here = 3 * window_byte(near, sample) + window_byte(near, neighbour);
        const int there = 3 * window_byte(far, sample) + window_byte(far, neighbour);
        value[m] = (3 * here + there + 8) >> 4;
    }
}

// Pixel (r, c) of a picture from bytes: r | g << 8 | b << 16
__device__ __forceinline__ uint32_t merge_pixel(const uint8_t* luma, const uint8_t* plane_b, const uint8_t* plane_r, uint32_t r, uint32_t c,
                                                const ColourShape& s) {
    const uint32_t i = r >> 1, j = c >> 1;
    const uint32_t i2 = (r & 1u) ? (i + 1u < s.hc ? i + 1u : s.hc - 1u) : (i > 0u ? i - 1u : 0u);
    const uint32_t j2 = (c & 1u) ? (j + 1u < s.wc ? j + 1u : s.wc - 1u) : (j > 0u ? j - 1u : 0u);
    const uint32_t near = i * s.Wc, far = i2 * s.Wc;
    const int c_b = (9 * (int)plane_b[near + j] + 3 * (int)plane_b[near + j2] + 3 * (int)plane_b[far + j] + (int)plane_b[far + j2] + 8) >> 4;
    const int c_r = (9 * (int)plane_r[near + j] + 3 * (int)plane_r[near + j2] + 3 * (int)plane_r[far + j] + (int)plane_r[far + j2] + 8) >> 4;
    return bt601_inverse((int)luma[r * s.W + c], c_b, c_r);
}

__global__ __launch_bounds__(256) void colour_merge_words_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb,
                                                                 const uint8_t* __restrict__ cr, u32x4* __restrict__ dst, ColourShape s,
                                                                 uint64_t pixels, uint64_t words) {
    __shared__ u32x4 tile[WORDS_PER_BLOCK];
    const uint64_t first = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * WORDS_LANE_PIXELS;
    u32x4* mine = tile + 3u * threadIdx.x;
    if (first >= pixels) {                              // behind the batch: zero bytes (stored only where the last word reaches)
        const u32x4 zero = {0u, 0u, 0u, 0u};
        mine[0] = zero, mine[1] = zero, mine[2] = zero;
    } else {
        const uint32_t picture_pixels = s.h * s.w;
        uint64_t img = first / picture_pixels;
        const uint32_t inside = (uint32_t)(first - img * picture_pixels);
        uint32_t r = inside / s.w, c = inside - r * s.w;
        const uint8_t* luma = y + img * s.H * s.W;
        const uint8_t* plane_b = cb + img * s.Hc * s.Wc;
        const uint8_t* plane_r = cr + img * s.Hc * s.Wc;
        if (c + WORDS_LANE_PIXELS <= s.w) {             // one row holds all 16
            const uint32_t i = r >> 1;
            const uint32_t i2 = (r & 1u) ? (i + 1u < s.hc ? i + 1u : s.hc - 1u) : (i > 0u ? i - 1u : 0u);
            const int first_column = (int)(c >> 1) - 1;
            uint32_t near[3], far[3];
            int c_b[17], c_r[17];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                near[t] = clamped_run4(plane_b + i * s.Wc, s.wc, first_column + 4 * t);
                far[t] = clamped_run4(plane_b + i2 * s.Wc, s.wc, first_column + 4 * t);
            }
            upsample_row16(near, far, c_b);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                near[t] = clamped_run4(plane_r + i * s.Wc, s.wc, first_column + 4 * t);
                far[t] = clamped_run4(plane_r + i2 * s.Wc, s.wc, first_column + 4 * t);
            }
            upsample_row16(near, far, c_r);
            const uint8_t* line = luma + r * s.W;
            const bool odd = (c & 1u) != 0u;
            uint32_t out[12];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t four = load_run4(line, line + s.w, line + c + 4 * g);
                uint32_t p[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int m = 4 * g + k;
                    p[k] = bt601_inverse((int)((four >> (8 * k)) & 255u), odd ? c_b[m + 1] : c_b[m], odd ? c_r[m + 1] : c_r[m]);
                }
                out[3 * g] = p[0] | (p[1] << 24);
                out[3 * g + 1] = (p[1] >> 8) | (p[2] << 16);
                out[3 * g + 2] = (p[2] >> 16) | (p[3] << 8);
            }
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                u32x4 word;
                word.x = out[4 * t], word.y = out[4 * t + 1], word.z = out[4 * t + 2], word.w = out[4 * t + 3];
                mine[t] = word;
            }
        } else {                                        // a row end, a picture end or the end of the batch inside the 16: by pixels
            uint8_t* bytes = reinterpret_cast<uint8_t*>(mine);
            for (uint32_t k = 0; k < WORDS_LANE_PIXELS; ++k) {
                uint32_t p = 0;
                if (first + k < pixels) {
                    p = merge_pixel(luma, plane_b, plane_r, r, c, s);
                    if (++c == s.w) {
                        c = 0;
                        if (++r == s.h) {
                            r = 0, ++img;
                            luma = y + img * s.H * s.W, plane_b = cb + img * s.Hc * s.Wc, plane_r = cr + img * s.Hc * s.Wc;      // formed, not read, behind the last picture
                        }
                    }
                }
                bytes[3u * k] = (uint8_t)p, bytes[3u * k + 1u] = (uint8_t)(p >> 8), bytes[3u * k + 2u] = (uint8_t)(p >> 16);
            }
        }
    }
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * WORDS_PER_BLOCK;
#pragma unroll
    for (uint32_t t = 0; t < 3; ++t) {
        const uint64_t word = base + t * 256u + threadIdx.x;
        if (word < words) dst[word] = tile[t * 256u + threadIdx.x];
    }
}

// ---- the merge of crops ----------------------------------------------------------------------------------------
// colour_merge_words_kernel for crops of a picture: y is dense [n][rh][rw], crop k the pixels at (y0, x0) = origins[k] of an h x w
// picture, cb and cr dense [n][rch][rcw], the chroma rectangle colour.chroma_region names for it, whose origin (cy0, cx0) the kernel
// derives from (y0, x0) by the same rule. The samples, the parity of the weights and the clamp of the neighbours are those of the
// pixel's position in the PICTURE (y0 + r, x0 + c against hc, wc); every chroma index is then shifted by (cy0, cx0). The 12-byte
// windows of the fast path reach up to three samples further than the 16 pixels need, so a run is loaded as a run only where it lies
// inside the crop's own chroma row and byte by byte, clamped into that row, elsewhere: nothing outside the three dense inputs is read.
struct CropShape {
    uint32_t n, hc, wc;                // crops; the real size of the picture's chroma planes
    uint32_t rh, rw, rch, rcw;         // the size of a crop and of its chroma rectangle
    uint32_t last_y0, last_x0;         // h - rh, w - rw: the last origin inside the picture
};

// colour.chroma_region's origin along one axis: one sample in front of the crop's first, clamped into the plane
__device__ __forceinline__ uint32_t chroma_origin(uint32_t origin, uint32_t size, uint32_t crop) {
    const uint32_t first = origin >> 1, start = first > 0u ? first - 1u : 0u;
    return start < size - crop ? start : size - crop;
}

// Four bytes of one row of a chroma crop (`width` samples that start at column `origin` of a plane `plane_width` wide), at the PLANE's
// columns first .. first + 3 clamped to [0, plane_width): a run where all four lie in the crop's row; a column outside the row -- never
// one the 16 pixels need -- reads the row's nearest sample
__device__ __forceinline__ uint32_t crop_run4(const uint8_t* line, uint32_t width, uint32_t plane_width, uint32_t origin, int first) {
    const int local = first - (int)origin;
    if (local >= 0 && (uint32_t)local + 4u <= width) return load_run4(line, line + width, line + local);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int column = first + k;
        const int at = (column < 0 ? 0 : ((uint32_t)column < plane_width ? column : (int)plane_width - 1)) - (int)origin;
        v |= (uint32_t)line[at < 0 ? 0 : ((uint32_t)at < width ? (uint32_t)at : width - 1u)] << (8 * k);
    }
    return v;
}

// Pixel (r, c) of the crop at (y0, x0), chroma origin (cy0, cx0), from bytes: r | g << 8 | b << 16
__device__ __forceinline__ uint32_t merge_crop_pixel(const uint8_t* luma, const uint8_t* plane_b, const uint8_t* plane_r, uint32_t r, uint32_t c,
                                                     uint32_t y0, uint32_t x0, uint32_t cy0, uint32_t cx0, const CropShape& s) {
    const uint32_t row = y0 + r, column = x0 + c, i = row >> 1, j = column >> 1;
    const uint32_t i2 = (row & 1u) ? (i + 1u < s.hc ? i + 1u : s.hc - 1u) : (i > 0u ? i - 1u : 0u);
    const uint32_t j2 = (column & 1u) ? (j + 1u < s.wc ? j + 1u : s.wc - 1u) : (j > 0u ? j - 1u : 0u);
    const uint32_t near = (i - cy0) * s.rcw, far = (i2 - cy0) * s.rcw, here = j - cx0, there = j2 - cx0;
    const int c_b = (9 * (int)plane_b[near + here] + 3 * (int)plane_b[near + there] + 3 * (int)plane_b[far + here] + (int)plane_b[far + there] + 8) >> 4;
    const int c_r = (9 * (int)plane_r[near + here] + 3 * (int)plane_r[near + there] + 3 * (int)plane_r[far + here] + (int)plane_r[far + there] + 8) >> 4;
    return bt601_inverse((int)luma[r * s.rw + c], c_b, c_r);
}

__global__ __launch_bounds__(256) void colour_merge_crops_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb,
                                                                 const uint8_t* __restrict__ cr, const int32_t* __restrict__ origins,
                                                                 u32x4* __restrict__ dst, CropShape s, uint64_t pixels, uint64_t words) {
    __shared__ u32x4 tile[WORDS_PER_BLOCK];
    const uint64_t first = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * WORDS_LANE_PIXELS;
    u32x4* mine = tile + 3u * threadIdx.x;
    if (first >= pixels) {                              // behind the batch: zero bytes (stored only where the last word reaches)
        const u32x4 zero = {0u, 0u, 0u, 0u};
        mine[0] = zero, mine[1] = zero, mine[2] = zero;
    } else {
        const uint32_t crop_pixels = s.rh * s.rw, chroma_pixels = s.rch * s.rcw;
        uint64_t img = first / crop_pixels;
        const uint32_t inside = (uint32_t)(first - img * crop_pixels);
        uint32_t r = inside / s.rw, c = inside - r * s.rw;
        // (an origin outside the picture is the host's to refuse; clamped here, so that even then no load leaves the inputs)
        uint32_t y0 = min((uint32_t)origins[2u * img], s.last_y0), x0 = min((uint32_t)origins[2u * img + 1u], s.last_x0);
        uint32_t cy0 = chroma_origin(y0, s.hc, s.rch), cx0 = chroma_origin(x0, s.wc, s.rcw);
        const uint8_t* luma = y + img * crop_pixels;
        const uint8_t* plane_b = cb + img * chroma_pixels;
        const uint8_t* plane_r = cr + img * chroma_pixels;
        if (c + WORDS_LANE_PIXELS <= s.rw) {            // one row of the crop holds all 16
            const uint32_t row = y0 + r, column = x0 + c, i = row >> 1;
            const uint32_t i2 = (row & 1u) ? (i + 1u < s.hc ? i + 1u : s.hc - 1u) : (i > 0u ? i - 1u : 0u);
            const uint32_t near_row = (i - cy0) * s.rcw, far_row = (i2 - cy0) * s.rcw;
            const int first_column = (int)(column >> 1) - 1;
            uint32_t near[3], far[3];
            int c_b[17], c_r[17];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                near[t] = crop_run4(plane_b + near_row, s.rcw, s.wc, cx0, first_column + 4 * t);
                far[t] = crop_run4(plane_b + far_row, s.rcw, s.wc, cx0, first_column + 4 * t);
            }
            upsample_row16(near, far, c_b);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                near[t] = crop_run4(plane_r + near_row, s.rcw, s.wc, cx0, first_column + 4 * t);
                far[t] = crop_run4(plane_r + far_row, s.rcw, s.wc, cx0, first_column + 4 * t);
            }
            upsample_row16(near, far, c_r);
            const uint8_t* line = luma + r * s.rw;
            const bool odd = (column & 1u) != 0u;
            uint32_t out[12];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t four = load_run4(line, line + s.rw, line + c + 4 * g);
                uint32_t p[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int m = 4 * g + k;
                    p[k] = bt601_inverse((int)((four >> (8 * k)) & 255u), odd ? c_b[m + 1] : c_b[m], odd ? c_r[m + 1] : c_r[m]);
                }
                out[3 * g] = p[0] | (p[1] << 24);
                out[3 * g + 1] = (p[1] >> 8) | (p[2] << 16);
                out[3 * g + 2] = (p[2] >> 16) | (p[3] << 8);
            }
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                u32x4 word;
                word.x = out[4 * t], word.y = out[4 * t + 1], word.z = out[4 * t + 2], word.w = out[4 * t + 3];
                mine[t] = word;
            }
        } else {                                        // a row end, a crop end or the end of the batch inside the 16: by pixels
            uint8_t* bytes = reinterpret_cast<uint8_t*>(mine);
            for (uint32_t k = 0; k < WORDS_LANE_PIXELS; ++k) {
                uint32_t p = 0;
                if (first + k < pixels) {
                    p = merge_crop_pixel(luma, plane_b, plane_r, r, c, y0, x0, cy0, cx0, s);
                    if (++c == s.rw) {
                        c = 0;
                        if (++r == s.rh) {
                            r = 0, ++img;
                            if (img < s.n) {            // the next crop has an origin of its own; behind the last one nothing is read
                                y0 = min((uint32_t)origins[2u * img], s.last_y0), x0 = min((uint32_t)origins[2u * img + 1u], s.last_x0);
                                cy0 = chroma_origin(y0, s.hc, s.rch), cx0 = chroma_origin(x0, s.wc, s.rcw);
                                luma = y + img * crop_pixels, plane_b = cb + img * chroma_pixels, plane_r = cr + img * chroma_pixels;
                            }
                        }
                    }
                }
                bytes[3u * k] = (uint8_t)p, bytes[3u * k + 1u] = (uint8_t)(p >> 8), bytes[3u * k + 2u] = (uint8_t)(p >> 16);
            }
        }
    }
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * WORDS_PER_BLOCK;
#pragma unroll
    for (uint32_t t = 0; t < 3; ++t) {
        const uint64_t word = base + t * 256u + threadIdx.x;
        if (word < words) dst[word] = tile[t * 256u + threadIdx.x];
    }
}

// ---- the luminance budget of a colour picture -------------------------------------------------------------------
// ratecontrol.colour_luma_budgets on the device, so that the budget of Y never visits the host: a lane owns one picture. With P =
// max(B - header_bytes, 0) the payload of its EAC1 blob (header_bytes: the size of container.py's colour header), out = max(max(P - upper_cb[point_cb], 0) - upper_cr[point_cr], 0): for the byte counts
// the bounds are (never negative) that is max(P - ub_cb - ub_cr, 0), and no difference leaves int64 for any B up to 2^62. A point
// outside [0, K) gives 0 and loads nothing from the tables.
constexpr int BUDGET_REST_LANES = 256;
__global__ __launch_bounds__(BUDGET_REST_LANES) void colour_budget_rest_kernel(const int64_t* __restrict__ budgets, const int64_t* __restrict__ upper_cb,
                                                                               const int32_t* __restrict__ point_cb, const int64_t* __restrict__ upper_cr,
                                                                               const int32_t* __restrict__ point_cr, int64_t* __restrict__ out,
                                                                               uint32_t n, uint32_t k_points, int64_t header_bytes) {
    const uint32_t i = blockIdx.x * (uint32_t)BUDGET_REST_LANES + threadIdx.x;
    if (i >= n) return;
    const int32_t pb = point_cb[i], pr = point_cr[i];
    int64_t rest = 0;
    if (pb >= 0 && (uint32_t)pb < k_points && pr >= 0 && (uint32_t)pr < k_points) {
        const int64_t budget = budgets[i];
        rest = budget > header_bytes ? budget - header_bytes : 0;
        const int64_t ub_cb = upper_cb[(uint64_t)i * k_points + (uint32_t)pb], ub_cr = upper_cr[(uint64_t)i * k_points + (uint32_t)pr];
        rest = rest > ub_cb ? rest - ub_cb : 0;
        rest = rest > ub_cr ? rest - ub_cr : 0;
    }
    out[i] = rest;
}

// ---- the luminance threshold of a colour picture ----------------------------------------------------------------
// ratecontrol.colour_luma_max_sse on the device, so that the threshold of Y never visits the host: a lane owns one picture.
// out = max(max(M - sse_cb, 0) - sse_cr, 0): for the squared errors they are (never negative) that is max(M - sse_cb - sse_cr, 0), and
// every difference is taken between two values in [0, 2^63), so nothing leaves int64 for any M up to 2^62. A negative M gives 0.
__global__ __launch_bounds__(BUDGET_REST_LANES) void colour_quality_rest_kernel(const int64_t* __restrict__ max_sse, const int64_t* __restrict__ sse_cb,
                                                                                const int64_t* __restrict__ sse_cr, int64_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * (uint32_t)BUDGET_REST_LANES + threadIdx.x;
    if (i >= n) return;
    int64_t rest = max_sse[i];
    const int64_t of_cb = sse_cb[i], of_cr = sse_cr[i];
    rest = rest > 0 ? rest : 0;
    rest = rest > of_cb ? rest - of_cb : 0;
    rest = rest > of_cr ? rest - of_cr : 0;
    out[i] = rest;
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

extern "C" int eae_hip_colour_merge_420_words(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint8_t* dst, uint64_t dst_bytes,
                                              int n, int h, int w, int H, int W, int Hc, int Wc, void* stream) {
    ColourShape s;
    if (!y || !cb || !cr || !dst || !colour_shape(n, h, w, H, W, Hc, Wc, s)) return EAE_HIP_BAD_ARGUMENT;
    const uint64_t pixels = (uint64_t)s.n * s.h * s.w;
    const uint64_t words = (pixels * 3u + 15u) / 16u;
    // whole aligned words, and room for every one of them: the last word is written whole, pad bytes included
    if ((((uintptr_t)dst) & 15u) || (dst_bytes & 15u) || dst_bytes / 16u < words) return EAE_HIP_BAD_ARGUMENT;
    const uint64_t blocks = (words + WORDS_PER_BLOCK - 1u) / WORDS_PER_BLOCK;          // one block per 768 words, whatever the size
    if (blocks > 0x7FFFFFFFull) return EAE_HIP_BAD_ARGUMENT;
    hipLaunchKernelGGL(colour_merge_words_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y, cb, cr,
                       reinterpret_cast<u32x4*>(dst), s, pixels, words);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_colour_merge_420_crops(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, const int32_t* origins, uint8_t* dst,
                                              uint64_t dst_bytes, int n, int h, int w, int rh, int rw, int rch, int rcw, void* stream) {
    if (!y || !cb || !cr || !origins || !dst || n <= 0 || h <= 0 || w <= 0 || rh <= 0 || rw <= 0 || rh > h || rw > w) return EAE_HIP_BAD_ARGUMENT;
    // colour_shape's limits: everything inside a picture, and so inside a crop, is addressed with 32 bits
    if ((uint64_t)h * (uint64_t)w * 3u > 0xFFFFFFFFull) return EAE_HIP_BAD_ARGUMENT;
    const int64_t hc = ((int64_t)h + 1) / 2, wc = ((int64_t)w + 1) / 2;
    // colour.chroma_region's size, which the host cut the chroma crops to
    const int64_t need_rch = hc < (int64_t)rh / 2 + 3 ? hc : (int64_t)rh / 2 + 3, need_rcw = wc < (int64_t)rw / 2 + 3 ? wc : (int64_t)rw / 2 + 3;
    if ((int64_t)rch != need_rch || (int64_t)rcw != need_rcw) return EAE_HIP_BAD_ARGUMENT;
    const uint64_t pixels = (uint64_t)n * (uint64_t)rh * (uint64_t)rw;
    const uint64_t words = (pixels * 3u + 15u) / 16u;
    // whole aligned words, and room for every one of them: the last word is written whole, pad bytes included
    if ((((uintptr_t)dst) & 15u) || (((uintptr_t)origins) & 3u) || (dst_bytes & 15u) || dst_bytes / 16u < words) return EAE_HIP_BAD_ARGUMENT;
    const uint64_t blocks = (words + WORDS_PER_BLOCK - 1u) / WORDS_PER_BLOCK;          // one block per 768 words, whatever the size
    if (blocks > 0x7FFFFFFFull) return EAE_HIP_BAD_ARGUMENT;
    CropShape s;
    s.n = (uint32_t)n, s.hc = (uint32_t)hc, s.wc = (uint32_t)wc;
    s.rh = (uint32_t)rh, s.rw = (uint32_t)rw, s.rch = (uint32_t)rch, s.rcw = (uint32_t)rcw;
    s.last_y0 = (uint32_t)(h - rh), s.last_x0 = (uint32_t)(w - rw);
    hipLaunchKernelGGL(colour_merge_crops_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y, cb, cr, origins,
                       reinterpret_cast<u32x4*>(dst), s, pixels, words);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_colour_budget_rest(const int64_t* budgets, const int64_t* upper_cb, const int32_t* point_cb, const int64_t* upper_cr,
                                          const int32_t* point_cr, int64_t* out, int n, int k_points, int64_t header_bytes, void* stream) {
    if (!budgets || !upper_cb || !point_cb || !upper_cr || !point_cr || !out || n <= 0 || k_points <= 0 || header_bytes < 0) return EAE_HIP_BAD_ARGUMENT;
    if ((((uintptr_t)budgets | (uintptr_t)upper_cb | (uintptr_t)upper_cr | (uintptr_t)out) & 7u) || (((uintptr_t)point_cb | (uintptr_t)point_cr) & 3u))
        return EAE_HIP_BAD_ARGUMENT;
    const uint32_t blocks = ((uint32_t)n + (uint32_t)BUDGET_REST_LANES - 1u) / (uint32_t)BUDGET_REST_LANES;      // one lane per picture, whatever n
    hipLaunchKernelGGL(colour_budget_rest_kernel, dim3(blocks), dim3(BUDGET_REST_LANES), 0, (hipStream_t)stream, budgets, upper_cb, point_cb,
                       upper_cr, point_cr, out, (uint32_t)n, (uint32_t)k_points, header_bytes);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_colour_quality_rest(const int64_t* max_sse, const int64_t* sse_cb, const int64_t* sse_cr, int64_t* out, int n, void* stream) {
    if (!max_sse || !sse_cb || !sse_cr || !out || n <= 0) return EAE_HIP_BAD_ARGUMENT;
    if (((uintptr_t)max_sse | (uintptr_t)sse_cb | (uintptr_t)sse_cr | (uintptr_t)out) & 7u) return EAE_HIP_BAD_ARGUMENT;
    const uint32_t blocks = ((uint32_t)n + (uint32_t)BUDGET_REST_LANES - 1u) / (uint32_t)BUDGET_REST_LANES;      // one lane per picture, whatever n
    hipLaunchKernelGGL(colour_quality_rest_kernel, dim3(blocks), dim3(BUDGET_REST_LANES), 0, (hipStream_t)stream, max_sse, sse_cb, sse_cr, out,
                       (uint32_t)n);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
