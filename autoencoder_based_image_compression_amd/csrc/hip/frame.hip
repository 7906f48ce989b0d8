// frame.hip -- images of any height and width: the two launches that stand between an h x w image and the
// H x W = ceil16(h) x ceil16(w) planes every transform kernel works on.
//   eae_hip_frame_pad_u8: u8 [n][h][w] (device or pinned host memory, rows at any byte address) -> u8 [n][H][W], edge replicated:
//     dst[i][y][x] = src[i][min(y, h - 1)][min(x, w - 1)]. A lane forms one 16-byte word of a destination row out of four dwords.
//   eae_hip_frame_sse_u8: sse[i] += sum over y < h, x < w of (ref[i][y][x] - rec[i][y][x])^2 with rec u8 [n][H][W], ref u8 [n][h][w]:
//     a lane takes four pixels of a row of both; the pixels of rec outside h x w are never loaded.
// Both read unaligned runs of four bytes with load_run4 (byte_runs.h): from the two aligned dwords around the run when both lie
// inside the tensor's bytes, else byte by byte.
#include "byte_runs.h"
#include "common.h"

namespace {

struct FrameShape {
    uint32_t n, h, w, H, W;
};

constexpr int PAD_BLOCKS = 1024;
__global__ __launch_bounds__(256) void frame_pad_kernel(const uint8_t* __restrict__ src, u32x4* __restrict__ dst, FrameShape s) {
    const uint32_t words_per_row = s.W >> 4;
    const uint64_t words = (uint64_t)s.n * s.H * words_per_row;
    const uint8_t* end = src + (uint64_t)s.n * s.h * s.w;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = i / words_per_row;                 // image * H + y
        const uint32_t x0 = (uint32_t)(i - row * words_per_row) << 4;
        const uint64_t img = row / s.H;
        const uint32_t y = (uint32_t)(row - img * s.H);
        const uint8_t* line = src + (img * s.h + (y < s.h ? y : s.h - 1u)) * s.w;
        uint32_t out[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t x = x0 + 4u * d;
            uint32_t v;
            if (x + 4u <= s.w) {
                v = load_run4(src, end, line + x);
            } else {                                            // the last real column repeats to the right
                v = 0;
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) v |= (uint32_t)line[x + j < s.w ? x + j : s.w - 1u] << (8 * j);
            }
            out[d] = v;
        }
        u32x4 word;
        word.x = out[0], word.y = out[1], word.z = out[2], word.w = out[3];
        dst[i] = word;
    }
}

constexpr int SSE_BLOCKS_PER_IMAGE = 64;
__global__ __launch_bounds__(256) void frame_sse_kernel(const uint8_t* __restrict__ rec, const uint8_t* __restrict__ ref,
                                                        unsigned long long* __restrict__ sse, FrameShape s, uint32_t blocks_per_image) {
    const uint32_t img = blockIdx.x / blocks_per_image, part = blockIdx.x - img * blocks_per_image;
    const uint32_t runs_per_row = (s.w + 3u) >> 2;
    const uint64_t runs = (uint64_t)s.h * runs_per_row;
    const uint8_t* rec_end = rec + (uint64_t)s.n * s.H * s.W;
    const uint8_t* ref_end = ref + (uint64_t)s.n * s.h * s.w;
    const uint8_t* rec_img = rec + (uint64_t)img * s.H * s.W;
    const uint8_t* ref_img = ref + (uint64_t)img * s.h * s.w;
    unsigned long long sum = 0;
    for (uint64_t i = (uint64_t)part * 256u + threadIdx.x; i < runs; i += (uint64_t)blocks_per_image * 256u) {
        const uint64_t y = i / runs_per_row;
        const uint32_t x = (uint32_t)(i - y * runs_per_row) << 2;
        const uint8_t* pa = rec_img + y * s.W + x;
        const uint8_t* pb = ref_img + y * s.w + x;
        uint32_t part_sum = 0;
        if (x + 4u <= s.w) {
            const uint32_t a = load_run4(rec, rec_end, pa), b = load_run4(ref, ref_end, pb);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = (int)((a >> (8 * j)) & 255u) - (int)((b >> (8 * j)) & 255u);
                part_sum += (uint32_t)(d * d);
            }
        } else {
            for (uint32_t j = 0; x + j < s.w; ++j) {
                const int d = (int)pa[j] - (int)pb[j];
                part_sum += (uint32_t)(d * d);
            }
        }
        sum += part_sum;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    __shared__ unsigned long long red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sse[img], red[0] + red[1] + red[2] + red[3]);
}

// H x W is the coded size of h x w: both sides rounded up to the next multiple of 16
bool is_coded_size(int h, int w, int H, int W) {
    return (int64_t)H == ((int64_t)h + 15) / 16 * 16 && (int64_t)W == ((int64_t)w + 15) / 16 * 16;
}

}  // namespace

extern "C" int eae_hip_frame_pad_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int H, int W, void* stream) {
    if (!src || !dst || n <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return EAE_HIP_BAD_ARGUMENT;
    if (!is_coded_size(h, w, H, W) || (((uintptr_t)dst) & 15u)) return EAE_HIP_BAD_SHAPE;      // 16-byte stores
    FrameShape s;
    s.n = (uint32_t)n, s.h = (uint32_t)h, s.w = (uint32_t)w, s.H = (uint32_t)H, s.W = (uint32_t)W;
    const uint64_t words = (uint64_t)n * (uint64_t)H * (uint64_t)(W / 16);
    const unsigned blocks = (unsigned)((words + 255) / 256 > (uint64_t)PAD_BLOCKS ? (uint64_t)PAD_BLOCKS : (words + 255) / 256);
    hipLaunchKernelGGL(frame_pad_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, (u32x4*)dst, s);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_frame_sse_u8(const uint8_t* rec, const uint8_t* ref, uint64_t* sse, int n, int h, int w, int H, int W, void* stream) {
    if (!rec || !ref || !sse || n <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return EAE_HIP_BAD_ARGUMENT;
    if (!is_coded_size(h, w, H, W) || (((uintptr_t)sse) & 7u)) return EAE_HIP_BAD_SHAPE;        // 64-bit atomics
    FrameShape s;
    s.n = (uint32_t)n, s.h = (uint32_t)h, s.w = (uint32_t)w, s.H = (uint32_t)H, s.W = (uint32_t)W;
    const uint64_t runs = (uint64_t)h * (((uint64_t)w + 3) / 4);
    uint64_t bpi = (runs + 1023) / 1024;        // four iterations of a block at least
    if (bpi > (uint64_t)SSE_BLOCKS_PER_IMAGE) bpi = SSE_BLOCKS_PER_IMAGE;
    if ((uint64_t)n * bpi > 0x7FFFFFFFull) return EAE_HIP_BAD_SHAPE;
    hipLaunchKernelGGL(frame_sse_kernel, dim3((unsigned)((uint64_t)n * bpi)), dim3(256), 0, (hipStream_t)stream, rec, ref,
                       reinterpret_cast<unsigned long long*>(sse), s, (uint32_t)bpi);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
