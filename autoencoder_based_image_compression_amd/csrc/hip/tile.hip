// tile.hip -- the two data movers of the tiled encode / decode (pipeline.tile_plan).
// A tiled call cuts the image into windows of one shape, runs the unchanged whole-path entry points (eae_hip_encode /
// eae_hip_decode) on a batch of windows, and keeps of every window only its interior, the part whose receptive field the
// window holds entirely. These kernels move the rectangles: full plane <-> batch of windows, driven by the plan rows. They
// compute nothing but the squared error of the stitched reconstruction; both are pure HBM copies.
//
// Plan row (int32, EAE_TILE_PLAN_COLS per window, every coordinate in latents = `unit` elements along each axis):
//   [0] image  [1, 2] window origin in the image  [3, 4] interior origin in the window  [5, 6] interior origin in the image
//   [7, 8] interior extent
// The full-plane side is addressed with 64-bit byte offsets: the point of tiling is planes the transform kernels cannot address.
#include "common.h"

namespace {

constexpr int TILE_THREADS = 256;
constexpr int TILE_UNROLL = 4;       // 16-byte chunks in flight per lane: four loads issued before the first store

struct Rect {
    uint64_t plane;      // byte offset of the rectangle's first byte in the full plane
    uint64_t window;     // same in the batch of windows
    uint32_t rows;       // element rows of the rectangle
    uint32_t chunks;     // 16-byte chunks per row
};

// The rectangle one plan row names: the whole window (gather) or the interior (stitch). Wave-uniform: scalar loads.
__device__ __forceinline__ Rect plan_rect(const int32_t* __restrict__ row, int g, bool whole_window, int unit, int unit_bytes,
                                          uint64_t plane_image_bytes, uint64_t plane_row_bytes, int window_h, int window_w,
                                          uint64_t window_bytes, uint64_t window_row_bytes) {
    const int img = row[0];
    const int pr = whole_window ? row[1] : row[5], pc = whole_window ? row[2] : row[6];
    const int wr = whole_window ? 0 : row[3], wc = whole_window ? 0 : row[4];
    const int er = whole_window ? window_h : row[7], ec = whole_window ? window_w : row[8];
    Rect r;
    r.plane = (uint64_t)img * plane_image_bytes + (uint64_t)pr * unit * plane_row_bytes + (uint64_t)pc * unit_bytes;
    r.window = (uint64_t)g * window_bytes + (uint64_t)wr * unit * window_row_bytes + (uint64_t)wc * unit_bytes;
    r.rows = (uint32_t)(er * unit);
    r.chunks = (uint32_t)(ec * unit_bytes / 16);
    return r;
}

// blockIdx.y = window of the group, blockIdx.x strides over the rectangle's 16-byte chunks. One global_load_dwordx4 and one
// global_store_dwordx4 per chunk.
template <bool TO_WINDOWS>
__global__ __launch_bounds__(TILE_THREADS) void tile_copy_kernel(uint8_t* __restrict__ plane, uint8_t* __restrict__ windows,
                                                                 const int32_t* __restrict__ plan, int unit, int unit_bytes,
                                                                 uint64_t plane_image_bytes, uint64_t plane_row_bytes, int window_h,
                                                                 int window_w, uint64_t window_bytes, uint64_t window_row_bytes) {
    const int g = blockIdx.y;
    const Rect r = plan_rect(plan + (size_t)g * EAE_TILE_PLAN_COLS, g, TO_WINDOWS, unit, unit_bytes, plane_image_bytes, plane_row_bytes,
                             window_h, window_w, window_bytes, window_row_bytes);
    const uint32_t total = r.rows * r.chunks;
    const uint32_t stride = gridDim.x * TILE_THREADS;
    for (uint32_t base = blockIdx.x * TILE_THREADS + threadIdx.x; base < total; base += stride * TILE_UNROLL) {
        u32x4 v[TILE_UNROLL];
        uint64_t dst[TILE_UNROLL];
#pragma unroll
        for (int j = 0; j < TILE_UNROLL; ++j) {
            const uint32_t i = base + j * stride;
            if (i < total) {
                const uint32_t row = i / r.chunks, k = i - row * r.chunks;
                const uint64_t p = r.plane + (uint64_t)row * plane_row_bytes + (uint64_t)k * 16u;
                const uint64_t w = r.window + (uint64_t)row * window_row_bytes + (uint64_t)k * 16u;
                v[j] = *reinterpret_cast<const u32x4*>((TO_WINDOWS ? plane : windows) + (TO_WINDOWS ? p : w));
                dst[j] = TO_WINDOWS ? w : p;
            }
        }
#pragma unroll
        for (int j = 0; j < TILE_UNROLL; ++j)
            if (base + j * stride < total) *reinterpret_cast<u32x4*>((TO_WINDOWS ? windows : plane) + dst[j]) = v[j];
    }
}

__device__ __forceinline__ uint32_t sq_diff4(uint32_t a, uint32_t b) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int d = (int)((a >> k) & 255u) - (int)((b >> k) & 255u);
        s += (uint32_t)(d * d);
    }
    return s;
}

// The uint8 reconstruction's interiors -> image (nullable), and with ref the exact squared error of exactly those pixels:
// per-lane uint64 partial, wave reduction, the block's four wave sums through LDS, one 64-bit atomic per block (every block works
// on one window, so one image). Integer sums: exact and independent of the order. All the blocks of an image add into one word,
// so the launch is sized for few of them (STITCH_CHUNKS_PER_LANE): one atomic per wave of a fine grid serialised on that word and
// took 5x the copy's time.
__global__ __launch_bounds__(TILE_THREADS) void tile_stitch_u8_kernel(const uint8_t* __restrict__ windows, uint8_t* __restrict__ image,
                                                                      const uint8_t* __restrict__ ref, unsigned long long* __restrict__ sse,
                                                                      const int32_t* __restrict__ plan, uint64_t plane_image_bytes,
                                                                      uint64_t plane_row_bytes, int window_h, int window_w,
                                                                      uint64_t window_bytes, uint64_t window_row_bytes) {
    const int g = blockIdx.y;
    const int32_t* row_plan = plan + (size_t)g * EAE_TILE_PLAN_COLS;
    const Rect r = plan_rect(row_plan, g, false, 16, 16, plane_image_bytes, plane_row_bytes, window_h, window_w, window_bytes,
                             window_row_bytes);
    const uint32_t total = r.rows * r.chunks;
    const uint32_t stride = gridDim.x * TILE_THREADS;
    uint64_t acc = 0;
    for (uint32_t base = blockIdx.x * TILE_THREADS + threadIdx.x; base < total; base += stride * TILE_UNROLL) {
        u32x4 v[TILE_UNROLL], q[TILE_UNROLL];
        uint64_t dst[TILE_UNROLL];
#pragma unroll
        for (int j = 0; j < TILE_UNROLL; ++j) {
            const uint32_t i = base + j * stride;
            if (i < total) {
                const uint32_t row = i / r.chunks, k = i - row * r.chunks;
                dst[j] = r.plane + (uint64_t)row * plane_row_bytes + (uint64_t)k * 16u;
                v[j] = *reinterpret_cast<const u32x4*>(windows + r.window + (uint64_t)row * window_row_bytes + (uint64_t)k * 16u);
                if (ref) q[j] = *reinterpret_cast<const u32x4*>(ref + dst[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < TILE_UNROLL; ++j) {
            if (base + j * stride < total) {
                if (image) *reinterpret_cast<u32x4*>(image + dst[j]) = v[j];
                if (ref) acc += sq_diff4(v[j].x, q[j].x) + sq_diff4(v[j].y, q[j].y) + sq_diff4(v[j].z, q[j].z) + sq_diff4(v[j].w, q[j].w);
            }
        }
    }
    if (ref) {
        __shared__ unsigned long long wave_sums[TILE_THREADS / 64];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor((unsigned long long)acc, m, 64);
        if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long total_sse = 0;
#pragma unroll
            for (int k = 0; k < TILE_THREADS / 64; ++k) total_sse += wave_sums[k];
            if (total_sse) atomicAdd(sse + row_plan[0], total_sse);
        }
    }
}

// Blocks per window: about `per_lane` chunks per lane, at least one block.
constexpr int COPY_CHUNKS_PER_LANE = TILE_UNROLL;
constexpr int STITCH_CHUNKS_PER_LANE = 4 * TILE_UNROLL;
unsigned blocks_per_window(uint64_t window_chunks, int per_lane) {
    const uint64_t per_block = (uint64_t)TILE_THREADS * per_lane;
    const uint64_t b = (window_chunks + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > 65535 ? 65535 : b));
}

// The argument checks both entry points share. Plane [n][h * unit][w * unit][elem_bytes], windows [n_windows][window_h * unit]
// [window_w * unit][elem_bytes]; every plan row must name rectangles inside both, its interior inside its window and at the
// same place of the image. Returns 0 or the EAE_HIP_* code.
int check_tile_args(const void* plane, int n, int h, int w, const void* windows, int window_h, int window_w, int unit,
                    int elem_bytes, const int32_t* plan, const int32_t* host_plan, int n_windows) {
    if (!plane || !windows || !plan || !host_plan) return EAE_HIP_BAD_ARGUMENT;
    if (n <= 0 || h <= 0 || w <= 0 || window_h <= 0 || window_w <= 0 || unit <= 0 || elem_bytes <= 0 || n_windows < 0)
        return EAE_HIP_BAD_ARGUMENT;
    const uint64_t unit_bytes = (uint64_t)unit * elem_bytes;
    if (unit_bytes % 16 != 0 || ((uintptr_t)plane & 15u) != 0 || ((uintptr_t)windows & 15u) != 0) return EAE_HIP_BAD_SHAPE;
    if (window_h > h || window_w > w) return EAE_HIP_BAD_SHAPE;
    // a window's chunk index and the grid are 32-bit
    if ((uint64_t)window_h * unit * window_w * (unit_bytes / 16) > 0x7FFFFFFFull || n_windows > 65535) return EAE_HIP_BAD_SHAPE;
    for (int g = 0; g < n_windows; ++g) {
        const int32_t* p = host_plan + (size_t)g * EAE_TILE_PLAN_COLS;
        const bool ok = p[0] >= 0 && p[0] < n && p[1] >= 0 && p[1] <= h - window_h && p[2] >= 0 && p[2] <= w - window_w &&
                        p[3] >= 0 && p[4] >= 0 && p[7] >= 0 && p[8] >= 0 && p[3] <= window_h - p[7] && p[4] <= window_w - p[8] &&
                        p[5] == p[1] + p[3] && p[6] == p[2] + p[4];
        if (!ok) return EAE_HIP_BAD_SHAPE;
    }
    return EAE_HIP_OK;
}

}  // namespace

extern "C" int eae_hip_tile_copy(void* plane, int n, int h, int w, void* windows, int window_h, int window_w, int unit,
                                 int elem_bytes, const int32_t* plan, const int32_t* host_plan, int n_windows, int to_windows,
                                 void* stream) {
    const int status = check_tile_args(plane, n, h, w, windows, window_h, window_w, unit, elem_bytes, plan, host_plan, n_windows);
    if (status != EAE_HIP_OK || n_windows == 0) return status;
    const int unit_bytes = unit * elem_bytes;
    const uint64_t plane_row_bytes = (uint64_t)w * unit_bytes;
    const uint64_t plane_image_bytes = (uint64_t)h * unit * plane_row_bytes;
    const uint64_t window_row_bytes = (uint64_t)window_w * unit_bytes;
    const uint64_t window_bytes = (uint64_t)window_h * unit * window_row_bytes;
    const dim3 grid(blocks_per_window(window_bytes / 16, COPY_CHUNKS_PER_LANE), (unsigned)n_windows);
    if (to_windows)
        hipLaunchKernelGGL(tile_copy_kernel<true>, grid, dim3(TILE_THREADS), 0, (hipStream_t)stream, (uint8_t*)plane, (uint8_t*)windows,
                           plan, unit, unit_bytes, plane_image_bytes, plane_row_bytes, window_h, window_w, window_bytes, window_row_bytes);
    else
        hipLaunchKernelGGL(tile_copy_kernel<false>, grid, dim3(TILE_THREADS), 0, (hipStream_t)stream, (uint8_t*)plane, (uint8_t*)windows,
                           plan, unit, unit_bytes, plane_image_bytes, plane_row_bytes, window_h, window_w, window_bytes, window_row_bytes);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_tile_stitch_u8(const uint8_t* windows, int window_h, int window_w, uint8_t* image, const uint8_t* ref_u8,
                                      uint64_t* sse, int n, int h, int w, const int32_t* plan, const int32_t* host_plan, int n_windows,
                                      void* stream) {
    if ((!image && !ref_u8) || (ref_u8 && !sse)) return EAE_HIP_BAD_ARGUMENT;
    if ((ref_u8 && ((uintptr_t)ref_u8 & 15u) != 0) || (image && ref_u8 && ((uintptr_t)image & 15u) != 0)) return EAE_HIP_BAD_SHAPE;
    const int status = check_tile_args(image ? (const void*)image : (const void*)ref_u8, n, h, w, windows, window_h, window_w, 16, 1,
                                       plan, host_plan, n_windows);
    if (status != EAE_HIP_OK || n_windows == 0) return status;
    const uint64_t plane_row_bytes = (uint64_t)w * 16;
    const uint64_t plane_image_bytes = (uint64_t)h * 16 * plane_row_bytes;
    const uint64_t window_row_bytes = (uint64_t)window_w * 16;
    const uint64_t window_bytes = (uint64_t)window_h * 16 * window_row_bytes;
    const dim3 grid(blocks_per_window(window_bytes / 16, ref_u8 ? STITCH_CHUNKS_PER_LANE : COPY_CHUNKS_PER_LANE), (unsigned)n_windows);
    hipLaunchKernelGGL(tile_stitch_u8_kernel, grid, dim3(TILE_THREADS), 0, (hipStream_t)stream, windows, image, ref_u8,
                       reinterpret_cast<unsigned long long*>(sse), plan, plane_image_bytes, plane_row_bytes, window_h, window_w,
                       window_bytes, window_row_bytes);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
