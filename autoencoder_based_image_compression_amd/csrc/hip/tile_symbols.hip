// tile_symbols.hip -- the two data movers of the tile-indexed container EAT1 (container.py).
// The coder reads every map as one contiguous run of symbols. A coding tile of a map is a rectangle of the map's plane, so the
// encoder gathers the tiles of a group into tile-major runs first, and the decoder turns the decoded tile-major runs back into the
// NHWC float latents the synthesis reads, dequantising on the way. Both are pure HBM copies.
//
// Plan row (int64, EAE_TILE_SYMBOLS_PLAN_COLS per tile, coordinates in latents):
//   [0] image  [1, 2] tile origin (row, col)  [3, 4] tile extent (rows, cols)  [5] element offset of the tile's map 0 in the
//   tile-major buffer; map m of the tile starts at [5] + m * rows * cols, pixels in raster order inside the tile.
// gather: the origin is in the symbol plane and the tile lies inside it. dequantize: image and origin are in the output sub-plane;
// the origin may be negative and the tile may reach past the sub-plane: only the pixels inside it are written.
// dequantize_placed (codec.RegionDecoder) splits the row: what never changes -- extent and offset, int64
// [EAE_TILE_SYMBOLS_SLOT_COLS] per slot -- is checked on the host like a plan row, and image and origin come from an int32
// [n_slots][4] array in device memory that the kernel reads and trusts for nothing.
#include "common.h"

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_UNROLL = 4;         // symbols in flight per lane: four loads issued before the first store
constexpr int DQ_PIX = 64;           // pixels per block of the dequantising transpose
constexpr int DQ_PITCH = EAE_C + 4;  // int16 per pixel row in LDS: 264 bytes keeps every row 8-byte aligned for ds_read_b64

// blockIdx.y = tile of the group, blockIdx.x = map. The destination run is contiguous; the source is `rows` row segments of
// the map. 2-byte loads and stores, consecutive lanes on consecutive symbols of both sides.
__global__ __launch_bounds__(TS_THREADS) void tile_symbols_gather_kernel(const int16_t* __restrict__ symbols, int16_t* __restrict__ out,
                                                                         const int64_t* __restrict__ plan, int64_t map_elems, int64_t w) {
    const int64_t* row = plan + (size_t)blockIdx.y * EAE_TILE_SYMBOLS_PLAN_COLS;
    const int64_t img = row[0], r0 = row[1], c0 = row[2], off = row[5];
    const uint32_t cols = (uint32_t)row[4];
    const uint32_t total = (uint32_t)row[3] * cols;
    const int m = blockIdx.x;
    const int16_t* src = symbols + (img * EAE_C + m) * map_elems + r0 * w + c0;
    int16_t* dst = out + off + (int64_t)m * total;
    for (uint32_t base = threadIdx.x; base < total; base += TS_THREADS * TS_UNROLL) {
        int16_t v[TS_UNROLL];
#pragma unroll
        for (int j = 0; j < TS_UNROLL; ++j) {
            const uint32_t i = base + j * TS_THREADS;
            if (i < total) {
                const uint32_t r = i / cols, c = i - r * cols;
                v[j] = src[(int64_t)r * w + c];
            }
        }
#pragma unroll
        for (int j = 0; j < TS_UNROLL; ++j) {
            const uint32_t i = base + j * TS_THREADS;
            if (i < total) dst[i] = v[j];
        }
    }
}

// blockIdx.y = tile, blockIdx.x = chunk of 64 pixels of the tile. Symbols of the chunk -> LDS as [pixel][map] (the global reads
// run along the pixels of one map, 128 bytes per wave), then every pixel's 128 channels leave as 32 16-byte stores of 4 channels.
// Exactly the arithmetic of dequantize_kernel (csrc/hip/container.hip): cq = bw * symbol, then cq + mean, no contraction.
// LDS: the reads are ds_read_b64 at dword 66 * pixel + 2 * quad, so each half-wave covers the 64 banks once; the 2-byte writes of a
// half-wave fall on 16 banks twice.
// ROWS: bin_widths and map_mean hold one row of 128 per image, f32 [n][128], and the block takes the row of its plan row's image
// (eae_hip_tile_symbols_dequantize_rows); else one row serves every image.
// PLACED: (rows, cols, offset) of the block's tile come from the static `plan` of EAE_TILE_SYMBOLS_SLOT_COLS columns, and (image,
// origin row, origin col) from placement[blockIdx.y][0..2], int32 words a step leaves in device memory: any value is harmless. An
// image outside [0, n) ends the block in front of every barrier and every access; the origins only ever enter the test that keeps
// a pixel inside hs x ws (64-bit sums of a 32-bit origin and a pixel index below 2^31). The rows are per image as with ROWS.
template <bool ROWS, bool PLACED>
__device__ __forceinline__ void tile_symbols_dequantize_body(const int16_t* __restrict__ tiles, const int64_t* __restrict__ plan,
                                                             const int32_t* __restrict__ placement, int64_t n,
                                                             const float* __restrict__ bin_widths, const float* __restrict__ map_mean,
                                                             float* __restrict__ out, int64_t hs, int64_t ws) {
    __shared__ __attribute__((aligned(16))) int16_t lds[DQ_PIX][DQ_PITCH];
    int64_t img, r0, c0, off;
    uint32_t cols, total;
    if (PLACED) {
        const int64_t* row = plan + (size_t)blockIdx.y * EAE_TILE_SYMBOLS_SLOT_COLS;
        const int32_t* place = placement + (size_t)blockIdx.y * 4;
        img = place[0], r0 = place[1], c0 = place[2], off = row[2];
        cols = (uint32_t)row[1];
        total = (uint32_t)row[0] * cols;
        if (img < 0 || img >= n) return;                       // block-uniform: an absent slot
    } else {
        const int64_t* row = plan + (size_t)blockIdx.y * EAE_TILE_SYMBOLS_PLAN_COLS;
        img = row[0], r0 = row[1], c0 = row[2], off = row[5];
        cols = (uint32_t)row[4];
        total = (uint32_t)row[3] * cols;
    }
    const uint32_t p0 = blockIdx.x * DQ_PIX;
    if (p0 >= total) return;                                   // block-uniform: this tile has fewer chunks than the largest
    const int16_t* src = tiles + off;
    const int tid = threadIdx.x;
    for (int i = tid; i < EAE_C * DQ_PIX; i += TS_THREADS) {
        const int ch = i >> 6, px = i & (DQ_PIX - 1);
        const uint32_t p = p0 + px;
        lds[px][ch] = p < total ? src[(int64_t)ch * total + p] : (int16_t)0;
    }
    __syncthreads();
    const int q = tid & 31, sub = tid >> 5;                    // channel quad, pixel of the pass
    float bw[4], m[4];
    if (ROWS) {
        bin_widths += img * EAE_C;
        if (map_mean) map_mean += img * EAE_C;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bw[k] = bin_widths[4 * q + k];
        m[k] = map_mean ? map_mean[4 * q + k] : 0.f;
    }
    for (int pass = 0; pass < DQ_PIX / 8; ++pass) {
        const int px = pass * 8 + sub;
        const uint32_t p = p0 + px;
        if (p >= total) break;
        const uint32_t r = p / cols, c = p - r * cols;
        const int64_t R = r0 + r, C = c0 + c;
        if (R < 0 || R >= hs || C < 0 || C >= ws) continue;
        const uint2 packed = *reinterpret_cast<const uint2*>(&lds[px][4 * q]);
        const int16_t s[4] = {(int16_t)(packed.x & 0xFFFFu), (int16_t)(packed.x >> 16), (int16_t)(packed.y & 0xFFFFu), (int16_t)(packed.y >> 16)};
        float4 v;
        float* vf = reinterpret_cast<float*>(&v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float cq = bw[k] * (float)s[k];
            vf[k] = cq + m[k];
        }
        *reinterpret_cast<float4*>(out + ((img * hs + R) * ws + C) * EAE_C + 4 * q) = v;
    }
}

__global__ __launch_bounds__(TS_THREADS) void tile_symbols_dequantize_kernel(const int16_t* __restrict__ tiles, const int64_t* __restrict__ plan,
                                                                             const float* __restrict__ bin_widths, const float* __restrict__ map_mean,
                                                                             float* __restrict__ out, int64_t hs, int64_t ws) {
    tile_symbols_dequantize_body<false, false>(tiles, plan, nullptr, 0, bin_widths, map_mean, out, hs, ws);
}

__global__ __launch_bounds__(TS_THREADS) void tile_symbols_dequantize_rows_kernel(const int16_t* __restrict__ tiles, const int64_t* __restrict__ plan,
                                                                                  const float* __restrict__ bin_widths_rows,
                                                                                  const float* __restrict__ map_mean_rows, float* __restrict__ out,
                                                                                  int64_t hs, int64_t ws) {
    tile_symbols_dequantize_body<true, false>(tiles, plan, nullptr, 0, bin_widths_rows, map_mean_rows, out, hs, ws);
}

__global__ __launch_bounds__(TS_THREADS) void tile_symbols_dequantize_placed_kernel(const int16_t* __restrict__ tiles, const int64_t* __restrict__ slots,
                                                                                    const int32_t* __restrict__ placement, int64_t n,
                                                                                    const float* __restrict__ bin_widths_rows,
                                                                                    const float* __restrict__ map_mean_rows, float* __restrict__ out,
                                                                                    int64_t hs, int64_t ws) {
    tile_symbols_dequantize_body<true, true>(tiles, slots, placement, n, bin_widths_rows, map_mean_rows, out, hs, ws);
}

// Largest tile of a plan (pixels), or -1 when a row is malformed. `inside`: rows must lie in an n x h x w plane (gather);
// otherwise only the image index is checked against n and the origin is free (dequantize). Every tile's run must fit in
// `buffer_elems` symbols.
int64_t check_symbols_plan(const int64_t* host_plan, int n_tiles, int64_t n, int64_t h, int64_t w, bool inside, int64_t buffer_elems) {
    int64_t largest = 0;
    for (int t = 0; t < n_tiles; ++t) {
        const int64_t* p = host_plan + (size_t)t * EAE_TILE_SYMBOLS_PLAN_COLS;
        if (p[0] < 0 || p[0] >= n || p[3] < 1 || p[4] < 1 || p[5] < 0) return -1;
        if (p[3] > 0x7FFFFFFFll || p[4] > 0x7FFFFFFFll || p[3] * p[4] > 0x7FFFFFFFll) return -1;   // a tile's pixel index is 32-bit
        if (inside && (p[1] < 0 || p[2] < 0 || p[1] > h - p[3] || p[2] > w - p[4])) return -1;
        if (!inside && (p[1] < -0x7FFFFFFFll || p[1] > 0x7FFFFFFFll || p[2] < -0x7FFFFFFFll || p[2] > 0x7FFFFFFFll)) return -1;
        if (p[5] > buffer_elems || EAE_C * p[3] * p[4] > buffer_elems - p[5]) return -1;
        if (p[3] * p[4] > largest) largest = p[3] * p[4];
    }
    return largest;
}

}  // namespace

extern "C" int eae_hip_tile_symbols_gather(const int16_t* symbols_planar, int n, int h, int w, int16_t* tiles, int64_t tile_elems,
                                           const int64_t* plan, const int64_t* host_plan, int n_tiles, void* stream) {
    if (!symbols_planar || !tiles || !plan || !host_plan || n <= 0 || h <= 0 || w <= 0 || tile_elems <= 0 || n_tiles < 0)
        return EAE_HIP_BAD_ARGUMENT;
    if (n_tiles > 65535 || check_symbols_plan(host_plan, n_tiles, n, h, w, true, tile_elems) < 0) return EAE_HIP_BAD_SHAPE;
    if (n_tiles == 0) return EAE_HIP_OK;
    hipLaunchKernelGGL(tile_symbols_gather_kernel, dim3(EAE_C, (unsigned)n_tiles), dim3(TS_THREADS), 0, (hipStream_t)stream,
                       symbols_planar, tiles, plan, (int64_t)h * w, (int64_t)w);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

namespace {

// The argument checks and the launch of both dequantising entry points; `rows`: one row of bin widths and means per image.
int launch_symbols_dequantize(bool rows, const int16_t* tiles, int64_t tile_elems, const int64_t* plan, const int64_t* host_plan, int n_tiles,
                              const float* bin_widths, const float* map_mean, float* shifted_out, int n, int hs, int ws, void* stream) {
    if (!tiles || !plan || !host_plan || !bin_widths || !shifted_out || tile_elems <= 0 || n_tiles < 0 || n <= 0 || hs <= 0 || ws <= 0)
        return EAE_HIP_BAD_ARGUMENT;
    if (((uintptr_t)shifted_out & 15u) != 0 || n_tiles > 65535) return EAE_HIP_BAD_SHAPE;
    const int64_t largest = check_symbols_plan(host_plan, n_tiles, n, hs, ws, false, tile_elems);
    if (largest < 0) return EAE_HIP_BAD_SHAPE;
    if (n_tiles == 0) return EAE_HIP_OK;
    const dim3 grid((unsigned)((largest + DQ_PIX - 1) / DQ_PIX), (unsigned)n_tiles);
    if (rows)
        hipLaunchKernelGGL(tile_symbols_dequantize_rows_kernel, grid, dim3(TS_THREADS), 0, (hipStream_t)stream, tiles, plan, bin_widths,
                           map_mean, shifted_out, (int64_t)hs, (int64_t)ws);
    else
        hipLaunchKernelGGL(tile_symbols_dequantize_kernel, grid, dim3(TS_THREADS), 0, (hipStream_t)stream, tiles, plan, bin_widths, map_mean,
                           shifted_out, (int64_t)hs, (int64_t)ws);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

}  // namespace

extern "C" int eae_hip_tile_symbols_dequantize(const int16_t* tiles, int64_t tile_elems, const int64_t* plan, const int64_t* host_plan,
                                               int n_tiles, const float* bin_widths, const float* map_mean, float* shifted_out, int n,
                                               int hs, int ws, void* stream) {
    return launch_symbols_dequantize(false, tiles, tile_elems, plan, host_plan, n_tiles, bin_widths, map_mean, shifted_out, n, hs, ws, stream);
}

extern "C" int eae_hip_tile_symbols_dequantize_rows(const int16_t* tiles, int64_t tile_elems, const int64_t* plan, const int64_t* host_plan,
                                                    int n_tiles, const float* bin_widths_rows, const float* map_mean_rows, float* shifted_out,
                                                    int n, int hs, int ws, void* stream) {
    return launch_symbols_dequantize(true, tiles, tile_elems, plan, host_plan, n_tiles, bin_widths_rows, map_mean_rows, shifted_out, n, hs, ws,
                                     stream);
}

namespace {

// check_symbols_plan for the static half of a placed plan: extent and offset of every slot, nothing about image and origin (the
// kernel checks those, step by step). Largest slot (pixels), or -1 when a row is malformed or its run leaves `buffer_elems` symbols.
int64_t check_symbols_slots(const int64_t* host_slots, int n_slots, int64_t buffer_elems) {
    int64_t largest = 0;
    for (int t = 0; t < n_slots; ++t) {
        const int64_t* p = host_slots + (size_t)t * EAE_TILE_SYMBOLS_SLOT_COLS;
        if (p[0] < 1 || p[1] < 1 || p[2] < 0) return -1;
        if (p[0] > 0x7FFFFFFFll || p[1] > 0x7FFFFFFFll || p[0] * p[1] > 0x7FFFFFFFll) return -1;   // a tile's pixel index is 32-bit
        if (p[2] > buffer_elems || EAE_C * p[0] * p[1] > buffer_elems - p[2]) return -1;
        if (p[0] * p[1] > largest) largest = p[0] * p[1];
    }
    return largest;
}

}  // namespace

extern "C" int eae_hip_tile_symbols_dequantize_placed(const int16_t* tiles, int64_t tile_elems, const int64_t* slots, const int64_t* host_slots,
                                                      int n_slots, const int32_t* placement, const float* bin_widths_rows,
                                                      const float* map_mean_rows, float* shifted_out, int n, int hs, int ws, void* stream) {
    if (!tiles || !slots || !host_slots || !placement || !bin_widths_rows || !shifted_out || tile_elems <= 0 || n_slots < 0 || n <= 0 ||
        hs <= 0 || ws <= 0)
        return EAE_HIP_BAD_ARGUMENT;
    if (((uintptr_t)shifted_out & 15u) != 0 || ((uintptr_t)placement & 3u) != 0 || n_slots > 65535) return EAE_HIP_BAD_SHAPE;
    const int64_t largest = check_symbols_slots(host_slots, n_slots, tile_elems);
    if (largest < 0) return EAE_HIP_BAD_SHAPE;
    if (n_slots == 0) return EAE_HIP_OK;
    const dim3 grid((unsigned)((largest + DQ_PIX - 1) / DQ_PIX), (unsigned)n_slots);
    hipLaunchKernelGGL(tile_symbols_dequantize_placed_kernel, grid, dim3(TS_THREADS), 0, (hipStream_t)stream, tiles, slots, placement,
                       (int64_t)n, bin_widths_rows, map_mean_rows, shifted_out, (int64_t)hs, (int64_t)ws);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
