// ladder.hip -- one pass over the latents for the K rate points of a ladder: per (image, rate point, map) the histogram of
// |symbol| clipped at the truncated unary length L, and the exact length of the bypass stream. The histogram is what
// lossless/stats.py:181-195 counts its binary decisions from (the tables of stats.py:13-68, one per multiplier) and what the
// arithmetic-coded stream's ideal cost is a sum over; the bypass length is LosslessCoder.cpp:22-37, 58-111, 232-252 (one sign bit
// per non-zero symbol, 2 n + 1 bits of Exp-Golomb suffix for |s| >= L). The symbol of every element at every point is the `rs` of
// quantize_kernel (quantize.hip), expression for expression: both divisions, both round-half-even, no contraction.
//
// Shape. y is [N][hw][128]: a lane owns a channel, so a wave's 64 lanes read 256 contiguous bytes and address 64 different columns
// of the block's LDS array [K][L + 1][128] -- ds_add_u32 banks are (address / 4) % 32 per 32-lane half, the column is the bank,
// whatever bin each lane counts into: no bank conflict, and no contention inside a wave. The four pixel rows of a block share the
// columns, so the counts are LDS adds (no return value, nothing waits for them). Bypass bits go to a second array [K][128], the
// bin widths of the K points sit in a third, read once from memory per block: (L + 3) * 512 bytes of LDS per point, 64 KB per
// block at most (eae_hip_ladder_max_points: 9 points at L = 10, 59.9 KB).
// A block takes `pixels` consecutive pixels of one image, chosen by the launcher so that the grid is at most two blocks per compute
// unit (what the LDS lets a CU hold: one block more is a second round, +30 % at K = 9) and never below 64: the flush is one global
// atomic per non-zero (k, bin, channel) of the block, 256 contiguous bytes per wave-instruction, and has to stay small beside the
// pixels * K * 128 symbols counted.
//
// Bound. 24 Kodak-sized images are 4.7 M latents, 18.9 MB read once: 3.2 us at the copy rate of DESIGN.md section 11. Every latent
// costs 2 K correctly rounded divisions (11 vector instructions each, the v_rcp_f32 at a quarter of the rate) plus two v_rndne, the
// bit count and two LDS adds: about 40 vector instructions per (latent, point), 26 M wave-instructions at K = 9 over 1024 SIMDs,
// 45 us and more at four cycles each. The divisions bind, not the HBM read. Measured (profiles/rate_ladder.md): 22 / 38 / 84 us at
// K = 1 / 3 / 9, 7.7 us per point.
//
// Tiles (eae_hip_ladder_histograms_tiles). The same counts per coding tile of th x tw latents: hist
// [N][K][T][128][L + 1], bypass_bits [N][K][T][128], T tiles row-major. The LDS array and the lane-is-a-channel layout stay; what
// changes is which pixels a block owns: tw consecutive pixels per row over th rows, walked in the tile's raster order, four pixels
// at a time. A block's LDS holds ONE set of counts (60 KB at K = 9), so a block serves one tile at a time and flushes K (L + 1) 128
// words per tile it touches. The launcher decides per shape:
//   * fewer tiles than two blocks per compute unit (24 images, tiles of 16: 144 tiles for 512 blocks): a tile is cut into chunks of
//     whole pixel rows of the block, as many as fill the grid, none below LADDER_MIN_PIXELS -- three chunks of 88 / 88 / 80 pixels
//     there, 432 blocks, a flush per 85 pixels where the whole-map kernel flushes per 76;
//   * that many tiles or more (tiles of 8: 576): whole tiles, dealt evenly to two blocks per compute unit, a block flushing after
//     each and finding its arrays zero again (the flush clears what it adds). 64 pixels per flush is the floor of the whole-map
//     kernel too; below it (edge tiles, tiles of 4) the flush leads: 12.7 K LDS words read per tile at K = 9, L = 10 whatever the
//     tile holds, though only the non-zero ones become atomics.
// Bound: the divisions, as above -- the same 40 vector instructions per (latent, point); the flush adds K (L + 1) 128 / 512 = 25
// LDS reads per thread and tile. Zeroing the accumulators is the caller's: N K T 128 (L + 1) 4 bytes, 7.3 MB at 24 Kodak images
// with tiles of 16, 29 MB with tiles of 8. Measured (profiles/tiled_budget_codec.md; 24 x 32 x 48 latents, K = 9, L = 10, device
// events, median of 30): 96.9 us with tiles of 16 against 82.5 us for ladder_kernel on the same latents (1.18), 140.3 us with tiles
// of 8 (1.70): 576 tiles on 512 blocks leave 64 blocks a second tile, 128 pixels where ladder_kernel's block counts 76 -- a second
// round of work, not the flush. Zeroing 8.6 / 34.5 MB of accumulators: 7.2 / 9.5 us.
//
// RDO (eae_hip_ladder_histograms_rdo, eae_hip_ladder_histograms_rdo_tiles). The same counts of the symbols the
// rate-distortion optimised quantiser chooses (latent_rows.hip, ratecontrol.rdo_quantize_numpy): before cq = bw r, an r of magnitude a
// in [1, min(L, 16)] goes one step nearer zero where 2 u + 1 < T[k][c][a - 1], u = |x| - a. The two kernel bodies are templates over
// what `ladder_round` is handed: NoRdo (nothing; ladder_kernel and ladder_tiles_kernel keep their signatures, their 660 and 1417
// instructions -- the scalar prologue is scheduled in another order, the loops are the same -- and their LDS) or Rdo (the table and
// min(L, 16)): no run-time branch in either instantiation, 33 VGPRs and no scratch in both whole-map kernels, 36 / 41 in the tiles'.
// Where the thresholds live. A lane owns a channel here (in rdo_rows_kernel a half-wave shares one), so [K][128][16] would be a gather
// of up to 64 rows of 64 bytes per load. Two designs:
//   (a) a copy BY MAGNITUDE, [K][16][128], made once by the caller (device.rdo_thresholds_by_magnitude), read from memory: the lanes
//       of a wave that hold the same magnitude read 256 contiguous bytes, a wave touches at most min(L, 16) such rows per point, the
//       whole table is 74 KB at K = 9 (L2-resident), and only an eligible lane loads -- a wave without one (most waves at a coarse
//       point) skips the instruction; the LDS budget, hence eae_hip_ladder_max_points, is the nearest-rounding kernels';
//   (b) the rows [K][min(L, 16)][128] staged in LDS beside the bins, conflict-free like them: 106 KB per block at K = 9, L = 10. The
//       device grants it (163,840 bytes of LDS per block on gfx950, read from its attributes), but a compute unit then holds ONE
//       block where it holds two today, and this file's launchers size their grids for two.
// (a) is what is built. Measured (profiles/rdo_ladder.md; 24 x 32 x 48 latents, K = 9, L = 10, lambda = 2 bw^2, device events,
// median of 30): 103.8 us against 81.6 us for ladder_kernel on the same latents (1.27), 122.1 against 95.8 at tiles of 16 (1.28),
// 188.7 against 140.8 at tiles of 8 (1.34) -- and the same times, within 1 us, with a table of zeros, where every load returns 0 and
// nothing is lowered. So what the count pays is the rule's arithmetic per (latent, point) -- the quotient kept, |r|, u, two compares,
// the row's address, the select and copysign: 742 instructions against 660 -- on a kernel its divisions already bind, not the table:
// there is no load time for (b) to win back, and it would cost half the occupancy. (b) was therefore not built.
#include "common.h"

namespace {
constexpr int LADDER_ROWS = 4;                      // pixel rows of a block; one channel per lane
constexpr int LADDER_THREADS = LADDER_ROWS * EAE_C;
constexpr int LADDER_LDS_BYTES = 64 * 1024;         // what one block may ask for
constexpr int LADDER_MIN_PIXELS = 64;
constexpr int LADDER_MAX_PIXELS = 1 << 20;          // 34 bypass bits per symbol at most: a block's sums fit 32 bits

constexpr int RDO_MAGNITUDES = 16;                  // ratecontrol.RDO_MAGNITUDES: the magnitudes 1 .. 16 have a threshold

// What the rate-distortion optimised count knows beyond the nearest-rounding one (file header, "RDO"): the thresholds of the K
// points by magnitude, [K][16][128], and min(L, 16) as a float. NoRdo is the nearest-rounding count's: nothing.
struct NoRdo {};
struct Rdo {
    const float* __restrict__ thresholds;           // [K][RDO_MAGNITUDES][128], in memory
    float amax;
};

// The r of one latent at point k: the nearest integer of the quotient ...
__device__ __forceinline__ float ladder_round(NoRdo, float centered, float bw, int, int) { return round_half_even(centered / bw); }

// ... or, statement for statement rdo_rows_kernel's and ratecontrol.rdo_quantize_numpy's, one step nearer zero where 2 u + 1 is below
// the threshold of (k, c, a). Only an eligible lane loads (a in [1, amax], tested in float: a NaN, an infinity or a huge a never
// becomes an index), so a wave without one -- most waves at a coarse point -- issues no load at all; t = 0 lowers nothing, 2 u + 1
// being at least 0.
__device__ __forceinline__ float ladder_round(Rdo rdo, float centered, float bw, int k, int c) {
    const float x = centered / bw;
    const float r = round_half_even(x);
    const float a = fabsf(r);
    const float u = fabsf(x) - a;
    float t = 0.f;
    if (a >= 1.f && a <= rdo.amax) t = rdo.thresholds[((size_t)k * RDO_MAGNITUDES + ((int)a - 1)) * EAE_C + c];
    return 2.f * u + 1.f < t ? r - copysignf(1.f, r) : r;
}

// One latent (already centred) of channel c at the K points: its bin and its bypass bits into the block's LDS arrays.
template <class R>
__device__ __forceinline__ void count_latent(R rdo, float centered, int c, int k_points, int length, const float* widths, unsigned int* bins,
                                             unsigned int* bits, unsigned int* __restrict__ range_errors) {
    const int nb = length + 1;
#pragma unroll 2
    for (int k = 0; k < k_points; ++k) {
        const float bw = widths[k * EAE_C + c];
        const float r = ladder_round(rdo, centered, bw, k, c);
        const float cq = bw * r;
        const float rs = round_half_even(cq / bw);              // compression.py:142: from cq / bw again, not from r
        if (!(fabsf(rs) < 32768.f)) {                           // tools.py:130-132: no bin, no bits (rare: straight to memory)
            if (range_errors) atomicAdd(&range_errors[k], 1u);
            continue;
        }
        const int a = (int)fabsf(rs);
        atomicAdd(&bins[(k * nb + min(a, length)) * EAE_C + c], 1u);
        unsigned int b = a != 0 ? 1u : 0u;                      // the sign
        if (a >= length) b += 2u * (31u - (unsigned int)__clz(a - length + 1)) + 1u;   // Exp-Golomb order 0 of |s| - L
        if (b) atomicAdd(&bits[k * EAE_C + c], b);
    }
}

template <class R>
__device__ __forceinline__ void ladder_body(R rdo, const float* __restrict__ y, const float* __restrict__ map_mean,
                                            const float* __restrict__ bin_widths_points, int k_points, int length,
                                            unsigned int* __restrict__ hist, unsigned long long* __restrict__ bypass_bits,
                                            unsigned int* __restrict__ range_errors, int hw, int chunks, int pixels) {
    extern __shared__ unsigned int lds[];
    const int nb = length + 1;
    unsigned int* bins = lds;                                        // [K][L + 1][128]
    unsigned int* bits = bins + k_points * nb * EAE_C;               // [K][128]
    float* widths = reinterpret_cast<float*>(bits + k_points * EAE_C);   // [K][128]
    const int tid = threadIdx.x;
    const int c = tid & (EAE_C - 1), row = tid >> 7;
    const int img = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    for (int i = tid; i < k_points * (nb + 1) * EAE_C; i += LADDER_THREADS) lds[i] = 0u;
    for (int i = tid; i < k_points * EAE_C; i += LADDER_THREADS) widths[i] = bin_widths_points[i];
    __syncthreads();
    const float m = map_mean ? map_mean[c] : 0.f;
    const int p0 = chunk * pixels;
    const int p1 = min(p0 + pixels, hw);
    const float* yc = y + (size_t)img * hw * EAE_C + c;
    for (int pix = p0 + row; pix < p1; pix += LADDER_ROWS)
        count_latent(rdo, yc[(size_t)pix * EAE_C] - m, c, k_points, length, widths, bins, bits, range_errors);
    __syncthreads();
    // flush in the outputs' order, [K][128][L + 1] and [K][128] of this image: consecutive lanes, consecutive addresses
    const int per_point = EAE_C * nb;
    unsigned int* h = hist + (size_t)img * k_points * per_point;
    for (int g = tid; g < k_points * per_point; g += LADDER_THREADS) {
        const int k = g / per_point, rem = g - k * per_point;
        const int ch = rem / nb, bin = rem - ch * nb;
        const unsigned int v = bins[(k * nb + bin) * EAE_C + ch];
        if (v) atomicAdd(&h[g], v);
    }
    if (bypass_bits) {
        unsigned long long* bb = bypass_bits + (size_t)img * k_points * EAE_C;
        for (int g = tid; g < k_points * EAE_C; g += LADDER_THREADS)
            if (bits[g]) atomicAdd(&bb[g], (unsigned long long)bits[g]);
    }
}

__global__ __launch_bounds__(LADDER_THREADS) void ladder_kernel(const float* __restrict__ y, const float* __restrict__ map_mean,
                                                                const float* __restrict__ bin_widths_points, int k_points, int length,
                                                                unsigned int* __restrict__ hist, unsigned long long* __restrict__ bypass_bits,
                                                                unsigned int* __restrict__ range_errors, int hw, int chunks, int pixels) {
    ladder_body(NoRdo{}, y, map_mean, bin_widths_points, k_points, length, hist, bypass_bits, range_errors, hw, chunks, pixels);
}

__global__ __launch_bounds__(LADDER_THREADS) void ladder_rdo_kernel(const float* __restrict__ y, const float* __restrict__ map_mean,
                                                                    const float* __restrict__ bin_widths_points,
                                                                    const float* __restrict__ thresholds, float amax, int k_points, int length,
                                                                    unsigned int* __restrict__ hist, unsigned long long* __restrict__ bypass_bits,
                                                                    unsigned int* __restrict__ range_errors, int hw, int chunks, int pixels) {
    ladder_body(Rdo{thresholds, amax}, y, map_mean, bin_widths_points, k_points, length, hist, bypass_bits, range_errors, hw, chunks, pixels);
}

// The same counts per coding tile (file header, "Tiles"). An ITEM is chunk `item % cpt` of entry `item / cpt` = image * T + tile:
// the pixels [chunk * per, (chunk + 1) * per) of the tile's raster (rows x cols of it, cols consecutive pixels per row; an edge
// tile is smaller and may leave its last chunks empty). A block takes the items [items * b / blocks, items * (b + 1) / blocks)
// one after the other and flushes after each: the LDS arrays are zero again when the next one starts.
template <class R>
__device__ __forceinline__ void ladder_tiles_body(
    R rdo, const float* __restrict__ y, const float* __restrict__ map_mean, const float* __restrict__ bin_widths_points, int k_points,
    int length, unsigned int* __restrict__ hist, unsigned long long* __restrict__ bypass_bits, unsigned int* __restrict__ range_errors, int h,
    int w, int th, int tw, int tiles_x, int nb_tiles, int cpt, int per, long items) {
    extern __shared__ unsigned int lds[];
    const int nb = length + 1;
    unsigned int* bins = lds;                                        // [K][L + 1][128]
    unsigned int* bits = bins + k_points * nb * EAE_C;               // [K][128]
    float* widths = reinterpret_cast<float*>(bits + k_points * EAE_C);   // [K][128]
    const int tid = threadIdx.x;
    const int c = tid & (EAE_C - 1), row = tid >> 7;
    for (int i = tid; i < k_points * (nb + 1) * EAE_C; i += LADDER_THREADS) lds[i] = 0u;
    for (int i = tid; i < k_points * EAE_C; i += LADDER_THREADS) widths[i] = bin_widths_points[i];
    __syncthreads();
    const float m = map_mean ? map_mean[c] : 0.f;
    const int per_point = EAE_C * nb;
    const long first = items * (long)blockIdx.x / (long)gridDim.x, last = items * ((long)blockIdx.x + 1) / (long)gridDim.x;
    for (long item = first; item < last; ++item) {
        const int chunk = (int)(item % cpt);
        const long entry = item / cpt;
        const int tile = (int)(entry % nb_tiles);
        const long img = entry / nb_tiles;
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int r0 = ty * th, c0 = tx * tw;
        const int rows = min(th, h - r0), cols = min(tw, w - c0);
        const int q0 = chunk * per, q1 = min(q0 + per, rows * cols);
        if (q0 >= q1) continue;                                      // (the whole block: nothing was counted, nothing to flush)
        const float* yc = y + (size_t)img * h * w * EAE_C + c;
        int q = q0 + row;
        int r = q / cols, col = q - r * cols;
        for (; q < q1; q += LADDER_ROWS) {
            count_latent(rdo, yc[((size_t)(r0 + r) * w + c0 + col) * EAE_C] - m, c, k_points, length, widths, bins, bits, range_errors);
            col += LADDER_ROWS;
            while (col >= cols) { col -= cols; ++r; }
        }
        __syncthreads();
        // flush in the outputs' order, [K][T][128][L + 1] and [K][T][128] of this image, and leave zeros behind
        for (int g = tid; g < k_points * per_point; g += LADDER_THREADS) {
            const int k = g / per_point, rem = g - k * per_point;
            const int ch = rem / nb, bin = rem - ch * nb;
            const unsigned int v = bins[(k * nb + bin) * EAE_C + ch];
            if (v) {
                atomicAdd(&hist[(((size_t)img * k_points + k) * nb_tiles + tile) * per_point + rem], v);
                bins[(k * nb + bin) * EAE_C + ch] = 0u;
            }
        }
        for (int g = tid; g < k_points * EAE_C; g += LADDER_THREADS) {
            const unsigned int v = bits[g];
            if (v) {
                const int k = g >> 7, ch = g & (EAE_C - 1);
                if (bypass_bits) atomicAdd(&bypass_bits[(((size_t)img * k_points + k) * nb_tiles + tile) * EAE_C + ch], (unsigned long long)v);
                bits[g] = 0u;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(LADDER_THREADS) void ladder_tiles_kernel(
    const float* __restrict__ y, const float* __restrict__ map_mean, const float* __restrict__ bin_widths_points, int k_points, int length,
    unsigned int* __restrict__ hist, unsigned long long* __restrict__ bypass_bits, unsigned int* __restrict__ range_errors, int h, int w,
    int th, int tw, int tiles_x, int nb_tiles, int cpt, int per, long items) {
    ladder_tiles_body(NoRdo{}, y, map_mean, bin_widths_points, k_points, length, hist, bypass_bits, range_errors, h, w, th, tw, tiles_x,
                      nb_tiles, cpt, per, items);
}

__global__ __launch_bounds__(LADDER_THREADS) void ladder_rdo_tiles_kernel(
    const float* __restrict__ y, const float* __restrict__ map_mean, const float* __restrict__ bin_widths_points,
    const float* __restrict__ thresholds, float amax, int k_points, int length, unsigned int* __restrict__ hist,
    unsigned long long* __restrict__ bypass_bits, unsigned int* __restrict__ range_errors, int h, int w, int th, int tw, int tiles_x,
    int nb_tiles, int cpt, int per, long items) {
    ladder_tiles_body(Rdo{thresholds, amax}, y, map_mean, bin_widths_points, k_points, length, hist, bypass_bits, range_errors, h, w, th, tw,
                      tiles_x, nb_tiles, cpt, per, items);
}

}  // namespace

extern "C" int eae_hip_ladder_max_points(int length) {
    if (length < 1 || length > 255) return 0;
    return LADDER_LDS_BYTES / ((length + 3) * EAE_C * 4);
}

namespace {
inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline float rdo_amax(int length) { return (float)(length < RDO_MAGNITUDES ? length : RDO_MAGNITUDES); }

// thresholds null: ladder_kernel; else ladder_rdo_kernel (the caller has checked the pointer)
int launch_ladder(const float* y, const float* map_mean, const float* bin_widths_points, const float* thresholds, int k_points, int length,
                  uint32_t* hist, uint64_t* bypass_bits, uint32_t* range_errors, int n, int hw, void* stream) {
    if (!y || !bin_widths_points || !hist || n <= 0 || hw <= 0) return EAE_HIP_BAD_ARGUMENT;
    if (length < 1 || length > 255 || k_points < 1 || k_points > eae_hip_ladder_max_points(length)) return EAE_HIP_BAD_ARGUMENT;
    // at most two blocks per compute unit, LADDER_MIN_PIXELS..LADDER_MAX_PIXELS pixels each, a whole number of pixel rows
    int cus = eae_compute_units();
    if (cus <= 0) cus = 256;
    long chunks = 2L * cus / n;                      // rounded down: one block more than the CUs hold at once is a second round
    const long most = ((long)hw + LADDER_MIN_PIXELS - 1) / LADDER_MIN_PIXELS, least = ((long)hw + LADDER_MAX_PIXELS - 1) / LADDER_MAX_PIXELS;
    if (chunks > most) chunks = most;
    if (chunks < least) chunks = least;
    int pixels = (int)(((long)hw + chunks - 1) / chunks);
    pixels = (pixels + LADDER_ROWS - 1) / LADDER_ROWS * LADDER_ROWS;
    chunks = ((long)hw + pixels - 1) / pixels;
    if ((long)n * chunks > 0x7FFFFFFFL) return EAE_HIP_BAD_SHAPE;
    const size_t lds_bytes = (size_t)k_points * (length + 3) * EAE_C * 4;
    const dim3 grid((unsigned)(n * chunks)), block(LADDER_THREADS);
    unsigned long long* bypass = reinterpret_cast<unsigned long long*>(bypass_bits);
    if (thresholds)
        hipLaunchKernelGGL(ladder_rdo_kernel, grid, block, lds_bytes, (hipStream_t)stream, y, map_mean, bin_widths_points, thresholds,
                           rdo_amax(length), k_points, length, hist, bypass, range_errors, hw, (int)chunks, pixels);
    else
        hipLaunchKernelGGL(ladder_kernel, grid, block, lds_bytes, (hipStream_t)stream, y, map_mean, bin_widths_points, k_points, length, hist,
                           bypass, range_errors, hw, (int)chunks, pixels);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

// thresholds null: ladder_tiles_kernel; else ladder_rdo_tiles_kernel
int launch_ladder_tiles(const float* y, const float* map_mean, const float* bin_widths_points, const float* thresholds, int k_points,
                        int length, uint32_t* hist, uint64_t* bypass_bits, uint32_t* range_errors, int n, int h, int w, int th, int tw,
                        void* stream) {
    if (!y || !bin_widths_points || !hist || n <= 0 || h <= 0 || w <= 0 || th <= 0 || tw <= 0) return EAE_HIP_BAD_ARGUMENT;
    if (length < 1 || length > 255 || k_points < 1 || k_points > eae_hip_ladder_max_points(length)) return EAE_HIP_BAD_ARGUMENT;
    if ((long)h * w > 0x3FFFFFFFL) return EAE_HIP_BAD_SHAPE;       // chunk * per, past the last chunk of a tile, stays an int
    th = th < h ? th : h;                            // container._clamped_coding_tile
    tw = tw < w ? tw : w;
    const long tiles_x = (w + tw - 1) / tw, nb_tiles = (long)((h + th - 1) / th) * tiles_x;
    const long entries = (long)n * nb_tiles;
    if (entries > 0x7FFFFFFFL) return EAE_HIP_BAD_SHAPE;
    // Chunks per tile: as many as bring the grid to two blocks per compute unit, none below LADDER_MIN_PIXELS pixels (a whole
    // number of pixel rows each) or above LADDER_MAX_PIXELS; with that many tiles or more, whole tiles, several per block.
    int cus = eae_compute_units();
    if (cus <= 0) cus = 256;
    const long tile_pixels = (long)th * tw;
    long cpt = 2L * cus / entries;
    const long most = (tile_pixels + LADDER_MIN_PIXELS - 1) / LADDER_MIN_PIXELS, least = (tile_pixels + LADDER_MAX_PIXELS - 1) / LADDER_MAX_PIXELS;
    if (cpt > most) cpt = most;
    if (cpt < least) cpt = least;
    int per = (int)((tile_pixels + cpt - 1) / cpt);
    per = (per + LADDER_ROWS - 1) / LADDER_ROWS * LADDER_ROWS;
    cpt = (tile_pixels + per - 1) / per;
    const long items = entries * cpt;
    if (items > 0x7FFFFFFFL) return EAE_HIP_BAD_SHAPE;
    const long blocks = items < 2L * cus ? items : 2L * cus;
    const size_t lds_bytes = (size_t)k_points * (length + 3) * EAE_C * 4;
    const dim3 grid((unsigned)blocks), block(LADDER_THREADS);
    unsigned long long* bypass = reinterpret_cast<unsigned long long*>(bypass_bits);
    if (thresholds)
        hipLaunchKernelGGL(ladder_rdo_tiles_kernel, grid, block, lds_bytes, (hipStream_t)stream, y, map_mean, bin_widths_points, thresholds,
                           rdo_amax(length), k_points, length, hist, bypass, range_errors, h, w, th, tw, (int)tiles_x, (int)nb_tiles, (int)cpt,
                           per, items);
    else
        hipLaunchKernelGGL(ladder_tiles_kernel, grid, block, lds_bytes, (hipStream_t)stream, y, map_mean, bin_widths_points, k_points, length,
                           hist, bypass, range_errors, h, w, th, tw, (int)tiles_x, (int)nb_tiles, (int)cpt, per, items);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
}  // namespace

extern "C" int eae_hip_ladder_histograms(const float* y, const float* map_mean, const float* bin_widths_points, int k_points, int length,
                                         uint32_t* hist, uint64_t* bypass_bits, uint32_t* range_errors, int n, int hw, void* stream) {
    return launch_ladder(y, map_mean, bin_widths_points, nullptr, k_points, length, hist, bypass_bits, range_errors, n, hw, stream);
}

extern "C" int eae_hip_ladder_histograms_tiles(const float* y, const float* map_mean, const float* bin_widths_points, int k_points,
                                               int length, uint32_t* hist, uint64_t* bypass_bits, uint32_t* range_errors, int n, int h,
                                               int w, int th, int tw, void* stream) {
    return launch_ladder_tiles(y, map_mean, bin_widths_points, nullptr, k_points, length, hist, bypass_bits, range_errors, n, h, w, th, tw,
                               stream);
}

extern "C" int eae_hip_ladder_histograms_rdo(const float* y, const float* map_mean, const float* bin_widths_points,
                                             const float* thresholds_by_magnitude, int k_points, int length, uint32_t* hist,
                                             uint64_t* bypass_bits, uint32_t* range_errors, int n, int hw, void* stream) {
    if (!thresholds_by_magnitude || !aligned_to(thresholds_by_magnitude, 16)) return EAE_HIP_BAD_ARGUMENT;
    return launch_ladder(y, map_mean, bin_widths_points, thresholds_by_magnitude, k_points, length, hist, bypass_bits, range_errors, n, hw,
                         stream);
}

extern "C" int eae_hip_ladder_histograms_rdo_tiles(const float* y, const float* map_mean, const float* bin_widths_points,
                                                   const float* thresholds_by_magnitude, int k_points, int length, uint32_t* hist,
                                                   uint64_t* bypass_bits, uint32_t* range_errors, int n, int h, int w, int th, int tw,
                                                   void* stream) {
    if (!thresholds_by_magnitude || !aligned_to(thresholds_by_magnitude, 16)) return EAE_HIP_BAD_ARGUMENT;
    return launch_ladder_tiles(y, map_mean, bin_widths_points, thresholds_by_magnitude, k_points, length, hist, bypass_bits, range_errors, n,
                               h, w, th, tw, stream);
}
