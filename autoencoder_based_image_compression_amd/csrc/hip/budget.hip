// budget.hip -- what a step of codec.BudgetCodec needs on the device beyond BatchCodec's launches:
//   eae_hip_ladder_select          the rate point of every image of a batch for its byte budget, from the histograms
//                                  eae_hip_ladder_histograms leaves (ratecontrol.upper_bounds_fixed + select_by_upper_bound,
//                                  element for element: integer arithmetic only, every logarithm comes in as a table)
//   eae_hip_ladder_select_tiles    the same from the counts per coding tile eae_hip_ladder_histograms_tiles leaves, for EAT1 blobs
//                                  (ratecontrol.upper_bounds_fixed_tiles), with prob_row in the run order of
//                                  codec.coding_tile_layout: two launches, the second after every image has its point
//   eae_hip_latent_quantize_rows   the quantiser half of eae_hip_latent_stage with one row of bin widths PER IMAGE, chosen through
//                                  a device array of points (the one eae_hip_ladder_select has just written)
//
// ladder_select. One block per image, a thread per (point, map): its L + 1 counts, L pairs of costs, one sum in 64 bits. The 64
// lanes of a wavefront share the point (128 maps = two waves), so a wave adds its bytes and its symbol count up with shuffles and
// leaves one LDS add per point; thread 0 then walks the K <= 32 points. N * K * 128 * (L + 1) words are read once (1.2 MB at
// 24 x 9 x 11): a few microseconds of latency, nothing to tune.
//
// latent_quantize_rows. latent_quarter_kernel (latent.hip) without gdn_3: four waves share 32 positions, a lane owns ONE position
// (lj) and 16 channels. The existing kernels keep the 128 bin widths in LDS per block, which is wrong as soon as a tile straddles
// two images (32 positions over n * hw rows: hw = 12 puts three images into one tile). Here the position's image picks the row:
// k = clamp(point[img]), and the lane reads its 16 bin widths from bin_widths_points[k] (K * 512 bytes, L2-resident; float4 loads,
// the 32 lanes of a half-wave that share an image read the same 16 bytes). Everything else -- the expressions, their order, the
// symbol stores, the dead-map flags, the three checks, inverse_gdn_4 on the MFMA -- is latent_quarter_kernel's: same bits.
#include "latent_body.h"

namespace {
constexpr int SELECT_THREADS = 256;
constexpr int SELECT_MAX_POINTS = 32;               // eae_hip_ladder_max_points(1)
constexpr int SELECT_MAX_MAP_SIZE = 1 << 24;        // L * map_size * 2^31 (the largest cost) stays below 2^63
constexpr unsigned long long FIXED_ONE = 1ull << 20;
constexpr unsigned long long C99 = 15204ull;        // ratecontrol.C99 = ceil(-log2(0.99) * 2^20)
constexpr unsigned long long ALLOWANCE_HIGH = 3ull; // ratecontrol.ALLOWANCE_HIGH

__global__ __launch_bounds__(SELECT_THREADS) void ladder_select_kernel(
    const unsigned int* __restrict__ hist, const unsigned long long* __restrict__ bypass_bits, const uint2* __restrict__ costs,
    const unsigned int* __restrict__ log_ceil, const unsigned int* __restrict__ log_floor, int k_points, int length, int idx_exception,
    long long header_bytes, int map_size, const long long* __restrict__ budgets, int exception_row_base, int* __restrict__ point,
    int* __restrict__ prob_row, long long* __restrict__ upper, unsigned int* __restrict__ flags) {
    __shared__ unsigned long long s_bytes[SELECT_MAX_POINTS];
    __shared__ unsigned long long s_count[SELECT_MAX_POINTS];
    __shared__ int s_point;
    const int tid = threadIdx.x, lane = tid & 63;
    const int img = blockIdx.x;
    const int nb = length + 1;
    if (tid < SELECT_MAX_POINTS) { s_bytes[tid] = 0ull; s_count[tid] = 0ull; }
    __syncthreads();
    for (int g = tid; g < k_points * EAE_C; g += SELECT_THREADS) {          // a wave's 64 items share k: whole waves run or idle
        const int k = g >> 7, m = g & (EAE_C - 1);
        const size_t map_index = ((size_t)img * k_points + k) * EAE_C + m;
        const unsigned int* h = hist + map_index * nb;
        unsigned long long total = 0ull;
        for (int j = 0; j < nb; ++j) total += h[j];
        // decision i: zeros = h[i], ones = the symbols of magnitude > i (ratecontrol.decision_counts)
        unsigned long long fp = 0ull, beyond = total;
        if (m == idx_exception) {
            for (int i = 0; i < length; ++i) {
                const unsigned long long z = h[i];
                beyond -= z;
                const unsigned long long o = beyond, t = z + o;
                if (t == 0ull) continue;
                if (z == 0ull) fp += o * C99;
                else if (o == 0ull) fp += z * C99;
                else {
                    // (indices clamped: counts that no map of map_size symbols can hold must not read past the tables)
                    const unsigned long long cap = (unsigned long long)map_size;
                    fp += t * log_ceil[t < cap ? t : cap] - z * log_floor[z < cap ? z : cap] - o * log_floor[o < cap ? o : cap];
                }
            }
        } else {
            const uint2* c = costs + ((size_t)k * EAE_C + m) * length;
            for (int i = 0; i < length; ++i) {
                const unsigned long long z = h[i];
                beyond -= z;
                const uint2 ci = c[i];
                fp += z * ci.x + beyond * ci.y;
            }
        }
        const unsigned long long bits = (fp + FIXED_ONE - 1ull) >> 20;
        unsigned long long bytes = ((bits + ALLOWANCE_HIGH + 7ull) >> 3) + ((bypass_bits[map_index] + 7ull) >> 3);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            bytes += __shfl_down(bytes, off, 64);
            total += __shfl_down(total, off, 64);
        }
        if (lane == 0) {
            atomicAdd(&s_bytes[k], bytes);
            atomicAdd(&s_count[k], total);
        }
    }
    __syncthreads();
    if (tid == 0) {
        // ratecontrol.select_by_upper_bound: the first valid point whose bound fits; else the last valid one; else K - 1
        const long long budget = budgets[img];
        const unsigned long long whole = (unsigned long long)EAE_C * (unsigned long long)map_size;
        int chosen = -1, last_valid = -1;
        for (int k = 0; k < k_points; ++k) {
            if (s_count[k] != whole) continue;
            last_valid = k;
            if (chosen < 0 && header_bytes + (long long)s_bytes[k] <= budget) chosen = k;
        }
        unsigned int f = 0u;
        if (chosen >= 0) f = 1u;
        else if (last_valid >= 0) chosen = last_valid;
        else { chosen = k_points - 1; f = 2u; }
        point[img] = chosen;
        flags[img] = f;
        s_point = chosen;
    }
    if (tid < k_points) upper[(size_t)img * k_points + tid] = header_bytes + (long long)s_bytes[tid];
    __syncthreads();
    if (tid < EAE_C) prob_row[(size_t)img * EAE_C + tid] = tid == idx_exception ? exception_row_base + img : s_point * EAE_C + tid;
}

// ladder_select_kernel on counts per coding tile (ratecontrol.upper_bounds_fixed_tiles): hist [N][K][T][128][L + 1], bypass_bits
// [N][K][T][128]. One block per image, an item per (point, tile, map); the 64 lanes of a wavefront share point and tile. The
// exception map keeps one row per image, so its whole-map counts are summed over the tiles first and turned into a pair of costs
// per (point, decision) in LDS -- Lceil[Z + O] - Lfloor[Z] for a zero, Lceil[Z + O] - Lfloor[O] for a one, C99 where the other
// count is 0 --, after which a tile of it is priced like a tile of any map.
// A point is VALID when the image's histograms at it hold 128 * map_size symbols IN ALL (s_count), where
// ratecontrol.valid_points asks the same of the sum: the two cannot differ, and both equal "every map holds map_size symbols", for
// counts a pass of ladder_tiles_kernel leaves (an element lands in one bin of its own map or in none); for other counts -- a map one
// symbol over, another one short -- the total decides here as it does on the host. ladder_select_kernel has the same caveat.
// One block per image reads K T 128 (L + 1) words, a lane its L + 1 counts at a stride of L + 1 words: 51 us at T = 6, 188 us at
// T = 24 on 24 images (profiles/tiled_budget_codec.md), more than the histogram pass in front of it there; a grid over
// (image, point) is the next step if tiles of 8 matter.
constexpr int SELECT_TILES_THREADS = 512;
// the launcher admits K <= eae_hip_ladder_max_points(L) = 65536 / ((L + 3) * 512), i.e. K (L + 3) <= 128: so the K (L + 1) words of
// s_whole and the K L pairs of s_own both fit 128 entries
constexpr int SELECT_MAX_PAIRS = 128;

__global__ __launch_bounds__(SELECT_TILES_THREADS) void ladder_select_tiles_kernel(
    const unsigned int* __restrict__ hist, const unsigned long long* __restrict__ bypass_bits, const uint2* __restrict__ costs,
    const unsigned int* __restrict__ log_ceil, const unsigned int* __restrict__ log_floor, int k_points, int length, int idx_exception,
    long long header_bytes, int map_size, int nb_tiles, const long long* __restrict__ budgets, int* __restrict__ point,
    long long* __restrict__ upper, unsigned int* __restrict__ flags) {
    __shared__ unsigned long long s_bytes[SELECT_MAX_POINTS];
    __shared__ unsigned long long s_count[SELECT_MAX_POINTS];
    __shared__ unsigned int s_whole[SELECT_MAX_PAIRS];              // [K][L + 1]: the exception map's counts over the whole map
    __shared__ uint2 s_own[SELECT_MAX_PAIRS];                       // [K][L]: what a zero and a one of its decisions cost
    const int tid = threadIdx.x, lane = tid & 63;
    const int img = blockIdx.x;
    const int nb = length + 1;
    if (tid < SELECT_MAX_POINTS) { s_bytes[tid] = 0ull; s_count[tid] = 0ull; }
    if (tid < SELECT_MAX_PAIRS) s_whole[tid] = 0u;
    __syncthreads();
    if (idx_exception >= 0) {
        for (int g = tid; g < k_points * nb_tiles * nb; g += SELECT_TILES_THREADS) {
            const int kt = g / nb, bin = g - kt * nb;
            const int k = kt / nb_tiles;
            const unsigned int v = hist[(((size_t)img * k_points * nb_tiles + kt) * EAE_C + idx_exception) * nb + bin];
            if (v) atomicAdd(&s_whole[k * nb + bin], v);
        }
        __syncthreads();
        if (tid < k_points) {
            const unsigned long long cap = (unsigned long long)map_size;
            unsigned long long beyond = 0ull;
            for (int j = 0; j < nb; ++j) beyond += s_whole[tid * nb + j];
            for (int i = 0; i < length; ++i) {
                const unsigned long long z = s_whole[tid * nb + i];
                beyond -= z;
                const unsigned long long o = beyond, t = z + o;
                uint2 own = make_uint2(0u, 0u);
                if (z == 0ull) own.y = (unsigned int)C99;
                else if (o == 0ull) own.x = (unsigned int)C99;
                else {
                    // (indices clamped: counts that no map of map_size symbols can hold must not read past the tables)
                    const unsigned int up = log_ceil[t < cap ? t : cap];
                    const unsigned int dz = log_floor[z < cap ? z : cap], dn = log_floor[o < cap ? o : cap];
                    own.x = up > dz ? up - dz : 0u;
                    own.y = up > dn ? up - dn : 0u;
                }
                s_own[tid * length + i] = own;
            }
        }
        __syncthreads();
    }
    for (int g = tid; g < k_points * nb_tiles * EAE_C; g += SELECT_TILES_THREADS) {  // a wave's 64 items share k and the tile
        const int kt = g >> 7, m = g & (EAE_C - 1);
        const int k = kt / nb_tiles;
        const size_t map_index = ((size_t)img * k_points * nb_tiles + kt) * EAE_C + m;
        const unsigned int* h = hist + map_index * nb;
        unsigned long long total = 0ull;
        for (int j = 0; j < nb; ++j) total += h[j];
        unsigned long long fp = 0ull, beyond = total;
        const bool own = m == idx_exception;
        const uint2* c = costs + ((size_t)k * EAE_C + m) * length;
        for (int i = 0; i < length; ++i) {
            const unsigned long long z = h[i];
            beyond -= z;
            const uint2 ci = own ? s_own[k * length + i] : c[i];
            fp += z * ci.x + beyond * ci.y;
        }
        const unsigned long long bits = (fp + FIXED_ONE - 1ull) >> 20;
        unsigned long long bytes = ((bits + ALLOWANCE_HIGH + 7ull) >> 3) + ((bypass_bits[map_index] + 7ull) >> 3);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            bytes += __shfl_down(bytes, off, 64);
            total += __shfl_down(total, off, 64);
        }
        if (lane == 0) {
            atomicAdd(&s_bytes[k], bytes);
            atomicAdd(&s_count[k], total);
        }
    }
    __syncthreads();
    if (tid == 0) {
        // ratecontrol.select_by_upper_bound: the first valid point whose bound fits; else the last valid one; else K - 1
        const long long budget = budgets[img];
        const unsigned long long whole = (unsigned long long)EAE_C * (unsigned long long)map_size;
        int chosen = -1, last_valid = -1;
        for (int k = 0; k < k_points; ++k) {
            if (s_count[k] != whole) continue;
            last_valid = k;
            if (chosen < 0 && header_bytes + (long long)s_bytes[k] <= budget) chosen = k;
        }
        unsigned int f = 0u;
        if (chosen >= 0) f = 1u;
        else if (last_valid >= 0) chosen = last_valid;
        else { chosen = k_points - 1; f = 2u; }
        point[img] = chosen;
        flags[img] = f;
    }
    if (tid < k_points) upper[(size_t)img * k_points + tid] = header_bytes + (long long)s_bytes[tid];
}

// prob_row in the RUN order of codec.coding_tile_layout: entry_image[e] is the image of run-order entry e (a value outside
// [0, N) is clamped), and the rows are those of ladder_select_kernel for that image.
__global__ __launch_bounds__(256) void tile_prob_rows_kernel(const int* __restrict__ point, const int* __restrict__ entry_image,
                                                             int n, int n_entries, int idx_exception, int exception_row_base,
                                                             int* __restrict__ prob_row) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)n_entries * EAE_C) return;
    const int m = (int)(g & (EAE_C - 1));
    int img = entry_image[g >> 7];
    img = img < 0 ? 0 : (img >= n ? n - 1 : img);
    prob_row[g] = m == idx_exception ? exception_row_base + img : point[img] * EAE_C + m;
}

// y, shifted_out and t_out carry no __restrict__, like latent_quarter_kernel's
template <bool IGDN_OUT>
__global__ __launch_bounds__(256) void latent_rows_kernel(const float* y, const float* __restrict__ map_mean,
                                                          const float* __restrict__ bin_widths_points, const int* __restrict__ point,
                                                          int k_points, const float* __restrict__ gamma_out,
                                                          const float* __restrict__ beta_out, float* shifted_out, float* t_out,
                                                          int16_t* __restrict__ symbols, unsigned int* __restrict__ nonzero,
                                                          unsigned int* __restrict__ checks, long rows, int hw) {
    __shared__ __attribute__((aligned(16))) float vec[2 * EAE_C];          // beta_out | map_mean
    __shared__ __attribute__((aligned(16))) float xch[4 * 4 * 64 * 4];     // [channel tile][g][lane][4]: the exchange, 16 KB
    __shared__ unsigned int tally[4][3];
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, lj = lane & 31;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < EAE_C) {
        vec[tid] = IGDN_OUT ? beta_out[tid] : 0.f;
        vec[EAE_C + tid] = map_mean ? map_mean[tid] : 0.f;
    }
    const long row = (long)blockIdx.x * 32 + lj;
    const bool valid = row < rows;
    const long img = row / hw;
    const int pix = (int)(row - img * hw);
    const int cw = 32 * w + 4 * hi;                          // this lane's channels: cw + 8 g + q
    const size_t obase = (size_t)(valid ? row : 0) * EAE_C + cw;
    // the row of bin widths of THIS position's image; a point outside [0, K) is clamped, a position past the last image takes row 0
    int k = valid ? point[img] : 0;
    k = k < 0 ? 0 : (k >= k_points ? k_points - 1 : k);
    const float* bw_row = bin_widths_points + (size_t)k * EAE_C + cw;
    f32x16 own;                                              // [4 g + q]
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 q = valid ? *reinterpret_cast<const float4*>(y + obase + 8 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
        own[4 * g + 0] = q.x; own[4 * g + 1] = q.y; own[4 * g + 2] = q.z; own[4 * g + 3] = q.w;
    }
    __syncthreads();                                         // vec
    // the quantiser on this wave's 32 channels (quantize.hip, statement for statement; latent_quarter_kernel's stores)
    const long img0 = ((long)blockIdx.x * 32) / hw;
    const bool one_image = __all(!valid || img == img0) != 0;
    const __amdgpu_buffer_rsrc_t sym_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        symbols ? symbols + (size_t)img0 * EAE_C * hw : nullptr, 0, symbols ? 0x7FFFFFFF : 0, 0x00020000);
    const int sym_lane = valid ? (int)((((img - img0) * EAE_C + 4 * hi) * hw + pix) * 2) : -1;     // bytes; -1: no store
    unsigned int bad = 0, not_quantized = 0, altered = 0, flag_bits = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 m4 = *reinterpret_cast<const float4*>(vec + EAE_C + cw + 8 * g);
        const float4 b4 = *reinterpret_cast<const float4*>(bw_row + 8 * g);
        const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, bw[4] = {b4.x, b4.y, b4.z, b4.w};
        float sh[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float yv = own[4 * g + q];
            const float centered = yv - mm[q];
            const float rr = round_half_even(centered / bw[q]);
            const float cq = bw[q] * rr;
            const float rs = round_half_even(cq / bw[q]);
            sh[q] = cq + mm[q];
            if (valid) {
                if (!(fabsf(rs) < 32768.f)) bad++;
                if (!(fabs((double)cq - (double)centered) < 1.5e-10)) not_quantized++;
                if (!((float)(int16_t)(int)rs * bw[q] == centered)) altered++;
            }
            const bool nz = valid && cq != 0.f;
            if (nonzero) {
                if (one_image) {
                    // one bit per channel of this tile: a half-wave's 32 positions share the channel
                    const unsigned long long any = __ballot(nz);
                    if ((unsigned int)any) flag_bits |= 1u << (8 * g + q);
                    if ((unsigned int)(any >> 32)) flag_bits |= 1u << (8 * g + 4 + q);
                } else if (nz) {
                    nonzero[img * EAE_C + cw + 8 * g + q] = 1u;                      // benign race: every writer stores 1
                }
            }
            if (symbols)
                __builtin_amdgcn_raw_buffer_store_b16((short)(int16_t)(int)rs, sym_rsrc, sym_lane, (32 * w + 8 * g + q) * hw * 2, 0);
        }
        if (valid && shifted_out) *reinterpret_cast<float4*>(shifted_out + obase + 8 * g) = make_float4(sh[0], sh[1], sh[2], sh[3]);
        own[4 * g + 0] = sh[0]; own[4 * g + 1] = sh[1]; own[4 * g + 2] = sh[2]; own[4 * g + 3] = sh[3];
    }
    if (nonzero && one_image && lane < 32 && ((flag_bits >> lane) & 1u)) nonzero[img0 * EAE_C + 32 * w + lane] = 1u;
    if (checks) {
        // one atomic per block and counter (latent_quarter_kernel)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            bad += __shfl_down(bad, off, 64);
            not_quantized += __shfl_down(not_quantized, off, 64);
            altered += __shfl_down(altered, off, 64);
        }
        if (lane == 0) { tally[w][0] = bad; tally[w][1] = not_quantized; tally[w][2] = altered; }
    }
    if (IGDN_OUT) {
        const f32x16 sq = squares_for_mfma(own);
        float4* slot = reinterpret_cast<float4*>(xch) + lane;    // [t][g][lane]
#pragma unroll
        for (int g = 0; g < 4; ++g) slot[(4 * w + g) * 64] = make_float4(sq[4 * g], sq[4 * g + 1], sq[4 * g + 2], sq[4 * g + 3]);
        __syncthreads();
        f32x16 full[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 q = slot[(4 * t + g) * 64];
                full[t][4 * g + 0] = q.x; full[t][4 * g + 1] = q.y; full[t][4 * g + 2] = q.z; full[t][4 * g + 3] = q.w;
            }
        f32x16 d[1] = {quarter_denominator<8>(full, gamma_out, w, lane)};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bt = *reinterpret_cast<const float4*>(vec + cw + 8 * g);
            d[0][4 * g + 0] = d[0][4 * g + 0] + bt.x;
            d[0][4 * g + 1] = d[0][4 * g + 1] + bt.y;
            d[0][4 * g + 2] = d[0][4 * g + 2] + bt.z;
            d[0][4 * g + 3] = d[0][4 * g + 3] + bt.w;
        }
        const f32x16 xn[1] = {own};
        gdn_tile<1, true, false>(xn, d, [&](int, int g, float4 v) {
            if (valid) *reinterpret_cast<float4*>(t_out + obase + 8 * g) = v;
        });
    }
    if (checks) {
        if (!IGDN_OUT) __syncthreads();                      // (with IGDN_OUT the exchange's barrier came after the tally)
        if (tid < 3) {
            const unsigned int sum = tally[0][tid] + tally[1][tid] + tally[2][tid] + tally[3][tid];
            if (sum) atomicAdd(&checks[tid], sum);
        }
    }
}

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
}  // namespace

extern "C" int eae_hip_ladder_select(const uint32_t* hist, const uint64_t* bypass_bits, const uint32_t* fixed_costs,
                                     const uint32_t* log2_tables, int k_points, int length, int idx_map_exception, int64_t header_bytes,
                                     int map_size, const int64_t* budgets, int exception_row_base, int32_t* point, int32_t* prob_row,
                                     int64_t* upper, uint32_t* flags, int n, void* stream) {
    if (!hist || !bypass_bits || !fixed_costs || !budgets || !point || !prob_row || !upper || !flags || n <= 0) return EAE_HIP_BAD_ARGUMENT;
    if (length < 1 || length > 255 || k_points < 1 || k_points > eae_hip_ladder_max_points(length) || k_points > SELECT_MAX_POINTS)
        return EAE_HIP_BAD_ARGUMENT;
    if (idx_map_exception >= EAE_C || (idx_map_exception >= 0 && !log2_tables)) return EAE_HIP_BAD_ARGUMENT;
    if (map_size < 1 || header_bytes < 0 || exception_row_base < 0) return EAE_HIP_BAD_ARGUMENT;
    if (!aligned_to(fixed_costs, 8) || !aligned_to(bypass_bits, 8) || !aligned_to(budgets, 8) || !aligned_to(upper, 8)) return EAE_HIP_BAD_ARGUMENT;
    if (map_size > SELECT_MAX_MAP_SIZE) return EAE_HIP_BAD_SHAPE;
    const int exception = idx_map_exception >= 0 ? idx_map_exception : -1;
    hipLaunchKernelGGL(ladder_select_kernel, dim3((unsigned)n), dim3(SELECT_THREADS), 0, (hipStream_t)stream, hist,
                       reinterpret_cast<const unsigned long long*>(bypass_bits), reinterpret_cast<const uint2*>(fixed_costs), log2_tables,
                       log2_tables ? log2_tables + (size_t)map_size + 1 : nullptr, k_points, length, exception, (long long)header_bytes,
                       map_size, reinterpret_cast<const long long*>(budgets), exception_row_base, point, prob_row,
                       reinterpret_cast<long long*>(upper), flags);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_ladder_select_tiles(const uint32_t* hist, const uint64_t* bypass_bits, const uint32_t* fixed_costs,
                                           const uint32_t* log2_tables, int k_points, int length, int idx_map_exception,
                                           int64_t header_bytes, int map_size, int nb_tiles, const int64_t* budgets,
                                           const int32_t* entry_image, int n_entries, int exception_row_base, int32_t* point,
                                           int32_t* prob_row, int64_t* upper, uint32_t* flags, int n, void* stream) {
    if (!hist || !bypass_bits || !fixed_costs || !budgets || !entry_image || !point || !prob_row || !upper || !flags || n <= 0)
        return EAE_HIP_BAD_ARGUMENT;
    if (length < 1 || length > 255 || k_points < 1 || k_points > eae_hip_ladder_max_points(length) || k_points > SELECT_MAX_POINTS)
        return EAE_HIP_BAD_ARGUMENT;
    if (idx_map_exception >= EAE_C || (idx_map_exception >= 0 && !log2_tables)) return EAE_HIP_BAD_ARGUMENT;
    if (map_size < 1 || nb_tiles < 1 || n_entries < 1 || header_bytes < 0 || exception_row_base < 0) return EAE_HIP_BAD_ARGUMENT;
    if (!aligned_to(fixed_costs, 8) || !aligned_to(bypass_bits, 8) || !aligned_to(budgets, 8) || !aligned_to(upper, 8)) return EAE_HIP_BAD_ARGUMENT;
    if (map_size > SELECT_MAX_MAP_SIZE || nb_tiles > map_size) return EAE_HIP_BAD_SHAPE;
    if ((long)k_points * nb_tiles * EAE_C * (length + 1) > 0x7FFFFFFFL || (long)n_entries * EAE_C > 0x7FFFFFFFL) return EAE_HIP_BAD_SHAPE;
    const int exception = idx_map_exception >= 0 ? idx_map_exception : -1;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ladder_select_tiles_kernel, dim3((unsigned)n), dim3(SELECT_TILES_THREADS), 0, s, hist,
                       reinterpret_cast<const unsigned long long*>(bypass_bits), reinterpret_cast<const uint2*>(fixed_costs), log2_tables,
                       log2_tables ? log2_tables + (size_t)map_size + 1 : nullptr, k_points, length, exception, (long long)header_bytes,
                       map_size, nb_tiles, reinterpret_cast<const long long*>(budgets), point, reinterpret_cast<long long*>(upper), flags);
    EAE_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(tile_prob_rows_kernel, dim3((unsigned)(((long)n_entries * EAE_C + 255) / 256)), dim3(256), 0, s, point, entry_image, n,
                       n_entries, exception, exception_row_base, prob_row);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_latent_quantize_rows(const float* y, const float* map_mean, const float* bin_widths_points, const int32_t* point,
                                            int k_points, const float* gamma_out_packed, const float* beta_out, float* shifted_out,
                                            float* t_out, int16_t* symbols_planar, uint32_t* nonzero_flags, uint32_t* checks, int n, int hw,
                                            void* stream) {
    if (!y || !bin_widths_points || !point || n <= 0 || hw <= 0 || k_points < 1) return EAE_HIP_BAD_ARGUMENT;
    if ((gamma_out_packed == nullptr) != (beta_out == nullptr) || (gamma_out_packed && !t_out)) return EAE_HIP_BAD_ARGUMENT;
    if (!aligned_to(y, 16) || !aligned_to(bin_widths_points, 16) || !aligned_to(shifted_out, 16) || !aligned_to(t_out, 16))
        return EAE_HIP_BAD_ARGUMENT;
    if (hw > (1 << 21)) return EAE_HIP_BAD_SHAPE;           // 32-bit symbol offsets inside the images of one tile
    const long rows = (long)n * hw;
    if ((rows + 31) / 32 > 0x7FFFFFFFL) return EAE_HIP_BAD_SHAPE;
    const unsigned grid = (unsigned)((rows + 31) / 32);
    hipStream_t s = (hipStream_t)stream;
    if (gamma_out_packed)
        hipLaunchKernelGGL((latent_rows_kernel<true>), dim3(grid), dim3(256), 0, s, y, map_mean, bin_widths_points, point, k_points,
                           gamma_out_packed, beta_out, shifted_out, t_out, symbols_planar, nonzero_flags, checks, rows, hw);
    else
        hipLaunchKernelGGL((latent_rows_kernel<false>), dim3(grid), dim3(256), 0, s, y, map_mean, bin_widths_points, point, k_points,
                           gamma_out_packed, beta_out, shifted_out, t_out, symbols_planar, nonzero_flags, checks, rows, hw);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
