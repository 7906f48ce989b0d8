// budget.hip -- what a step of codec.BudgetCodec needs on the device beyond BatchCodec's launches:
//   eae_hip_ladder_select          the rate point of every image of a batch for its byte budget, from the histograms
//                                  eae_hip_ladder_histograms leaves (ratecontrol.upper_bounds_fixed + select_by_upper_bound,
//                                  element for element: integer arithmetic only, every logarithm comes in as a table)
//   eae_hip_ladder_select_tiles    the same from the counts per coding tile eae_hip_ladder_histograms_tiles leaves, for EAT1 blobs
//                                  (ratecontrol.upper_bounds_fixed_tiles), with prob_row in the run order of
//                                  codec.coding_tile_layout: two launches, the second after every image has its point
// (the quantiser that takes the points these write, eae_hip_latent_quantize_rows, is latent_rows.hip)
//
// ladder_select. One block per image, a thread per (point, map): its L + 1 counts, L pairs of costs, one sum in 64 bits. The 64
// lanes of a wavefront share the point (128 maps = two waves), so a wave adds its bytes and its symbol count up with shuffles and
// leaves one LDS add per point; thread 0 then walks the K <= 32 points. N * K * 128 * (L + 1) words are read once (1.2 MB at
// 24 x 9 x 11): a few microseconds of latency, nothing to tune.
#include "common.h"

namespace {
constexpr int SELECT_THREADS = 256;
constexpr int SELECT_MAX_POINTS = 32;               // eae_hip_ladder_max_points(1)
constexpr int SELECT_MAX_MAP_SIZE = 1 << 24;        // L * map_size * 2^31 (the largest cost) stays below 2^63
constexpr unsigned long long FIXED_ONE = 1ull << 20;
constexpr unsigned long long C99 = 15204ull;        // ratecontrol.C99 = ceil(-log2(0.99) * 2^20)
constexpr unsigned long long ALLOWANCE_HIGH = 3ull; // ratecontrol.ALLOWANCE_HIGH

// A map whose decisions have a pair of costs each: decision i has zeros = h[i], ones = the symbols of magnitude > i
// (ratecontrol.decision_counts), pair(i) is what a zero and a one of it cost. Returns the map's bits in 2^-20ths.
template <typename Pair>
__device__ __forceinline__ unsigned long long priced_by_pairs(const unsigned int* h, unsigned long long total, int length,
                                                              Pair pair) {
    unsigned long long fp = 0ull, beyond = total;
    for (int i = 0; i < length; ++i) {
        const unsigned long long z = h[i];
        beyond -= z;
        const uint2 ci = pair(i);
        fp += z * ci.x + beyond * ci.y;
    }
    return fp;
}

// A map's bound in bytes from its bits, then the bytes and the symbols of the wave's 64 maps, which share the point: one LDS add each
__device__ __forceinline__ void add_map_to_point(unsigned long long fp, unsigned long long bypass, unsigned long long total, int lane,
                                                 unsigned long long* point_bytes, unsigned long long* point_count) {
    const unsigned long long bits = (fp + FIXED_ONE - 1ull) >> 20;
    unsigned long long bytes = ((bits + ALLOWANCE_HIGH + 7ull) >> 3) + ((bypass + 7ull) >> 3);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        bytes += __shfl_down(bytes, off, 64);
        total += __shfl_down(total, off, 64);
    }
    if (lane == 0) {
        atomicAdd(point_bytes, bytes);
        atomicAdd(point_count, total);
    }
}

// ratecontrol.select_by_upper_bound, by one thread: the first valid point whose bound fits; else the last valid one; else K - 1.
// A point is valid when its histograms hold all 128 * map_size symbols. Returns the point, *flag as ratecontrol's.
__device__ __forceinline__ int select_by_upper_bound(const unsigned long long* s_bytes, const unsigned long long* s_count, int k_points,
                                                     long long header_bytes, int map_size, long long budget, unsigned int* flag) {
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
    *flag = f;
    return chosen;
}

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
        unsigned long long fp = 0ull;
        if (m == idx_exception) {
            unsigned long long beyond = total;
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
            fp = priced_by_pairs(h, total, length, [&](int i) { return c[i]; });
        }
        add_map_to_point(fp, bypass_bits[map_index], total, lane, &s_bytes[k], &s_count[k]);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned int f;
        const int chosen = select_by_upper_bound(s_bytes, s_count, k_points, header_bytes, map_size, budgets[img], &f);
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
        const bool own = m == idx_exception;
        const uint2* c = costs + ((size_t)k * EAE_C + m) * length;
        const unsigned long long fp = priced_by_pairs(h, total, length, [&](int i) { return own ? s_own[k * length + i] : c[i]; });
        add_map_to_point(fp, bypass_bits[map_index], total, lane, &s_bytes[k], &s_count[k]);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned int f;
        point[img] = select_by_upper_bound(s_bytes, s_count, k_points, header_bytes, map_size, budgets[img], &f);
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

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what both selections refuse, with the code they refuse it with; EAE_HIP_OK otherwise
int select_refusal(const uint32_t* hist, const uint64_t* bypass_bits, const uint32_t* fixed_costs, const uint32_t* log2_tables, int k_points,
                   int length, int idx_map_exception, int64_t header_bytes, int map_size, const int64_t* budgets, int exception_row_base,
                   const int32_t* point, const int32_t* prob_row, const int64_t* upper, const uint32_t* flags, int n) {
    if (!hist || !bypass_bits || !fixed_costs || !budgets || !point || !prob_row || !upper || !flags || n <= 0) return EAE_HIP_BAD_ARGUMENT;
    if (length < 1 || length > 255 || k_points < 1 || k_points > eae_hip_ladder_max_points(length) || k_points > SELECT_MAX_POINTS)
        return EAE_HIP_BAD_ARGUMENT;
    if (idx_map_exception >= EAE_C || (idx_map_exception >= 0 && !log2_tables)) return EAE_HIP_BAD_ARGUMENT;
    if (map_size < 1 || header_bytes < 0 || exception_row_base < 0) return EAE_HIP_BAD_ARGUMENT;
    if (!aligned_to(fixed_costs, 8) || !aligned_to(bypass_bits, 8) || !aligned_to(budgets, 8) || !aligned_to(upper, 8)) return EAE_HIP_BAD_ARGUMENT;
    if (map_size > SELECT_MAX_MAP_SIZE) return EAE_HIP_BAD_SHAPE;
    return EAE_HIP_OK;
}
}  // namespace

extern "C" int eae_hip_ladder_select(const uint32_t* hist, const uint64_t* bypass_bits, const uint32_t* fixed_costs,
                                     const uint32_t* log2_tables, int k_points, int length, int idx_map_exception, int64_t header_bytes,
                                     int map_size, const int64_t* budgets, int exception_row_base, int32_t* point, int32_t* prob_row,
                                     int64_t* upper, uint32_t* flags, int n, void* stream) {
    const int refusal = select_refusal(hist, bypass_bits, fixed_costs, log2_tables, k_points, length, idx_map_exception, header_bytes, map_size,
                                       budgets, exception_row_base, point, prob_row, upper, flags, n);
    if (refusal != EAE_HIP_OK) return refusal;
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
    if (!entry_image || nb_tiles < 1 || n_entries < 1) return EAE_HIP_BAD_ARGUMENT;
    const int refusal = select_refusal(hist, bypass_bits, fixed_costs, log2_tables, k_points, length, idx_map_exception, header_bytes, map_size,
                                       budgets, exception_row_base, point, prob_row, upper, flags, n);
    if (refusal != EAE_HIP_OK) return refusal;
    if (nb_tiles > map_size) return EAE_HIP_BAD_SHAPE;
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
