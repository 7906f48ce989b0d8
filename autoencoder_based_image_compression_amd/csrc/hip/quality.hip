// quality.hip -- what a step of codec.QualityCodec needs on the device beyond BudgetCodec's launches:
//   eae_hip_quality_search         one round of the bisection that finds, per image, the coarsest rate point whose squared error against
//                                  the input stays within max_sse (ratecontrol.select_by_quality, element for element: integers only)
//   eae_hip_quality_search_tiles   the same round for codec.TiledQualityCodec: the coder's rows per stream of a
//                                  step in coding tiles, in the run order of codec.coding_tile_layout
//
// The step launches it nb_rounds + 1 times, round = 0..nb_rounds, with a quantiser launch and a synthesis pass between two rounds:
// round r - 1 leaves in `point` the point to try, the synthesis adds that point's squared error into `probe_acc`, round r reads it,
// moves (L, R) and leaves the next point. Nothing but `round` differs between the launches and nothing depends on the step's
// contents, so the chain is the same every step and a captured graph replays it.
//
// One block per image, 128 threads: thread 0 holds the bisection -- a dozen integer operations --, then every thread writes its
// map's row of the coder's table for the point just written. N * 128 words are written per round: latency, nothing to tune.
#include "common.h"

namespace {
constexpr int QUALITY_THREADS = EAE_C;
constexpr int QUALITY_MAX_IMAGES = 65535;

// the point a round probes from the state in front of it: the middle of a live interval, else max(L, first) (nothing moves)
__device__ __forceinline__ int probe_of(int lo, int hi, int first) { return hi - lo > 1 ? (lo + hi) >> 1 : (lo > first ? lo : first); }

__device__ __forceinline__ int clamp_point(int k, int k_points) { return k < 0 ? 0 : (k >= k_points ? k_points - 1 : k); }

// thread 0 of an image's block: one round of the bisection for image `img`; writes state, probe_acc, point, flags and the trace and
// returns the point it left
__device__ __forceinline__ int search_round(int img, const int* __restrict__ first, const long long* __restrict__ max_sse,
                                            int* __restrict__ state, unsigned long long* __restrict__ probe_acc, int* __restrict__ point,
                                            int* __restrict__ trace_point, long long* __restrict__ trace_sse,
                                            unsigned int* __restrict__ flags, int k_points, int nb_rounds, int round) {
    // (a first outside the ladder is clamped: no row of the table and no row of bin widths lies beyond it)
    const int f = clamp_point(first[img], k_points);
    int lo, hi, next;
    unsigned int met = 0u;
    if (round == 0) {
        lo = f - 1;
        hi = k_points;
        for (int r = 0; r < nb_rounds; ++r) {
            trace_point[(size_t)img * nb_rounds + r] = -1;
            trace_sse[(size_t)img * nb_rounds + r] = -1ll;
        }
    } else {
        lo = state[2 * img];
        hi = state[2 * img + 1];
        const int probed = probe_of(lo, hi, f);
        const long long sse = (long long)probe_acc[img];
        trace_point[(size_t)img * nb_rounds + round - 1] = probed;
        trace_sse[(size_t)img * nb_rounds + round - 1] = sse;
        if (hi - lo > 1) {
            if (sse <= max_sse[img]) lo = probed;
            else hi = probed;
        }
    }
    if (round < nb_rounds) next = probe_of(lo, hi, f);
    else { met = lo >= f ? 1u : 0u; next = met ? lo : f; }
    next = clamp_point(next, k_points);             // (a state this kernel did not write must not name a row outside the ladder)
    state[2 * img] = lo;
    state[2 * img + 1] = hi;
    probe_acc[img] = 0ull;
    point[img] = next;
    flags[img] = met;
    return next;
}

__global__ __launch_bounds__(QUALITY_THREADS) void quality_search_kernel(
    const int* __restrict__ first, const long long* __restrict__ max_sse, int* __restrict__ state,
    unsigned long long* __restrict__ probe_acc, int* __restrict__ point, int* __restrict__ prob_row, int* __restrict__ trace_point,
    long long* __restrict__ trace_sse, unsigned int* __restrict__ flags, int k_points, int nb_rounds, int round, int idx_exception,
    int exception_row_base) {
    __shared__ int s_point;
    const int tid = threadIdx.x;
    const int img = blockIdx.x;
    if (tid == 0) s_point = search_round(img, first, max_sse, state, probe_acc, point, trace_point, trace_sse, flags, k_points, nb_rounds, round);
    __syncthreads();
    prob_row[(size_t)img * EAE_C + tid] = tid == idx_exception ? exception_row_base + img : s_point * EAE_C + tid;
}

// The same round for a step in coding tiles (codec.TiledQualityCodec): the rows of the image's point for each of
// its nb_tiles entries, at the place the coder takes the entry from. run_entry[img * nb_tiles + t] is the run-order index of tile t of
// the image (codec.coding_tile_layout); a value outside [0, n * nb_tiles) is skipped. One block per image, as above, and not a grid
// over the entries: a block must read the state and probe_acc the PREVIOUS launch left, and thread 0 of its image's block writes them.
__global__ __launch_bounds__(QUALITY_THREADS) void quality_search_tiles_kernel(
    const int* __restrict__ first, const long long* __restrict__ max_sse, int* __restrict__ state,
    unsigned long long* __restrict__ probe_acc, int* __restrict__ point, int* __restrict__ prob_row, int* __restrict__ trace_point,
    long long* __restrict__ trace_sse, unsigned int* __restrict__ flags, const int* __restrict__ run_entry, int nb_tiles, int n_entries,
    int k_points, int nb_rounds, int round, int idx_exception, int exception_row_base) {
    __shared__ int s_point;
    const int tid = threadIdx.x;
    const int img = blockIdx.x;
    if (tid == 0) s_point = search_round(img, first, max_sse, state, probe_acc, point, trace_point, trace_sse, flags, k_points, nb_rounds, round);
    __syncthreads();
    const int row = tid == idx_exception ? exception_row_base + img : s_point * EAE_C + tid;
    for (int t = 0; t < nb_tiles; ++t) {
        const int e = run_entry[(size_t)img * nb_tiles + t];
        if (e >= 0 && e < n_entries) prob_row[(size_t)e * EAE_C + tid] = row;
    }
}

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// ceil(log2(k + 1)) for k >= 1: the bits of k (ratecontrol.quality_rounds)
inline int rounds_of(int k_points) {
    int r = 0;
    for (unsigned int k = (unsigned int)k_points; k; k >>= 1) ++r;
    return r;
}

// what both entry points refuse
inline int check_search(const int32_t* first, const int64_t* max_sse, int32_t* state, uint64_t* probe_acc, int32_t* point, int32_t* prob_row,
                        int32_t* trace_point, int64_t* trace_sse, uint32_t* flags, int k_points, int nb_rounds, int round,
                        int idx_map_exception, int exception_row_base, int n) {
    if (!first || !max_sse || !state || !probe_acc || !point || !prob_row || !trace_point || !trace_sse || !flags || n <= 0)
        return EAE_HIP_BAD_ARGUMENT;
    if (k_points < 1 || nb_rounds != rounds_of(k_points) || round < 0 || round > nb_rounds) return EAE_HIP_BAD_ARGUMENT;
    if (idx_map_exception >= EAE_C || exception_row_base < 0) return EAE_HIP_BAD_ARGUMENT;
    if (!aligned_to(max_sse, 8) || !aligned_to(probe_acc, 8) || !aligned_to(trace_sse, 8)) return EAE_HIP_BAD_ARGUMENT;
    return EAE_HIP_OK;
}
}  // namespace

extern "C" int eae_hip_quality_search(const int32_t* first, const int64_t* max_sse, int32_t* state, uint64_t* probe_acc, int32_t* point,
                                      int32_t* prob_row, int32_t* trace_point, int64_t* trace_sse, uint32_t* flags, int k_points,
                                      int nb_rounds, int round, int idx_map_exception, int exception_row_base, int n, void* stream) {
    const int refused = check_search(first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags, k_points, nb_rounds,
                                     round, idx_map_exception, exception_row_base, n);
    if (refused != EAE_HIP_OK) return refused;
    if (n > QUALITY_MAX_IMAGES) return EAE_HIP_BAD_SHAPE;
    const int exception = idx_map_exception >= 0 ? idx_map_exception : -1;
    hipLaunchKernelGGL(quality_search_kernel, dim3((unsigned)n), dim3(QUALITY_THREADS), 0, (hipStream_t)stream, first,
                       reinterpret_cast<const long long*>(max_sse), state, reinterpret_cast<unsigned long long*>(probe_acc), point, prob_row,
                       trace_point, reinterpret_cast<long long*>(trace_sse), flags, k_points, nb_rounds, round, exception,
                       exception_row_base);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_quality_search_tiles(const int32_t* first, const int64_t* max_sse, int32_t* state, uint64_t* probe_acc,
                                            int32_t* point, int32_t* prob_row, int32_t* trace_point, int64_t* trace_sse, uint32_t* flags,
                                            const int32_t* run_entry, int nb_tiles, int k_points, int nb_rounds, int round,
                                            int idx_map_exception, int exception_row_base, int n, void* stream) {
    const int refused = check_search(first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags, k_points, nb_rounds,
                                     round, idx_map_exception, exception_row_base, n);
    if (refused != EAE_HIP_OK) return refused;
    if (!run_entry || nb_tiles < 1) return EAE_HIP_BAD_ARGUMENT;
    if ((long)n * nb_tiles > QUALITY_MAX_IMAGES) return EAE_HIP_BAD_SHAPE;
    const int exception = idx_map_exception >= 0 ? idx_map_exception : -1;
    hipLaunchKernelGGL(quality_search_tiles_kernel, dim3((unsigned)n), dim3(QUALITY_THREADS), 0, (hipStream_t)stream, first,
                       reinterpret_cast<const long long*>(max_sse), state, reinterpret_cast<unsigned long long*>(probe_acc), point, prob_row,
                       trace_point, reinterpret_cast<long long*>(trace_sse), flags, run_entry, nb_tiles, n * nb_tiles, k_points, nb_rounds,
                       round, exception, exception_row_base);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
