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
#include "common.h"

namespace {
constexpr int LADDER_ROWS = 4;                      // pixel rows of a block; one channel per lane
constexpr int LADDER_THREADS = LADDER_ROWS * EAE_C;
constexpr int LADDER_LDS_BYTES = 64 * 1024;         // what one block may ask for
constexpr int LADDER_MIN_PIXELS = 64;
constexpr int LADDER_MAX_PIXELS = 1 << 20;          // 34 bypass bits per symbol at most: a block's sums fit 32 bits

__global__ __launch_bounds__(LADDER_THREADS) void ladder_kernel(const float* __restrict__ y, const float* __restrict__ map_mean,
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
    for (int pix = p0 + row; pix < p1; pix += LADDER_ROWS) {
        const float centered = yc[(size_t)pix * EAE_C] - m;
#pragma unroll 2
        for (int k = 0; k < k_points; ++k) {
            const float bw = widths[k * EAE_C + c];
            const float r = round_half_even(centered / bw);
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
}  // namespace

extern "C" int eae_hip_ladder_max_points(int length) {
    if (length < 1 || length > 255) return 0;
    return LADDER_LDS_BYTES / ((length + 3) * EAE_C * 4);
}

extern "C" int eae_hip_ladder_histograms(const float* y, const float* map_mean, const float* bin_widths_points, int k_points, int length,
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
    hipLaunchKernelGGL(ladder_kernel, dim3((unsigned)(n * chunks)), dim3(LADDER_THREADS), lds_bytes, (hipStream_t)stream, y, map_mean,
                       bin_widths_points, k_points, length, hist, reinterpret_cast<unsigned long long*>(bypass_bits), range_errors, hw,
                       (int)chunks, pixels);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
