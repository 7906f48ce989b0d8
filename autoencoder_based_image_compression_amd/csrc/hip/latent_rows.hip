// latent_rows.hip -- the quantiser half of eae_hip_latent_stage with one row of bin widths PER IMAGE, chosen through a device array of
// points (the one eae_hip_ladder_select has just written; DESIGN.md sections 19 and 23):
//   eae_hip_latent_quantize_rows   image i is quantised with bin_widths_points[point[i]]
//   eae_hip_latent_quantize_rdo    the same with one more input, a table of thresholds float32 [K][128][16]
//                                  (ratecontrol.rdo_thresholds): a latent whose nearest symbol has magnitude a in [1, min(L, 16)] is
//                                  coded one step nearer zero when the squared error that step adds, in bins (u + 1)^2 - u^2 = 2 u + 1
//                                  with u = |x| - a, is below thresholds[k][c][a - 1], the price lambda (B(a) - B(a - 1)) / bw^2 of
//                                  what the step saves. The rule is ratecontrol.rdo_quantize_numpy, element for element.
//
// Both kernels run the four-wave body of quarter_body.h (four waves share 32 positions, a lane owns ONE position and 16 channels)
// without gdn_3. latent_quarter_kernel keeps the 128 bin widths in LDS per block, which is wrong as soon as a tile straddles two
// images (32 positions over n * hw rows: hw = 12 puts three images into one tile). Here the position's image picks the row:
// k = clamp(point[img]), and the lane reads its 16 bin widths from bin_widths_points[k] (K * 512 bytes, L2-resident; float4 loads,
// the 32 lanes of a half-wave that share an image read the same 16 bytes). latent_rows_kernel rounds the quotient like
// latent_quarter_kernel; rdo_rows_kernel hands the body the r it chose in front.
//
// Where the table of thresholds is read from. It is 8 KB per point and the column depends on the data. The 32 lanes of a half-wave
// share a channel, so one load instruction touches at most two rows of 64 bytes, one per half-wave: two cache lines whatever the
// symbols are. Staging the block's 8 KB in LDS would cost every block 2048 words of loads and stores for 4096 latents of which most
// are 0 and look nothing up, and it would need the per-lane path anyway where a tile straddles two images. So the table is read
// through the cache, and only by the waves that need it:
//   pass 1  the 16 quotients, and whether the nearest integer of any of them is eligible;
//   lookup  if ANY lane of the wave has an eligible element (a wave-uniform branch: a wave over a flat region skips it), the 16
//           thresholds are loaded back to back at a clamped column -- an element that is not eligible reads column 0 of its row and
//           ignores it -- so the wave waits for memory once, not once per element;
//   pass 2  the shared body on the final r.
// A NaN, an infinity or a huge quotient fails `a >= 1 && a <= amax` in float and never becomes an index.
#include "quarter_body.h"

namespace {
constexpr int RDO_MAGNITUDES = 16;                          // ratecontrol.RDO_MAGNITUDES: the columns of a row of thresholds

// the row of THIS position's image; a point outside [0, K) is clamped, a position past the last image takes row 0
__device__ __forceinline__ int clamped_point(const int* __restrict__ point, int k_points, const QuarterLane p) {
    const int k = p.valid ? point[p.img] : 0;
    return k < 0 ? 0 : (k >= k_points ? k_points - 1 : k);
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
    const QuarterLane p = quarter_lane(rows, hw);
    if (p.tid < EAE_C) {
        vec[p.tid] = IGDN_OUT ? beta_out[p.tid] : 0.f;
        vec[EAE_C + p.tid] = map_mean ? map_mean[p.tid] : 0.f;
    }
    const float* bw_row = bin_widths_points + (size_t)clamped_point(point, k_points, p) * EAE_C + p.cw;
    const f32x16 own = quarter_load(y, p);
    __syncthreads();                                         // vec
    quarter_quantise<IGDN_OUT, false>(
        own, p, vec + EAE_C, vec, xch, tally, gamma_out, nullptr, shifted_out, t_out, symbols, nonzero, checks, hw,
        [&](int g) { return *reinterpret_cast<const float4*>(bw_row + 8 * g); },
        [](int, float centered, float bw) { return round_half_even(centered / bw); });
}

template <bool IGDN_OUT>
__global__ __launch_bounds__(256) void rdo_rows_kernel(const float* y, const float* __restrict__ map_mean,
                                                       const float* __restrict__ bin_widths_points,
                                                       const float* __restrict__ thresholds_points, const int* __restrict__ point,
                                                       int k_points, float amax, const float* __restrict__ gamma_out,
                                                       const float* __restrict__ beta_out, float* shifted_out, float* t_out,
                                                       int16_t* __restrict__ symbols, unsigned int* __restrict__ nonzero,
                                                       unsigned int* __restrict__ checks, long rows, int hw) {
    __shared__ __attribute__((aligned(16))) float vec[2 * EAE_C];          // beta_out | map_mean
    __shared__ __attribute__((aligned(16))) float xch[4 * 4 * 64 * 4];     // [channel tile][g][lane][4]: the exchange, 16 KB
    __shared__ unsigned int tally[4][3];
    const QuarterLane p = quarter_lane(rows, hw);
    if (p.tid < EAE_C) {
        vec[p.tid] = IGDN_OUT ? beta_out[p.tid] : 0.f;
        vec[EAE_C + p.tid] = map_mean ? map_mean[p.tid] : 0.f;
    }
    const int k = clamped_point(point, k_points, p);
    const float* bw_row = bin_widths_points + (size_t)k * EAE_C + p.cw;
    const float* thr_row = thresholds_points + ((size_t)k * EAE_C + p.cw) * RDO_MAGNITUDES;
    const f32x16 own = quarter_load(y, p);
    __syncthreads();                                         // vec
    // pass 1: the quotient of every element (quantize.hip's first statements), and whether any of them can be lowered
    f32x16 xr;                                               // x until the lookup, the final r behind it
    bool wanted = false;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 m4 = *reinterpret_cast<const float4*>(vec + EAE_C + p.cw + 8 * g);
        const float4 b4 = *reinterpret_cast<const float4*>(bw_row + 8 * g);
        const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, bw[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float centered = own[4 * g + q] - mm[q];
            const float x = centered / bw[q];
            const float a = fabsf(round_half_even(x));
            xr[4 * g + q] = x;
            wanted |= a >= 1.f && a <= amax;
        }
    }
    // lookup: wave-uniform, all 16 loads in flight together; an element that is not eligible reads column 0 and ignores it
    if (__any(wanted)) {
        float thr[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float a = fabsf(round_half_even(xr[i]));
            const float column = (a >= 1.f && a <= amax) ? a : 1.f;          // chosen in float: a NaN or a huge a is never converted
            thr[i] = thr_row[(8 * (i >> 2) + (i & 3)) * RDO_MAGNITUDES + (int)column - 1];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float x = xr[i];
            const float r = round_half_even(x);
            const float a = fabsf(r);
            const float u = fabsf(x) - a;
            const bool lower = a >= 1.f && a <= amax && 2.f * u + 1.f < thr[i];
            xr[i] = lower ? r - copysignf(1.f, r) : r;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) xr[i] = round_half_even(xr[i]);
    }
    // pass 2: the shared body from the final r on
    quarter_quantise<IGDN_OUT, false>(
        own, p, vec + EAE_C, vec, xch, tally, gamma_out, nullptr, shifted_out, t_out, symbols, nonzero, checks, hw,
        [&](int g) { return *reinterpret_cast<const float4*>(bw_row + 8 * g); }, [&](int i, float, float) { return xr[i]; });
}

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// thresholds_points null: latent_rows_kernel, `length` unused; else rdo_rows_kernel (the caller has checked both)
int launch_quantize_rows(const float* y, const float* map_mean, const float* bin_widths_points, const float* thresholds_points,
                         const int32_t* point, int k_points, int length, const float* gamma_out_packed, const float* beta_out,
                         float* shifted_out, float* t_out, int16_t* symbols_planar, uint32_t* nonzero_flags, uint32_t* checks, int n,
                         int hw, void* stream) {
    if (!y || !bin_widths_points || !point || n <= 0 || hw <= 0 || k_points < 1) return EAE_HIP_BAD_ARGUMENT;
    if ((gamma_out_packed == nullptr) != (beta_out == nullptr) || (gamma_out_packed && !t_out)) return EAE_HIP_BAD_ARGUMENT;
    if (!aligned_to(y, 16) || !aligned_to(bin_widths_points, 16) || !aligned_to(shifted_out, 16) || !aligned_to(t_out, 16))
        return EAE_HIP_BAD_ARGUMENT;
    if (hw > (1 << 21)) return EAE_HIP_BAD_SHAPE;           // 32-bit symbol offsets inside the images of one tile
    const long rows = (long)n * hw;
    if ((rows + 31) / 32 > 0x7FFFFFFFL) return EAE_HIP_BAD_SHAPE;
    const dim3 grid((unsigned)((rows + 31) / 32)), block(256);
    const float amax = (float)(length < RDO_MAGNITUDES ? length : RDO_MAGNITUDES);
    hipStream_t s = (hipStream_t)stream;
    if (thresholds_points)
        hipLaunchKernelGGL(gamma_out_packed ? rdo_rows_kernel<true> : rdo_rows_kernel<false>, grid, block, 0, s, y, map_mean, bin_widths_points,
                           thresholds_points, point, k_points, amax, gamma_out_packed, beta_out, shifted_out, t_out, symbols_planar,
                           nonzero_flags, checks, rows, hw);
    else
        hipLaunchKernelGGL(gamma_out_packed ? latent_rows_kernel<true> : latent_rows_kernel<false>, grid, block, 0, s, y, map_mean,
                           bin_widths_points, point, k_points, gamma_out_packed, beta_out, shifted_out, t_out, symbols_planar, nonzero_flags,
                           checks, rows, hw);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
}  // namespace

extern "C" int eae_hip_latent_quantize_rows(const float* y, const float* map_mean, const float* bin_widths_points, const int32_t* point,
                                            int k_points, const float* gamma_out_packed, const float* beta_out, float* shifted_out,
                                            float* t_out, int16_t* symbols_planar, uint32_t* nonzero_flags, uint32_t* checks, int n, int hw,
                                            void* stream) {
    return launch_quantize_rows(y, map_mean, bin_widths_points, nullptr, point, k_points, 0, gamma_out_packed, beta_out, shifted_out, t_out,
                                symbols_planar, nonzero_flags, checks, n, hw, stream);
}

extern "C" int eae_hip_latent_quantize_rdo(const float* y, const float* map_mean, const float* bin_widths_points,
                                           const float* thresholds_points, const int32_t* point, int k_points, int length,
                                           const float* gamma_out_packed, const float* beta_out, float* shifted_out, float* t_out,
                                           int16_t* symbols_planar, uint32_t* nonzero_flags, uint32_t* checks, int n, int hw,
                                           void* stream) {
    if (!thresholds_points || !aligned_to(thresholds_points, 16) || length < 1 || length > 255) return EAE_HIP_BAD_ARGUMENT;
    return launch_quantize_rows(y, map_mean, bin_widths_points, thresholds_points, point, k_points, length, gamma_out_packed, beta_out,
                                shifted_out, t_out, symbols_planar, nonzero_flags, checks, n, hw, stream);
}
