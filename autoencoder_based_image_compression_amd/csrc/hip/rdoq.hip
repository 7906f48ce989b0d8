// rdoq.hip -- the rate-distortion optimised quantiser:
//   eae_hip_latent_quantize_rdo    eae_hip_latent_quantize_rows (budget.hip) with one more input, a table of thresholds
//                                  float32 [K][128][16] (ratecontrol.rdo_thresholds): a latent whose nearest symbol has magnitude
//                                  a in [1, min(L, 16)] is coded one step nearer zero when the squared error that step adds, in
//                                  bins (u + 1)^2 - u^2 = 2 u + 1 with u = |x| - a, is below thresholds[k][c][a - 1], the price
//                                  lambda (B(a) - B(a - 1)) / bw^2 of what the step saves. The rule is
//                                  ratecontrol.rdo_quantize_numpy, element for element.
//
// rdo_rows_kernel is latent_rows_kernel: the same tile (32 positions per block, four waves of 32 channels, a lane owns one position
// and 16 channels), the same row per image through `point`, and from the final r on the same statements in the same order -- cq, rs,
// the three checks, the dead-map flags, the symbol stores, inverse_gdn_4 on the MFMA. What is new sits in front of them.
//
// Where the table is read from. It is 8 KB per point and the column depends on the data. The 32 lanes of a half-wave share a channel,
// so one load instruction touches at most two rows of 64 bytes, one per half-wave: two cache lines whatever the symbols are. Staging
// the block's 8 KB in LDS would cost every block 2048 words of loads and stores for 4096 latents of which most are 0 and look nothing
// up, and it would need the per-lane path anyway where a tile straddles two images. So the table is read through the cache, and only
// by the waves that need it:
//   pass 1  the 16 quotients, and whether the nearest integer of any of them is eligible;
//   lookup  if ANY lane of the wave has an eligible element (a wave-uniform branch: a wave over a flat region skips it), the 16
//           thresholds are loaded back to back at a clamped column -- an element that is not eligible reads column 0 of its row and
//           ignores it -- so the wave waits for memory once, not once per element;
//   pass 2  latent_rows_kernel's statements on the final r.
// A NaN, an infinity or a huge quotient fails `a >= 1 && a <= amax` in float and never becomes an index.
#include "latent_body.h"

namespace {
constexpr int RDO_MAGNITUDES = 16;                          // ratecontrol.RDO_MAGNITUDES: the columns of a row of thresholds

// y, shifted_out and t_out carry no __restrict__, like latent_rows_kernel's
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
    // the rows of THIS position's image; a point outside [0, K) is clamped, a position past the last image takes row 0
    int k = valid ? point[img] : 0;
    k = k < 0 ? 0 : (k >= k_points ? k_points - 1 : k);
    const float* bw_row = bin_widths_points + (size_t)k * EAE_C + cw;
    const float* thr_row = thresholds_points + ((size_t)k * EAE_C + cw) * RDO_MAGNITUDES;
    f32x16 own;                                              // [4 g + q]
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 q = valid ? *reinterpret_cast<const float4*>(y + obase + 8 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
        own[4 * g + 0] = q.x; own[4 * g + 1] = q.y; own[4 * g + 2] = q.z; own[4 * g + 3] = q.w;
    }
    __syncthreads();                                         // vec
    // pass 1: the quotient of every element (quantize.hip's first statements), and whether any of them can be lowered
    f32x16 xr;                                               // x until the lookup, the final r behind it
    bool wanted = false;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 m4 = *reinterpret_cast<const float4*>(vec + EAE_C + cw + 8 * g);
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
    // pass 2: latent_rows_kernel from the final r on, statement for statement
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
            const float rr = xr[4 * g + q];
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

extern "C" int eae_hip_latent_quantize_rdo(const float* y, const float* map_mean, const float* bin_widths_points,
                                           const float* thresholds_points, const int32_t* point, int k_points, int length,
                                           const float* gamma_out_packed, const float* beta_out, float* shifted_out, float* t_out,
                                           int16_t* symbols_planar, uint32_t* nonzero_flags, uint32_t* checks, int n, int hw,
                                           void* stream) {
    if (!y || !bin_widths_points || !thresholds_points || !point || n <= 0 || hw <= 0 || k_points < 1) return EAE_HIP_BAD_ARGUMENT;
    if (length < 1 || length > 255) return EAE_HIP_BAD_ARGUMENT;
    if ((gamma_out_packed == nullptr) != (beta_out == nullptr) || (gamma_out_packed && !t_out)) return EAE_HIP_BAD_ARGUMENT;
    if (!aligned_to(y, 16) || !aligned_to(bin_widths_points, 16) || !aligned_to(thresholds_points, 16) || !aligned_to(shifted_out, 16) ||
        !aligned_to(t_out, 16))
        return EAE_HIP_BAD_ARGUMENT;
    if (hw > (1 << 21)) return EAE_HIP_BAD_SHAPE;           // 32-bit symbol offsets inside the images of one tile
    const long rows = (long)n * hw;
    if ((rows + 31) / 32 > 0x7FFFFFFFL) return EAE_HIP_BAD_SHAPE;
    const unsigned grid = (unsigned)((rows + 31) / 32);
    const float amax = (float)(length < RDO_MAGNITUDES ? length : RDO_MAGNITUDES);
    hipStream_t s = (hipStream_t)stream;
    if (gamma_out_packed)
        hipLaunchKernelGGL((rdo_rows_kernel<true>), dim3(grid), dim3(256), 0, s, y, map_mean, bin_widths_points, thresholds_points, point,
                           k_points, amax, gamma_out_packed, beta_out, shifted_out, t_out, symbols_planar, nonzero_flags, checks, rows, hw);
    else
        hipLaunchKernelGGL((rdo_rows_kernel<false>), dim3(grid), dim3(256), 0, s, y, map_mean, bin_widths_points, thresholds_points, point,
                           k_points, amax, gamma_out_packed, beta_out, shifted_out, t_out, symbols_planar, nonzero_flags, checks, rows, hw);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
