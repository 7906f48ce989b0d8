// quarter_body.h -- the latent stage on a block of four wavefronts that share 32 positions, one 32-channel tile each: the body of
// latent_quarter_kernel (latent.hip: gdn_3, quantiser, inverse_gdn_4 with one row of bin widths) and of latent_rows_kernel and
// rdo_rows_kernel (latent_rows.hip: quantiser and inverse_gdn_4 with a row of bin widths per image). latent.hip says why four waves.
// Every wave keeps the squares of all 128 channels of the 32 positions in registers as the B operand (each wave squares and orders its
// own 32 channels, then they exchange through LDS, lane-private slots) but accumulates, normalises, quantises and stores only its own
// 32 channels. Same FMA chain per element and same statements as gdn.hip and quantize.hip: same bits.
// The kernels differ in two expressions only, which they pass to quarter_quantise as callables: where a lane's four bin widths of
// group g come from, and the rounded quotient of an element.
#pragma once
#include "latent_body.h"

// Where a lane of the block stands: wave w owns channels 32 w .. 32 w + 31, lane (hi, lj) of it position lj of the tile and the
// 16 channels cw + 8 g + q. Passed BY VALUE: behind a reference the compiler recomputed the address of the per-lane dead-map flag
// at each of its 16 stores (30 instructions and two registers more; profiles/quarter_body.md).
struct QuarterLane {
    int tid, lane, hi, lj, w, pix, cw;
    long row, img;                // position in [0, N * hw), its image; pix: its pixel there
    bool valid;                   // row < rows
    size_t obase;                 // of this lane's first channel in an [N][hw][128] tensor (row 0 when not valid)
};

__device__ __forceinline__ QuarterLane quarter_lane(long rows, int hw) {
    QuarterLane p;
    p.tid = threadIdx.x; p.lane = p.tid & 63; p.hi = p.lane >> 5; p.lj = p.lane & 31;
    p.w = __builtin_amdgcn_readfirstlane(p.tid >> 6);
    p.row = (long)blockIdx.x * 32 + p.lj;
    p.valid = p.row < rows;
    p.img = p.row / hw;
    p.pix = (int)(p.row - p.img * hw);
    p.cw = 32 * p.w + 4 * p.hi;
    p.obase = (size_t)(p.valid ? p.row : 0) * EAE_C + p.cw;
    return p;
}

// the lane's 16 channels, [4 g + q]; zeros for a position past the last image
__device__ __forceinline__ f32x16 quarter_load(const float* x, const QuarterLane p) {
    f32x16 own;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 q = p.valid ? *reinterpret_cast<const float4*>(x + p.obase + 8 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
        own[4 * g + 0] = q.x; own[4 * g + 1] = q.y; own[4 * g + 2] = q.z; own[4 * g + 3] = q.w;
    }
    return own;
}

// One normalisation of the tile: every wave publishes the squares of its channels in xch ([channel tile][g][lane][4], 16 KB), reads
// all four tiles back behind ONE barrier (which also covers what the block wrote to LDS before it), and normalises its own channels
// with gamma on the MFMA and beta from LDS (128 floats); store(0, g, float4) gets the results. A second call needs a barrier in
// front of it: every wave has to be done reading the first exchange.
template <bool INVERSE, typename Store>
__device__ __forceinline__ void quarter_normalise(const f32x16 own, float* xch, const float* __restrict__ gamma_packed, const float* beta_lds,
                                                  const QuarterLane p, Store store) {
    float4* slot = reinterpret_cast<float4*>(xch) + p.lane;  // + (4 t + g) * 64: [t][g][lane]
    const f32x16 sq = squares_for_mfma(own);
#pragma unroll
    for (int g = 0; g < 4; ++g) slot[(4 * p.w + g) * 64] = make_float4(sq[4 * g], sq[4 * g + 1], sq[4 * g + 2], sq[4 * g + 3]);
    __syncthreads();
    f32x16 full[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 q = slot[(4 * t + g) * 64];
            full[t][4 * g + 0] = q.x; full[t][4 * g + 1] = q.y; full[t][4 * g + 2] = q.z; full[t][4 * g + 3] = q.w;
        }
    f32x16 d[1] = {quarter_denominator<8>(full, gamma_packed, p.w, p.lane)};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 bt = *reinterpret_cast<const float4*>(beta_lds + p.cw + 8 * g);
        d[0][4 * g + 0] = d[0][4 * g + 0] + bt.x;
        d[0][4 * g + 1] = d[0][4 * g + 1] + bt.y;
        d[0][4 * g + 2] = d[0][4 * g + 2] + bt.z;
        d[0][4 * g + 3] = d[0][4 * g + 3] + bt.w;
    }
    const f32x16 xn[1] = {own};
    gdn_tile<1, INVERSE, false>(xn, d, store);
}

// The quantiser on this wave's 32 channels (quantize.hip, statement for statement) and everything behind it: the three data checks,
// the dead-map flags, the planar symbols, y_out / shifted_out, inverse_gdn_4 into t_out (IGDN_OUT) and the counters of `checks`.
// Every output pointer may be null (t_out with IGDN_OUT may not). The block's LDS: mean_lds and beta_out_lds (128 floats each, filled
// and behind a barrier), xch (quarter_normalise; XCH_USED: an earlier exchange went through it) and tally.
//   bin_widths(g)                  the lane's four bin widths of channels cw + 8 g .. + 3
//   quotient(i, centered, bw)      the rounded quotient of element i = 4 g + q: round_half_even(centered / bw), or the caller's choice
template <bool IGDN_OUT, bool XCH_USED, typename BinWidths, typename Quotient>
__device__ __forceinline__ void quarter_quantise(f32x16 own, const QuarterLane p, const float* mean_lds, const float* beta_out_lds,
                                                 float* xch, unsigned int (*tally)[3], const float* __restrict__ gamma_out, float* y_out,
                                                 float* shifted_out, float* t_out, int16_t* symbols, unsigned int* nonzero,
                                                 unsigned int* checks, int hw, BinWidths bin_widths, Quotient quotient) {
    const int lane = p.lane, w = p.w, cw = p.cw;
    const bool valid = p.valid;
    // Planar symbols: the lanes of a half-wave write neighbouring pixels of one map; offsets are relative to the tile's first image
    // so that 32 bits do
    const long img0 = ((long)blockIdx.x * 32) / hw;
    const bool one_image = __all(!valid || p.img == img0) != 0;
    const __amdgpu_buffer_rsrc_t sym_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        symbols ? symbols + (size_t)img0 * EAE_C * hw : nullptr, 0, symbols ? 0x7FFFFFFF : 0, 0x00020000);
    const int sym_lane = valid ? (int)((((p.img - img0) * EAE_C + 4 * p.hi) * hw + p.pix) * 2) : -1;     // bytes; -1: no store
    unsigned int bad = 0, not_quantized = 0, altered = 0, flag_bits = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 m4 = *reinterpret_cast<const float4*>(mean_lds + cw + 8 * g);
        const float4 b4 = bin_widths(g);
        const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, bw[4] = {b4.x, b4.y, b4.z, b4.w};
        float sh[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float yv = own[4 * g + q];
            const float centered = yv - mm[q];
            const float rr = quotient(4 * g + q, centered, bw[q]);
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
                    nonzero[p.img * EAE_C + cw + 8 * g + q] = 1u;                    // benign race: every writer stores 1
                }
            }
            if (symbols)
                __builtin_amdgcn_raw_buffer_store_b16((short)(int16_t)(int)rs, sym_rsrc, sym_lane, (32 * w + 8 * g + q) * hw * 2, 0);
        }
        if (valid && y_out)
            *reinterpret_cast<float4*>(y_out + p.obase + 8 * g) = make_float4(own[4 * g], own[4 * g + 1], own[4 * g + 2], own[4 * g + 3]);
        if (valid && shifted_out) *reinterpret_cast<float4*>(shifted_out + p.obase + 8 * g) = make_float4(sh[0], sh[1], sh[2], sh[3]);
        own[4 * g + 0] = sh[0]; own[4 * g + 1] = sh[1]; own[4 * g + 2] = sh[2]; own[4 * g + 3] = sh[3];
    }
    if (nonzero && one_image && lane < 32 && ((flag_bits >> lane) & 1u)) nonzero[img0 * EAE_C + 32 * w + lane] = 1u;
#ifndef EAE_LATENT_NOCHECKS
    if (checks) {
        // one atomic per block and counter: all 4,608 waves adding to the same three words would queue behind each other in L2
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            bad += __shfl_down(bad, off, 64);
            not_quantized += __shfl_down(not_quantized, off, 64);
            altered += __shfl_down(altered, off, 64);
        }
        if (lane == 0) { tally[w][0] = bad; tally[w][1] = not_quantized; tally[w][2] = altered; }
    }
#endif
    if (IGDN_OUT) {
        if (XCH_USED) __syncthreads();                       // every wave has read the earlier exchange
        quarter_normalise<true>(own, xch, gamma_out, beta_out_lds, p, [&](int, int g, float4 v) {
            if (valid) *reinterpret_cast<float4*>(t_out + p.obase + 8 * g) = v;
        });
    }
#ifndef EAE_LATENT_NOCHECKS
    if (checks) {
        if (!IGDN_OUT) __syncthreads();                      // (with IGDN_OUT the exchange's barrier came after the tally)
        if (p.tid < 3) {
            const unsigned int sum = tally[0][p.tid] + tally[1][p.tid] + tally[2][p.tid] + tally[3][p.tid];
            if (sum) atomicAdd(&checks[p.tid], sum);
        }
    }
#endif
}
