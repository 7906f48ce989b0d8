// wave_scan.h -- prefix sums over the 64 lanes of a wavefront (gfx9 DPP), shared by the coder's data-parallel passes
// (coder_simd.hip) and the container index (codec_container.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Exclusive prefix sum over the 64 lanes, and the total. Data-parallel primitives, not cross-lane loads: four row_shr steps scan
// the rows of 16 lanes, row_bcast:15 / :31 carry the row totals on (the sequence LLVM's atomic optimiser emits for gfx9): 6 DPP
// additions where six __shfl_up rounds were 6 x (ds_bpermute + compare + add).
__device__ __forceinline__ uint32_t wave_exclusive_scan(uint32_t v, uint32_t& total) {
    int inc = (int)v;
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xF, 0xF, false);     // row_shr:1
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xF, 0xF, false);     // row_shr:2
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xF, 0xF, false);     // row_shr:4
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xF, 0xF, false);     // row_shr:8
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x142, 0xA, 0xF, false);     // row_bcast:15 into rows 1 and 3
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x143, 0xC, 0xF, false);     // row_bcast:31 into rows 2 and 3
    total = (uint32_t)__builtin_amdgcn_readlane(inc, 63);
    return (uint32_t)inc - v;
}
