// byte_runs.h -- unaligned runs of four bytes out of a dense u8 tensor (frame.hip, colour.hip), read the way publish_crops does
// (codec_decode.hip): from the two aligned dwords around the run, combined by v_alignbyte_b32, when both lie inside the tensor --
// the bounds are those of the tensor's bytes, not of its allocation: an aligned dword that starts in front of the first byte or
// ends behind the last one is never loaded --, else byte by byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The four bytes at `addr` .. `addr + 3`, all inside [begin, end), little endian.
__device__ __forceinline__ uint32_t load_run4(const uint8_t* begin, const uint8_t* end, const uint8_t* addr) {
    const uintptr_t a = (uintptr_t)addr, aligned = a & ~(uintptr_t)3;
    if (aligned >= (uintptr_t)begin && aligned + 8 <= (uintptr_t)end) {
        const uint32_t lo = *reinterpret_cast<const uint32_t*>(aligned);
        const uint32_t hi = *reinterpret_cast<const uint32_t*>(aligned + 4);
        return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(a & 3u));
    }
    return (uint32_t)addr[0] | ((uint32_t)addr[1] << 8) | ((uint32_t)addr[2] << 16) | ((uint32_t)addr[3] << 24);
}
