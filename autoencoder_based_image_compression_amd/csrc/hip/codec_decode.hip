// codec_decode.hip -- the two launches codec.BatchDecoder needs beside the ones the container path already has (DESIGN.md
// section 14), and the publish of codec.RegionDecoder (section 17: eae_hip_publish_crops, at the end of the namespace). container.decode_images uploads the payload with a synchronous copy and dequantises a whole blob with one row of
// bin widths and means; a resident decoder replays one captured step per slot, so (1) the payload comes out of the slot's pinned
// buffer by a kernel whose length is read on the device -- a replay moves the bytes the step has, not the buffer's capacity --
// and (2) the images of one step may come from different blobs, each with its own bin widths and means.
#include "common.h"

namespace {

// The mirror of publish_prefix_kernel (codec_container.hip): the first *nbytes bytes (at most `capacity`) of pinned, device-mapped
// host memory, rounded up to whole 16-byte words, into device memory: one 16-byte load and store per lane, a fixed grid striding
// over the words. Nothing at or beyond the last of those words is written. The consumer is a later launch of the same stream.
constexpr int FETCH_BLOCKS = 64;
__global__ __launch_bounds__(256) void fetch_prefix_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, uint64_t capacity,
                                                           const uint64_t* __restrict__ nbytes) {
    uint64_t n = *nbytes;
    if (n > capacity) n = capacity;
    const uint64_t words = (n + 15u) >> 4;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x)
        dst[i] = __builtin_nontemporal_load(src + i);
}

constexpr int DQ_THREADS = 256;
constexpr int DQ_PIX = 64;           // pixels per block
constexpr int DQ_PITCH = EAE_C + 4;  // int16 per pixel row in LDS: 264 bytes keeps every row 8-byte aligned for ds_read_b64

// blockIdx.y = image, blockIdx.x = chunk of 64 pixels. tile_symbols_dequantize_kernel (tile_symbols.hip) for whole maps, with the
// image's own row of bin widths and means: the chunk's symbols -> LDS as [pixel][map] (the global reads run along the pixels of one
// map, 128 bytes per wave), then every pixel's 128 channels leave as 32 16-byte stores of 4 channels, a half-wave per pixel.
// Exactly the arithmetic of dequantize_kernel (container.hip): cq = bw * symbol, then cq + mean, no contraction.
// LDS: the reads are ds_read_b64 at dword 66 * pixel + 2 * quad, so each half-wave covers the 64 banks once. The 2-byte writes of a
// wave go to one map of 64 pixels, dword 66 * pixel + map / 2: the 32 pixels of a half-wave fall on 32 different banks.
__global__ __launch_bounds__(DQ_THREADS) void dequantize_rows_kernel(const int16_t* __restrict__ symbols, const float* __restrict__ bin_widths,
                                                                     const float* __restrict__ map_mean, float* __restrict__ cq_out,
                                                                     float* __restrict__ shifted_out, int hw) {
    __shared__ __attribute__((aligned(16))) int16_t lds[DQ_PIX][DQ_PITCH];
    const size_t img = blockIdx.y;
    const int p0 = blockIdx.x * DQ_PIX;
    const int16_t* src = symbols + img * EAE_C * (size_t)hw;
    const int tid = threadIdx.x;
    for (int i = tid; i < EAE_C * DQ_PIX; i += DQ_THREADS) {
        const int ch = i >> 6, px = i & (DQ_PIX - 1);
        const int p = p0 + px;
        lds[px][ch] = p < hw ? src[(size_t)ch * hw + p] : (int16_t)0;
    }
    __syncthreads();
    const int q = tid & 31, sub = tid >> 5;                    // channel quad, pixel of the pass
    float bw[4], m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bw[k] = bin_widths[img * EAE_C + 4 * q + k];
        m[k] = map_mean ? map_mean[img * EAE_C + 4 * q + k] : 0.f;
    }
    for (int pass = 0; pass < DQ_PIX / 8; ++pass) {
        const int px = pass * 8 + sub;
        const int p = p0 + px;
        if (p >= hw) break;
        const uint2 packed = *reinterpret_cast<const uint2*>(&lds[px][4 * q]);
        const int16_t s[4] = {(int16_t)(packed.x & 0xFFFFu), (int16_t)(packed.x >> 16), (int16_t)(packed.y & 0xFFFFu), (int16_t)(packed.y >> 16)};
        float4 cq, shifted;
        float* cf = reinterpret_cast<float*>(&cq);
        float* sf = reinterpret_cast<float*>(&shifted);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cf[k] = bw[k] * (float)s[k];                       // tools.py:929 with round(x / bw) == symbol
            sf[k] = cf[k] + m[k];                              // reconstructing_eae_kodak.py:192
        }
        const size_t idx = (img * (size_t)hw + p) * EAE_C + 4 * q;
        if (cq_out) *reinterpret_cast<float4*>(cq_out + idx) = cq;
        if (shifted_out) *reinterpret_cast<float4*>(shifted_out + idx) = shifted;
    }
}

// eae_hip_publish_crops (codec.RegionDecoder): one ch x cw rectangle out of each of n planes u8 [n][H][W],
// at origins the step left in device memory, into dst = [n][ch][cw] u8, flat. A lane forms one 16-byte word of dst -- the only
// store width that goes to pinned memory -- out of four dwords. A dword whose four bytes lie in one row of one crop comes from the
// two aligned dwords of the plane around its (unaligned) source address, combined by v_alignbyte_b32; a dword that crosses the end
// of a row or of a crop, the tail of dst, and a source dword that would reach past the planes, are gathered byte by byte. The
// bytes behind the last crop in the last word are zero. Origins are clamped to [0, H - ch] x [0, W - cw] here, so no load leaves
// the planes whatever the words hold. Visibility to the host as publish_kernel (misc.hip).
struct CropShape {
    uint32_t n, H, W, ch, cw;
    uint64_t total;          // n * ch * cw
    uint64_t plane_bytes;    // n * H * W
};

__device__ __forceinline__ int clamp_origin(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// byte offset, in the planes, of pixel (0, 0) of crop k
__device__ __forceinline__ uint64_t crop_base(const int32_t* __restrict__ origins, const CropShape& s, uint32_t k) {
    const int oy = clamp_origin(origins[2 * k], (int)(s.H - s.ch)), ox = clamp_origin(origins[2 * k + 1], (int)(s.W - s.cw));
    return ((uint64_t)k * s.H + (uint32_t)oy) * s.W + (uint32_t)ox;
}

constexpr int CROP_BLOCKS = 256;
__global__ __launch_bounds__(256) void publish_crops_kernel(const uint8_t* __restrict__ planes, const int32_t* __restrict__ origins,
                                                            u32x4* __restrict__ dst, CropShape s) {
    const uint64_t words = (s.total + 15u) >> 4;
    const uint32_t per_crop = s.ch * s.cw;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t out[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint64_t b = 16 * i + 4 * (uint64_t)d;
            uint32_t v = 0;
            if (b < s.total) {
                uint32_t k = (uint32_t)(b / per_crop);
                const uint32_t rem = (uint32_t)(b - (uint64_t)k * per_crop);
                uint32_t y = rem / s.cw, x = rem - y * s.cw;
                uint64_t base = crop_base(origins, s, k);
                const uint64_t addr = base + (uint64_t)y * s.W + x;
                const uint64_t aligned = addr & ~(uint64_t)3;
                if (x + 4 <= s.cw && aligned + 8 <= s.plane_bytes) {
                    const uint32_t lo = *reinterpret_cast<const uint32_t*>(planes + aligned);
                    const uint32_t hi = *reinterpret_cast<const uint32_t*>(planes + aligned + 4);
                    v = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(addr & 3u));
                } else {
                    for (int j = 0; j < 4 && k < s.n; ++j) {
                        v |= (uint32_t)planes[base + (uint64_t)y * s.W + x] << (8 * j);
                        if (++x == s.cw) {
                            x = 0;
                            if (++y == s.ch) {
                                y = 0;
                                if (++k < s.n) base = crop_base(origins, s, k);
                            }
                        }
                    }
                }
            }
            out[d] = v;
        }
        u32x4 word;
        word.x = out[0], word.y = out[1], word.z = out[2], word.w = out[3];
        dst[i] = word;
    }
    __threadfence_system();
}

}  // namespace

extern "C" int eae_hip_publish_crops(const uint8_t* planes, int n, int H, int W, const int32_t* origins, int ch, int cw, void* dst,
                                     uint64_t dst_capacity_bytes, void* stream) {
    if (!planes || !origins || !dst || n <= 0 || H <= 0 || W <= 0 || ch <= 0 || cw <= 0) return EAE_HIP_BAD_ARGUMENT;
    if ((((uintptr_t)dst) & 15u) || (dst_capacity_bytes & 15u) || (((uintptr_t)planes) & 3u) || (((uintptr_t)origins) & 3u))
        return EAE_HIP_BAD_ARGUMENT;      // 16-byte stores, aligned dword loads
    if (ch > H || cw > W) return EAE_HIP_BAD_SHAPE;
    const uint64_t total = (uint64_t)n * (uint64_t)ch * (uint64_t)cw;
    if ((uint64_t)ch * (uint64_t)cw > 0x7FFFFFFFull || ((total + 15u) & ~(uint64_t)15u) > dst_capacity_bytes) return EAE_HIP_BAD_SHAPE;
    CropShape s;
    s.n = (uint32_t)n, s.H = (uint32_t)H, s.W = (uint32_t)W, s.ch = (uint32_t)ch, s.cw = (uint32_t)cw;
    s.total = total;
    s.plane_bytes = (uint64_t)n * (uint64_t)H * (uint64_t)W;
    const uint64_t words = (total + 15u) >> 4;
    const unsigned blocks = (unsigned)((words + 255) / 256 > (uint64_t)CROP_BLOCKS ? (uint64_t)CROP_BLOCKS : (words + 255) / 256);
    hipLaunchKernelGGL(publish_crops_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, planes, origins, (u32x4*)dst, s);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_fetch_prefix(const void* src_host_mapped, void* dst_device, uint64_t capacity_bytes, const uint64_t* nbytes_device,
                                    void* stream) {
    if (!src_host_mapped || !dst_device || !nbytes_device || (capacity_bytes & 15u)) return EAE_HIP_BAD_ARGUMENT;
    if (((uintptr_t)src_host_mapped | (uintptr_t)dst_device) & 15u) return EAE_HIP_BAD_ARGUMENT;      // 16-byte loads and stores
    if (((uintptr_t)nbytes_device) & 7u) return EAE_HIP_BAD_ARGUMENT;
    if (capacity_bytes == 0) return EAE_HIP_OK;
    hipLaunchKernelGGL(fetch_prefix_kernel, dim3(FETCH_BLOCKS), dim3(256), 0, (hipStream_t)stream, (const u32x4*)src_host_mapped,
                       (u32x4*)dst_device, capacity_bytes, nbytes_device);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_dequantize_maps_rows(const int16_t* symbols_planar, const float* bin_widths_rows, const float* map_mean_rows,
                                            float* cq_out, float* shifted_out, int n, int hw, int c, void* stream) {
    if (!symbols_planar || !bin_widths_rows || (!cq_out && !shifted_out) || n <= 0 || hw <= 0) return EAE_HIP_BAD_ARGUMENT;
    if (c != EAE_C || n > 65535) return EAE_HIP_BAD_SHAPE;
    if ((((uintptr_t)cq_out) | ((uintptr_t)shifted_out)) & 15u) return EAE_HIP_BAD_SHAPE;            // 16-byte stores
    const int chunks = (int)(((int64_t)hw + DQ_PIX - 1) / DQ_PIX);
    hipLaunchKernelGGL(dequantize_rows_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(DQ_THREADS), 0, (hipStream_t)stream, symbols_planar,
                       bin_widths_rows, map_mean_rows, cq_out, shifted_out, hw);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
