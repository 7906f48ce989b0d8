// codec_container.hip -- what lets codec.BatchCodec hand out containers without a host round trip.
// container.encode_images fetches the bit counts, forms the payload offsets with a numpy cumsum, uploads them, packs, and copies
// the payload back; when an exception map is used it also forms that map's probability row on the host (container._exception_rows,
// from stats.py:181-195). Four launches do the same on the device with device-resident arguments only, so they sit inside
// the coder side of a step (and inside its captured hipGraph): probability rows from the histograms the step has anyway, the
// exclusive prefix sum over the 2 * n_maps piece lengths, the pack under an overflow flag (eae_hip_coder_pack_indexed: the pack
// kernel of container.hip), and a copy of just the packed bytes into pinned host memory.
#include "common.h"
#include "wave_scan.h"

namespace {

// wave_exclusive_scan's six DPP steps (wave_scan.h) on a 64-bit value: the halves move separately, the addition is 64-bit.
// Inclusive: lane l gets the sum over lanes 0..l.
__device__ __forceinline__ uint64_t wave_inclusive_scan64(uint64_t v) {
#define EAE_SCAN64_STEP(ctrl_, rows_)                                                                             \
    {                                                                                                             \
        const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, ctrl_, rows_, 0xF, false);   \
        const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), ctrl_, rows_, 0xF, false); \
        v += ((uint64_t)hi_ << 32) | lo_;                                                                         \
    }
    EAE_SCAN64_STEP(0x111, 0xF)      // row_shr:1
    EAE_SCAN64_STEP(0x112, 0xF)      // row_shr:2
    EAE_SCAN64_STEP(0x114, 0xF)      // row_shr:4
    EAE_SCAN64_STEP(0x118, 0xF)      // row_shr:8
    EAE_SCAN64_STEP(0x142, 0xA)      // row_bcast:15 into rows 1 and 3
    EAE_SCAN64_STEP(0x143, 0xC)      // row_bcast:31 into rows 2 and 3
#undef EAE_SCAN64_STEP
    return v;
}

// Entry e = 2 m + piece of the payload (image -> map -> arithmetic-coded bytes, bypass bytes) is as long as move_streams_kernel
// (container.hip) copies: the piece's bits rounded up to bytes, clamped to its half of the stream region.
constexpr int INDEX_THREADS = 1024;
constexpr int INDEX_WAVES = INDEX_THREADS / 64;

// One block scans all entries in chunks of INDEX_THREADS: a DPP scan per wavefront, the wavefronts' totals through LDS, the
// chunks' totals in a register every thread carries. A step has a few thousand entries (6,144 for 24 Kodak images): a grid-wide
// scan would spend more on its hand-overs than this block on its six chunks.
__global__ __launch_bounds__(INDEX_THREADS) void index_streams_kernel(uint64_t entries, uint64_t entries_per_image,
                                                                      const uint32_t* __restrict__ bac_bits,
                                                                      const uint32_t* __restrict__ bypass_bits, uint64_t half_stride,
                                                                      uint64_t capacity, uint64_t* offsets, uint64_t* index) {
    __shared__ uint64_t wave_total[INDEX_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < entries; base += INDEX_THREADS) {
        const uint64_t e = base + threadIdx.x;
        uint64_t len = 0;
        if (e < entries) {
            len = ((uint64_t)((e & 1u) ? bypass_bits[e >> 1] : bac_bits[e >> 1]) + 7u) >> 3;
            if (len > half_stride) len = half_stride;
        }
        const uint64_t inclusive = wave_inclusive_scan64(len);
        if (lane == 63u) wave_total[wave] = inclusive;
        __syncthreads();
        uint64_t before = carry, chunk = 0;
        for (uint32_t w = 0; w < (uint32_t)INDEX_WAVES; ++w) {
            const uint64_t t = wave_total[w];
            if (w < wave) before += t;
            chunk += t;
        }
        if (e < entries) offsets[e] = before + inclusive - len;
        carry += chunk;
        __syncthreads();      // wave_total is rewritten by the next chunk
    }
    // the offsets this block wrote are visible to all of it behind the barrier above: an image's bytes are the distance between
    // its first entry and the next image's
    const uint64_t images = entries / entries_per_image;
    for (uint64_t i = threadIdx.x; i < images; i += INDEX_THREADS) {
        const uint64_t first = offsets[i * entries_per_image];
        const uint64_t next = i + 1 < images ? offsets[(i + 1) * entries_per_image] : carry;
        index[2 + i] = next - first;
    }
    if (threadIdx.x == 0) {
        index[0] = carry;
        index[1] = carry > capacity ? 1u : 0u;
    }
}

// ---- the index of a step coded in tiles (eae_hip_coder_index_tiles) ---------------------------------------
// An entry is one (image, coding tile): maps_per_entry maps, 2 * maps_per_entry pieces. The coder keeps the entries of one shape
// class side by side (RUN order: bit counts, stream regions and offsets), the payload keeps them image -> tile (PAYLOAD order), and
// a piece is clamped to half of its own class's stride. table[2 p], table[2 p + 1]: the run-order index of payload-order entry p
// and the half stride of its class. Two levels instead of one block over every piece (36,864 for 24 Kodak images in tiles of 16 x
// 16): a block per entry scans the entry's pieces, one block scans the entries' totals, a block per entry adds the entry's base.
// The slot of an entry's first piece carries the hand-over between the three launches: its own local offset is zero, so it holds
// the entry's bytes behind the first launch, the entry's offset in the payload behind the second -- its final value --, and the
// third reads it and leaves it alone. A table row that names no entry of the step is skipped by all three.
constexpr int ENTRY_THREADS = 256;
constexpr int ENTRY_WAVES = ENTRY_THREADS / 64;

__global__ __launch_bounds__(ENTRY_THREADS) void index_entry_pieces_kernel(uint64_t entries, uint32_t maps_per_entry,
                                                                           const uint32_t* __restrict__ bac_bits,
                                                                           const uint32_t* __restrict__ bypass_bits,
                                                                           const uint64_t* __restrict__ table, uint64_t* offsets) {
    __shared__ uint64_t wave_total[ENTRY_WAVES];
    const uint64_t run_entry = table[2 * (uint64_t)blockIdx.x], half_stride = table[2 * (uint64_t)blockIdx.x + 1];
    if (run_entry >= entries) return;                      // block-uniform, in front of every barrier
    const uint64_t first = run_entry * maps_per_entry;     // the entry's first stream
    const uint64_t pieces = 2 * (uint64_t)maps_per_entry;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < pieces; base += ENTRY_THREADS) {
        const uint64_t j = base + threadIdx.x;
        uint64_t len = 0;
        if (j < pieces) {
            len = ((uint64_t)((j & 1u) ? bypass_bits[first + (j >> 1)] : bac_bits[first + (j >> 1)]) + 7u) >> 3;
            if (len > half_stride) len = half_stride;
        }
        const uint64_t inclusive = wave_inclusive_scan64(len);
        if (lane == 63u) wave_total[wave] = inclusive;
        __syncthreads();
        uint64_t before = carry, chunk = 0;
        for (uint32_t w = 0; w < (uint32_t)ENTRY_WAVES; ++w) {
            const uint64_t t = wave_total[w];
            if (w < wave) before += t;
            chunk += t;
        }
        if (j < pieces && j != 0) offsets[2 * first + j] = before + inclusive - len;
        carry += chunk;
        __syncthreads();      // wave_total is rewritten by the next chunk
    }
    if (threadIdx.x == 0) offsets[2 * first] = carry;
}

// index_streams_kernel's scan over the entries' bytes in payload order, read from and written back to the slots of the entries'
// first pieces; then the bytes of every image, the total and the overflow flag as index_streams_kernel leaves them.
__global__ __launch_bounds__(INDEX_THREADS) void index_entry_bases_kernel(uint64_t entries, uint64_t entries_per_image,
                                                                          uint32_t maps_per_entry, const uint64_t* __restrict__ table,
                                                                          uint64_t capacity, uint64_t* offsets, uint64_t* index) {
    __shared__ uint64_t wave_total[INDEX_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < entries; base += INDEX_THREADS) {
        const uint64_t p = base + threadIdx.x;
        uint64_t* slot = nullptr;
        if (p < entries && table[2 * p] < entries) slot = offsets + 2 * table[2 * p] * maps_per_entry;
        const uint64_t len = slot ? *slot : 0;
        const uint64_t inclusive = wave_inclusive_scan64(len);
        if (lane == 63u) wave_total[wave] = inclusive;
        __syncthreads();
        uint64_t before = carry, chunk = 0;
        for (uint32_t w = 0; w < (uint32_t)INDEX_WAVES; ++w) {
            const uint64_t t = wave_total[w];
            if (w < wave) before += t;
            chunk += t;
        }
        if (slot) *slot = before + inclusive - len;
        carry += chunk;
        __syncthreads();      // wave_total is rewritten by the next chunk; the slots written are visible to the block behind it
    }
    // an image's bytes are the distance between its first entry's offset and the next image's (a skipped row counts from zero)
    const uint64_t images = entries / entries_per_image;
    for (uint64_t i = threadIdx.x; i < images; i += INDEX_THREADS) {
        const uint64_t a = table[2 * i * entries_per_image];
        const uint64_t b = i + 1 < images ? table[2 * (i + 1) * entries_per_image] : 0;
        const uint64_t first = a < entries ? offsets[2 * a * maps_per_entry] : 0;
        const uint64_t next = i + 1 < images ? (b < entries ? offsets[2 * b * maps_per_entry] : 0) : carry;
        index[2 + i] = next - first;
    }
    if (threadIdx.x == 0) {
        index[0] = carry;
        index[1] = carry > capacity ? 1u : 0u;
    }
}

__global__ __launch_bounds__(ENTRY_THREADS) void index_entry_add_kernel(uint64_t entries, uint32_t maps_per_entry,
                                                                        const uint64_t* __restrict__ table, uint64_t* offsets) {
    const uint64_t run_entry = table[2 * (uint64_t)blockIdx.x];
    if (run_entry >= entries) return;
    uint64_t* entry = offsets + 2 * run_entry * maps_per_entry;
    const uint64_t entry_base = entry[0];                  // nobody writes it here
    for (uint64_t j = threadIdx.x; j < 2 * (uint64_t)maps_per_entry; j += ENTRY_THREADS)
        if (j != 0) entry[j] += entry_base;
}

// The first *nbytes bytes (at most `capacity`) of `src`, rounded up to whole 16-byte words, into pinned host memory: one 16-byte
// load and store per lane, a fixed grid striding over the words. The length is read on the device, so the launch has no
// host-dependent argument. Visibility as publish_kernel (misc.hip): a system-scope fence behind the stores, and the host looks
// only after a later launch of the same stream has published the step counter.
constexpr int PREFIX_BLOCKS = 64;
__global__ __launch_bounds__(256) void publish_prefix_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, uint64_t capacity,
                                                             const uint64_t* __restrict__ nbytes) {
    uint64_t n = *nbytes;
    if (n > capacity) n = capacity;
    const uint64_t words = (n + 15u) >> 4;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x)
        dst[i] = __builtin_nontemporal_load(src + i);
    __threadfence_system();
}

// container._exception_rows per image: the decisions of the truncated unary prefix counted from the histogram of the exception
// map (stats.py:181-195): position j sees a zero for every symbol of magnitude j and a one for every symbol of a larger magnitude,
// i.e. for map_size minus the symbols of magnitude <= j -- which needs no bin beyond |s| = L - 1, so symbols outside the
// histogram's radius (>= L) are counted right without being seen. One block per image, thread j forms position j.
__global__ __launch_bounds__(256) void exception_rows_kernel(const uint32_t* __restrict__ hist, int radius, uint32_t map_size, int length,
                                                             double* __restrict__ rows) {
    __shared__ uint32_t wave_total[4];
    const uint32_t* h = hist + (size_t)blockIdx.x * (2u * (uint32_t)radius + 1u);
    const int j = threadIdx.x;
    uint32_t zeros = 0;
    if (j < length) zeros = h[radius + j] + (j ? h[radius - j] : 0u);
    uint32_t total;
    uint32_t upto = wave_exclusive_scan(zeros, total) + zeros;      // magnitudes <= j, within this wavefront
    if ((threadIdx.x & 63u) == 0u) wave_total[threadIdx.x >> 6] = total;
    __syncthreads();
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) upto += wave_total[w];
    if (j < length) {
        const uint32_t ones = upto < map_size ? map_size - upto : 0u;
        const double decisions = (double)zeros + (double)ones;
        double p = 0.5;                                             // 0 / 0 (stats.py:56-66)
        if (decisions != 0.) {
            p = (double)zeros / decisions;
            if (p == 0.) p = 0.01;
            if (p == 1.) p = 0.99;
        }
        rows[(size_t)blockIdx.x * length + j] = p;
    }
}

}  // namespace

extern "C" int eae_hip_coder_index_streams(uint32_t n_maps, uint32_t maps_per_image, const uint32_t* bac_bits, const uint32_t* bypass_bits,
                                           uint64_t stream_stride_bytes, uint64_t capacity_bytes, uint64_t* offsets_out, uint64_t* index_out,
                                           void* stream) {
    if (!bac_bits || !bypass_bits || !offsets_out || !index_out || n_maps == 0 || maps_per_image == 0 || stream_stride_bytes < 2)
        return EAE_HIP_BAD_ARGUMENT;
    if (n_maps % maps_per_image != 0) return EAE_HIP_BAD_SHAPE;
    hipLaunchKernelGGL(index_streams_kernel, dim3(1), dim3(INDEX_THREADS), 0, (hipStream_t)stream, 2 * (uint64_t)n_maps,
                       2 * (uint64_t)maps_per_image, bac_bits, bypass_bits, stream_stride_bytes / 2, capacity_bytes, offsets_out, index_out);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_coder_index_tiles(uint32_t n_streams, uint32_t maps_per_entry, uint32_t entries_per_image, const uint32_t* bac_bits,
                                         const uint32_t* bypass_bits, const uint64_t* entry_table, uint64_t capacity_bytes,
                                         uint64_t* offsets_out, uint64_t* index_out, void* stream) {
    if (!bac_bits || !bypass_bits || !entry_table || !offsets_out || !index_out || n_streams == 0 || maps_per_entry == 0 ||
        entries_per_image == 0)
        return EAE_HIP_BAD_ARGUMENT;
    if ((uint64_t)n_streams % ((uint64_t)maps_per_entry * entries_per_image) != 0) return EAE_HIP_BAD_SHAPE;
    const uint64_t entries = n_streams / maps_per_entry;
    hipLaunchKernelGGL(index_entry_pieces_kernel, dim3((unsigned)entries), dim3(ENTRY_THREADS), 0, (hipStream_t)stream, entries,
                       maps_per_entry, bac_bits, bypass_bits, entry_table, offsets_out);
    EAE_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(index_entry_bases_kernel, dim3(1), dim3(INDEX_THREADS), 0, (hipStream_t)stream, entries,
                       (uint64_t)entries_per_image, maps_per_entry, entry_table, capacity_bytes, offsets_out, index_out);
    EAE_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(index_entry_add_kernel, dim3((unsigned)entries), dim3(ENTRY_THREADS), 0, (hipStream_t)stream, entries,
                       maps_per_entry, entry_table, offsets_out);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_publish_prefix(const void* src_device, void* dst_host_mapped, uint64_t capacity_bytes, const uint64_t* nbytes_device,
                                      void* stream) {
    if (!src_device || !dst_host_mapped || !nbytes_device || (capacity_bytes & 15u)) return EAE_HIP_BAD_ARGUMENT;
    if (((uintptr_t)src_device | (uintptr_t)dst_host_mapped) & 15u) return EAE_HIP_BAD_ARGUMENT;      // 16-byte loads and stores
    if (((uintptr_t)nbytes_device) & 7u) return EAE_HIP_BAD_ARGUMENT;
    if (capacity_bytes == 0) return EAE_HIP_OK;
    hipLaunchKernelGGL(publish_prefix_kernel, dim3(PREFIX_BLOCKS), dim3(256), 0, (hipStream_t)stream, (const u32x4*)src_device,
                       (u32x4*)dst_host_mapped, capacity_bytes, nbytes_device);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}

extern "C" int eae_hip_exception_rows(int n, const uint32_t* hist, const uint32_t* overflow, int radius, int map_size, int length,
                                      double* rows_out, void* stream) {
    if (!hist || !overflow || !rows_out || n <= 0 || map_size <= 0 || length < 1 || length > 255) return EAE_HIP_BAD_ARGUMENT;
    if (radius < length) return EAE_HIP_BAD_ARGUMENT;      // every magnitude below L needs its own bin
    hipLaunchKernelGGL(exception_rows_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, hist, radius, (uint32_t)map_size, length, rows_out);
    EAE_HIP_CHECK_LAUNCH();
    return EAE_HIP_OK;
}
