// fill.h -- stream-ordered fills by a kernel (misc.hip), for launches that a caller may capture into a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// `bytes` bytes of device memory at `dst_device` set to `value` on `stream`, by a kernel and not by hipMemsetAsync: a kernel node of a
// captured step replays with the arguments it was captured with. Any size and alignment; a failed launch
// is returned, as hipMemsetAsync returns it.
int eae_fill_async(void* dst_device, uint8_t value, uint64_t bytes, hipStream_t stream);
