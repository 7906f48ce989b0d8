// bt601.h -- tls.rgb_to_ycbcr (tools.py:1019-1083) per pixel, for the kernels that turn RGB into YCbCr (quantize.hip:
// rgb_to_ycbcr_kernel; colour.hip: colour_split_kernel): ITU-R BT.601 in float64, terms added left to right as numpy evaluates
// them, clip to [0, 255], round half to even, uint8. The constants are the same IEEE doubles Python forms (65.481/255. etc.).
// tests/test_gpu_surface.py holds rgb_to_ycbcr_kernel, hence these three functions, to the reference on all 2^24 colours.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint8_t bt601_u8(double x) { return (uint8_t)rint(fmin(fmax(x, 0.), 255.)); }

__device__ __forceinline__ uint8_t bt601_y(double r, double g, double b) {
    return bt601_u8(16. + (65.481 / 255.) * r + (128.553 / 255.) * g + (24.966 / 255.) * b);
}
__device__ __forceinline__ uint8_t bt601_cb(double r, double g, double b) {
    return bt601_u8(128. - (37.797 / 255.) * r - (74.203 / 255.) * g + (112. / 255.) * b);
}
__device__ __forceinline__ uint8_t bt601_cr(double r, double g, double b) {
    return bt601_u8(128. + (112. / 255.) * r - (93.786 / 255.) * g - (18.214 / 255.) * b);
}
