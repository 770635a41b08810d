// The FP8 storage format (include/mmrag.h MMRAG_F8E4M3): one definition of the encoder and the decoder for
// every kernel that writes or reads code rows (common.hip's collection rows, maxsim.hip's token rows).
#pragma once
#include <hip/hip_runtime.h>

namespace mmrag_impl {

// OCP E4M3 code of x * 256, round to nearest even; subnormals kept, |y| > 448 saturates to 448 (0x7e), NaN stores +0.
// Written out in integer arithmetic: the hardware converter's NaN and saturation rules depend on mode bits this
// library does not own.
__device__ inline unsigned char f8_encode(float x) {
    const float y = x * 256.0f;
    if (y != y) return 0;
    const unsigned sign = (__float_as_uint(y) >> 24) & 0x80u;
    const float a = fabsf(y);
    if (a > 448.0f) return (unsigned char)(sign | 0x7eu);
    if (a < 0.015625f) return (unsigned char)(sign | (unsigned)rintf(a * 512.0f));   // subnormal step 2^-9; 8 = 2^-6
    unsigned u = __float_as_uint(a);
    u += 0x7ffffu + ((u >> 20) & 1u);
    return (unsigned char)(sign | ((u >> 20) - (120u << 3)));
}

// decode(code) / 256; the two NaN codes (0x7f, 0xff) are never stored and read back as NaN
__device__ inline float f8_decode_unscaled(unsigned char c) {
    const int e = (c >> 3) & 15, m = c & 7;
    float v = e == 0 ? (float)m * 0x1p-17f : ldexpf((float)(8 + m), e - 18);
    if ((c & 0x7f) == 0x7f) v = __builtin_nanf("");
    return (c & 0x80) ? -v : v;
}

}  // namespace mmrag_impl
