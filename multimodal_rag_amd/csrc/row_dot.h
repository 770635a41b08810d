// The float32 dot product of two stored rows by one wave: what mmrag_rows_dot (lexical.hip) returns and what
// mmrag_rescore_topk (rescore.hip) ranks by -- one function, so the two agree bit for bit.  Internal, gfx950 only.
#pragma once
#include "mmrag_internal.h"

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <type_traits>

namespace mmrag_impl {

// the element type of a full-precision storage dtype (the constant with_elem_type hands out)
template <int DT>
using elem_t = std::conditional_t<DT == MMRAG_F32, float, std::conditional_t<DT == MMRAG_F16, __half, __hip_bfloat16>>;

template <typename T>
__device__ inline float elem_to_float(T x) {
    return (float)x;
}
template <>
__device__ inline float elem_to_float<__hip_bfloat16>(__hip_bfloat16 x) {
    return __bfloat162float(x);
}

// sum over j < d of a[j] * c[j]: lane j accumulates columns j, j + 64, ... with fmaf, then the xor butterfly 32 .. 1
// (every lane returns the sum).  The order is fixed, so the result depends on the two rows and d alone.
template <typename T>
__device__ inline float wave_row_dot(const T *a, const T *c, int d, int lane) {
    float s = 0.0f;
    for (int j = lane; j < d; j += 64) s = fmaf(elem_to_float(a[j]), elem_to_float(c[j]), s);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

}  // namespace mmrag_impl
