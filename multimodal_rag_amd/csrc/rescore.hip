// Exact re-scoring of candidate lists for FP8 collections (gfx950): the FP8 scan plane over-fetches C candidates per
// query, this kernel scores them against the full-precision plane and keeps the best k.
//
// One launch, one 512-thread workgroup per query.  The 8 waves take the candidates round-robin; a wave computes one
// float32 dot product with the same function as rows_dot_kernel (lexical.hip), row_dot.h's wave_row_dot -- lane j
// accumulates columns j, j + 64, ... with fmaf, then the xor-shuffle tree 32 .. 1 -- so a rescored score is
// bit-identical to mmrag_rows_dot's for that pair whatever B, C or the candidate's position (a score of -0 is returned as +0: the sort key folds the two zeros).  The
// (score, row) keys are bitonic-sorted in LDS (deep_select.h's sort; C <= 4096, 32 KiB): keys are distinct for distinct rows, so the order
// (score desc, row asc) does not depend on how the candidates were listed.  No atomics on floats, no host sync.
#include "deep_select.h"
#include "row_dot.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int RS_THREADS = 512;
constexpr int RS_MAX_C = MMRAG_MAX_RESCORE_CANDIDATES;

template <typename T>
__global__ __launch_bounds__(RS_THREADS) void rescore_topk_kernel(const T *__restrict__ q, const T *__restrict__ plane,
                                                                  long long ld, int d,
                                                                  const long long *__restrict__ cand, int C, int k,
                                                                  float *__restrict__ out_s,
                                                                  long long *__restrict__ out_r) {
    __shared__ unsigned long long keys[RS_MAX_C];
    __shared__ int sh_len;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    cand += (size_t)b * C;
    if (tid == 0) sh_len = C;
    __syncthreads();
    // a negative row ends the list: everything from the first one on is ignored
    int first = C;
    for (int c = tid; c < C; c += RS_THREADS)
        if (cand[c] < 0 && c < first) first = c;
    if (first < C) atomicMin(&sh_len, first);
    __syncthreads();
    const int len = sh_len;
    unsigned P = 1;
    while (P < (unsigned)C) P <<= 1;

    const T *a = q + (size_t)b * ld;
    for (int c = wave; c < len; c += RS_THREADS / 64) {
        const long long row = cand[c];
        const T *v = plane + (size_t)row * ld;
        const float s = wave_row_dot(a, v, d, lane);
        if (lane == 0) keys[c] = deep_key(s, (int)row);
    }
    for (unsigned i = (unsigned)len + tid; i < P; i += RS_THREADS) keys[i] = 0ull;   // below every real key
    __syncthreads();
    lds_bitonic_sort_desc<RS_THREADS>(keys, P, tid);
    out_s += (size_t)b * k;
    out_r += (size_t)b * k;
    for (int i = tid; i < k; i += RS_THREADS) {
        if (i < len) {
            const unsigned long long key = keys[i];
            out_s[i] = deep_key_score(key);
            out_r[i] = (long long)(int)~(unsigned)key;
        } else {
            out_s[i] = NEG_INF;
            out_r[i] = -1;
        }
    }
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

int mmrag_rescore_topk(const void *q, const void *plane, int64_t ld, int dtype, int d, const int64_t *cand_rows, int B,
                       int C, int k, float *out_scores, int64_t *out_rows, void *stream) {
    MMRAG_CHECK_ARG(dtype >= 0 && dtype <= 2, "rescore_topk: the plane must be float32, float16 or bfloat16 (dtype %d)",
                    dtype);
    MMRAG_CHECK_ARG(B > 0, "rescore_topk: B must be positive (got %d)", B);
    MMRAG_CHECK_ARG(C >= 1 && C <= RS_MAX_C, "rescore_topk: C=%d outside 1..%d", C, RS_MAX_C);
    MMRAG_CHECK_ARG(k >= 1 && k <= C, "rescore_topk: k=%d outside 1..C=%d", k, C);
    MMRAG_CHECK_ARG(d > 0 && ld >= d, "rescore_topk: need 0 < d <= ld (d=%d ld=%lld)", d, (long long)ld);
    MMRAG_CHECK_ARG(q && plane && cand_rows && out_scores && out_rows, "rescore_topk: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long long *cand = (const long long *)cand_rows;
    long long *orr = (long long *)out_rows;
    with_elem_type(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)::value>;
        rescore_topk_kernel<T><<<B, RS_THREADS, 0, s>>>((const T *)q, (const T *)plane, ld, d, cand, C, k, out_scores,
                                                        orr);
    });
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // extern "C"
