// Span head of the extractive reader (BertForQuestionAnswering's qa_outputs and the answer-span search), for gfx950.
//
// One launch after the last encoder layer, one workgroup of 4 waves per packed [CLS] question [SEP] passage [SEP]
// sequence (at most 512 tokens):
//   1. logits   ls[t] = <hidden[t], qa_w[0]> + qa_b[0], le[t] = <hidden[t], qa_w[1]> + qa_b[1] for every token, kept in
//               LDS (written to HBM only when the caller passes out_logits).  qa_w is staged in LDS once; lane l of
//               every wave always multiplies the same 16-byte chunks l and l + 64 of a row, so it lifts its slice of
//               qa_w from LDS into registers before the row loop.  A lane's two partial sums run over its elements in
//               ascending k; the 64 lanes are folded by a fixed xor butterfly.  Which rows a wave takes depends on the
//               position inside the sequence only, so a sequence's logits do not depend on its batch.
//   2. lse      log-sum-exp of the start and of the end logits over position 0 and the passage tokens (the mask of
//               Hugging Face's question-answering decode with impossible answers allowed); null = ls[0] + le[0].
//   3. spans    n rounds of a workgroup arg-max over the candidates (i, j), ctx_start <= i <= j < ctx_start + ctx_len,
//               j - i < L, score ls[i] + le[j] (float32) above -inf: higher score, then lower i, then lower j.  A
//               candidate that shares a token with a span taken in an earlier round is not eligible (a per-token mask
//               in LDS: thread i walks j upward and stops at the first taken token).  A round without an eligible
//               candidate writes (-1, -1) and -inf.
// No atomics, no workspace, nothing read by the host: the launch can be captured into a graph, identical calls give
// identical bits.
#include "mmrag_internal.h"

#include <limits.h>
#include <math.h>

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int SPAN_T = MMRAG_MAX_READER_TOKENS;   // tokens of a sequence
constexpr int SPAN_ROWS = 4;                      // rows a wave loads before it multiplies them
constexpr int SPAN_NONE = INT_MAX;                // packed (i, j) of "no candidate"

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

struct SpanArgs {
    const _Float16 *hidden;
    int ld, H;
    const float *qa_w, *qa_b;
    const int32_t *cu, *ctx_start, *ctx_len;
    int T, L, n;
    int32_t *out_span;
    float *out_score, *out_null, *out_lse, *out_logits;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// (score, packed i << 16 | j): a before b when its score is higher, then when its packed index is lower
__device__ __forceinline__ bool span_before(float sa, int ia, float sb, int ib) {
    return sa > sb || (sa == sb && ia < ib);
}

__global__ __launch_bounds__(256) void span_select_kernel(SpanArgs p) {
    __shared__ __attribute__((aligned(16))) float w_lds[2 * 1024];
    __shared__ float ls[SPAN_T], le[SPAN_T];
    __shared__ unsigned char taken[SPAN_T];
    __shared__ float red_f[2][4];
    __shared__ int red_i[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s0 = p.cu[b], s1 = p.cu[b + 1];
    const int cs = p.ctx_start[b], cl = p.ctx_len[b];
    const long long len = (long long)s1 - s0;
    const bool ok = s0 >= 0 && s1 <= p.T && len >= 1 && len <= SPAN_T && cl >= 0 && cs >= 1 && (long long)cs + cl <= len;
    if (!ok) {   // nothing of the sequence is read
        if (tid < p.n) {
            p.out_span[((size_t)b * p.n + tid) * 2] = -1, p.out_span[((size_t)b * p.n + tid) * 2 + 1] = -1;
            p.out_score[(size_t)b * p.n + tid] = -INFINITY;
        }
        if (tid == 0) p.out_null[b] = p.out_lse[2 * b] = p.out_lse[2 * b + 1] = __builtin_nanf("");
        return;
    }
    const int n_tok = (int)len, H = p.H, nch = H >> 3;   // 16-byte chunks of a row: 8 .. 128

    // ---- 1. logits
    for (int i = tid; i < 2 * H; i += 256) w_lds[(i / H) * 1024 + i % H] = p.qa_w[i];
    for (int i = tid; i < SPAN_T; i += 256) taken[i] = 0;
    __syncthreads();
    const bool has0 = lane < nch, has1 = lane + 64 < nch;
    float w0[2][8], w1[2][8];   // [chunk of the lane][k]: its slice of the start row and of the end row
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const bool has = c == 0 ? has0 : has1;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            w0[c][k] = has ? w_lds[(lane + 64 * c) * 8 + k] : 0.f;
            w1[c][k] = has ? w_lds[1024 + (lane + 64 * c) * 8 + k] : 0.f;
        }
    }
    const float b0 = p.qa_b[0], b1 = p.qa_b[1];
    for (int base = wave * SPAN_ROWS; base < n_tok; base += 4 * SPAN_ROWS) {
        uint4 x[SPAN_ROWS][2];
#pragma unroll
        for (int r = 0; r < SPAN_ROWS; ++r) {
            x[r][0] = x[r][1] = uint4{0u, 0u, 0u, 0u};
            if (base + r < n_tok) {
                const uint4 *row = (const uint4 *)(p.hidden + (size_t)(s0 + base + r) * p.ld);
                if (has0) x[r][0] = row[lane];
                if (has1) x[r][1] = row[lane + 64];
            }
        }
#pragma unroll
        for (int r = 0; r < SPAN_ROWS; ++r) {
            if (base + r >= n_tok) break;   // wave-uniform
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const half8_t h = __builtin_bit_cast(half8_t, x[r][c]);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    a0 = fmaf((float)h[k], w0[c][k], a0);
                    a1 = fmaf((float)h[k], w1[c][k], a1);
                }
            }
            a0 = wave_sum(a0) + b0, a1 = wave_sum(a1) + b1;
            if (lane == 0) {
                ls[base + r] = a0, le[base + r] = a1;
                if (p.out_logits != nullptr) {
                    p.out_logits[(size_t)(s0 + base + r) * 2] = a0;
                    p.out_logits[(size_t)(s0 + base + r) * 2 + 1] = a1;
                }
            }
        }
    }
    __syncthreads();

    // ---- 2. normalisers over position 0 and the passage tokens: slot 0 = [CLS], slot q >= 1 = token cs + q - 1
    {
        float v0[2], v1[2], m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int q = tid + 256 * u, t = q == 0 ? 0 : cs + q - 1;
            const bool in = q <= cl;
            v0[u] = in ? ls[t] : -INFINITY, v1[u] = in ? le[t] : -INFINITY;
            m0 = fmaxf(m0, v0[u]), m1 = fmaxf(m1, v1[u]);
        }
        // q runs to cl <= 511 < 512 slots: two per thread cover it
        m0 = wave_max(m0), m1 = wave_max(m1);
        if (lane == 0) red_f[0][wave] = m0, red_f[1][wave] = m1;
        __syncthreads();
        m0 = fmaxf(fmaxf(red_f[0][0], red_f[0][1]), fmaxf(red_f[0][2], red_f[0][3]));
        m1 = fmaxf(fmaxf(red_f[1][0], red_f[1][1]), fmaxf(red_f[1][2], red_f[1][3]));
        __syncthreads();
        float e0 = 0.f, e1 = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (tid + 256 * u <= cl) e0 += expf(v0[u] - m0), e1 += expf(v1[u] - m1);
        }
        e0 = wave_sum(e0), e1 = wave_sum(e1);
        if (lane == 0) red_f[0][wave] = e0, red_f[1][wave] = e1;
        __syncthreads();
        if (tid == 0) {
            e0 = ((red_f[0][0] + red_f[0][1]) + red_f[0][2]) + red_f[0][3];
            e1 = ((red_f[1][0] + red_f[1][1]) + red_f[1][2]) + red_f[1][3];
            p.out_lse[2 * b] = m0 + logf(e0), p.out_lse[2 * b + 1] = m1 + logf(e1);
            p.out_null[b] = ls[0] + le[0];
        }
        __syncthreads();
    }

    // ---- 3. span search
    const int c_end = cs + cl;
    for (int round = 0; round < p.n; ++round) {
        float best = -INFINITY;
        int at = SPAN_NONE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = cs + tid + 256 * u;
            if (i >= c_end) continue;
            const int j_end = i + p.L < c_end ? i + p.L : c_end;
            const float si = ls[i];
            for (int j = i; j < j_end; ++j) {   // ascending (i, j) with a strict >: the first of equal scores stays
                if (taken[j]) break;
                const float s = si + le[j];
                if (s > best) best = s, at = (i << 16) | j;
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float so = __shfl_xor(best, m, 64);
            const int io = __shfl_xor(at, m, 64);
            if (span_before(so, io, best, at)) best = so, at = io;
        }
        if (lane == 0) red_f[0][wave] = best, red_i[wave] = at;
        __syncthreads();
        best = red_f[0][0], at = red_i[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            if (span_before(red_f[0][w], red_i[w], best, at)) best = red_f[0][w], at = red_i[w];
        }
        const bool found = at != SPAN_NONE;
        const int bi = found ? at >> 16 : -1, bj = found ? at & 0xffff : -1;
        if (tid == 0) {
            p.out_span[((size_t)b * p.n + round) * 2] = bi, p.out_span[((size_t)b * p.n + round) * 2 + 1] = bj;
            p.out_score[(size_t)b * p.n + round] = found ? best : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tid + 256 * u;
            if (found && t >= bi && t <= bj) taken[t] = 1;
        }
        __syncthreads();
    }
}

}  // namespace

int launch_span_select(const void *hidden, int ld, int H, const float *qa_w, const float *qa_b, const int32_t *cu_seqlens,
                       const int32_t *ctx_start, const int32_t *ctx_len, int64_t T, int B, int max_answer_tokens,
                       int n_best, int32_t *out_span, float *out_score, float *out_null, float *out_lse,
                       float *out_logits, hipStream_t s) {
    MMRAG_CHECK_ARG(hidden && qa_w && qa_b && cu_seqlens && ctx_start && ctx_len && out_span && out_score && out_null &&
                        out_lse, "span_select: null pointer");
    MMRAG_CHECK_ARG(T > 0 && T < INT_MAX && B > 0, "span_select: bad shape T=%lld B=%d", (long long)T, B);
    MMRAG_CHECK_ARG(H >= 64 && H % 64 == 0 && H <= 1024, "span_select: hidden must be a multiple of 64, at most 1024 "
                    "(hidden=%d)", H);
    MMRAG_CHECK_ARG(ld >= H && ld % 8 == 0, "span_select: ld must be a multiple of 8, at least hidden (ld=%d)", ld);
    MMRAG_CHECK_ARG(max_answer_tokens >= 1 && max_answer_tokens <= MMRAG_MAX_ANSWER_TOKENS,
                    "span_select: max_answer_tokens = %d (1..%d)", max_answer_tokens, MMRAG_MAX_ANSWER_TOKENS);
    MMRAG_CHECK_ARG(n_best >= 1 && n_best <= MMRAG_MAX_READER_SPANS, "span_select: n_best = %d (1..%d)", n_best,
                    MMRAG_MAX_READER_SPANS);
    MMRAG_CHECK_ARG(((uintptr_t)hidden % 16) == 0 && ((uintptr_t)qa_w % 4) == 0, "span_select: hidden must be 16-byte "
                    "aligned");
    SpanArgs p;
    p.hidden = (const _Float16 *)hidden, p.ld = ld, p.H = H, p.qa_w = qa_w, p.qa_b = qa_b;
    p.cu = cu_seqlens, p.ctx_start = ctx_start, p.ctx_len = ctx_len;
    p.T = (int)T, p.L = max_answer_tokens, p.n = n_best;
    p.out_span = out_span, p.out_score = out_score, p.out_null = out_null, p.out_lse = out_lse, p.out_logits = out_logits;
    span_select_kernel<<<(unsigned)B, 256, 0, s>>>(p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // namespace mmrag_impl

extern "C" {

int mmrag_span_select(const void *hidden, int ld, int hidden_dim, const float *qa_w, const float *qa_b,
                      const int32_t *cu_seqlens, const int32_t *ctx_start, const int32_t *ctx_len, int64_t T, int B,
                      int max_answer_tokens, int n_best, int32_t *out_span, float *out_score, float *out_null,
                      float *out_lse, float *out_logits, void *stream) {
    return mmrag_impl::launch_span_select(hidden, ld, hidden_dim, qa_w, qa_b, cu_seqlens, ctx_start, ctx_len, T, B,
                                          max_answer_tokens, n_best, out_span, out_score, out_null, out_lse, out_logits,
                                          (hipStream_t)stream);
}

}  // extern "C"
