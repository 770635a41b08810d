// Late-interaction scoring (ColBERT's MaxSim) of (query, passage) pairs over per-token unit rows
// (include/mmrag.h mmrag_maxsim_scores).
//
// One workgroup per pair.  The query's tokens (at most 128) are the A tile of pair_tile.h's body, the passage is walked
// in 128-token B tiles; the ring runs over ALL (passage tile, K-slab) items without draining between passage tiles and
// the query's slabs are fetched again for each passage tile (L2), as the k-means assign step does with its row tile.
// Buffer descriptors are built per SEQUENCE: rows past a sequence's last token read as zero, whatever follows them
// in the buffer.
//
// Epilogue.  After a passage tile's last slab every lane folds its 64 accumulators into a running (best, arg) for its
// 16 query rows: columns ascend with the passage tile and inside the lane and only a strictly greater score replaces,
// so the lowest index wins a tie.  Columns j >= d_len are set to -inf by INDEX first: a zero row is not "no token", and
// a query token whose similarities are all negative must not match padding.  After the last passage tile the 16 lanes
// that share rows are folded by an xor butterfly, the two waves that share rows through LDS, both with "greater score,
// else lower index".  Threads i < q_len store row i's (best, arg); thread 0 then adds the q_len maxima in ascending i.
// Query rows i >= q_len are computed (they are zero rows) and dropped: never written, never summed.
#include <math.h>

#include "f8_codec.h"
#include "pair_tile.h"

namespace mmrag_impl {

struct MaxSimParams {
    const char *q_tok, *d_tok;
    unsigned q_rb, d_rb;            // row pitch in bytes
    long long q_rows, d_rows;       // rows the two buffers hold
    int nk;                         // K-slabs that hold the dim columns
    const int *q_start, *q_len, *d_start, *d_len;
    int n_q, n_d;                   // entries of the two sequence tables
    const int *pair_q, *pair_d;
    float *out_sum, *out_best_sim;
    int *out_best_idx;
};

// (v, i) <- the better of (v, i) and (ov, oi): the greater score, else the lower index
__device__ inline void ms_better(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

// DT: MMRAG_F16 (unit rows) or MMRAG_F8E4M3 (code rows of both sides: the accumulators hold 2^16 times the similarity,
// maxima are compared there and scaled, exactly, where they leave for `best` and the outputs)
template <int DT>
__global__ __launch_bounds__(256, 2) void maxsim_kernel(const MaxSimParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(PT == MMRAG_MAX_LATE_QUERY_TOKENS, "the query is one A tile");
    static_assert(PT_LDS + 2 * PT * 8 + PT * 4 <= 80 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    __shared__ float red_v[2][PT];
    __shared__ int red_a[2][PT];
    __shared__ float best[PT];

    const int pair = blockIdx.x;
    const float NEG_INF = -__builtin_inff();
    // every thread reads the same table entries: the checks below are uniform over the workgroup
    const int pq = p.pair_q[pair], pd = p.pair_d[pair];
    bool ok = pq >= 0 && pq < p.n_q && pd >= 0 && pd < p.n_d;
    int qs = 0, ql = 0, ds = 0, dl = 0;
    if (ok) {
        qs = p.q_start[pq], ql = p.q_len[pq], ds = p.d_start[pd], dl = p.d_len[pd];
        ok = ql >= 1 && ql <= MMRAG_MAX_LATE_QUERY_TOKENS && dl >= 1 && dl <= MMRAG_MAX_LATE_DOC_TOKENS && qs >= 0 &&
             ds >= 0 && (long long)qs + ql <= p.q_rows && (long long)ds + dl <= p.d_rows;
    }
    if (!ok) {
        if (threadIdx.x == 0) p.out_sum[pair] = __builtin_nanf("");
        return;
    }

    const int wave_id = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const PairTileCtx c = pair_tile_ctx(threadIdx.x, wave_id < 2 ? p.q_rb : p.d_rb, smem);
    const int wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;
    const int nct = (dl + PT - 1) / PT;
    const PairTileSrc q_src = {p.q_tok + (size_t)qs * p.q_rb, (unsigned)ql * p.q_rb};
    const char *const d_base = p.d_tok + (size_t)ds * p.d_rb;

    // running best of this lane's query rows wm * 64 + 16 a + 4 g4 + r over the passage columns it has seen
    float bv[4][4];
    int ba[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            bv[a][r] = NEG_INF;
            ba[a][r] = 0;
        }

    pair_tile_ring<DT>(
        c, smem, p.nk, nct,
        [&](int ct) {      // (the query tile, passage tile ct): the B side is the one that moves
            const int d_left = dl - ct * PT;
            const PairTileSrc d_src = {d_base + (size_t)ct * PT * p.d_rb, (unsigned)(d_left < PT ? d_left : PT) * p.d_rb};
            return wave < 2 ? q_src : d_src;
        },
        [&](int ct, const f32x4_t (&acc)[4][4]) {
            // ---- acc[a][b][r] = <query row wm*64 + 16a + 4 g4 + r, passage token ct * 128 + wn*64 + 16b + c16>
            const int col0 = ct * PT + wn * 64 + c16;
            const bool ragged = (ct + 1) * PT > dl;     // uniform: only the last passage tile can hold columns >= d_len
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int col = col0 + 16 * b;
                const bool pad = ragged && col >= dl;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = pad ? NEG_INF : acc[a][b][r];
                        if (v > bv[a][r]) {
                            bv[a][r] = v;
                            ba[a][r] = col;
                        }
                    }
            }
        });
    // one ring per workgroup: the barrier below is the fold's, the ring needs none

    // ---- fold the 16 lanes that hold other columns of the same rows, then the two waves wn = 0, 1
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {
                const float ov = __shfl_xor(bv[a][r], m);
                const int oa = __shfl_xor(ba[a][r], m);
                ms_better(bv[a][r], ba[a][r], ov, oa);
            }
            if (c16 == 0) {
                red_v[wn][wm * 64 + 16 * a + 4 * g4 + r] = bv[a][r];
                red_a[wn][wm * 64 + 16 * a + 4 * g4 + r] = ba[a][r];
            }
        }
    __syncthreads();
    if ((int)threadIdx.x < ql) {
        const int t = threadIdx.x;
        float v = red_v[0][t];
        int arg = red_a[0][t];
        ms_better(v, arg, red_v[1][t], red_a[1][t]);
        if constexpr (DT == MMRAG_F8E4M3) v *= PT_ACC_SCALE<DT>;
        best[t] = v;
        if (p.out_best_sim != nullptr) p.out_best_sim[(size_t)pair * PT + t] = v;
        if (p.out_best_idx != nullptr) p.out_best_idx[(size_t)pair * PT + t] = arg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.0f;
        for (int i = 0; i < ql; ++i) sum += best[i];    // ascending i: the sum's bits are defined
        p.out_sum[pair] = sum;
    }
#endif
}

}  // namespace mmrag_impl

namespace mmrag_impl {

// csrc/f8_codec.h's encoder over rows: dst[r, c] = code of src[r, c] for c < d, code 0 for d <= c < dst_ld
template <typename T>
__global__ __launch_bounds__(256) void f8_encode_rows_kernel(const T *__restrict__ src, int64_t src_ld,
                                                             unsigned char *__restrict__ dst, int64_t dst_ld,
                                                             int64_t m, int d) {
    const int64_t per_row = dst_ld / 4, total = m * per_row;      // four codes (one 32-bit store) per thread and step
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        const int c0 = (int)(i - r * per_row) * 4;
        unsigned w = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c0 + e < d) w |= (unsigned)f8_encode((float)src[r * src_ld + c0 + e]) << (8 * e);
        *(unsigned *)(dst + r * dst_ld + c0) = w;
    }
}

template <int DT>
static int maxsim_scores_impl(const char *who, const void *q_tok, int64_t q_rows, int64_t q_ld, const void *d_tok,
                              int64_t d_rows, int64_t d_ld, int dim, const int32_t *q_start, const int32_t *q_len,
                              int n_q, const int32_t *d_start, const int32_t *d_len, int n_d, const int32_t *pair_q,
                              const int32_t *pair_d, int P, float *out_sum, float *out_best_sim,
                              int32_t *out_best_idx, void *stream) {
    MMRAG_CHECK_ARG(q_tok && d_tok && q_start && q_len && d_start && d_len && pair_q && pair_d && out_sum,
                    "%s: null pointer", who);
    MMRAG_CHECK_ARG(dim > 0 && dim % 64 == 0 && dim <= 1024,
                    "%s: dim must be a multiple of 64, at most 1024 (dim=%d)", who, dim);
    for (const int64_t ld : {q_ld, d_ld}) {
        const int st = DT == MMRAG_F8E4M3 ? check_code_rows(who, ld, dim)
                                          : check_stored_rows(who, "scored", "score", ld, DT, dim);
        if (st != MMRAG_OK) return st;
    }
    MMRAG_CHECK_ARG(P >= 1 && P <= 65535, "%s: P=%d outside 1..65535", who, P);
    MMRAG_CHECK_ARG(n_q >= 1 && n_d >= 1 && q_rows >= 1 && d_rows >= 1 && q_rows < (1LL << 31) && d_rows < (1LL << 31),
                    "%s: need at least one sequence and one row on each side, fewer than 2^31 rows "
                    "(n_q=%d n_d=%d q_rows=%lld d_rows=%lld)", who, n_q, n_d, (long long)q_rows, (long long)d_rows);
    MMRAG_CHECK_ARG(((uintptr_t)q_tok % 16) == 0 && ((uintptr_t)d_tok % 16) == 0,
                    "%s: token rows must be 16-byte aligned", who);
    MaxSimParams p;
    p.q_tok = (const char *)q_tok, p.d_tok = (const char *)d_tok;
    p.q_rb = stored_row_bytes(q_ld, DT), p.d_rb = stored_row_bytes(d_ld, DT);
    p.q_rows = q_rows, p.d_rows = d_rows;
    p.nk = stored_k_slabs(dim, DT);
    p.q_start = q_start, p.q_len = q_len, p.d_start = d_start, p.d_len = d_len;
    p.n_q = n_q, p.n_d = n_d;
    p.pair_q = pair_q, p.pair_d = pair_d;
    p.out_sum = out_sum, p.out_best_sim = out_best_sim, p.out_best_idx = out_best_idx;
    hipLaunchKernelGGL(maxsim_kernel<DT>, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // namespace mmrag_impl

extern "C" {

int mmrag_maxsim_scores(const void *q_tok, int64_t q_rows, int64_t q_ld, const void *d_tok, int64_t d_rows,
                        int64_t d_ld, int dim, const int32_t *q_start, const int32_t *q_len, int n_q,
                        const int32_t *d_start, const int32_t *d_len, int n_d, const int32_t *pair_q,
                        const int32_t *pair_d, int P, float *out_sum, float *out_best_sim, int32_t *out_best_idx,
                        void *stream) {
    return mmrag_impl::maxsim_scores_impl<MMRAG_F16>("maxsim_scores", q_tok, q_rows, q_ld, d_tok, d_rows, d_ld, dim,
                                                     q_start, q_len, n_q, d_start, d_len, n_d, pair_q, pair_d, P,
                                                     out_sum, out_best_sim, out_best_idx, stream);
}

int mmrag_maxsim_scores_f8(const void *q_codes, int64_t q_rows, int64_t q_ld, const void *d_codes, int64_t d_rows,
                           int64_t d_ld, int dim, const int32_t *q_start, const int32_t *q_len, int n_q,
                           const int32_t *d_start, const int32_t *d_len, int n_d, const int32_t *pair_q,
                           const int32_t *pair_d, int P, float *out_sum, float *out_best_sim, int32_t *out_best_idx,
                           void *stream) {
    return mmrag_impl::maxsim_scores_impl<MMRAG_F8E4M3>("maxsim_scores_f8", q_codes, q_rows, q_ld, d_codes, d_rows,
                                                        d_ld, dim, q_start, q_len, n_q, d_start, d_len, n_d, pair_q,
                                                        pair_d, P, out_sum, out_best_sim, out_best_idx, stream);
}

int mmrag_f8_encode_rows(const void *src, int src_dtype, int64_t m, int d, int64_t src_ld, void *dst, int64_t dst_ld,
                         void *stream) {
    using namespace mmrag_impl;
    MMRAG_CHECK_ARG(src && dst, "f8_encode_rows: null pointer");
    MMRAG_CHECK_ARG(src_dtype == MMRAG_F16 || src_dtype == MMRAG_F32,
                    "f8_encode_rows: the source must be MMRAG_F16 or MMRAG_F32 (src_dtype=%d)", src_dtype);
    MMRAG_CHECK_ARG(m >= 0 && d > 0 && src_ld >= d && dst_ld >= d,
                    "f8_encode_rows: need m >= 0 and 0 < d <= src_ld, dst_ld (m=%lld d=%d src_ld=%lld dst_ld=%lld)",
                    (long long)m, d, (long long)src_ld, (long long)dst_ld);
    if (int st = check_code_rows("f8_encode_rows", dst_ld, d)) return st;
    MMRAG_CHECK_ARG(((uintptr_t)dst % 16) == 0, "f8_encode_rows: dst must be 16-byte aligned");
    if (m == 0) return MMRAG_OK;
    const int64_t total = m * (dst_ld / 4);
    int64_t grid = (total + 255) / 256;
    const int64_t most = (int64_t)mmrag::num_cus() * 8;
    grid = grid > most ? most : grid;
    hipStream_t s = (hipStream_t)stream;
    if (src_dtype == MMRAG_F16)
        hipLaunchKernelGGL(f8_encode_rows_kernel<_Float16>, dim3((unsigned)grid), dim3(256), 0, s,
                           (const _Float16 *)src, src_ld, (unsigned char *)dst, dst_ld, m, d);
    else
        hipLaunchKernelGGL(f8_encode_rows_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, (const float *)src,
                           src_ld, (unsigned char *)dst, dst_ld, m, d);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // extern "C"
