// Maximal-marginal-relevance selection on gfx950: the device half of VectorIndex.mmr_search.
//
// One workgroup of 1024 threads (16 waves) per query.  The query's C candidates (the dense hits, best first) keep their
// relevance `rel`, their running `maxsim` against the picked set, their rows and a `taken` flag in LDS.  Step 0 picks
// candidate 0; every later step
//   1. takes the row of the last pick from LDS (the staged rows, or a copy made for this step),
//   2. gives every wave the free candidates i = wave, wave + 16, ...: 16-byte loads of both rows, a float32 fmaf chain
//      per lane, a butterfly reduction over the wave, maxsim[i] = max(maxsim[i], sim), v_i = lam * rel_i - (1 - lam) *
//      maxsim[i], and the wave's running best (v descending, position ascending),
//   3. exchanges the 16 waves' bests through LDS (one barrier); every thread then knows the pick.
// No atomics on global memory, no float atomics, no host synchronisation: the call can be captured into a graph.
//
// Two forms of the same arithmetic.  STAGED: the candidate rows are gathered into LDS once (C * row bytes <= 128 KiB:
// 50 x 768 fp16 is 75 KiB) and all k steps run from there.  Streamed: the candidate rows are re-read from global memory
// (L2) at every step and only the picked row is copied to LDS (rows up to 16 KiB; longer ones are read in place).
//
// sim(i, j) is summed in one fixed order whatever B, C, k, the grid or the form: the row is cut into 16-byte chunks,
// lane l of the wave adds the elements of chunks l, l + 64, ... in ascending order into one float32 accumulator with
// fmaf, and the 64 accumulators are added by the xor butterfly 32, 16, 8, 4, 2, 1.
#include "mmrag_internal.h"

#include <limits.h>
#include <math.h>

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int MMR_THREADS = 1024;   // 16 waves, 4 per SIMD: a step is a chain of LDS round trips, more waves hide them
constexpr int MMR_WAVES = MMR_THREADS / 64;
constexpr int MMR_MAX_C = MMRAG_MAX_MMR_CANDIDATES;
constexpr int MMR_STAGE_BYTES = 128 * 1024;   // staged candidate rows (one workgroup per CU at this size)
constexpr int MMR_PROW_BYTES = 16 * 1024;     // streamed form: the picked row's copy
constexpr float MMR_NEG_INF = -__builtin_inff();

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// s += a . b over one 16-byte chunk, elements in ascending order; MASK: only the first `valid` elements
template <int DT, bool MASK>
__device__ __forceinline__ float chunk_fma(const uint4 a, const uint4 b, float s, int valid) {
    if (DT == MMRAG_F32) {
        const float af[4] = {__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w)};
        const float bf[4] = {__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w)};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool on = !MASK || t < valid;
            s = fmaf(on ? af[t] : 0.0f, on ? bf[t] : 0.0f, s);
        }
    } else if (DT == MMRAG_F16) {
        const half8 ah = __builtin_bit_cast(half8, a), bh = __builtin_bit_cast(half8, b);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const bool on = !MASK || t < valid;
            s = fmaf(on ? (float)ah[t] : 0.0f, on ? (float)bh[t] : 0.0f, s);
        }
    } else {
        const unsigned aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int t = 0; t < 8; ++t) {   // bf16 -> float32: the 16 bits are the float's upper half
            const bool on = !MASK || t < valid;
            const float x = __uint_as_float((t & 1) ? (aw[t >> 1] & 0xffff0000u) : (aw[t >> 1] << 16));
            const float y = __uint_as_float((t & 1) ? (bw[t >> 1] & 0xffff0000u) : (bw[t >> 1] << 16));
            s = fmaf(on ? x : 0.0f, on ? y : 0.0f, s);
        }
    }
    return s;
}

// the whole wave: <a, b> over nfull whole chunks and `tail` elements of chunk nfull; every lane gets the sum
template <int DT>
__device__ __forceinline__ float wave_dot(const uint4 *a, const uint4 *b, int nfull, int tail, int lane) {
    float s = 0.0f;
    for (int j = lane; j < nfull; j += 64) s = chunk_fma<DT, false>(a[j], b[j], s, 0);
    if (tail && lane == (nfull & 63)) s = chunk_fma<DT, true>(a[nfull], b[nfull], s, tail);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

struct MmrParams {
    const char *corpus;
    long long row_bytes;     // ld * element size, a multiple of 16
    int d;
    const float *cand_s;     // [B, C]
    const long long *cand_r;
    int C, k;
    float lam, oml;          // lambda and 1 - lambda (float32)
    float *out_s;            // [B, k]
    long long *out_r;
    int *out_p;
    float *out_v;
};

template <int DT, bool STAGED>
__global__ __launch_bounds__(MMR_THREADS) void mmr_select_kernel(const MmrParams p) {
    __shared__ uint4 stage[(STAGED ? MMR_STAGE_BYTES : MMR_PROW_BYTES) / 16];
    __shared__ float rel[MMR_MAX_C], maxsim[MMR_MAX_C];
    __shared__ long long rows[MMR_MAX_C];
    __shared__ int taken[MMR_MAX_C];
    __shared__ float wave_v[2][MMR_WAVES];
    __shared__ int wave_i[2][MMR_WAVES];
    __shared__ int n_valid;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t q = blockIdx.x;
    const int C = p.C, k = p.k;
    constexpr int EPC = DT == MMRAG_F32 ? 4 : 8;   // elements per 16-byte chunk
    const int nfull = p.d / EPC, tail = p.d % EPC, nch = nfull + (tail ? 1 : 0);

    if (tid == 0) n_valid = C;
    __syncthreads();
    for (int i = tid; i < C; i += MMR_THREADS) {
        const long long r = p.cand_r[q * C + i];
        rows[i] = r;
        rel[i] = p.cand_s[q * C + i];
        maxsim[i] = MMR_NEG_INF;
        taken[i] = 0;
        if (r < 0) atomicMin(&n_valid, i);   // LDS: the list ends at its first -1
    }
    __syncthreads();
    const int cnt = n_valid;
    const int nk = k < cnt ? k : cnt;
    for (int t = nk + tid; t < k; t += MMR_THREADS) {
        p.out_s[q * k + t] = MMR_NEG_INF;
        p.out_r[q * k + t] = -1;
        p.out_p[q * k + t] = -1;
        p.out_v[q * k + t] = MMR_NEG_INF;
    }
    if (nk == 0) return;

    if (STAGED) {   // gather the candidate rows into LDS: chunk f of the gathered block is stage[f]
        const int total = cnt * nch;
        for (int f = tid; f < total; f += MMR_THREADS) {
            const int r = f / nch, j = f - r * nch;
            stage[f] = ((const uint4 *)(p.corpus + (size_t)rows[r] * p.row_bytes))[j];
        }
        __syncthreads();
    }
    const bool prow_in_lds = STAGED || nch * 16 <= MMR_PROW_BYTES;

    int win = 0;
    float win_v = rel[0];
    for (int t = 0;; ++t) {
        if (tid == 0) {
            p.out_s[q * k + t] = rel[win];
            p.out_r[q * k + t] = rows[win];
            p.out_p[q * k + t] = win;
            p.out_v[q * k + t] = win_v;
        }
        if (t == nk - 1) break;
        if ((win & (MMR_WAVES - 1)) == w && lane == 0) taken[win] = 1;   // read by this wave only
        const uint4 *grow = (const uint4 *)(p.corpus + (size_t)rows[win] * p.row_bytes);
        if (!STAGED && prow_in_lds) {
            // (every wave left its dot products of the previous step before that step's barrier)
            for (int j = tid; j < nch; j += MMR_THREADS) stage[j] = grow[j];
            __syncthreads();
        }
        float best_v = MMR_NEG_INF;
        int best_i = INT_MAX;
        for (int i = w; i < cnt; i += MMR_WAVES) {
            if (taken[i]) continue;
            float s;
            if (STAGED)
                s = wave_dot<DT>(stage + (size_t)i * nch, stage + (size_t)win * nch, nfull, tail, lane);
            else if (prow_in_lds)
                s = wave_dot<DT>((const uint4 *)(p.corpus + (size_t)rows[i] * p.row_bytes), stage, nfull, tail, lane);
            else
                s = wave_dot<DT>((const uint4 *)(p.corpus + (size_t)rows[i] * p.row_bytes), grow, nfull, tail, lane);
            const float ms = fmaxf(maxsim[i], s);
            if (lane == 0) maxsim[i] = ms;
            const float v = __fmul_rn(p.lam, rel[i]) - __fmul_rn(p.oml, ms);
            if (best_i == INT_MAX || v > best_v) {   // i ascends: a tie keeps the lower position
                best_v = v;
                best_i = i;
            }
        }
        if (lane == 0) {
            wave_v[t & 1][w] = best_v;
            wave_i[t & 1][w] = best_i;
        }
        __syncthreads();
        win = INT_MAX;
        win_v = MMR_NEG_INF;
#pragma unroll
        for (int j = 0; j < MMR_WAVES; ++j) {
            const float v = wave_v[t & 1][j];
            const int i = wave_i[t & 1][j];
            if (i != INT_MAX && (win == INT_MAX || v > win_v || (v == win_v && i < win))) {
                win = i;
                win_v = v;
            }
        }
        if (win == INT_MAX) {   // not reachable with nk <= cnt: pad what is left rather than index with it
            for (int u = t + 1 + tid; u < k; u += MMR_THREADS) {
                p.out_s[q * k + u] = MMR_NEG_INF;
                p.out_r[q * k + u] = -1;
                p.out_p[q * k + u] = -1;
                p.out_v[q * k + u] = MMR_NEG_INF;
            }
            return;
        }
    }
}

template <int DT>
void mmr_launch(const MmrParams &p, int B, bool staged, hipStream_t s) {
    if (staged)
        mmr_select_kernel<DT, true><<<B, MMR_THREADS, 0, s>>>(p);
    else
        mmr_select_kernel<DT, false><<<B, MMR_THREADS, 0, s>>>(p);
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

// debug form of mmrag_mmr_select (tests and tools/mmr_bench.py; not in include/mmrag.h): dbg & 1 = the streamed form
// also where the staged one fits
int mmrag_internal_mmr_select_ex(const void *corpus, int64_t ld, int dtype, int d, const float *cand_scores,
                                 const int64_t *cand_rows, int B, int C, int k, float lambda, float *out_scores,
                                 int64_t *out_rows, int32_t *out_pos, float *out_mmr, void *workspace,
                                 size_t workspace_bytes, void *stream, unsigned dbg) {
    (void)workspace;
    (void)workspace_bytes;
    MMRAG_CHECK_ARG(dtype >= 0 && dtype <= 2, "mmr_select: bad dtype %d", dtype);
    MMRAG_CHECK_ARG(C >= 1 && C <= MMRAG_MAX_MMR_CANDIDATES && k >= 1 && k <= C,
                    "mmr_select: need 1 <= k <= C <= %d (got k=%d C=%d)", MMRAG_MAX_MMR_CANDIDATES, k, C);
    MMRAG_CHECK_ARG(lambda >= 0.0f && lambda <= 1.0f, "mmr_select: lambda=%g outside [0, 1]", (double)lambda);
    MMRAG_CHECK_ARG(B > 0, "mmr_select: B must be positive (got %d)", B);
    MMRAG_CHECK_ARG(d > 0 && ld >= d && (ld * esize(dtype)) % 16 == 0,
                    "mmr_select: bad shape d=%d ld=%lld (rows must be a multiple of 16 bytes)", d, (long long)ld);
    MMRAG_CHECK_ARG(corpus && cand_scores && cand_rows && out_scores && out_rows && out_pos && out_mmr,
                    "mmr_select: null pointer");
    MMRAG_CHECK_ARG(((uintptr_t)corpus % 16) == 0, "mmr_select: corpus must be 16-byte aligned");
    MmrParams p;
    p.corpus = (const char *)corpus;
    p.row_bytes = (long long)ld * esize(dtype);
    p.d = d;
    p.cand_s = cand_scores;
    p.cand_r = (const long long *)cand_rows;
    p.C = C;
    p.k = k;
    p.lam = lambda;
    p.oml = 1.0f - lambda;
    p.out_s = out_scores;
    p.out_r = (long long *)out_rows;
    p.out_p = out_pos;
    p.out_v = out_mmr;
    const long long chunks = ((long long)d * esize(dtype) + 15) / 16;
    const bool staged = !(dbg & 1u) && (long long)C * chunks * 16 <= MMR_STAGE_BYTES;
    hipStream_t s = (hipStream_t)stream;
    with_elem_type(dtype, [&](auto tag) { mmr_launch<decltype(tag)::value>(p, B, staged, s); });
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

size_t mmrag_mmr_select_workspace_bytes(int B, int C, int d, int dtype) {
    (void)B;
    (void)C;
    (void)d;
    (void)dtype;
    return 0;   // everything the selection needs lives in LDS
}

int mmrag_mmr_select(const void *corpus, int64_t ld, int dtype, int d, const float *cand_scores,
                     const int64_t *cand_rows, int B, int C, int k, float lambda, float *out_scores, int64_t *out_rows,
                     int32_t *out_pos, float *out_mmr, void *workspace, size_t workspace_bytes, void *stream) {
    return mmrag_internal_mmr_select_ex(corpus, ld, dtype, d, cand_scores, cand_rows, B, C, k, lambda, out_scores,
                                        out_rows, out_pos, out_mmr, workspace, workspace_bytes, stream, 0u);
}

}  // extern "C"
