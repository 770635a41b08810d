// Exact impact scoring of learned sparse vectors over the inverted index (include/mmrag.h mmrag_impact_topk): the
// search half of multimodal_rag_amd/sparse.py.  The index is the CSR mmrag_lexical_csr_build makes of the forward log
// with the 8-bit impact in the place of tf: term t's postings (row, impact) at term_off[t] .. term_off[t + 1), by row.
//
// Scoring follows lexical.hip's bm25_score_kernel: one workgroup per (query, block of IMP_R rows) with an LDS
// accumulator, the block's slice of each query term's postings found by two binary searches, the terms taken one after
// the other with a barrier between them (rows within a term are distinct, so no two lanes add to one slot).  The
// accumulator is int32: a score is at most 255 * 255 * 64 < 2^24, so the sum is exact, does not depend on any order and
// converts to float32 without rounding.
//
// Expansion terms are common: most rows match something, and a query's matches overflow the candidate slots as soon as
// n does.  So the call runs under candidate_select.h's bounded_scan_select (a 2048-row block is 16 of its 128-row
// tiles): with n above the slots, tau_q is first raised to the k-th best score of a strided sample of blocks, the main
// pass appends only scores at or above it, and a query that still overflows is produced again alone into n slots.
// Exact in every regime: a bound from a sample never exceeds the true k-th score.
#include "candidate_select.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int IMP_THREADS = 256;
constexpr int IMP_R = 2048;                              // rows per scoring workgroup (8 KiB LDS accumulator)
constexpr int IMP_TILES = IMP_R / BOUND_TILE_ROWS;       // the driver's tiles per block
constexpr unsigned IMP_DBG_NO_BOUND = 1u;                // no bound stages: every match survives the main pass

struct ImpactParams {
    const long long *term_off;
    const int *post_row, *post_imp;
    int n_terms;
    const int *q_off, *q_terms, *q_imp;
    const uint32_t *alive_bits;
    long long n;
    long long n_blocks, walk;   // this launch visits block i * n_blocks / walk for i in 0 .. walk
    int q_base;                 // query of blockIdx.y = 0
    const float *tau;           // [B] of the whole batch, or null: no bound
    long long cap;
    unsigned *cnt;
    float *cand_s;
    int *cand_r;
};

__device__ inline long long imp_lower_bound(const int *__restrict__ rows, long long lo, long long hi, long long x) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)rows[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(IMP_THREADS) void impact_score_kernel(const ImpactParams p) {
    __shared__ int acc[IMP_R];
    __shared__ long long rlo[MMRAG_MAX_SPARSE_QUERY_TERMS], rhi[MMRAG_MAX_SPARSE_QUERY_TERMS];
    __shared__ int wq[MMRAG_MAX_SPARSE_QUERY_TERMS];
    __shared__ int any;
    const int tid = threadIdx.x, slot = blockIdx.y, q = p.q_base + slot;
    const long long blk = (long long)blockIdx.x * p.n_blocks / p.walk;
    const long long r0 = blk * IMP_R;
    const long long r1 = r0 + IMP_R < p.n ? r0 + IMP_R : p.n;
    const int t0 = p.q_off[q], nt = p.q_off[q + 1] - t0;
    if (t0 < 0 || nt < 1 || nt > MMRAG_MAX_SPARSE_QUERY_TERMS) return;      // uniform: such a query matches nothing
    if (tid == 0) any = 0;
    __syncthreads();
    // the block's slice of each term's postings: two searches per term, one per lane
    for (int i = tid; i < 2 * nt; i += IMP_THREADS) {
        const int t = p.q_terms[t0 + (i >> 1)], w = p.q_imp[t0 + (i >> 1)];
        long long at = 0;
        if (t >= 0 && t < p.n_terms && w >= 1 && w <= 255)
            at = imp_lower_bound(p.post_row, p.term_off[t], p.term_off[t + 1], (i & 1) ? r1 : r0);
        if (i & 1) {
            rhi[i >> 1] = at;
        } else {
            rlo[i >> 1] = at;
            wq[i >> 1] = w;
        }
    }
    __syncthreads();
    if (tid < nt && rhi[tid] > rlo[tid]) any = 1;
    __syncthreads();
    if (!any) return;      // no posting of any query term in this block
    for (int i = tid; i < IMP_R; i += IMP_THREADS) acc[i] = 0;
    __syncthreads();
    for (int j = 0; j < nt; ++j) {
        const int w = wq[j];
        for (long long i = rlo[j] + tid; i < rhi[j]; i += IMP_THREADS) {
            const long long r = p.post_row[i];
            if (r >= r0 && r < r1) acc[r - r0] += w * p.post_imp[i];      // (the searches put r there; a malformed CSR
        }                                                                 //  must not write outside acc)
        __syncthreads();   // the next term may add to the same rows
    }
    const int lane = tid & 63;
    const float tau = p.tau != nullptr ? p.tau[q] : -__builtin_inff();
    for (int i0 = 0; i0 < IMP_R; i0 += IMP_THREADS) {
        const long long r = r0 + i0 + tid;
        const int si = acc[i0 + tid];
        const float s = (float)si;
        bool hit = r < r1 && si > 0 && s >= tau;
        if (hit && p.alive_bits) hit = (p.alive_bits[r >> 5] >> (r & 31)) & 1u;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
        if (!m) continue;
        unsigned base = 0;
        const int leader = __builtin_ctzll(m);
        if (lane == leader) base = atomicAdd(&p.cnt[slot], (unsigned)__popcll(m));
        base = __shfl(base, leader);
        if (hit) {
            const unsigned long long at = (unsigned long long)base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            if (at < (unsigned long long)p.cap) {
                p.cand_s[(size_t)slot * p.cap + at] = s;
                p.cand_r[(size_t)slot * p.cap + at] = (int)r;
            }
        }
    }
}

int impact_topk_impl(const int64_t *term_off, const int32_t *post_row, const int32_t *post_imp, int n_terms, int64_t n,
                     const int32_t *q_off, const int32_t *q_terms, const int32_t *q_imp, int B, int k,
                     const uint32_t *alive_bits, float *out_scores, int64_t *out_rows, void *workspace,
                     size_t workspace_bytes, void *stream, int64_t cap_override, unsigned dbg) {
    MMRAG_CHECK_ARG(B >= 1 && B <= 65535, "impact_topk: B=%d outside 1..65535", B);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K_DEEP, "impact_topk: k=%d outside 1..%d", k, MMRAG_MAX_K_DEEP);
    MMRAG_CHECK_ARG(n >= 0 && n < (int64_t)INT_MAX - IMP_R, "impact_topk: n=%lld out of range", (long long)n);
    MMRAG_CHECK_ARG(n_terms >= 0 && n_terms <= MMRAG_MAX_SPARSE_VOCAB, "impact_topk: n_terms=%d outside 0..%d", n_terms,
                    MMRAG_MAX_SPARSE_VOCAB);
    MMRAG_CHECK_ARG(out_scores && out_rows && q_off, "impact_topk: null pointer");
    MMRAG_CHECK_ARG(cap_override >= 0, "impact_topk: negative capacity");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0 || n_terms == 0)   // nothing can match
        return candidate_fill_empty(out_scores, (long long *)out_rows, B, k, s);
    MMRAG_CHECK_ARG(term_off && post_row && post_imp && q_terms && q_imp, "impact_topk: null pointer");
    ImpactParams p = {};
    p.term_off = (const long long *)term_off;
    p.post_row = post_row;
    p.post_imp = post_imp;
    p.n_terms = n_terms;
    p.q_off = q_off;
    p.q_terms = q_terms;
    p.q_imp = q_imp;
    p.alive_bits = alive_bits;
    p.n = n;
    p.n_blocks = (n + IMP_R - 1) / IMP_R;
    // queries q0 .. q0 + Bq over `walk` of the driver's 128-row tiles: the blocks that hold as many rows, spread evenly
    const auto produce = [&](ScanPass, int q0, int Bq, long long walk, const float *tau, float *cand_s, int *cand_r,
                             unsigned *counts, long long slots) -> int {
        ImpactParams pc = p;
        long long blocks = (walk + IMP_TILES - 1) / IMP_TILES;
        pc.walk = blocks < 1 ? 1 : (blocks > p.n_blocks ? p.n_blocks : blocks);
        pc.q_base = q0;
        pc.tau = tau;
        pc.cap = slots;
        pc.cnt = counts;
        pc.cand_s = cand_s;
        pc.cand_r = cand_r;
        impact_score_kernel<<<dim3((unsigned)pc.walk, (unsigned)Bq), IMP_THREADS, 0, s>>>(pc);
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    };
    return bounded_scan_select("impact_topk", B, n, k, cap_override, (dbg & IMP_DBG_NO_BOUND) != 0u, 0, nullptr,
                               out_scores, (long long *)out_rows, workspace, workspace_bytes, 0, s,
                               [](char *) { return MMRAG_OK; }, produce);
}

}  // namespace

int impact_block_rows() { return IMP_R; }

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

size_t mmrag_impact_topk_workspace_bytes(int B, int64_t n, int k) {
    if (B < 1 || B > 65535 || n < 0 || n >= (int64_t)INT_MAX - IMP_R || k < 1 || k > MMRAG_MAX_K_DEEP) return 0;
    return bounded_scan_layout(B, n > 0 ? n : 1, k, 0, false).select_bytes;
}

// mmrag_impact_topk with a smaller candidate capacity (cap_override > 0) and debug switches (dbg & 1: no bound stages):
// the tests that pin the overflow re-run and the unbounded scan at small n.  Exported for them, deliberately absent from
// include/mmrag.h.
int mmrag_internal_impact_topk_ex(const int64_t *term_off, const int32_t *post_row, const int32_t *post_imp, int n_terms,
                                  int64_t n, const int32_t *q_off, const int32_t *q_terms, const int32_t *q_imp, int B,
                                  int k, const uint32_t *alive_bits, float *out_scores, int64_t *out_rows,
                                  void *workspace, size_t workspace_bytes, void *stream, int64_t cap_override,
                                  unsigned dbg) {
    return impact_topk_impl(term_off, post_row, post_imp, n_terms, n, q_off, q_terms, q_imp, B, k, alive_bits,
                            out_scores, out_rows, workspace, workspace_bytes, stream, cap_override, dbg);
}

int mmrag_impact_topk(const int64_t *term_off, const int32_t *post_row, const int32_t *post_imp, int n_terms, int64_t n,
                      const int32_t *q_off, const int32_t *q_terms, const int32_t *q_imp, int B, int k,
                      const uint32_t *alive_bits, float *out_scores, int64_t *out_rows, void *workspace,
                      size_t workspace_bytes, void *stream) {
    return impact_topk_impl(term_off, post_row, post_imp, n_terms, n, q_off, q_terms, q_imp, B, k, alive_bits,
                            out_scores, out_rows, workspace, workspace_bytes, stream, 0, 0u);
}

}  // extern "C"
