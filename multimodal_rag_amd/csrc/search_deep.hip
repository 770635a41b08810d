// Exact deep top-k (k up to MMRAG_MAX_K_DEEP = 4096) for query batches on gfx950: a threshold-filter scan plus a
// per-query radix select, instead of the register lists of search.hip (which hold at most 20 entries).
//
//   1. bound passes: scan a strided sample of whole 256-row tiles (spread over the collection: rows are stored in
//      document order, a prefix would be biased) and keep every score >= tau_q; the select kernel turns those
//      candidates into tau_q = max(tau_q, their k-th best).  The k-th best of any subset of live rows is at most the
//      true k-th score, so tau_q stays a valid lower bound (-inf while fewer than k rows were seen).  The first sample
//      runs at tau = -inf; later, larger samples reuse the previous tau so their survivors still fit the buffer.
//   2. main pass: every tile, every score >= tau_q appended as (score, local row) to that query's buffer of C slots
//      (filter mode K = 0 of the slab-ring cosine_topk_kernel in search.hip: the MFMA sequence, K-slab order and WN plan
//      of a list search of the same B, so the scores are bit-identical to mmrag_cosine_topk's).  Each query's counter
//      keeps the true survivor count S_q; appends past C are dropped.
//   3. select: one workgroup per query, radix select over the 64-bit key (order-preserving score bits << 32 | ~row):
//      keys are distinct, ties go to the lower row and exactly min(k, S_q) keys are taken; the winners are
//      bitonic-sorted in LDS and written as [B, k] (score desc, row + row_offset), (-inf, -1) padded.
//   4. overflow (S_q > C): the counters are read on the host once (the only stream synchronisation; none when n <= C,
//      where nothing can overflow) and each such query is re-run alone with the same tau_q into a buffer of n slots.
//      No retries: the count is known, so the re-run fits on the first try.
#include "deep_select.h"

#include <stdlib.h>

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int DEEP_TM = 256;               // corpus rows per tile of the slab-ring kernel
constexpr int DEEP_SAMPLE0_TILES = 48;     // first bound sample: 12288 rows, the select's LDS key cache
constexpr int DEEP_MAX_STAGES = 8;

// debug switches of mmrag_internal_cosine_topk_deep_ex (tests only)
constexpr unsigned DEEP_DBG_NO_BOUND = 1u;  // no bound passes: tau = -inf, every live row survives the main pass

struct DeepPlan {
    int B, WN, grid_y, n_tiles;
    long long cap;                          // C: candidate slots per query
    int n_stages;
    int stage_tiles[DEEP_MAX_STAGES], stage_stride[DEEP_MAX_STAGES];
};

DeepPlan make_deep_plan(int B, long long n, int k, long long cap_override, unsigned dbg) {
    DeepPlan pl;
    pl.WN = B <= 64 ? 2 : (B <= 128 ? 4 : 8);   // the list search's plan for this B (search.hip make_plan)
    const int qrows = 32 * pl.WN;
    pl.B = B;
    pl.grid_y = (B + qrows - 1) / qrows;
    pl.n_tiles = (int)((n + DEEP_TM - 1) / DEEP_TM);
    const long long c = 32LL * k > 16384 ? 32LL * k : 16384;
    pl.cap = (c + 255) / 256 * 256;
    if (cap_override > 0 && cap_override < pl.cap) pl.cap = cap_override;
    pl.n_stages = 0;
    if (n <= pl.cap || (dbg & DEEP_DBG_NO_BOUND)) return pl;  // every live row fits: no bound needed
    // main-pass survivors ~ k * n / m for a bound from m sampled rows: aim at C / 4
    const long long target_rows = (4LL * k * n + pl.cap - 1) / pl.cap;
    const long long target = (target_rows + DEEP_TM - 1) / DEEP_TM;
    long long t = DEEP_SAMPLE0_TILES < pl.n_tiles ? DEEP_SAMPLE0_TILES : pl.n_tiles;
    for (;;) {
        pl.stage_tiles[pl.n_stages] = (int)t;
        pl.stage_stride[pl.n_stages] = (int)(pl.n_tiles / t);
        ++pl.n_stages;
        if (t >= target || pl.n_stages == DEEP_MAX_STAGES) break;
        // the next sample's survivors ~ k * m' / m must fit C / 4 as well
        long long nt = t * pl.cap / (4LL * k);
        if (nt > target) nt = target;
        if (nt > pl.n_tiles) nt = pl.n_tiles;
        if (nt <= t) break;
        t = nt;
    }
    return pl;
}

int deep_walkers(int tiles, int grid_y) {
    const int cus = num_cus();
    int gx = tiles < cus ? tiles : cus;
    if (grid_y > 1 && tiles >= cus) {
        const int w = cus / grid_y / 8 * 8;   // all query groups of a tile resident together (as search.hip)
        gx = w >= 8 ? w : (cus / grid_y > 0 ? cus / grid_y : 1);
    }
    return gx < 1 ? 1 : gx;
}

struct DeepWs {
    size_t off_cnt, off_one_cnt, off_tau, off_bs, off_br, off_os, off_or, total;
};

DeepWs deep_ws_layout(const DeepPlan &pl, long long n) {
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    DeepWs w;
    w.off_cnt = 0;
    // per real query (padding query slots of a workgroup never pass the filter): counter, tau, C candidates
    w.off_one_cnt = up((size_t)pl.B * sizeof(unsigned));
    w.off_tau = w.off_one_cnt + 256;
    w.off_bs = up(w.off_tau + (size_t)pl.B * sizeof(float));
    w.off_br = up(w.off_bs + (size_t)pl.B * pl.cap * sizeof(float));
    // one query x n slots: the re-run of an overflowed query
    w.off_os = up(w.off_br + (size_t)pl.B * pl.cap * sizeof(int));
    w.off_or = up(w.off_os + (size_t)n * sizeof(float));
    w.total = up(w.off_or + (size_t)n * sizeof(int));
    return w;
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

size_t mmrag_cosine_topk_deep_workspace_bytes(int B, int64_t n, int k) {
    if (B <= 0 || n < 0 || k < 1 || k > MMRAG_MAX_K_DEEP) return 0;
    return deep_ws_layout(make_deep_plan(B, n, k, 0, 0u), n).total;
}

// mmrag_cosine_topk_deep with debug switches (DEEP_DBG_*) and a smaller candidate capacity (cap > 0): the tests that
// pin the overflow re-run and the unbounded scan.  Exported for them, deliberately absent from include/mmrag.h.
int mmrag_internal_cosine_topk_deep_ex(const void *q, const void *corpus, int B, int64_t n, int d, int64_t ld,
                                       int dtype, int k, int64_t row_offset, const uint32_t *alive_bits,
                                       float *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes,
                                       void *stream, unsigned dbg, int64_t cap) {
    MMRAG_CHECK_ARG(dtype >= 0 && dtype <= MMRAG_F8E4M3, "cosine_topk_deep: bad dtype %d", dtype);
    MMRAG_CHECK_ARG(B > 0, "cosine_topk_deep: B must be positive (got %d)", B);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K_DEEP, "cosine_topk_deep: k=%d outside 1..%d", k, MMRAG_MAX_K_DEEP);
    MMRAG_CHECK_ARG(n >= 0 && n < (int64_t)INT_MAX - DEEP_TM, "cosine_topk_deep: n=%lld out of range", (long long)n);
    MMRAG_CHECK_ARG(d > 0 && ld >= d, "cosine_topk_deep: need 0 < d <= ld (d=%d ld=%lld)", d, (long long)ld);
    const int64_t row_bytes = ld * esize(dtype);
    MMRAG_CHECK_ARG(row_bytes % SLAB == 0, "cosine_topk_deep: row bytes %lld not a multiple of %d (use mmrag_padded_dim)",
                    (long long)row_bytes, SLAB);
    MMRAG_CHECK_ARG(row_bytes * DEEP_TM < (int64_t)UINT_MAX, "cosine_topk_deep: rows too long");
    MMRAG_CHECK_ARG(q, "cosine_topk_deep: null q");
    MMRAG_CHECK_ARG(n == 0 || corpus, "cosine_topk_deep: null corpus");
    MMRAG_CHECK_ARG(((uintptr_t)q % 16) == 0 && ((uintptr_t)corpus % 16) == 0,
                    "cosine_topk_deep: q/corpus must be 16-byte aligned");
    MMRAG_CHECK_ARG(out_scores && out_rows, "cosine_topk_deep: null output");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        const long long total = (long long)B * k;
        deep_fill_empty_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(out_scores, (long long *)out_rows, total);
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    }
    const DeepPlan pl = make_deep_plan(B, n, k, cap, dbg);
    const DeepWs wl = deep_ws_layout(pl, n);
    if (!workspace || workspace_bytes < wl.total) {
        set_error("cosine_topk_deep: workspace %zu bytes < required %zu", workspace_bytes, wl.total);
        return MMRAG_EWORKSPACE;
    }
    MMRAG_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "cosine_topk_deep: workspace must be 16-byte aligned");

    char *ws = (char *)workspace;
    unsigned *cnt = (unsigned *)(ws + wl.off_cnt);
    unsigned *one_cnt = (unsigned *)(ws + wl.off_one_cnt);
    float *tau = (float *)(ws + wl.off_tau);
    KParams p = {};
    p.q = (const char *)q;
    p.corpus = (const char *)corpus;
    p.alive_bits = alive_bits;
    p.cand_s = (float *)(ws + wl.off_bs);
    p.cand_r = (int *)(ws + wl.off_br);
    p.n = n;
    p.B = B;
    p.row_bytes = (unsigned)row_bytes;
    p.n_lists = 0;
    p.tile0 = 0;
    p.thr0 = nullptr;
    p.p_static = INT_MAX / 2;
    p.deep_cnt = cnt;
    p.deep_cap = (int)pl.cap;

    // 1. bound passes (tau starts at -inf: the bit pattern 0xff800000)
    if (pl.n_stages > 0) {
        MMRAG_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)tau, (int)0xff800000u, (size_t)B, s));
        p.thr0 = tau;
    }
    for (int st = 0; st < pl.n_stages; ++st) {
        MMRAG_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)B * sizeof(unsigned), s));
        KParams ps = p;
        ps.n_tiles = pl.stage_tiles[st];
        ps.tile_stride = pl.stage_stride[st];
        if (int e = deep_filter_launch(dtype, pl.WN, ps, deep_walkers(ps.n_tiles, pl.grid_y), pl.grid_y, s)) return e;
        deep_select_kernel<<<B, SEL_THREADS, 0, s>>>(p.cand_s, p.cand_r, cnt, pl.cap, k, 0, 1, nullptr, nullptr, tau);
        MMRAG_CHECK_HIP(hipGetLastError());
    }
    // 2. main pass over every tile, 3. select (queries that overflowed C are skipped)
    MMRAG_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)B * sizeof(unsigned), s));
    p.n_tiles = pl.n_tiles;
    p.tile_stride = 1;
    if (int e = deep_filter_launch(dtype, pl.WN, p, deep_walkers(p.n_tiles, pl.grid_y), pl.grid_y, s)) return e;
    deep_select_kernel<<<B, SEL_THREADS, 0, s>>>(p.cand_s, p.cand_r, cnt, pl.cap, k, row_offset, 0, out_scores,
                                                 (long long *)out_rows, nullptr);
    MMRAG_CHECK_HIP(hipGetLastError());
    if (n <= pl.cap) return MMRAG_OK;   // no query can have more than n survivors

    // 4. overflow: one read of the counters (the call's only synchronisation), then each query with S_q > C alone,
    //    same WN plan (bit-identical scores), same tau_q, n slots
    unsigned *host_cnt = (unsigned *)malloc((size_t)B * sizeof(unsigned));
    if (!host_cnt) {
        set_error("cosine_topk_deep: out of host memory");
        return MMRAG_EHIP;
    }
    hipError_t e = hipMemcpyAsync(host_cnt, cnt, (size_t)B * sizeof(unsigned), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        free(host_cnt);
        set_error("cosine_topk_deep: reading the survivor counts failed: %s", hipGetErrorString(e));
        return MMRAG_EHIP;
    }
    int status = MMRAG_OK;
    for (int qi = 0; qi < B && status == MMRAG_OK; ++qi) {
        if (host_cnt[qi] <= (unsigned)pl.cap) continue;
        KParams p1 = p;
        p1.q = (const char *)q + (size_t)qi * row_bytes;
        p1.B = 1;
        p1.thr0 = pl.n_stages > 0 ? tau + qi : nullptr;
        p1.cand_s = (float *)(ws + wl.off_os);
        p1.cand_r = (int *)(ws + wl.off_or);
        p1.deep_cnt = one_cnt;
        p1.deep_cap = (int)n;
        e = hipMemsetAsync(one_cnt, 0, sizeof(unsigned), s);
        if (e != hipSuccess) {
            set_error("cosine_topk_deep: hipMemsetAsync failed: %s", hipGetErrorString(e));
            status = MMRAG_EHIP;
            break;
        }
        // grid_y = 1: one query; the WN (and with it the MFMA path) stays the batch's
        status = deep_filter_launch(dtype, pl.WN, p1, deep_walkers(p1.n_tiles, 1), 1, s);
        if (status != MMRAG_OK) break;
        deep_select_kernel<<<1, SEL_THREADS, 0, s>>>(p1.cand_s, p1.cand_r, one_cnt, n, k, row_offset, 0,
                                                     out_scores + (size_t)qi * k, (long long *)out_rows + (size_t)qi * k,
                                                     nullptr);
        e = hipGetLastError();
        if (e != hipSuccess) {
            set_error("cosine_topk_deep: select launch failed: %s", hipGetErrorString(e));
            status = MMRAG_EHIP;
        }
    }
    free(host_cnt);
    return status;
}

int mmrag_cosine_topk_deep(const void *q, const void *corpus, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                           int64_t row_offset, const uint32_t *alive_bits, float *out_scores, int64_t *out_rows,
                           void *workspace, size_t workspace_bytes, void *stream) {
    return mmrag_internal_cosine_topk_deep_ex(q, corpus, B, n, d, ld, dtype, k, row_offset, alive_bits, out_scores,
                                              out_rows, workspace, workspace_bytes, stream, 0u, 0);
}

}  // extern "C"
