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
// Steps 2 to 4 are the driver of candidate_select.h (shared with the BM25 search) around this file's two filter launches.
#include "candidate_select.h"

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
    pl.WN = plan_wn(B);   // the list search's plan for this B
    const int qrows = 32 * pl.WN;
    pl.B = B;
    pl.grid_y = (B + qrows - 1) / qrows;
    pl.n_tiles = (int)((n + DEEP_TM - 1) / DEEP_TM);
    pl.cap = candidate_capacity(k);
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

// per real query (padding query slots of a workgroup never pass the filter): counter, tau, C candidates
CandWs deep_ws_layout(const DeepPlan &pl, long long n) { return candidate_ws_layout(pl.B, pl.cap, n, true); }

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
    if (int st = check_search_args("cosine_topk_deep", MMRAG_MAX_K_DEEP, q, corpus, B, n, d, ld, dtype, k)) return st;
    MMRAG_CHECK_ARG(out_scores && out_rows, "cosine_topk_deep: null output");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return candidate_fill_empty(out_scores, (long long *)out_rows, B, k, s);
    const DeepPlan pl = make_deep_plan(B, n, k, cap, dbg);
    const CandWs wl = deep_ws_layout(pl, n);
    if (!workspace || workspace_bytes < wl.total) {
        set_error("cosine_topk_deep: workspace %zu bytes < required %zu", workspace_bytes, wl.total);
        return MMRAG_EWORKSPACE;
    }
    MMRAG_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "cosine_topk_deep: workspace must be 16-byte aligned");

    char *ws = (char *)workspace;
    unsigned *cnt = (unsigned *)(ws + wl.off_cnt);
    float *tau = (float *)(ws + wl.off_floats);
    KParams p = {};
    p.q = (const char *)q;
    p.corpus = (const char *)corpus;
    p.alive_bits = alive_bits;
    p.cand_s = (float *)(ws + wl.off_bs);
    p.cand_r = (int *)(ws + wl.off_br);
    p.n = n;
    p.B = B;
    p.row_bytes = (unsigned)(ld * esize(dtype));
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
        if (int e = deep_filter_launch(dtype, pl.WN, ps, plan_walkers(ps.n_tiles, pl.grid_y), pl.grid_y, s)) return e;
        deep_select_kernel<<<B, SEL_THREADS, 0, s>>>(p.cand_s, p.cand_r, cnt, pl.cap, k, 0, 1, nullptr, nullptr, tau);
        MMRAG_CHECK_HIP(hipGetLastError());
    }
    // 2. main pass over every tile, 3. select, 4. each query with S_q > C alone: same WN plan (and with it the MFMA path:
    //    bit-identical scores) on a grid of one query group, same tau_q
    p.n_tiles = pl.n_tiles;
    p.tile_stride = 1;
    const auto filter_into = [&](KParams kp, int grid_y, float *cand_s, int *cand_r, unsigned *counts, long long slots) {
        kp.cand_s = cand_s;
        kp.cand_r = cand_r;
        kp.deep_cnt = counts;
        kp.deep_cap = (int)slots;
        return deep_filter_launch(dtype, pl.WN, kp, plan_walkers(kp.n_tiles, grid_y), grid_y, s);
    };
    return candidate_select(
        "cosine_topk_deep", B, n, pl.cap, k, row_offset, out_scores, (long long *)out_rows, ws, wl, s,
        [&](float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return filter_into(p, pl.grid_y, cand_s, cand_r, counts, slots);
        },
        [&](int qi, float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            KParams p1 = p;
            p1.q = p.q + (size_t)qi * p.row_bytes;
            p1.B = 1;
            p1.thr0 = pl.n_stages > 0 ? tau + qi : nullptr;
            return filter_into(p1, 1, cand_s, cand_r, counts, slots);
        });
}

int mmrag_cosine_topk_deep(const void *q, const void *corpus, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                           int64_t row_offset, const uint32_t *alive_bits, float *out_scores, int64_t *out_rows,
                           void *workspace, size_t workspace_bytes, void *stream) {
    return mmrag_internal_cosine_topk_deep_ex(q, corpus, B, n, d, ld, dtype, k, row_offset, alive_bits, out_scores,
                                              out_rows, workspace, workspace_bytes, stream, 0u, 0);
}

}  // extern "C"
