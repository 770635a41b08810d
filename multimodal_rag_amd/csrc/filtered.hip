// Filtered retrieval (include/mmrag.h mmrag_filter_eval, mmrag_filtered_topk): metadata filters evaluated on the device
// and a batch of queries answered in one masked scan, each query seeing only the rows of ITS filter's bitmap.
//
// mmrag_filter_eval: F postfix programs over typed metadata columns, n rows -> F bitmaps of W = 4 ceil(n / 128) words.
// One lane per row, 256 rows per workgroup.  A lane reads its row's value of every column once (a string ordinal as a
// double, missing as NaN) and keeps them in its own LDS slots; then every program runs on it: the instruction stream is
// the same for all lanes (uniform loads), the boolean stack is one 32-bit register.  IEEE comparisons against NaN give
// match_where's answer for a missing value (false for == > >= < <= in, true for != not-in), so there is no special case.
// A wave's 64 results become two words by ballot, written by lane 0 with plain stores; bits at and past n are zero.
//
// mmrag_filtered_topk:
//   1. union: per tile of 128 queries the OR of the bitmaps of the filters in it, uni[qt][W].
//   2. scan: boosted.hip's scan with scoped.hip's skip rule.  Q . X^T with pair_tile.h's body, a 128-row tile of stored
//      rows as A and a 128-query tile as B; rows past n and queries past B read as zero through the buffer descriptor.
//      Workgroups are persistent over row tiles.  Before anything is fetched all four waves read the tile's four words
//      of every query tile's union: the same scalar mask of wanted query tiles in each, so the workgroup branches as one
//      and the ring's barriers are reached by all waves or by none.  An item (row tile, query tile) in which no query
//      sees a row is never issued; a row tile nobody wants costs those words only.  The ring runs over the K-slabs of
//      the wanted query tiles without draining.  After a query tile's last slab a lane reads, for each of its 4 query
//      columns, the 8 bytes of that query's bitmap that cover its wave's 64 rows, tests its 16 bits and the score
//      against tau, and appends the survivors as (score, local row) through the query's counter.
//      A filter can pass most of the collection, so when n exceeds the candidate slots the scan first runs over a
//      strided sample of whole tiles and deep_select_kernel's bound mode sets tau_q to the k-th best of the VISIBLE
//      sampled rows: the k-th best of any subset of a query's visible rows is at most its true k-th, whatever the
//      filter (tau_q stays -inf while fewer than k visible rows were sampled).
//   3. select and overflow.  Steps 2 and 3 run under candidate_select.h's bounded_scan_select (plan, workspace,
//      stages, main pass, select, re-runs); this file supplies the unions and the producer.
// The K order is slab_step's, so a score's bits depend on the query row, the stored row and d alone and equal
// mmrag_scoped_topk's: not on the batch, the filters, the grid, tau or whether bound passes ran.
// The scan body and the union kernel are masked_scan.h's, shared with range.hip.
#include "masked_scan.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int FE_THREADS = 256;          // rows of a filter_eval workgroup

// ---- filter programs ----------------------------------------------------------------------------------------------
struct FilterEvalParams {
    const mmrag_filter_op *ops;
    int n_ops;
    const int *prog_off;   // [F + 1]
    int F;
    const double *set_values;
    int n_set;
    const void *col[MMRAG_MAX_FILTER_COLUMNS];
    int kind[MMRAG_MAX_FILTER_COLUMNS];
    int n_col;
    long long n;
    const unsigned *alive;
    unsigned *out;         // [F, W]
    long long W;
};

// A malformed table never reads out of range: a program outside ops[0 .. n_ops) or longer than MMRAG_MAX_FILTER_OPS
// matches nothing, a column index outside 0..n_col-1 reads as missing, a set outside set_values[0 .. n_set) as empty.
__global__ __launch_bounds__(FE_THREADS) void filter_eval_kernel(const FilterEvalParams p) {
    __shared__ double colv[MMRAG_MAX_FILTER_COLUMNS][FE_THREADS];
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x * FE_THREADS + tid;
    const bool in = row < p.n;
    for (int c = 0; c < p.n_col; ++c) {
        double v = __builtin_nan("");
        if (in) {
            if (p.kind[c] == MMRAG_FILTER_NUMBER) {
                v = ((const double *)p.col[c])[row];
            } else {
                const int o = ((const int *)p.col[c])[row];
                if (o >= 0) v = (double)o;
            }
        }
        colv[c][tid] = v;      // read back by this thread only
    }
    const bool live = in && (p.alive == nullptr || ((p.alive[row >> 5] >> (row & 31)) & 1u) != 0u);
    const long long w0 = ((long long)blockIdx.x * FE_THREADS + (tid & ~63)) >> 5;   // this wave's first word
    for (int f = 0; f < p.F; ++f) {
        const int lo = p.prog_off[f], hi = p.prog_off[f + 1];
        const bool ok = lo >= 0 && hi > lo && hi <= p.n_ops && hi - lo <= MMRAG_MAX_FILTER_OPS;
        unsigned st = 0;       // the boolean stack: bit 0 is the top
        if (ok) {
            for (int i = lo; i < hi; ++i) {
                const mmrag_filter_op op = p.ops[i];
                if (op.code == MMRAG_FILTER_AND || op.code == MMRAG_FILTER_OR) {
                    const unsigned a = st & 1u;
                    st >>= 1;
                    st = op.code == MMRAG_FILTER_AND ? (st & (~1u | a)) : (st | a);
                    continue;
                }
                bool r = false;
                if (op.code == MMRAG_FILTER_TRUE) {
                    r = true;
                } else if (op.code >= MMRAG_FILTER_EQ && op.code <= MMRAG_FILTER_NIN) {
                    const double v = (unsigned)op.column < (unsigned)p.n_col ? colv[op.column][tid] : __builtin_nan("");
                    const double x = op.value;
                    switch (op.code) {
                    case MMRAG_FILTER_EQ: r = v == x; break;
                    case MMRAG_FILTER_NE: r = v != x; break;
                    case MMRAG_FILTER_GT: r = v > x; break;
                    case MMRAG_FILTER_GE: r = v >= x; break;
                    case MMRAG_FILTER_LT: r = v < x; break;
                    case MMRAG_FILTER_LE: r = v <= x; break;
                    default: {
                        int len = op.set_len;
                        if (op.set_off < 0 || len < 0 || len > MMRAG_MAX_FILTER_SET || op.set_off > p.n_set - len) len = 0;
                        bool hit = false;
                        for (int j = 0; j < len; ++j) hit |= v == p.set_values[op.set_off + j];
                        r = op.code == MMRAG_FILTER_IN ? hit : !hit;
                    }
                    }
                }
                st = (st << 1) | (unsigned)r;
            }
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(ok && (st & 1u) != 0u && live);
        if ((tid & 63) == 0) {
            unsigned *o = p.out + (size_t)f * p.W;
            if (w0 < p.W) o[w0] = (unsigned)m;
            if (w0 + 1 < p.W) o[w0 + 1] = (unsigned)(m >> 32);
        }
    }
}

// ---- the masked scan (masked_scan.h) with the top-k epilogue ------------------------------------------------------
struct FilteredParams : MaskedScanParams {
    const float *tau;       // [B], or null: -inf
    float *cand_s;
    int *cand_r;
    unsigned *cnt;
    unsigned cap;
};

template <int DT>
__global__ __launch_bounds__(256, 2) void filtered_scan_kernel(const FilteredParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    masked_scan_body<DT>(p, smem, [&](int col, unsigned vis, const f32x4_t (&acc)[4][4], int b, int lrow0) {
        if (vis == 0u) return;
        const float t = p.tau != nullptr ? p.tau[col] : NEG_INF;
        const unsigned hit = scores_at_least(acc, b, t) & vis;
        if (hit == 0u) return;
        append_candidates(hit, acc, b, lrow0, p.cnt + col, p.cand_s + (size_t)col * p.cap,
                          p.cand_r + (size_t)col * p.cap, p.cap);
    });
#endif
}

template <int DT>
int launch_scan(const FilteredParams &p, hipStream_t s) {
    hipLaunchKernelGGL(filtered_scan_kernel<DT>, dim3(scan_grid(p.walk)), dim3(256), 0, s, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

int64_t mmrag_filter_words(int64_t n) { return n < 0 || n >= (1LL << 31) ? 0 : filter_words(n); }

int mmrag_filter_eval(const mmrag_filter_op *ops, int n_ops, const int32_t *prog_off, int F, const double *set_values,
                      int n_set, const void *const *columns, const int32_t *kinds, int n_columns, int64_t n,
                      const uint32_t *alive_bits, uint32_t *out_bits, void *stream) {
    MMRAG_CHECK_ARG(ops && prog_off && out_bits, "filter_eval: null pointer");
    MMRAG_CHECK_ARG(F >= 1, "filter_eval: need F >= 1 programs (F=%d)", F);
    MMRAG_CHECK_ARG(n_ops >= 1, "filter_eval: need n_ops >= 1 (n_ops=%d)", n_ops);
    MMRAG_CHECK_ARG(n_set >= 0 && (set_values || n_set == 0), "filter_eval: null set_values with n_set=%d", n_set);
    MMRAG_CHECK_ARG(n >= 0 && n < (1LL << 31), "filter_eval: need 0 <= n < 2^31 (n=%lld)", (long long)n);
    MMRAG_CHECK_ARG(n_columns >= 0 && n_columns <= MMRAG_MAX_FILTER_COLUMNS, "filter_eval: n_columns=%d outside 0..%d",
                    n_columns, MMRAG_MAX_FILTER_COLUMNS);
    MMRAG_CHECK_ARG(n_columns == 0 || (columns && kinds), "filter_eval: null column table");
    FilterEvalParams p;
    for (int c = 0; c < MMRAG_MAX_FILTER_COLUMNS; ++c) {
        p.col[c] = nullptr;
        p.kind[c] = MMRAG_FILTER_NUMBER;
    }
    for (int c = 0; c < n_columns; ++c) {
        MMRAG_CHECK_ARG(columns[c] || n == 0, "filter_eval: column %d is null", c);
        MMRAG_CHECK_ARG(kinds[c] == MMRAG_FILTER_NUMBER || kinds[c] == MMRAG_FILTER_STRING,
                        "filter_eval: column %d has kind %d", c, kinds[c]);
        p.col[c] = columns[c];
        p.kind[c] = kinds[c];
    }
    if (n == 0) return MMRAG_OK;      // W == 0: nothing to write
    p.ops = ops;
    p.n_ops = n_ops;
    p.prog_off = prog_off;
    p.F = F;
    p.set_values = set_values;
    p.n_set = n_set;
    p.n_col = n_columns;
    p.n = n;
    p.alive = alive_bits;
    p.out = out_bits;
    p.W = filter_words(n);
    const unsigned blocks = (unsigned)((n + FE_THREADS - 1) / FE_THREADS);
    hipLaunchKernelGGL(filter_eval_kernel, dim3(blocks), dim3(FE_THREADS), 0, (hipStream_t)stream, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

size_t mmrag_filtered_topk_workspace_bytes(int B, int64_t n, int k) {
    if (B <= 0 || n < 0 || n >= (1LL << 31) || k < 1 || k > MMRAG_MAX_K_DEEP) return 0;
    return bounded_scan_layout(B, n, k, 0, false).select_bytes + filtered_union_bytes(B, n);
}

// mmrag_filtered_topk with a smaller candidate capacity (cap_override > 0), debug switches (FI_DBG_*) and an optional
// device counter of the (row tile, query tile) items the main pass issues: the tests that pin the overflow re-run, the
// unbounded scan and the skip rule, and the bench.  Exported for them, deliberately absent from include/mmrag.h.
int mmrag_internal_filtered_topk_ex(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                                    int64_t row_offset, const int32_t *filter_of_query, int F, const uint32_t *vis_bits,
                                    float *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes,
                                    void *stream, int64_t cap_override, unsigned dbg, uint64_t *items_issued) {
    MMRAG_CHECK_ARG(q && rows && filter_of_query, "filtered_topk: null pointer");
    MMRAG_CHECK_ARG(out_scores && out_rows, "filtered_topk: null output");
    if (int st = check_stored_rows("filtered_topk", "searched by filter", "search", ld, dtype, d, &n)) return st;
    MMRAG_CHECK_ARG(n < (1LL << 31), "filtered_topk: need n < 2^31 (n=%lld)", (long long)n);
    MMRAG_CHECK_ARG(vis_bits || n == 0, "filtered_topk: null vis_bits");
    MMRAG_CHECK_ARG(B >= 1, "filtered_topk: need B >= 1 (B=%d)", B);
    MMRAG_CHECK_ARG(F >= 1, "filtered_topk: need F >= 1 filters (F=%d)", F);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K_DEEP, "filtered_topk: k=%d outside 1..%d", k, MMRAG_MAX_K_DEEP);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return candidate_fill_empty(out_scores, (long long *)out_rows, B, k, s);

    FilteredParams p;
    p.rows = (const char *)rows;
    p.n = n;
    p.row_bytes = stored_row_bytes(ld, dtype);
    p.nk = stored_k_slabs(d, dtype);
    p.vis = vis_bits;
    p.F = F;
    p.W = filter_words(n);
    p.T = (n + PT - 1) / PT;
    unsigned *uni = nullptr;      // the caller's extra bytes: the batch's unions, then one query tile's for a re-run
    const int nqt_all = (B + PT - 1) / PT;

    // queries q0 .. q0 + Bq over `walk` tiles into their slots.  The batch's unions serve every pass of it; a query
    // produced again alone gets its own.  The main pass counts the items it issues.
    const auto produce = [&](ScanPass pass, int q0, int Bq, long long walk, const float *tau, float *cand_s, int *cand_r,
                             unsigned *counts, long long slots) -> int {
        const unsigned *um = uni;
        if (pass == SCAN_PASS_RERUN) {
            unsigned *own = uni + (size_t)nqt_all * p.W;
            if (int e = launch_unions(filter_of_query + q0, Bq, F, vis_bits, p.W, own, s)) return e;
            um = own;
        }
        return for_scan_chunks(Bq, PT, [&](int first, int Bc, int nqt, int t0) -> int {
            FilteredParams pc = p;
            const int c0 = q0 + first;
            pc.q = (const char *)q + (size_t)c0 * p.row_bytes;
            pc.filter_of_query = filter_of_query + c0;
            pc.tau = tau != nullptr ? tau + c0 : nullptr;
            pc.B = Bc;
            pc.nqt = nqt;
            pc.uni = um + (size_t)t0 * p.W;
            pc.walk = walk;
            pc.cap = (unsigned)slots;
            pc.cand_s = cand_s + (size_t)first * slots;
            pc.cand_r = cand_r + (size_t)first * slots;
            pc.cnt = counts + first;
            pc.items = pass == SCAN_PASS_MAIN ? (unsigned long long *)items_issued : nullptr;
            return with_elem_type(dtype, [&](auto tag) { return launch_scan<decltype(tag)::value>(pc, s); });
        });
    };
    if (items_issued) MMRAG_CHECK_HIP(hipMemsetAsync(items_issued, 0, sizeof(uint64_t), s));
    return bounded_scan_select(
        "filtered_topk", B, n, k, cap_override, (dbg & FI_DBG_NO_BOUND) != 0u, row_offset, nullptr, out_scores,
        (long long *)out_rows, workspace, workspace_bytes, filtered_union_bytes(B, n), s,
        [&](char *extra) {      // the unions of the batch, once for every pass
            uni = (unsigned *)extra;
            return launch_unions(filter_of_query, B, F, vis_bits, p.W, uni, s);
        },
        produce);
}

int mmrag_filtered_topk(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                        int64_t row_offset, const int32_t *filter_of_query, int F, const uint32_t *vis_bits,
                        float *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream) {
    return mmrag_internal_filtered_topk_ex(q, rows, B, n, d, ld, dtype, k, row_offset, filter_of_query, F, vis_bits,
                                           out_scores, out_rows, workspace, workspace_bytes, stream, 0, 0u, nullptr);
}

}  // extern "C"
