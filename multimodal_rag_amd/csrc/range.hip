// Range retrieval (include/mmrag.h mmrag_range_scan): for each query of a batch, HOW MANY of the rows it may see score
// at or above its threshold, how those rows spread over the values of up to MMRAG_MAX_FACET_COLUMNS metadata columns,
// and the `limit` best of them -- in one exact scan.  The [B, n] score matrix is never written.
//
// The scan is masked_scan.h's (filtered.hip's): persistent workgroups over 128-row tiles, a 128-query tile as B, the
// union-bitmap skip.  Without bitmaps every row below n is visible and every item is issued.  The epilogue keeps two
// masks per lane and query column over the lane's 16 rows:
//   pass = visible and score >= threshold[col]      -> out_count[col] += popc(pass), one integer atomic; per facet
//          column, the passing rows' codes are read and each run of equal slots among the lane's rows is one integer
//          atomic on that slot (the rows of a document are stored together, so a run is usually the whole lane).
//   hit  = pass and score >= tau[col]               -> appended to the query's candidate slots as filtered.hip does.
// Counts are integers: the tables do not depend on the order the atomics arrive in.
//
// Hits are a top-`limit` of the passing rows, so filtered.hip's plan applies with tau starting at the threshold: when n
// exceeds the candidate slots, bound passes over sampled tiles raise tau_q to max(threshold_q, the limit-th best visible
// sampled score), and the main pass appends only scores at or above it.  The tables are accumulated in the MAIN pass
// only: bound passes and the re-run of a query whose survivors overflowed its slots launch the kernel with null table
// pointers.  limit == 0 takes none of the candidate machinery: no bound passes, no select, no host synchronisation.
#include "masked_scan.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

struct RangeParams : MaskedScanParams {
    const float *thr;       // [B]
    const float *tau;       // [B], or null: the threshold
    unsigned *out_count;    // [B], or null: this launch counts nothing (a bound pass, a re-run)
    unsigned *out_facets;   // [B, facet_stride]
    const int *facet_col[MMRAG_MAX_FACET_COLUMNS];
    int facet_size[MMRAG_MAX_FACET_COLUMNS];   // G_c
    int facet_off[MMRAG_MAX_FACET_COLUMNS];    // sum of G_c' + 1 over c' < c
    int n_facets;
    long long facet_stride; // sum of G_c + 1
    float *cand_s;          // null: no hits are collected (limit == 0)
    int *cand_r;
    unsigned *cnt;
    unsigned cap;
};

template <int DT>
__global__ __launch_bounds__(256, 2) void range_scan_kernel(const RangeParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    masked_scan_body<DT>(p, smem, [&](int col, unsigned vis, const f32x4_t (&acc)[4][4], int b, int lrow0) {
        if (vis == 0u) return;
        const float thr = p.thr[col];
        const unsigned pass = scores_at_least(acc, b, thr) & vis;
        if (pass == 0u) return;
        if (p.out_count != nullptr) {
            atomicAdd(p.out_count + col, (unsigned)__popc(pass));
            for (int c = 0; c < p.n_facets; ++c) {
                const int *const codes = p.facet_col[c];
                const unsigned G = (unsigned)p.facet_size[c];
                unsigned *const slots = p.out_facets + (size_t)col * p.facet_stride + p.facet_off[c];
                // runs of equal slots among the passing rows, in row order; a code outside 0..G-1 is slot G
                unsigned run_slot = 0, run = 0;
                for (unsigned m = pass; m != 0u; m &= m - 1u) {
                    const int bit = __builtin_ctz(m);
                    const unsigned code = (unsigned)codes[lrow0 + 16 * (bit >> 2) + (bit & 3)];   // a row below n
                    const unsigned slot = code < G ? code : G;
                    if (run != 0u && slot != run_slot) {
                        atomicAdd(slots + run_slot, run);
                        run = 0;
                    }
                    run_slot = slot;
                    ++run;
                }
                atomicAdd(slots + run_slot, run);
            }
        }
        if (p.cand_s == nullptr) return;
        // tau >= threshold where it is given, so pass and score >= tau is `hit`
        const unsigned hit = p.tau != nullptr ? pass & scores_at_least(acc, b, p.tau[col]) : pass;
        if (hit == 0u) return;
        append_candidates(hit, acc, b, lrow0, p.cnt + col, p.cand_s + (size_t)col * p.cap,
                          p.cand_r + (size_t)col * p.cap, p.cap);
    });
#endif
}

template <int DT>
int launch_range_scan(const RangeParams &p, hipStream_t s) {
    hipLaunchKernelGGL(range_scan_kernel<DT>, dim3(scan_grid(p.walk)), dim3(256), 0, s, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

// facet_slots (the sum of G_c + 1) is part of the signature for a later LDS or workspace pre-aggregation of the tables;
// today the tables are the caller's outputs and the size does not depend on it.
size_t mmrag_range_scan_workspace_bytes(int B, int64_t n, int limit, int facet_slots) {
    if (B <= 0 || n < 0 || n >= (1LL << 31) || limit < 0 || limit > MMRAG_MAX_K_DEEP || facet_slots < 0) return 0;
    // [the bounded scan's blocks, limit > 0 only | the union bitmaps]
    return (limit > 0 ? bounded_scan_layout(B, n, limit, 0, false).select_bytes : 0) + filtered_union_bytes(B, n) + 256;
}

// mmrag_range_scan with a smaller candidate capacity (cap_override > 0) and debug switches (FI_DBG_NO_BOUND: no bound
// passes, tau stays the threshold): the tests that pin the overflow re-run and the unbounded scan at small n.  Exported
// for them, deliberately absent from include/mmrag.h.
int mmrag_internal_range_scan_ex(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype,
                                 const float *threshold, int limit, int64_t row_offset, const int32_t *filter_of_query,
                                 int F, const uint32_t *vis_bits, const int32_t *const *facet_cols,
                                 const int32_t *facet_sizes, int n_facets, uint32_t *out_count, uint32_t *out_facets,
                                 float *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes,
                                 void *stream, int64_t cap_override, unsigned dbg) {
    MMRAG_CHECK_ARG(q && rows && threshold && out_count, "range_scan: null pointer");
    if (int st = check_stored_rows("range_scan", "range-scanned", "scan", ld, dtype, d, &n)) return st;
    MMRAG_CHECK_ARG(n < (1LL << 31), "range_scan: need n < 2^31 (n=%lld)", (long long)n);
    MMRAG_CHECK_ARG(B >= 1, "range_scan: need B >= 1 (B=%d)", B);
    MMRAG_CHECK_ARG(limit >= 0 && limit <= MMRAG_MAX_K_DEEP, "range_scan: limit=%d outside 0..%d", limit,
                    MMRAG_MAX_K_DEEP);
    MMRAG_CHECK_ARG(limit == 0 || (out_scores && out_rows), "range_scan: null hit outputs with limit=%d", limit);
    MMRAG_CHECK_ARG(vis_bits == nullptr || (filter_of_query && F >= 1),
                    "range_scan: vis_bits needs filter_of_query and F >= 1 (F=%d)", F);
    MMRAG_CHECK_ARG(n_facets >= 0 && n_facets <= MMRAG_MAX_FACET_COLUMNS, "range_scan: n_facets=%d outside 0..%d",
                    n_facets, MMRAG_MAX_FACET_COLUMNS);
    MMRAG_CHECK_ARG(n_facets == 0 || (facet_cols && facet_sizes && out_facets), "range_scan: null facet table");
    MMRAG_CHECK_ARG(n_facets != 0 || out_facets == nullptr, "range_scan: out_facets without facet columns");
    RangeParams p;
    long long stride = 0;
    for (int c = 0; c < MMRAG_MAX_FACET_COLUMNS; ++c) {
        p.facet_col[c] = nullptr;
        p.facet_size[c] = 0;
        p.facet_off[c] = 0;
    }
    for (int c = 0; c < n_facets; ++c) {
        MMRAG_CHECK_ARG(facet_cols[c] || n == 0, "range_scan: facet column %d is null", c);
        MMRAG_CHECK_ARG(facet_sizes[c] >= 0 && stride + facet_sizes[c] + 1 < (1LL << 31),
                        "range_scan: facet column %d has %d slots (need >= 0, 2^31 in all)", c, facet_sizes[c]);
        p.facet_col[c] = facet_cols[c];
        p.facet_size[c] = facet_sizes[c];
        p.facet_off[c] = (int)stride;
        stride += (long long)facet_sizes[c] + 1;
    }
    hipStream_t s = (hipStream_t)stream;

    // both tables are zero before the main pass adds to them
    MMRAG_CHECK_HIP(hipMemsetAsync(out_count, 0, (size_t)B * sizeof(unsigned), s));
    if (n_facets > 0) MMRAG_CHECK_HIP(hipMemsetAsync(out_facets, 0, (size_t)B * (size_t)stride * sizeof(unsigned), s));
    if (n == 0) return limit > 0 ? candidate_fill_empty(out_scores, (long long *)out_rows, B, limit, s) : MMRAG_OK;

    p.rows = (const char *)rows;
    p.n = n;
    p.row_bytes = stored_row_bytes(ld, dtype);
    p.nk = stored_k_slabs(d, dtype);
    p.vis = vis_bits;
    p.F = F;
    p.W = filter_words(n);
    p.T = (n + PT - 1) / PT;
    p.items = nullptr;
    p.n_facets = n_facets;
    p.facet_stride = stride;
    unsigned *uni = nullptr;      // with bitmaps: the batch's unions, then one query tile's for a re-run
    const size_t union_bytes = vis_bits != nullptr ? filtered_union_bytes(B, n) : 0;
    const int nqt_all = (B + PT - 1) / PT;
    // the unions of the batch, once for every pass; none without bitmaps
    const auto prepare = [&](char *extra) -> int {
        if (vis_bits == nullptr) return MMRAG_OK;
        uni = (unsigned *)extra;
        return launch_unions(filter_of_query, B, F, vis_bits, p.W, uni, s);
    };
    // queries q0 .. q0 + Bq over `walk` tiles.  The main pass is the one that counts and tabulates; a query produced
    // again alone gets its own unions.  cand_s == null: no candidates are collected.
    const auto produce = [&](ScanPass pass, int q0, int Bq, long long walk, const float *tau, float *cand_s, int *cand_r,
                             unsigned *counts, long long slots) -> int {
        const unsigned *um = uni;
        if (pass == SCAN_PASS_RERUN && uni != nullptr) {
            unsigned *own = uni + (size_t)nqt_all * p.W;
            if (int e = launch_unions(filter_of_query + q0, Bq, F, vis_bits, p.W, own, s)) return e;
            um = own;
        }
        const bool tables = pass == SCAN_PASS_MAIN;
        return for_scan_chunks(Bq, PT, [&](int first, int Bc, int nqt, int t0) -> int {
            RangeParams pc = p;
            const int c0 = q0 + first;
            pc.q = (const char *)q + (size_t)c0 * p.row_bytes;
            pc.filter_of_query = filter_of_query != nullptr ? filter_of_query + c0 : nullptr;
            pc.thr = threshold + c0;
            pc.tau = tau != nullptr ? tau + c0 : nullptr;
            pc.B = Bc;
            pc.nqt = nqt;
            pc.uni = um != nullptr ? um + (size_t)t0 * p.W : nullptr;
            pc.walk = walk;
            pc.out_count = tables ? out_count + c0 : nullptr;
            pc.out_facets = tables && n_facets > 0 ? out_facets + (size_t)c0 * (size_t)stride : nullptr;
            pc.cap = (unsigned)slots;
            pc.cand_s = cand_s != nullptr ? cand_s + (size_t)first * slots : nullptr;
            pc.cand_r = cand_s != nullptr ? cand_r + (size_t)first * slots : nullptr;
            pc.cnt = cand_s != nullptr ? counts + first : nullptr;
            return with_elem_type(dtype, [&](auto tag) { return launch_range_scan<decltype(tag)::value>(pc, s); });
        });
    };

    if (limit == 0) {
        // counts and facets only: one pass, nothing to select, nothing read back; the workspace holds the unions alone
        if (union_bytes > 0 && (!workspace || workspace_bytes < union_bytes)) {
            set_error("range_scan: workspace %zu bytes < required %zu", workspace_bytes, union_bytes);
            return MMRAG_EWORKSPACE;
        }
        if (union_bytes > 0 && ((uintptr_t)workspace % 16) != 0) {
            set_error("range_scan: workspace must be 16-byte aligned");
            return MMRAG_EWORKSPACE;
        }
        if (int e = prepare((char *)workspace)) return e;
        return produce(SCAN_PASS_MAIN, 0, B, p.T, nullptr, nullptr, nullptr, nullptr, 0);
    }
    // Hits are a top-`limit`: the bounded sequence with tau starting at the threshold.  Bound passes raise tau_q to the
    // limit-th best visible sampled score above it; re-runs keep tau_q and touch no table.
    return bounded_scan_select("range_scan", B, n, limit, cap_override, (dbg & FI_DBG_NO_BOUND) != 0u, row_offset,
                               threshold, out_scores, (long long *)out_rows, workspace, workspace_bytes, union_bytes, s,
                               prepare, produce);
}

int mmrag_range_scan(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype,
                     const float *threshold, int limit, int64_t row_offset, const int32_t *filter_of_query, int F,
                     const uint32_t *vis_bits, const int32_t *const *facet_cols, const int32_t *facet_sizes, int n_facets,
                     uint32_t *out_count, uint32_t *out_facets, float *out_scores, int64_t *out_rows, void *workspace,
                     size_t workspace_bytes, void *stream) {
    return mmrag_internal_range_scan_ex(q, rows, B, n, d, ld, dtype, threshold, limit, row_offset, filter_of_query, F,
                                        vis_bits, facet_cols, facet_sizes, n_facets, out_count, out_facets, out_scores,
                                        out_rows, workspace, workspace_bytes, stream, 0, 0u);
}

}  // extern "C"
