// The host sequence around deep_select.h's select, shared by the deep top-k (search_deep.hip) and the BM25 search
// (lexical.hip): a producer appends (score, local row) candidates to B x cap slots and counts them per query, the select
// turns each query's slots into its sorted top-k, and a query whose candidates overflowed its slots is produced again
// alone into n slots.  The callers supply the two producer launches.
// For the scans over 128-row tiles (boosted.hip, filtered.hip, range.hip, recommend.hip) the whole bounded sequence is
// here as well, once: bounded_scan_select owns the plan, the workspace layout and its checks, the tau start, the bound
// stages and the call of candidate_select, and takes ONE producer; the *_workspace_bytes functions size themselves by
// its bounded_scan_layout.  for_scan_chunks cuts a batch into launches of at most SCAN_MAX_TILES column tiles for every
// scan that has such a limit.  Internal, gfx950 only.
#pragma once
#include "deep_select.h"

#include <stdlib.h>

namespace mmrag_impl {

namespace {

// candidate slots per query for a top-k of k: 32 k, at least 16384, in whole 256s
inline long long candidate_capacity(int k) {
    return (long long)mmrag::align_up((size_t)(32LL * k > 16384 ? 32LL * k : 16384), 256);
}

// ---- the bound stages of a scan over 128-row tiles (boosted.hip, filtered.hip, range.hip, recommend.hip) -------------
constexpr int BOUND_TILE_ROWS = 128;     // pair_tile.h's PT
constexpr int BOUND_SAMPLE0_TILES = 96;  // first bound sample: 12288 rows, the select's LDS key cache
constexpr int BOUND_MAX_STAGES = 8;

struct BoundPlan {
    long long cap;          // candidate slots per query
    int n_stages;
    long long stage_tiles[BOUND_MAX_STAGES];
};

// search_deep.hip's make_deep_plan in 128-row tiles: a scan first runs over a strided sample of whole tiles (stage i
// visits stage_tiles[i] of them) and deep_select_kernel's bound mode raises tau_q to the k-th best sampled score; the
// k-th best of ANY subset of a query's candidates is at most its true k-th, whatever a prior, a filter or a score
// function does, so the plan is the same for all of them.  The stages are planned against the capacity of k itself: a
// smaller cap_override (tests) only makes the slots fewer, so that queries overflow.  `no_bound`: no stages (tests).
inline BoundPlan make_bound_plan(long long n, int k, long long cap_override, bool no_bound) {
    BoundPlan pl;
    const long long C = candidate_capacity(k);
    pl.cap = cap_override > 0 && cap_override < C ? cap_override : C;
    pl.n_stages = 0;
    if (n <= C || no_bound) return pl;   // every row fits: no bound needed
    const long long n_tiles = (n + BOUND_TILE_ROWS - 1) / BOUND_TILE_ROWS;
    // main-pass survivors ~ k * n / m for a bound from m sampled rows: aim at C / 4
    const long long target_rows = (4LL * k * n + C - 1) / C;
    const long long target = (target_rows + BOUND_TILE_ROWS - 1) / BOUND_TILE_ROWS;
    long long t = BOUND_SAMPLE0_TILES < n_tiles ? BOUND_SAMPLE0_TILES : n_tiles;
    for (;;) {
        pl.stage_tiles[pl.n_stages++] = t;
        if (t >= target || pl.n_stages == BOUND_MAX_STAGES) break;
        // the next sample's survivors ~ k * m' / m must fit C / 4 as well
        long long nt = t * C / (4LL * k);
        if (nt > target) nt = target;
        if (nt > n_tiles) nt = n_tiles;
        if (nt <= t) break;
        t = nt;
    }
    return pl;
}

struct CandWs {
    size_t off_cnt, off_one_cnt, off_floats, off_bs, off_br, off_os, off_or, total;
};

// The B counters stay first (off_cnt == 0) and the driver leaves the main pass's counts in them: the re-run has its own
// counter.  tools/boost_bench.py and tools/recommend_bench.py read the survivors per query from there.
// [B counters | the re-run's counter | B floats, if asked for | B x cap scores | B x cap rows | n scores | n rows],
// every block on a 256-byte boundary
inline CandWs candidate_ws_layout(int B, long long cap, long long n, bool per_query_floats) {
    CandWs w;
    w.off_cnt = 0;
    w.off_one_cnt = mmrag::align_up((size_t)B * sizeof(unsigned), 256);
    w.off_floats = w.off_one_cnt + 256;
    w.off_bs = mmrag::align_up(w.off_floats + (per_query_floats ? (size_t)B * sizeof(float) : 0), 256);
    w.off_br = mmrag::align_up(w.off_bs + (size_t)B * cap * sizeof(float), 256);
    // one query x n slots: the re-run of an overflowed query
    w.off_os = mmrag::align_up(w.off_br + (size_t)B * cap * sizeof(int), 256);
    w.off_or = mmrag::align_up(w.off_os + (size_t)n * sizeof(float), 256);
    w.total = mmrag::align_up(w.off_or + (size_t)n * sizeof(int), 256);
    return w;
}

// The buffers of a bound stage: candidate_capacity(k) slots per query, what the stages were planned against, whatever
// cap_override says.  The override (tests) makes the MAIN pass's slots fewer, so that queries overflow and are produced
// again under the tau the stages found; a stage that appended into fewer than k slots could never hold k candidates
// and would leave tau where it started.  Counters and per-query floats lie where the main pass's layout has them (they
// do not depend on the slots), the scores start at the same offset, and a stage is over before the main pass begins:
// a call with stages needs the larger of the two layouts, which is what the *_workspace_bytes functions return.
inline CandWs bound_stage_layout(int B, int k, long long n, const CandWs &main_layout, size_t *total) {
    const CandWs w = candidate_ws_layout(B, candidate_capacity(k), n, true);
    *total = w.total > main_layout.total ? w.total : main_layout.total;
    return w;
}

// every output (-inf, -1): an empty collection, or nothing that can match
inline int candidate_fill_empty(float *out_s, long long *out_r, int B, int k, hipStream_t s) {
    const long long total = (long long)B * k;
    deep_fill_empty_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(out_s, out_r, total);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

// out_s / out_r [B, k] = each query's top-k (score desc, row + row_offset; (-inf, -1) padded) of what the producers
// append.  `ws` is laid out by candidate_ws_layout(B, cap, n, ...).  Both launchers return a status:
//   launch_batch(cand_s, cand_r, cnt, cap)     all B queries: query b into slots [b * cap, (b + 1) * cap), count in cnt[b]
//   launch_one(qi, cand_s, cand_r, cnt, cap)   query qi alone into slots [0, cap = n), count in cnt[0]
// A counter keeps the TRUE number of candidates; appends past cap are dropped.  The counters are read on the host
// once (the call's only stream synchronisation; none when n <= cap, where nothing can overflow), and since a query
// has at most n candidates its re-run fits on the first try.  `name` is the entry point, for error texts.
template <typename LaunchBatch, typename LaunchOne>
int candidate_select(const char *name, int B, long long n, long long cap, int k, long long row_offset, float *out_s,
                     long long *out_r, char *ws, const CandWs &wl, hipStream_t s, LaunchBatch &&launch_batch,
                     LaunchOne &&launch_one) {
    unsigned *cnt = (unsigned *)(ws + wl.off_cnt), *one_cnt = (unsigned *)(ws + wl.off_one_cnt);
    float *bs = (float *)(ws + wl.off_bs), *os = (float *)(ws + wl.off_os);
    int *br = (int *)(ws + wl.off_br), *orr = (int *)(ws + wl.off_or);
    MMRAG_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)B * sizeof(unsigned), s));
    if (int st = launch_batch(bs, br, cnt, cap)) return st;
    deep_select_kernel<<<B, SEL_THREADS, 0, s>>>(bs, br, cnt, cap, k, row_offset, 0, out_s, out_r, nullptr);
    MMRAG_CHECK_HIP(hipGetLastError());
    if (n <= cap) return MMRAG_OK;   // no query can have more than n candidates

    struct HostCounts {
        unsigned *v;
        ~HostCounts() { free(v); }
    } host = {(unsigned *)malloc((size_t)B * sizeof(unsigned))};
    if (!host.v) {
        mmrag::set_error("%s: out of host memory", name);
        return MMRAG_EHIP;
    }
    hipError_t e = hipMemcpyAsync(host.v, cnt, (size_t)B * sizeof(unsigned), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        mmrag::set_error("%s: reading the candidate counts failed: %s", name, hipGetErrorString(e));
        return MMRAG_EHIP;
    }
    for (int qi = 0; qi < B; ++qi) {
        if (host.v[qi] <= (unsigned)cap) continue;
        e = hipMemsetAsync(one_cnt, 0, sizeof(unsigned), s);
        if (e == hipSuccess) {
            if (int st = launch_one(qi, os, orr, one_cnt, n)) return st;
            deep_select_kernel<<<1, SEL_THREADS, 0, s>>>(os, orr, one_cnt, n, k, row_offset, 0, out_s + (size_t)qi * k,
                                                         out_r + (size_t)qi * k, nullptr);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            mmrag::set_error("%s: overflow re-run failed: %s", name, hipGetErrorString(e));
            return MMRAG_EHIP;
        }
    }
    return MMRAG_OK;
}

// ---- the launches of a scan over 128-row tiles ----------------------------------------------------------------------
// Column tiles (128 rows of the batch side) of one scan launch: a kernel keeps their "wanted" flags in one 64-bit mask
constexpr int SCAN_MAX_TILES = 64;

// Bq batch entries, `per_tile` of them to a column tile (128 queries; 8 recommend requests of 16 example rows), as
// launches of at most SCAN_MAX_TILES column tiles: launch(first entry of the chunk, its entries, its column tiles, its
// first column tile) returns a status
template <typename Launch>
inline int for_scan_chunks(int Bq, int per_tile, Launch &&launch) {
    const int tiles = (Bq + per_tile - 1) / per_tile;
    for (int t0 = 0; t0 < tiles; t0 += SCAN_MAX_TILES) {
        const int first = t0 * per_tile;
        const int Bc = Bq - first < SCAN_MAX_TILES * per_tile ? Bq - first : SCAN_MAX_TILES * per_tile;
        if (int st = launch(first, Bc, (Bc + per_tile - 1) / per_tile, t0)) return st;
    }
    return MMRAG_OK;
}

// ---- the bounded scan: plan, workspace, bound stages, main pass, select, overflow re-runs ---------------------------
struct BoundedScanWs {
    BoundPlan pl;
    CandWs main, stage;     // the main pass's blocks (pl.cap slots) and a bound stage's (stage_cap slots)
    long long stage_cap;
    size_t select_bytes;    // what the two need; the caller's extra bytes lie behind them
};

// cap_override == 0 and !no_bound give the public size: candidate_capacity(k) slots, which no call exceeds
inline BoundedScanWs bounded_scan_layout(int B, long long n, int k, long long cap_override, bool no_bound) {
    BoundedScanWs l;
    l.pl = make_bound_plan(n, k, cap_override, no_bound);
    l.main = candidate_ws_layout(B, l.pl.cap, n, true);
    l.select_bytes = l.main.total;
    l.stage = l.pl.n_stages > 0 ? bound_stage_layout(B, k, n, l.main, &l.select_bytes) : l.main;
    l.stage_cap = l.pl.n_stages > 0 ? candidate_capacity(k) : l.pl.cap;
    return l;
}

enum ScanPass { SCAN_PASS_BOUND, SCAN_PASS_MAIN, SCAN_PASS_RERUN };

// Everything of a bounded top-k scan between "arguments checked, n > 0" and the caller's finish kernel (boosted.hip,
// filtered.hip, range.hip, recommend.hip): out_s / out_r [B, k] = each query's top-k of what `produce` appends.
//   1. the plan (make_bound_plan) and the workspace [select_bytes | extra_bytes of the caller's], checked: too small or
//      not 16-byte aligned is MMRAG_EWORKSPACE under `name`;
//   2. prepare(the caller's extra bytes) -> status, once, before any pass (union bitmaps; nothing for most);
//   3. with stages: tau_q starts at tau_init[q] (null: -inf), and each stage zeroes the counters, produces over its
//      sample of tiles into the stage's slots and raises tau_q to the k-th best of them (deep_select_kernel's bound mode);
//   4. candidate_select: the main pass over all T tiles, the select, and each overflowed query alone into n slots.
//   produce(pass, q0, Bq, walk, tau, cand_s, cand_r, counts, slots) -> status
// appends, for queries q0 .. q0 + Bq of the batch over `walk` tiles, every (score, local row) at or above tau[q]
// (`tau`: the B floats of the whole batch, null without stages: the caller's own floor) to query q's slots
// cand_s / cand_r [(q - q0) * slots ..), counting in counts[q - q0].  `pass` says which of the three callers it is: what
// only the main pass may do (count, tabulate) and what a re-run needs (its own unions) hang on it.
template <typename Prepare, typename Produce>
int bounded_scan_select(const char *name, int B, long long n, int k, long long cap_override, bool no_bound,
                        long long row_offset, const float *tau_init, float *out_s, long long *out_r, void *workspace,
                        size_t workspace_bytes, size_t extra_bytes, hipStream_t s, Prepare &&prepare,
                        Produce &&produce) {
    const BoundedScanWs l = bounded_scan_layout(B, n, k, cap_override, no_bound);
    const size_t need = l.select_bytes + extra_bytes;
    if (!workspace || workspace_bytes < need) {
        mmrag::set_error("%s: workspace %zu bytes < required %zu", name, workspace_bytes, need);
        return MMRAG_EWORKSPACE;
    }
    if (((uintptr_t)workspace % 16) != 0) {
        mmrag::set_error("%s: workspace must be 16-byte aligned", name);
        return MMRAG_EWORKSPACE;
    }
    char *ws = (char *)workspace;
    unsigned *cnt = (unsigned *)(ws + l.main.off_cnt);
    float *tau = nullptr;
    if (int e = prepare(ws + l.select_bytes)) return e;

    if (l.pl.n_stages > 0) {
        tau = (float *)(ws + l.main.off_floats);
        if (tau_init != nullptr)
            MMRAG_CHECK_HIP(hipMemcpyAsync(tau, tau_init, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, s));
        else      // -inf: the bit pattern 0xff800000
            MMRAG_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)tau, (int)0xff800000u, (size_t)B, s));
    }
    float *st_s = (float *)(ws + l.stage.off_bs);
    int *st_r = (int *)(ws + l.stage.off_br);
    for (int st = 0; st < l.pl.n_stages; ++st) {
        MMRAG_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)B * sizeof(unsigned), s));
        if (int e = produce(SCAN_PASS_BOUND, 0, B, l.pl.stage_tiles[st], (const float *)tau, st_s, st_r, cnt, l.stage_cap))
            return e;
        deep_select_kernel<<<B, SEL_THREADS, 0, s>>>(st_s, st_r, cnt, l.stage_cap, k, 0, 1, nullptr, nullptr, tau);
        MMRAG_CHECK_HIP(hipGetLastError());
    }
    const long long T = (n + BOUND_TILE_ROWS - 1) / BOUND_TILE_ROWS;
    return candidate_select(
        name, B, n, l.pl.cap, k, row_offset, out_s, out_r, ws, l.main, s,
        [&](float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return produce(SCAN_PASS_MAIN, 0, B, T, (const float *)tau, cand_s, cand_r, counts, slots);
        },
        [&](int qi, float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return produce(SCAN_PASS_RERUN, qi, 1, T, (const float *)tau, cand_s, cand_r, counts, slots);
        });
}

}  // namespace

}  // namespace mmrag_impl
