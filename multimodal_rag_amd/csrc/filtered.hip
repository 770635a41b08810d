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
//      filter (tau_q stays -inf while fewer than k visible rows were sampled).  Stages as boosted.hip plans them.
//   3. select and overflow: candidate_select.h's driver, unchanged.
// The K order is slab_step's, so a score's bits depend on the query row, the stored row and d alone and equal
// mmrag_scoped_topk's: not on the batch, the filters, the grid, tau or whether bound passes ran.
#include "candidate_select.h"
#include "pair_tile.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int FI_MAX_QT = 64;            // query tiles of one scan launch: their "wanted" flags are one 64-bit mask
constexpr int FI_SAMPLE0_TILES = 96;     // first bound sample: 12288 rows, the select's LDS key cache
constexpr int FI_MAX_STAGES = 8;
constexpr int FE_THREADS = 256;          // rows of a filter_eval workgroup

// debug switches of mmrag_internal_filtered_topk_ex (tests only)
constexpr unsigned FI_DBG_NO_BOUND = 1u;  // no bound passes: tau = -inf, every visible row survives the main pass

inline long long filter_words(long long n) { return 4 * ((n + PT - 1) / PT); }

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

// ---- the masked scan ----------------------------------------------------------------------------------------------
struct FilteredParams {
    const char *rows;
    const char *q;
    long long n;
    int B;
    unsigned row_bytes;     // ld * element size, of the rows and of the queries
    int nk;                 // K-slabs that hold the d logical columns
    int nqt;                // query tiles, <= FI_MAX_QT
    const unsigned *uni;    // [nqt, W]: the union bitmaps of this launch's query tiles
    const unsigned *vis;    // [F, W]
    const int *filter_of_query;
    int F;
    long long W;
    const float *tau;       // [B], or null: -inf
    float *cand_s;
    int *cand_r;
    unsigned *cnt;
    unsigned cap;
    long long T;            // row tiles of the collection
    long long walk;         // tiles this launch visits: tile i * T / walk for i in 0 .. walk (walk == T: every tile)
    unsigned long long *items;   // optional: += the (row tile, query tile) items this launch issues
};

struct FilteredPlan {
    long long cap;          // candidate slots per query
    int n_stages;
    long long stage_tiles[FI_MAX_STAGES];
};

// boosted.hip's make_boosted_plan: the argument there (survivors ~ k n / m for a bound from m sampled rows) holds for the
// visible rows of any filter, with fewer survivors the fewer rows a filter passes.
FilteredPlan make_filtered_plan(long long n, int k, long long cap_override, unsigned dbg) {
    FilteredPlan pl;
    const long long C = candidate_capacity(k);
    pl.cap = cap_override > 0 && cap_override < C ? cap_override : C;
    pl.n_stages = 0;
    if (n <= C || (dbg & FI_DBG_NO_BOUND)) return pl;   // every row fits: no bound needed
    const long long n_tiles = (n + PT - 1) / PT;
    const long long target_rows = (4LL * k * n + C - 1) / C;
    const long long target = (target_rows + PT - 1) / PT;
    long long t = FI_SAMPLE0_TILES < n_tiles ? FI_SAMPLE0_TILES : n_tiles;
    for (;;) {
        pl.stage_tiles[pl.n_stages++] = t;
        if (t >= target || pl.n_stages == FI_MAX_STAGES) break;
        long long nt = t * C / (4LL * k);
        if (nt > target) nt = target;
        if (nt > n_tiles) nt = n_tiles;
        if (nt <= t) break;
        t = nt;
    }
    return pl;
}

// uni[qt, :] = OR of vis[f, :] over the filters f of queries 128 qt .. 128 qt + 127 (a run of equal filters is read
// once; a filter outside 0..F-1 sees nothing, here and in the scan).  Grid (words / 256, query tiles).
__global__ __launch_bounds__(256) void filtered_union_kernel(const int *__restrict__ filter_of_query, int B, int F,
                                                             const unsigned *__restrict__ vis, long long W,
                                                             unsigned *__restrict__ uni) {
    __shared__ int list[PT];
    __shared__ int n_list;
    const int qt = blockIdx.y;
    if (threadIdx.x == 0) {
        int m = 0, prev = -1;
        const int hi = B - qt * PT < PT ? B - qt * PT : PT;
        for (int i = 0; i < hi; ++i) {
            const int f = filter_of_query[qt * PT + i];
            if ((unsigned)f >= (unsigned)F || f == prev) continue;
            prev = f;
            list[m++] = f;
        }
        n_list = m;
    }
    __syncthreads();
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w >= W) return;
    unsigned acc = 0;
    for (int i = 0; i < n_list; ++i) acc |= vis[(size_t)list[i] * W + w];
    uni[(size_t)qt * W + w] = acc;
}

template <int DT>
__global__ __launch_bounds__(256, 2) void filtered_scan_kernel(const FilteredParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];

    const unsigned RB = p.row_bytes;
    const PairTileCtx c = pair_tile_ctx(threadIdx.x, RB, smem);
    const int wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;
    const int nk = p.nk, nqt = p.nqt;
    const long long W = p.W;

    for (long long i = blockIdx.x; i < p.walk; i += gridDim.x) {
        const long long tile = i * p.T / p.walk;      // < T
        const long long row0 = tile * PT;
        const long long left = p.n - row0;            // >= 1
        const int in_tile = left < PT ? (int)left : PT;
        // the tile's rows below n, per bitmap word: a bitmap from elsewhere may hold bits at and past n
        unsigned vm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cnt = in_tile - 32 * j;
            vm[j] = cnt >= 32 ? ~0u : (cnt <= 0 ? 0u : (1u << cnt) - 1u);
        }
        // bit qt: the item (this row tile, query tile qt) has a visible row.  Every lane of every wave reads the same
        // words, so this is the same scalar in all four waves
        const unsigned *const uw = p.uni + 4 * tile;
        unsigned long long active = 0;
        for (int qt = 0; qt < nqt; ++qt) {
            const unsigned *u = uw + (size_t)qt * W;
            if (((u[0] & vm[0]) | (u[1] & vm[1]) | (u[2] & vm[2]) | (u[3] & vm[3])) != 0u) active |= 1ull << qt;
        }
        active = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(active >> 32)) << 32) |
                 (unsigned)__builtin_amdgcn_readfirstlane((unsigned)active);
        // uniform: the whole workgroup takes this path; nothing was fetched, no LDS is touched
        if (active == 0ull) continue;
        if (p.items != nullptr && threadIdx.x == 0) atomicAdd(p.items, (unsigned long long)__popcll(active));

        const char *const rows_base = p.rows + (size_t)row0 * RB;
        const unsigned rows_bytes = (unsigned)in_tile * RB;
        const int total = nk * __popcll(active);
        unsigned long long i_left = active;
        int issued = 0, i_ks = 0;
        auto issue = [&]() {
            // ring item `issued` = K-slab i_ks of (this row tile, the lowest query tile left in i_left)
            const int qt = __builtin_ctzll(i_left);
            const int q_left = p.B - qt * PT;
            const char *base = wave < 2 ? rows_base : p.q + (size_t)qt * PT * RB;
            const unsigned bytes = wave < 2 ? rows_bytes : (unsigned)(q_left < PT ? q_left : PT) * RB;
            pair_tile_issue(c, make_rsrc(base, bytes), issued % PT_NSTAGE, i_ks);
            ++issued;
            if (++i_ks == nk) {
                i_ks = 0;
                i_left &= i_left - 1;
            }
        };

        // this wave's 64 rows below n
        const unsigned long long valid = ((unsigned long long)vm[2 * wm + 1] << 32) | vm[2 * wm];
        f32x4_t acc[4][4];
        pair_tile_clear(acc);
        unsigned long long c_left = active;
        issue();
        int ks = 0;
        for (int it = 0; it < total; ++it) {
            wait_vmcnt<0>();     // two stages: item `it` is the only one in flight
            __builtin_amdgcn_s_barrier();
            if (issued < total) issue();
            slab_step<DT>(smem + (it % PT_NSTAGE) * PT_STAGE, c, acc);
            if (++ks < nk) continue;
            // ---- the query tile is complete: acc[a][b][r] = <row wm*64 + 16a + 4 g4 + r, query col0 + 16b>
            ks = 0;
            const int qt = __builtin_ctzll(c_left);
            c_left &= c_left - 1;
            const unsigned *const uq = uw + (size_t)qt * W + 2 * wm;
            const unsigned long long mw = (((unsigned long long)uq[1] << 32) | uq[0]) & valid;
            if (mw != 0ull) {      // some query of the tile sees one of this wave's rows
                const int lrow0 = (int)row0 + wm * 64 + 4 * g4;      // n < 2^31 (the entry point's check)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int col = qt * PT + wn * 64 + 16 * b + c16;
                    if (col >= p.B) continue;
                    const int f = p.filter_of_query[col];
                    if ((unsigned)f >= (unsigned)p.F) continue;
                    const unsigned *const vq = p.vis + (size_t)f * W + 4 * tile + 2 * wm;
                    const unsigned long long mv = (((unsigned long long)vq[1] << 32) | vq[0]) & valid;
                    // this lane's 16 rows: bit 4a + r of `vis` = row 16a + 4 g4 + r of the wave's 64 is visible
                    unsigned vis = 0;
#pragma unroll
                    for (int a = 0; a < 4; ++a) vis |= (unsigned)((mv >> (16 * a + 4 * g4)) & 15ull) << (4 * a);
                    if (vis == 0u) continue;
                    const float t = p.tau != nullptr ? p.tau[col] : NEG_INF;
                    unsigned hit = 0;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r) hit |= (unsigned)(acc[a][b][r] >= t) << (4 * a + r);
                    hit &= vis;
                    if (hit == 0u) continue;
                    // reserve the slots with one returning atomic; the counter keeps the true count, slots at or past
                    // cap are not written
                    unsigned at = atomicAdd(p.cnt + col, (unsigned)__popc(hit));
                    float *bs = p.cand_s + (size_t)col * p.cap;
                    int *br = p.cand_r + (size_t)col * p.cap;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if ((hit >> (4 * a + r)) & 1u) {
                                if (at < p.cap) {
                                    bs[at] = acc[a][b][r];
                                    br[at] = lrow0 + 16 * a + r;
                                }
                                ++at;
                            }
                }
            }
            pair_tile_clear(acc);
        }
        __syncthreads();   // every wave is done with the ring before the next tile's first slab lands
    }
#endif
}

template <int DT>
int launch_scan(const FilteredParams &p, hipStream_t s) {
    long long g = 2LL * num_cus();    // persistent grid: two workgroups per CU (the LDS allows two)
    if (g > p.walk) g = p.walk;
    hipLaunchKernelGGL(filtered_scan_kernel<DT>, dim3((unsigned)g), dim3(256), 0, s, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

// the union bitmaps: one per query tile of the batch and one for a re-run
inline size_t filtered_union_bytes(int B, long long n) {
    return align_up(((size_t)(B + PT - 1) / PT + 1) * (size_t)filter_words(n) * sizeof(unsigned), 256);
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
    return candidate_ws_layout(B, candidate_capacity(k), n, true).total + filtered_union_bytes(B, n);
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

    const FilteredPlan pl = make_filtered_plan(n, k, cap_override, dbg);
    const CandWs wl = candidate_ws_layout(B, pl.cap, n, true);
    const size_t need = wl.total + filtered_union_bytes(B, n);
    if (!workspace || workspace_bytes < need) {
        set_error("filtered_topk: workspace %zu bytes < required %zu", workspace_bytes, need);
        return MMRAG_EWORKSPACE;
    }
    if (((uintptr_t)workspace % 16) != 0) {
        set_error("filtered_topk: workspace must be 16-byte aligned");
        return MMRAG_EWORKSPACE;
    }

    char *ws = (char *)workspace;
    unsigned *cnt = (unsigned *)(ws + wl.off_cnt);
    float *tau = (float *)(ws + wl.off_floats);
    unsigned *uni = (unsigned *)(ws + wl.total);
    FilteredParams p;
    p.rows = (const char *)rows;
    p.q = (const char *)q;
    p.n = n;
    p.B = B;
    p.row_bytes = stored_row_bytes(ld, dtype);
    p.nk = stored_k_slabs(d, dtype);
    p.nqt = 0;
    p.uni = uni;
    p.vis = vis_bits;
    p.filter_of_query = filter_of_query;
    p.F = F;
    p.W = filter_words(n);
    p.tau = nullptr;
    p.cand_s = (float *)(ws + wl.off_bs);
    p.cand_r = (int *)(ws + wl.off_br);
    p.cnt = cnt;
    p.cap = (unsigned)pl.cap;
    p.T = (n + PT - 1) / PT;
    p.walk = p.T;
    p.items = nullptr;
    const int nqt_all = (B + PT - 1) / PT;
    const unsigned wblocks = (unsigned)((p.W + 255) / 256);

    // the unions of queries q0 .. q0 + Bq of the caller's batch into um[0 .. ceil(Bq / 128))
    const auto unions = [&](int q0, int Bq, unsigned *um) -> int {
        const int tiles = (Bq + PT - 1) / PT;
        for (int t0 = 0; t0 < tiles; t0 += FI_MAX_QT) {
            const int nt = tiles - t0 < FI_MAX_QT ? tiles - t0 : FI_MAX_QT;
            hipLaunchKernelGGL(filtered_union_kernel, dim3(wblocks, (unsigned)nt), dim3(256), 0, s,
                               filter_of_query + q0 + t0 * PT, Bq - t0 * PT, F, vis_bits, p.W, um + (size_t)t0 * p.W);
            MMRAG_CHECK_HIP(hipGetLastError());
        }
        return MMRAG_OK;
    };
    // queries q0 .. q0 + Bq over `walk` tiles into their slots, their unions in um: scans of at most FI_MAX_QT query
    // tiles each
    const auto produce = [&](int q0, int Bq, long long walk, const unsigned *um, float *cand_s, int *cand_r,
                             unsigned *counts, long long slots, unsigned long long *items) -> int {
        const int tiles = (Bq + PT - 1) / PT;
        for (int t0 = 0; t0 < tiles; t0 += FI_MAX_QT) {
            FilteredParams pc = p;
            const int c0 = q0 + t0 * PT;
            pc.q = p.q + (size_t)c0 * p.row_bytes;
            pc.filter_of_query = filter_of_query + c0;
            pc.tau = p.tau != nullptr ? p.tau + c0 : nullptr;
            pc.B = Bq - t0 * PT < FI_MAX_QT * PT ? Bq - t0 * PT : FI_MAX_QT * PT;
            pc.nqt = (pc.B + PT - 1) / PT;
            pc.uni = um + (size_t)t0 * p.W;
            pc.walk = walk;
            pc.cap = (unsigned)slots;
            pc.cand_s = cand_s + (size_t)(t0 * PT) * slots;
            pc.cand_r = cand_r + (size_t)(t0 * PT) * slots;
            pc.cnt = counts + t0 * PT;
            pc.items = items;
            if (int st = with_elem_type(dtype, [&](auto tag) { return launch_scan<decltype(tag)::value>(pc, s); }))
                return st;
        }
        return MMRAG_OK;
    };

    // 1. the unions of the batch, once for every pass
    if (int e = unions(0, B, uni)) return e;
    // 2. bound passes (tau starts at -inf: the bit pattern 0xff800000)
    if (pl.n_stages > 0) {
        MMRAG_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)tau, (int)0xff800000u, (size_t)B, s));
        p.tau = tau;
    }
    for (int st = 0; st < pl.n_stages; ++st) {
        MMRAG_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)B * sizeof(unsigned), s));
        if (int e = produce(0, B, pl.stage_tiles[st], uni, p.cand_s, p.cand_r, cnt, pl.cap, nullptr)) return e;
        deep_select_kernel<<<B, SEL_THREADS, 0, s>>>(p.cand_s, p.cand_r, cnt, pl.cap, k, 0, 1, nullptr, nullptr, tau);
        MMRAG_CHECK_HIP(hipGetLastError());
    }
    if (items_issued) MMRAG_CHECK_HIP(hipMemsetAsync(items_issued, 0, sizeof(uint64_t), s));
    // 3. main pass over every tile, select, and each query with more survivors than slots alone, same tau_q
    return candidate_select(
        "filtered_topk", B, n, pl.cap, k, row_offset, out_scores, (long long *)out_rows, ws, wl, s,
        [&](float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return produce(0, B, p.T, uni, cand_s, cand_r, counts, slots, (unsigned long long *)items_issued);
        },
        [&](int qi, float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            unsigned *um = uni + (size_t)nqt_all * p.W;
            if (int e = unions(qi, 1, um)) return e;
            return produce(qi, 1, p.T, um, cand_s, cand_r, counts, slots, nullptr);
        });
}

int mmrag_filtered_topk(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                        int64_t row_offset, const int32_t *filter_of_query, int F, const uint32_t *vis_bits,
                        float *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream) {
    return mmrag_internal_filtered_topk_ex(q, rows, B, n, d, ld, dtype, k, row_offset, filter_of_query, F, vis_bits,
                                           out_scores, out_rows, workspace, workspace_bytes, stream, 0, 0u, nullptr);
}

}  // extern "C"
