// Fused cosine GEMM + top-k for gfx950 (MI355X): the retrieve half of the hot path.
//
// Replaces chromadb's collection.query (reference call site app/utils/embedder.py:595-601)
// with an exact search:  S = corpus . Q^T  on the matrix cores, top-k selected in the GEMM
// epilogue, so the [B, n] score matrix never exists in HBM.
//
// Shape of the computation (DESIGN.md "search kernel"):
//   * persistent grid: one 512-thread workgroup per CU walks corpus tiles of 256 rows
//     (tile = blockIdx.x + i * gridDim.x); HBM traffic = the corpus, read exactly once;
//   * K is streamed in 128-byte slabs (64 fp16 / 32 fp32 per row) through an NSTAGE-deep
//     LDS ring filled by LDS-DMA (`buffer_load_dwordx4 ... lds`, bounds-checked by the
//     buffer descriptor so ragged tiles read zeros); the query slab rides along (L2-resident);
//   * LDS rows are 128 B; the 16-byte chunk index is XOR-swizzled with (row>>1)&7 on the
//     DMA *source* address and on the ds_read_b128 address (conflict-free fragment reads);
//   * MFMA orientation D[corpus row][query] = A(corpus) x B(Q^T): the query sits on the
//     lane (col = lane & 31), corpus rows sit in the 16 accumulator registers, so top-k
//     selection per query is lane-local register work with no cross-lane traffic;
//   * NW waves = WM x WN (8 waves, or 16 = 4 per SIMD for the 256-query shape: the extra waves
//     hide LDS-read and barrier latency); each wave owns 32 queries x (256/WM) corpus rows;
//   * selection: each lane keeps a sorted K-list (score desc) for its query over the rows it
//     sees; an element enters only if it beats a running threshold (k-th best of the union
//     of the two half-wave lists of that query) -- after the first tiles almost nothing does;
//   * masked / out-of-range rows start their accumulator at -inf, so they cost nothing in
//     the epilogue;
//   * every lane list is written once at kernel end; a second tiny kernel merges the
//     gridDim.x * WM * 2 lists per query into the final [B, k] (ties -> lower row).
//   * K = 0 is the filter mode of the deep top-k (search_deep.hip): no lists; the epilogue appends
//     every score >= thr0[q] to a per-query buffer, one returning atomic per lane per tile.
//
// The kernel's body is slab_ring_body.inc, included textually here and by the FP8 kernel of search_f8.hip (its
// differences sit in the body behind `if constexpr (DT == MMRAG_F8E4M3)`); slab_ring.h holds what both units share.
#include "slab_ring.h"

#include <stdlib.h>

using namespace mmrag;

namespace mmrag_impl {

template <int DT, int WN, int K, int NSTAGE, int NW, bool SEEDED>
__global__ __launch_bounds__(64 * NW, NW / 4) void cosine_topk_kernel(const KParams p) {
#if defined(__HIP_DEVICE_COMPILE__)  // amdgcn builtins below: the host pass only needs the launch stub
#include "slab_ring_body.inc"
#endif  // __HIP_DEVICE_COMPILE__
}

// ---------------------------------------------------------------------------------------------
// merge: per query, reduce `n_cand` (score, row) candidates to the top-k under (score desc,
// row asc).  One 256-thread workgroup per query.  Candidate c of query q lives at
//   (c / inner) * outer_stride + q * q_stride + (c % inner)
// which covers both the kernel's [B, n_lists*K] lists (inner = n_cand) and an all-gathered
// [G, B, k] block (inner = k, outer_stride = B*k, q_stride = k).
// ---------------------------------------------------------------------------------------------
template <int K>
struct FullList {
    float v[K];
    long long r[K];
    __device__ inline void init() {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            v[i] = NEG_INF;
            r[i] = LLONG_MAX;
        }
    }
    __device__ inline void insert(float x, long long xr) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const bool b = better(x, xr, v[j], r[j]);
            const float nv = b ? x : v[j];
            const float nx = b ? v[j] : x;
            const long long nr = b ? xr : r[j];
            const long long nxr = b ? r[j] : xr;
            v[j] = nv;
            x = nx;
            r[j] = nr;
            xr = nxr;
        }
    }
    __device__ inline void pop() {
#pragma unroll
        for (int j = 0; j + 1 < K; ++j) {
            v[j] = v[j + 1];
            r[j] = r[j + 1];
        }
        v[K - 1] = NEG_INF;
        r[K - 1] = LLONG_MAX;
    }
};

// K rounds of wave-wide arg-best over the lanes' list heads; lane 0 receives the results
template <int K>
__device__ inline void wave_extract(FullList<K> &l, float *out_v, long long *out_r) {
#pragma unroll
    for (int round = 0; round < K; ++round) {
        float s = l.v[0];
        long long r = l.r[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float os = __shfl_xor(s, off);
            const long long orr = __shfl_xor(r, off);
            if (better(os, orr, s, r)) {
                s = os;
                r = orr;
            }
        }
        out_v[round] = s;
        out_r[round] = r;
        if (l.v[0] == s && l.r[0] == r) l.pop();
    }
}

template <int K, typename RowT>
__global__ __launch_bounds__(256) void merge_topk_kernel(const float *__restrict__ cs,
                                                          const RowT *__restrict__ cr, long long n_cand,
                                                          long long inner, long long outer_stride,
                                                          long long q_stride, int k_out,
                                                          long long row_offset, float *__restrict__ out_s,
                                                          long long *__restrict__ out_r,
                                                          float *__restrict__ thr0, float *__restrict__ seed_s,
                                                          int *__restrict__ seed_r, long long seed_q_stride) {
    __shared__ float sh_v[4 * K];
    __shared__ long long sh_r[4 * K];
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    constexpr long long PAD = sizeof(RowT) == 4 ? (long long)INT_MAX : LLONG_MAX;

    FullList<K> l;
    l.init();
    for (long long c = threadIdx.x; c < n_cand; c += 256) {
        const long long a = (c / inner) * outer_stride + (long long)q * q_stride + (c % inner);
        const float s = cs[a];
        long long r = (long long)cr[a];
        if (r == PAD || r < 0) continue;  // padding entry
        if (better(s, r, l.v[K - 1], l.r[K - 1])) l.insert(s, r);
    }
    float ov[K];
    long long orr[K];
    wave_extract<K>(l, ov, orr);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            sh_v[wave * K + i] = ov[i];
            sh_r[wave * K + i] = orr[i];
        }
    }
    __syncthreads();
    if (wave == 0) {
        l.init();
        for (int i = lane; i < 4 * K; i += 64)
            if (sh_r[i] != LLONG_MAX) l.insert(sh_v[i], sh_r[i]);
        wave_extract<K>(l, ov, orr);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < K; ++i) {
                if (i < k_out) {
                    const bool valid = orr[i] != LLONG_MAX && ov[i] > NEG_INF;
                    out_s[(size_t)q * k_out + i] = valid ? ov[i] : NEG_INF;
                    out_r[(size_t)q * k_out + i] = valid ? orr[i] + row_offset : -1;
                }
            }
            if (thr0 != nullptr) {
                // sample pre-pass: thr0[q] = k-th score of the sample's exact top-K (a valid lower bound of the
                // final k-th score; -inf when the sample held fewer than K live rows), and the sample's top-K
                // becomes one more candidate list of the final merge (seed_* points at that list slot)
                const bool full = orr[K - 1] != LLONG_MAX && ov[K - 1] > NEG_INF;
                thr0[q] = full ? ov[K - 1] : NEG_INF;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const bool valid = orr[i] != LLONG_MAX && ov[i] > NEG_INF;
                    seed_s[(size_t)q * seed_q_stride + i] = valid ? ov[i] : NEG_INF;
                    seed_r[(size_t)q * seed_q_stride + i] = valid ? (int)orr[i] : INT_MAX;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------------------------
struct Plan {
    int K;        // list depth: 5, 10 or 20
    int WN;       // waves along queries
    int NW;       // waves per workgroup
    int grid_x, grid_y;
    int n_tiles;
    int n_lists;
    int b_pad;
    int pre_tiles;  // > 0: a sample pre-pass over the first pre_tiles tiles seeds the selection thresholds
    bool qs_ok;     // shape goes to the query-stationary kernel (search_qs.hip) when dtype / row length allow
    bool qs_room;   // ... could go there (debug switch DBG_FORCE_QS): the workspace keeps room for its sample pass
};

// debug switches of mmrag_internal_cosine_topk_lists_ex (tests and A/B tools only; never set by the product)
constexpr unsigned DBG_NO_PREPASS = 1u, DBG_8_WAVES = 2u, DBG_NO_QS = 4u, DBG_FORCE_QS = 8u;
// query-stationary shapes: the three-launch plan of search_qs.hip instead of the single-launch walk (A/B, tests); the
// walk's MFMA shape forced to 32x32x16 / 16x16x32; no dynamic tile hand-out; no in-kernel threshold seeding
constexpr unsigned DBG_OLD_QS = 0x10000u, DBG_MFMA32 = 0x20000u, DBG_MFMA16 = 0x40000u, DBG_NO_DYN = 0x80000u,
                   DBG_NO_SEED = 0x100000u;

// n_lists, b_pad and pre_tiles depend on (B, n, k) only: mmrag_cosine_topk_select and the workspace query
// have no dtype, so both kernels keep the same list layout
Plan make_plan(int B, long long n, int k, unsigned dbg = 0) {
    Plan pl;
    pl.K = k <= 5 ? 5 : (k <= 10 ? 10 : 20);
    pl.WN = plan_wn(B);
    const int qrows = 32 * pl.WN;
    pl.grid_y = (B + qrows - 1) / qrows;
    pl.n_tiles = (int)((n + TM - 1) / TM);
    const int cus = num_cus();
    pl.grid_x = plan_walkers(pl.n_tiles, pl.grid_y);
    pl.NW = (pl.K == 5 && pl.WN == 8 && !(dbg & DBG_8_WAVES)) ? 16 : 8;  // 4 waves/SIMD hide LDS + barrier latency
    // Sample pre-pass (256-query shape, and every shape with deep lists: there the epilogue, not HBM, is
    // what thresholds relieve).
    // The exact top-K of the first `cus` tiles gives every query a threshold as tight as if each
    // workgroup had already seen 65k rows, so the main pass almost never takes the insertion path.
    pl.pre_tiles = 0;
    const bool want_pre = (pl.WN == 8 || pl.K > 5) && pl.n_tiles >= 3 * cus;
    if (want_pre && !(dbg & DBG_NO_PREPASS)) pl.pre_tiles = cus;
    pl.n_lists = pl.grid_x + (want_pre ? 1 : 0);  // one merged list per workgroup per query (+ the sample's)
    pl.b_pad = pl.grid_y * qrows;
    // query-stationary kernels: more than 128 queries and a long shard.  They need >= 256 rows per walker to run at
    // all (qs_room).  The single-launch walk (list depth 5) pays from 3.75 tiles of 256 rows per CU
    // (profiles/r03_config_sweep.txt, walk vs slab-ring: 1M rows 379 vs 467 us, 500k 224 vs 258, 250k 154 vs 158,
    // 125k 112 vs 99); the three-launch plan (depth 10) from about 6 (profiles/r02_config_sweep.txt: its launches have
    // ~35 us of fixed cost each).
    pl.qs_room = pl.WN == 8 && pl.n_tiles >= cus;
    const bool long_enough = pl.K <= 5 ? pl.n_tiles * 4 >= 15 * cus : pl.n_tiles >= 6 * cus;
    pl.qs_ok = pl.qs_room && !(dbg & DBG_NO_QS) && (long_enough || (dbg & DBG_FORCE_QS));
    return pl;
}

template <int DT, int WN, int K, int NSTAGE, int NW = 8, bool SEEDED = false>
void launch_main(const KParams &p, dim3 grid, hipStream_t s) {
    KParams kp = p;
    kp.walkers = (int)grid.x;
    kp.share_l2 = grid.y > 1;
    cosine_topk_kernel<DT, WN, K, NSTAGE, NW, SEEDED><<<grid.x * grid.y, 64 * NW, 0, s>>>(kp);
}

// deep lists (K = 10, 20): 8 waves (2 per SIMD, 256 registers each) hold the lists next to the accumulators
template <int DT, int K>
void dispatch_deep(const Plan &pl, const KParams &p, dim3 grid, hipStream_t s) {
    if (pl.WN == 2) launch_main<DT, 2, K, 3>(p, grid, s);
    else if (pl.WN == 4) launch_main<DT, 4, K, 3>(p, grid, s);
    else if (p.thr0) launch_main<DT, 8, K, 2, 8, true>(p, grid, s);
    else launch_main<DT, 8, K, 2>(p, grid, s);
}

template <int DT>
int dispatch_main(const Plan &pl, const KParams &p, hipStream_t s) {
    dim3 grid(pl.grid_x, pl.grid_y);
    if (pl.K == 5) {
        if (pl.WN == 2) launch_main<DT, 2, 5, 3>(p, grid, s);
        else if (pl.WN == 4) launch_main<DT, 4, 5, 3>(p, grid, s);
        else if (pl.NW == 16 && p.thr0) launch_main<DT, 8, 5, 2, 16, true>(p, grid, s);
        else if (pl.NW == 16) launch_main<DT, 8, 5, 2, 16>(p, grid, s);
        else if (p.thr0) launch_main<DT, 8, 5, 2, 8, true>(p, grid, s);
        else launch_main<DT, 8, 5, 2>(p, grid, s);
    } else if (pl.K == 10) {
        dispatch_deep<DT, 10>(pl, p, grid, s);
    } else {
        dispatch_deep<DT, 20>(pl, p, grid, s);
    }
    return MMRAG_OK;
}

// filter mode (K = 0) for search_deep.hip: the list search's WN plan and wave shapes (16 waves at WN = 8, as depth 5;
// 8 for fp32, whose bf16 split does not fit 128 registers without spilling)
template <int DT>
void launch_filter(int WN, const KParams &p, dim3 grid, hipStream_t s) {
    if (WN == 2) launch_main<DT, 2, 0, 3>(p, grid, s);
    else if (WN == 4) launch_main<DT, 4, 0, 3>(p, grid, s);
    else if constexpr (DT == MMRAG_F32) launch_main<DT, 8, 0, 2, 8>(p, grid, s);
    else launch_main<DT, 8, 0, 2, 16>(p, grid, s);
}

int deep_filter_launch(int dtype, int WN, const KParams &p, int grid_x, int grid_y, hipStream_t s) {
    if (dtype == MMRAG_F8E4M3) return f8_filter_launch(WN, p, grid_x, grid_y, s);
    const dim3 grid(grid_x, grid_y);
    with_elem_type(dtype, [&](auto tag) { launch_filter<decltype(tag)::value>(WN, p, grid, s); });
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

template <typename RowT>
int launch_merge(int K, const float *cs, const RowT *cr, long long n_cand, long long inner,
                 long long outer_stride, long long q_stride, int B, int k_out, long long row_offset,
                 float *out_s, long long *out_r, hipStream_t s, float *thr0 = nullptr, float *seed_s = nullptr,
                 int *seed_r = nullptr, long long seed_q_stride = 0) {
    if (K == 5)
        merge_topk_kernel<5, RowT><<<B, 256, 0, s>>>(cs, cr, n_cand, inner, outer_stride, q_stride, k_out,
                                                     row_offset, out_s, out_r, thr0, seed_s, seed_r, seed_q_stride);
    else if (K == 10)
        merge_topk_kernel<10, RowT><<<B, 256, 0, s>>>(cs, cr, n_cand, inner, outer_stride, q_stride, k_out,
                                                      row_offset, out_s, out_r, thr0, seed_s, seed_r, seed_q_stride);
    else
        merge_topk_kernel<20, RowT><<<B, 256, 0, s>>>(cs, cr, n_cand, inner, outer_stride, q_stride, k_out,
                                                      row_offset, out_s, out_r, thr0, seed_s, seed_r, seed_q_stride);
    return MMRAG_OK;
}

__global__ void fill_empty_kernel(float *s, long long *r, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        s[i] = NEG_INF;
        r[i] = -1;
    }
}

__global__ void fill_seed_empty_kernel(float *s, int *r, long long q_stride, int K, long long n_queries) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n_queries)
        for (int i = 0; i < K; ++i) {
            s[q * q_stride + i] = NEG_INF;
            r[q * q_stride + i] = INT_MAX;
        }
}

int check_search_args(const char *name, int k_max, const void *q, const void *corpus, int B, int64_t n, int d, int64_t ld,
                      int dtype, int k) {
    MMRAG_CHECK_ARG(dtype >= 0 && dtype <= MMRAG_F8E4M3, "%s: bad dtype %d", name, dtype);
    MMRAG_CHECK_ARG(B > 0, "%s: B must be positive (got %d)", name, B);
    MMRAG_CHECK_ARG(k >= 1 && k <= k_max, "%s: k=%d outside 1..%d", name, k, k_max);
    MMRAG_CHECK_ARG(n >= 0 && n < (int64_t)INT_MAX - TM, "%s: n=%lld out of range", name, (long long)n);
    MMRAG_CHECK_ARG(d > 0 && ld >= d, "%s: need 0 < d <= ld (d=%d ld=%lld)", name, d, (long long)ld);
    const int64_t row_bytes = ld * esize(dtype);
    MMRAG_CHECK_ARG(row_bytes % SLAB == 0, "%s: row bytes %lld not a multiple of %d (use mmrag_padded_dim)", name,
                    (long long)row_bytes, SLAB);
    MMRAG_CHECK_ARG(row_bytes * TM < (int64_t)UINT_MAX, "%s: rows too long", name);
    MMRAG_CHECK_ARG(q, "%s: null q", name);
    MMRAG_CHECK_ARG(n == 0 || corpus, "%s: null corpus", name);
    MMRAG_CHECK_ARG(((uintptr_t)q % 16) == 0 && ((uintptr_t)corpus % 16) == 0, "%s: q/corpus must be 16-byte aligned",
                    name);
    return MMRAG_OK;
}

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

// workspace: [cand_s entries f32][cand_r entries i32][thr0 b_pad f32][sample top_s b_pad*K f32][pad][sample top_r b_pad*K i64]
struct WsLayout {
    size_t entries, off_r, off_thr, off_ts, off_tr, off_cnt, cnt_bytes, off_pub, off_pthr, off_tk, xch_end, total;
};
static WsLayout ws_layout(const Plan &pl) {
    WsLayout w;
    w.entries = (size_t)pl.b_pad * pl.n_lists * pl.K;
    w.off_r = w.entries * sizeof(float);
    w.off_thr = w.off_r + w.entries * sizeof(int);
    w.off_ts = w.off_thr + (size_t)pl.b_pad * sizeof(float);
    w.off_tr = (w.off_ts + (size_t)pl.b_pad * pl.K * sizeof(float) + 15) / 16 * 16;
    // query-stationary kernel: the per-workgroup bests of its sample pass
    w.off_cnt = (w.off_tr + (size_t)pl.b_pad * pl.K * sizeof(long long) + 63) / 64 * 64;
    w.cnt_bytes = 0;
    w.off_pub = w.off_cnt + w.cnt_bytes;
    // single-launch walk: the exchange block [bests b_pad x walkers | thresholds b_pad | tickets per query group],
    // filled with the bit pattern of -inf before every launch (the three-launch plan uses the first part only)
    w.off_pthr = w.off_pub + (pl.qs_room ? (size_t)pl.b_pad * pl.grid_x * sizeof(float) : 0);
    w.off_tk = w.off_pthr + (pl.qs_room ? (size_t)pl.b_pad * sizeof(float) : 0);
    w.xch_end = w.off_tk + (pl.qs_room ? ((size_t)pl.grid_y * sizeof(unsigned) + 63) / 64 * 64 : 0);
    w.total = w.xch_end;
    return w;
}

size_t mmrag_cosine_topk_workspace_bytes(int B, int64_t n, int k) {
    if (B <= 0 || n < 0 || k < 1 || k > MMRAG_MAX_K) return 0;
    return ws_layout(make_plan(B, n, k)).total + 256;
}

// mmrag_cosine_topk_lists with debug switches (DBG_*): kernel-shape A/B runs and the tests that pin every code
// path against the oracle.  Exported for them, deliberately absent from include/mmrag.h.
int mmrag_internal_cosine_topk_lists_ex(const void *q, const void *corpus, int B, int64_t n, int d, int64_t ld,
                                        int dtype, int k, const uint32_t *alive_bits, void *workspace,
                                        size_t workspace_bytes, void *stream, unsigned dbg) {
    if (int st = check_search_args("cosine_topk", MMRAG_MAX_K, q, corpus, B, n, d, ld, dtype, k)) return st;
    if (n == 0) return MMRAG_OK;
    const Plan pl = make_plan(B, n, k, dbg);
    const WsLayout wl = ws_layout(pl);
    if (!workspace || workspace_bytes < wl.total) {
        set_error("cosine_topk: workspace %zu bytes < required %zu", workspace_bytes, wl.total);
        return MMRAG_EWORKSPACE;
    }
    MMRAG_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "cosine_topk: workspace must be 16-byte aligned");

    KParams p;
    p.q = (const char *)q;
    p.corpus = (const char *)corpus;
    p.alive_bits = alive_bits;
    p.cand_s = (float *)workspace;
    p.cand_r = (int *)((char *)workspace + wl.off_r);
    p.n = n;
    p.B = B;
    p.row_bytes = (unsigned)(ld * esize(dtype));
    p.n_tiles = pl.n_tiles;
    p.n_lists = pl.n_lists;
    p.tile0 = 0;
    p.thr0 = nullptr;
    p.dbg = dbg;
    // (per workgroup: 8 words in the three-launch kernel, 32 in the walk kernel -- room for the larger)
    p.stamps = ((dbg & DBG_QS_CLOCK) && workspace_bytes >= wl.total + 256 * (size_t)(pl.grid_x * pl.grid_y)) ? (unsigned long long *)((char *)workspace + wl.total) : nullptr;
    p.walkers = pl.grid_x;
    p.share_l2 = pl.grid_y > 1;
    p.sample_best = nullptr;
    p.pub_best = nullptr;
    p.pub_thr = nullptr;
    p.tickets = nullptr;
    p.p_static = INT_MAX / 2;
    hipStream_t s = (hipStream_t)stream;
    const size_t seed_off = (size_t)(pl.n_lists - 1) * pl.K;  // the sample's list: last slot of every query
    const int walk_mfma = (dbg & DBG_MFMA32) ? 32 : ((dbg & DBG_MFMA16) ? 16 : (pl.K == 5 ? QSW_DEFAULT_MFMA : 32));
    if (pl.qs_ok && !(dbg & DBG_OLD_QS) && qsw_supported(dtype, p.row_bytes, pl.K, walk_mfma)) {
        // single-launch walk (search_qsw.hip): thresholds are exchanged inside the launch through a block the host fills
        // with -inf first; the last tenth of the tiles is handed out by ticket when there is one query group
        const int tiles = (int)((n + QS_TILE_ROWS - 1) / QS_TILE_ROWS);
        const int per = tiles / pl.grid_x;
        p.n_tiles = tiles;
        p.pub_best = nullptr;
        p.pub_thr = nullptr;
        p.tickets = nullptr;
        p.p_static = INT_MAX / 2;
        const bool seed = per >= 12 && !(dbg & DBG_NO_SEED);
        const bool dyn = pl.grid_y == 1 && per >= 24 && !(dbg & DBG_NO_DYN);
        if (seed || dyn) {
            MMRAG_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)((char *)workspace + wl.off_pub), (int)TICKET0,
                                              (wl.xch_end - wl.off_pub) / 4, s));
            if (seed) {
                p.pub_best = (float *)((char *)workspace + wl.off_pub);
                p.pub_thr = (float *)((char *)workspace + wl.off_pthr);
            }
            if (dyn) {
                p.tickets = (unsigned *)((char *)workspace + wl.off_tk);
                const int tail = per / 10 > 3 ? per / 10 : 3;
                p.p_static = per - tail;   // >= 21
            }
        }
        if (int st = qsw_launch(dtype, pl.K, walk_mfma, p, pl.grid_x, pl.grid_y, s)) return st;
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    }
    if (pl.qs_ok && qs_supported(dtype, p.row_bytes, pl.K)) {
        // query-stationary kernel.  Long shards: (1) a sample pass over the first pre_tiles * 256 rows that keeps
        // only each workgroup's best score per query, (2) thr0[q] = K-th largest of those bests, (3) the walk over
        // ALL rows (the sample again: it kept no candidates) with every lane's threshold warm from the first tile.
        const int tiles = (int)((n + QS_TILE_ROWS - 1) / QS_TILE_ROWS);
        float *thr0 = nullptr;
        if (pl.pre_tiles > 0) {
            KParams ks = p;
            ks.n_tiles = pl.pre_tiles * (TM / QS_TILE_ROWS);
            ks.sample_best = (float *)((char *)workspace + wl.off_pub);
            if (int st = qs_launch(dtype, pl.K, ks, pl.grid_x, pl.grid_y, s)) return st;
            thr0 = (float *)((char *)workspace + wl.off_thr);
            if (int st = qs_seed_thresholds(pl.K, ks.sample_best, pl.grid_x, pl.b_pad, thr0, s)) return st;
        }
        p.n_tiles = tiles;
        p.thr0 = thr0;
        if (int st = qs_launch(dtype, pl.K, p, pl.grid_x, pl.grid_y, s)) return st;
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    }
    auto run = [&](int tile0, int n_tiles, int grid_x, const float *thr0) -> int {
        KParams kp = p;
        kp.tile0 = tile0;
        kp.n_tiles = n_tiles;
        kp.thr0 = thr0;
        Plan lp = pl;
        lp.grid_x = grid_x;
        if (dtype == MMRAG_F8E4M3) return f8_lists_launch(lp.K, lp.WN, kp, lp.grid_x, lp.grid_y, s);
        return with_elem_type(dtype, [&](auto tag) { return dispatch_main<decltype(tag)::value>(lp, kp, s); });
    };
    if (pl.pre_tiles > 0) {
        // 1. sample pre-pass over the first pre_tiles tiles, one per workgroup
        float *thr0 = (float *)((char *)workspace + wl.off_thr);
        float *top_s = (float *)((char *)workspace + wl.off_ts);
        long long *top_r = (long long *)((char *)workspace + wl.off_tr);
        const int pre = pl.pre_tiles;
        const int pre_grid = pre < pl.grid_x ? pre : pl.grid_x;
        if (int st = run(0, pre, pre_grid, nullptr)) return st;
        MMRAG_CHECK_HIP(hipGetLastError());
        // 2. its exact top-K per query, 3. seed thresholds + keep it as the last candidate list
        const long long n_cand = (long long)pre_grid * pl.K;
        launch_merge<int>(pl.K, p.cand_s, p.cand_r, n_cand, n_cand, 0, (long long)pl.n_lists * pl.K, B, pl.K, 0, top_s,
                          top_r, s, thr0, p.cand_s + seed_off, p.cand_r + seed_off, (long long)pl.n_lists * pl.K);
        MMRAG_CHECK_HIP(hipGetLastError());
        // 4. main pass over the remaining tiles, selection armed with the sample thresholds
        if (int st = run(pre, pl.n_tiles - pre, pl.grid_x, thr0)) return st;
    } else {
        if (pl.n_lists > pl.grid_x) {
            // (debug: pre-pass switched off) the sample's list slot exists but nothing fills it
            const long long total = (long long)pl.b_pad;
            fill_seed_empty_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(
                p.cand_s + seed_off, p.cand_r + seed_off, (long long)pl.n_lists * pl.K, pl.K, total);
        }
        if (int st = run(0, pl.n_tiles, pl.grid_x, nullptr)) return st;
    }
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

// which kernel a (B, n, ld, dtype, k) search runs on: 2 = single-launch walk (search_qsw.hip), 1 = three-launch
// query-stationary (search_qs.hip), 0 = slab-ring.  For the
// bench's roofline label and the tools; not part of the public ABI.
int mmrag_internal_search_uses_qs(int B, int64_t n, int64_t ld, int dtype, int k) {
    if (B <= 0 || n <= 0 || k <= 0 || k > MMRAG_MAX_K) return 0;
    const Plan pl = make_plan(B, n, k, 0u);
    const unsigned rb = (unsigned)(ld * esize(dtype));
    if (!pl.qs_ok) return 0;
    if (qsw_supported(dtype, rb, pl.K, QSW_DEFAULT_MFMA)) return 2;   // the single-launch walk (search_qsw.hip)
    return qs_supported(dtype, rb, pl.K) ? 1 : 0;
}

int mmrag_cosine_topk_lists(const void *q, const void *corpus, int B, int64_t n, int d, int64_t ld, int dtype,
                            int k, const uint32_t *alive_bits, void *workspace, size_t workspace_bytes,
                            void *stream) {
    return mmrag_internal_cosine_topk_lists_ex(q, corpus, B, n, d, ld, dtype, k, alive_bits, workspace,
                                               workspace_bytes, stream, 0u);
}

int mmrag_cosine_topk_select(int B, int64_t n, int k, int64_t row_offset, const void *workspace,
                             float *out_scores, int64_t *out_rows, void *stream) {
    MMRAG_CHECK_ARG(B > 0 && n >= 0 && k >= 1 && k <= MMRAG_MAX_K, "cosine_topk_select: bad shape");
    MMRAG_CHECK_ARG(out_scores && out_rows, "cosine_topk_select: null output");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        const long long total = (long long)B * k;
        fill_empty_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(out_scores, (long long *)out_rows, total);
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    }
    MMRAG_CHECK_ARG(workspace, "cosine_topk_select: null workspace");
    const Plan pl = make_plan(B, n, k);
    const WsLayout wl = ws_layout(pl);
    const float *cand_s = (const float *)workspace;
    const int *cand_r = (const int *)((const char *)workspace + wl.off_r);
    const long long n_cand = (long long)pl.n_lists * pl.K;
    launch_merge<int>(pl.K, cand_s, cand_r, n_cand, n_cand, 0, n_cand, B, k, row_offset, out_scores,
                      (long long *)out_rows, s);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

int mmrag_cosine_topk(const void *q, const void *corpus, int B, int64_t n, int d, int64_t ld, int dtype,
                      int k, int64_t row_offset, const uint32_t *alive_bits, float *out_scores,
                      int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream) {
    if (int st = mmrag_cosine_topk_lists(q, corpus, B, n, d, ld, dtype, k, alive_bits, workspace, workspace_bytes,
                                         stream))
        return st;
    return mmrag_cosine_topk_select(B, n, k, row_offset, workspace, out_scores, out_rows, stream);
}

int mmrag_merge_topk(const float *scores, const int64_t *rows, int G, int B, int k_in, int k,
                     float *out_scores, int64_t *out_rows, void *stream) {
    MMRAG_CHECK_ARG(scores && rows && out_scores && out_rows, "merge_topk: null pointer");
    MMRAG_CHECK_ARG(G > 0 && B > 0 && k_in > 0, "merge_topk: bad shape G=%d B=%d k_in=%d", G, B, k_in);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K, "merge_topk: k=%d outside 1..%d", k, MMRAG_MAX_K);
    const int K = k <= 5 ? 5 : (k <= 10 ? 10 : 20);
    launch_merge<long long>(K, scores, (const long long *)rows, (long long)G * k_in, k_in, (long long)B * k_in,
                            k_in, B, k, 0, out_scores, (long long *)out_rows, (hipStream_t)stream);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // extern "C"
