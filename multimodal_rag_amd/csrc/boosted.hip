// Boosted top-k (include/mmrag.h mmrag_boosted_topk): a batch of queries against the stored rows, ranked by
// final[b][r] = fmaf(weight[b], prior[r], <q_b, x_r>) -- a per-row score prior applied INSIDE one exact scan.  A row
// with a large prior and a middling cosine belongs in the answer but is in no cosine top-k, so the prior cannot be
// applied to a finished list.
//
//   1. bound passes, only when n exceeds the candidate capacity: the scan kernel below over a sample of whole 128-row
//      tiles spread evenly over the collection (rows are in ingest order and a recency prior rises with the row number:
//      a prefix would be biased), every live final >= tau_q appended; deep_select_kernel in its bound mode then sets
//      tau_q = max(tau_q, the k-th best of those).  The k-th best of ANY subset of live rows is at most the true k-th
//      final, whatever the prior looks like, so tau_q stays a valid lower bound (-inf while fewer than k rows were seen).
//      The stages grow as search_deep.hip's do.
//   2. main pass: every tile, every live final >= tau_q appended as (final, local row) through the query's counter.
//   3. select and overflow: an overflowed query is produced again alone with the same tau_q into n slots.
// The sequence itself -- plan, workspace, stages, main pass, select, re-runs -- is candidate_select.h's
// bounded_scan_select; this file supplies the producer.
//
// scan kernel: scoped.hip's scan without the scope test.  Q . X^T with pair_tile.h's body, a 128-row tile of stored rows
// as A and a 128-query tile as B; rows past n and queries past B read as zero through the buffer descriptor.  Workgroups
// are persistent over row tiles.  Every wave reads the tile's 128 priors and alive bits once (two rows per lane, plain
// vector loads); a tile with no live row is skipped without a fetch.  The ring runs over the K-slabs of all the query
// tiles without draining between them.  After a query tile's last slab a lane takes its 16 rows' priors by __shfl, reads
// weight and tau of its 4 query columns, forms final with one fmaf and appends the finals that reach tau.  The K order is
// slab_step's, so a dot's bits depend on the query row, the stored row and d alone (and equal mmrag_scoped_topk's), and
// final's on those plus weight[b] and prior[r]: not on the batch, the grid, tau or whether bound passes ran.
#include "candidate_select.h"
#include "pair_tile.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

// debug switches of mmrag_internal_boosted_topk_ex (tests only)
constexpr unsigned BO_DBG_NO_BOUND = 1u;  // no bound passes: tau = -inf, every live row survives the main pass

struct BoostedParams {
    const char *rows;
    const char *q;
    long long n;
    int B;
    unsigned row_bytes;     // ld * element size, of the rows and of the queries
    int nk;                 // K-slabs that hold the d logical columns
    int nqt;                // query tiles, <= SCAN_MAX_TILES
    const unsigned *alive;
    const float *prior;     // [n]
    const float *weight;    // [B]
    const float *tau;       // [B], or null: -inf
    float *cand_s;
    int *cand_r;
    unsigned *cnt;
    unsigned cap;
    long long T;            // row tiles of the collection
    long long walk;         // tiles this launch visits: tile i * T / walk for i in 0 .. walk (walk == T: every tile)
};

static_assert(BOUND_TILE_ROWS == PT, "the bound stages are planned in this scan's tiles");

template <int DT>
__global__ __launch_bounds__(256, 2) void boosted_scan_kernel(const BoostedParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];

    const unsigned RB = p.row_bytes;
    const PairTileCtx c = pair_tile_ctx(threadIdx.x, RB, smem);
    const int lane = c.lane, wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;

    for (long long i = blockIdx.x; i < p.walk; i += gridDim.x) {
        const PairRowTile rt = pair_row_tile(i, p.T, p.walk, p.n);
        const long long row0 = rt.row0;
        unsigned long long m0, m1;
        pair_tile_live_rows(row0, lane, p.n, p.alive, m0, m1);
        // uniform: the whole workgroup takes this path; nothing was fetched, no LDS is touched
        if ((m0 | m1) == 0ull) continue;
        // priors of rows `lane` and `lane + 64` of the tile
        float pr[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long long r = row0 + lane + 64 * h;
            pr[h] = r < p.n ? p.prior[r] : 0.0f;
        }

        const PairTileSrc rows_src = {p.rows + (size_t)row0 * RB, (unsigned)rt.rows * RB};
        const unsigned long long mw = wm ? m1 : m0;      // this wave's 64 rows
        const float pw = wm ? pr[1] : pr[0];
        pair_tile_ring<DT>(
            c, smem, p.nk, p.nqt,
            [&](int qt) {      // (this row tile, query tile qt)
                const int q_left = p.B - qt * PT;
                const PairTileSrc q_src = {p.q + (size_t)qt * PT * RB, (unsigned)(q_left < PT ? q_left : PT) * RB};
                return wave < 2 ? rows_src : q_src;
            },
            [&](int qt, const f32x4_t (&acc)[4][4]) {
                // ---- acc[a][b][r] = <row wm*64 + 16a + 4 g4 + r, query qt * 128 + wn*64 + 16b + c16>
                if (mw == 0ull) return;
                // this lane's 16 rows: bit 4a + r of `vis` = row 16a + 4 g4 + r of the wave's 64 is live
                float my_p[16];
                unsigned vis = 0;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int src = 16 * a + 4 * g4 + r;
                        my_p[4 * a + r] = __shfl(pw, src);
                        vis |= (unsigned)((mw >> src) & 1ull) << (4 * a + r);
                    }
                const int lrow0 = (int)row0 + wm * 64 + 4 * g4;      // n < 2^31 (the entry point's check)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int col = qt * PT + wn * 64 + 16 * b + c16;
                    if (col >= p.B || vis == 0u) continue;
                    const float w = p.weight[col];
                    const float t = p.tau != nullptr ? p.tau[col] : NEG_INF;
                    float fin[16];
                    unsigned hit = 0;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float f = __builtin_fmaf(w, my_p[4 * a + r], acc[a][b][r]);   // one rounding
                            fin[4 * a + r] = f;
                            hit |= (unsigned)(f >= t) << (4 * a + r);
                        }
                    hit &= vis;
                    if (hit == 0u) continue;
                    // reserve the slots with one returning atomic; the counter keeps the true count, slots at or past
                    // cap are not written
                    unsigned at = atomicAdd(p.cnt + col, (unsigned)__popc(hit));
                    float *bs = p.cand_s + (size_t)col * p.cap;
                    int *br = p.cand_r + (size_t)col * p.cap;
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if ((hit >> j) & 1u) {
                            if (at < p.cap) {
                                bs[at] = fin[j];
                                br[at] = lrow0 + 16 * (j >> 2) + (j & 3);
                            }
                            ++at;
                        }
                }
            });
        __syncthreads();   // the ring's contract: every wave is done with it before the next tile's first slab lands
    }
#endif
}

// out_boost[i] = weight[b] * prior[row] of winner i = (b, slot), 0 in padding: the exact float32 product
__global__ __launch_bounds__(256) void boosted_finish_kernel(const long long *__restrict__ out_r,
                                                            const float *__restrict__ prior,
                                                            const float *__restrict__ weight, long long row_offset,
                                                            long long n, int k, long long total,
                                                            float *__restrict__ out_boost) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long r = out_r[i];
    float v = 0.0f;
    if (r >= 0) {
        const long long local = r - row_offset;
        if (local >= 0 && local < n) v = __fmul_rn(weight[i / k], prior[local]);
    }
    out_boost[i] = v;
}

template <int DT>
int launch_scan(const BoostedParams &p, hipStream_t s) {
    hipLaunchKernelGGL(boosted_scan_kernel<DT>, dim3(scan_grid(p.walk)), dim3(256), 0, s, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

size_t mmrag_boosted_topk_workspace_bytes(int B, int64_t n, int k) {
    if (B <= 0 || n < 0 || n >= (1LL << 31) || k < 1 || k > MMRAG_MAX_K_DEEP) return 0;
    return bounded_scan_layout(B, n, k, 0, false).select_bytes;
}

// mmrag_boosted_topk with a smaller candidate capacity (cap_override > 0) and debug switches (BO_DBG_*): the tests that
// pin the overflow re-run and the unbounded scan.  Exported for them, deliberately absent from include/mmrag.h.
int mmrag_internal_boosted_topk_ex(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                                   int64_t row_offset, const uint32_t *alive_bits, const float *prior,
                                   const float *weight, float *out_scores, int64_t *out_rows, float *out_boost,
                                   void *workspace, size_t workspace_bytes, void *stream, int64_t cap_override,
                                   unsigned dbg) {
    MMRAG_CHECK_ARG(q && rows && weight, "boosted_topk: null pointer");
    MMRAG_CHECK_ARG(out_scores && out_rows, "boosted_topk: null output");
    if (int st = check_stored_rows("boosted_topk", "searched with a prior", "search", ld, dtype, d, &n)) return st;
    MMRAG_CHECK_ARG(n < (1LL << 31), "boosted_topk: need n < 2^31 (n=%lld)", (long long)n);
    MMRAG_CHECK_ARG(prior || n == 0, "boosted_topk: null prior");
    MMRAG_CHECK_ARG(B >= 1, "boosted_topk: need B >= 1 (B=%d)", B);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K_DEEP, "boosted_topk: k=%d outside 1..%d", k, MMRAG_MAX_K_DEEP);
    hipStream_t s = (hipStream_t)stream;
    const long long total_out = (long long)B * k;
    if (n == 0) {
        if (out_boost) MMRAG_CHECK_HIP(hipMemsetAsync(out_boost, 0, (size_t)total_out * sizeof(float), s));
        return candidate_fill_empty(out_scores, (long long *)out_rows, B, k, s);
    }

    BoostedParams p;
    p.rows = (const char *)rows;
    p.n = n;
    p.row_bytes = stored_row_bytes(ld, dtype);
    p.nk = stored_k_slabs(d, dtype);
    p.alive = alive_bits;
    p.prior = prior;
    p.T = (n + PT - 1) / PT;
    // queries q0 .. q0 + Bq of the caller's batch over `walk` tiles into their slots
    const auto produce = [&](ScanPass, int q0, int Bq, long long walk, const float *tau, float *cand_s, int *cand_r,
                             unsigned *counts, long long slots) -> int {
        return for_scan_chunks(Bq, PT, [&](int first, int Bc, int nqt, int) -> int {
            BoostedParams pc = p;
            const int c0 = q0 + first;
            pc.q = (const char *)q + (size_t)c0 * p.row_bytes;
            pc.weight = weight + c0;
            pc.tau = tau != nullptr ? tau + c0 : nullptr;
            pc.B = Bc;
            pc.nqt = nqt;
            pc.walk = walk;
            pc.cap = (unsigned)slots;
            pc.cand_s = cand_s + (size_t)first * slots;
            pc.cand_r = cand_r + (size_t)first * slots;
            pc.cnt = counts + first;
            return with_elem_type(dtype, [&](auto tag) { return launch_scan<decltype(tag)::value>(pc, s); });
        });
    };
    if (int st = bounded_scan_select("boosted_topk", B, n, k, cap_override, (dbg & BO_DBG_NO_BOUND) != 0u, row_offset,
                                     nullptr, out_scores, (long long *)out_rows, workspace, workspace_bytes, 0, s,
                                     [](char *) { return MMRAG_OK; }, produce))
        return st;
    if (out_boost) {
        boosted_finish_kernel<<<(unsigned)((total_out + 255) / 256), 256, 0, s>>>(
            (const long long *)out_rows, prior, weight, row_offset, n, k, total_out, out_boost);
        MMRAG_CHECK_HIP(hipGetLastError());
    }
    return MMRAG_OK;
}

// The bound plan of mmrag_boosted_topk, mmrag_filtered_topk, mmrag_range_scan (k = limit) and mmrag_recommend_topk
// (candidate_select.h's make_bound_plan; dbg & 1 = no bound passes): *slots = the candidate slots per query,
// stage_tiles[0 .. return value) = the 128-row tiles of each bound stage.  The tests restate it and compare.  Exported
// for them, deliberately absent from include/mmrag.h.
int mmrag_internal_bound_plan(int64_t n, int k, int64_t cap_override, unsigned dbg, int64_t *slots,
                              int64_t stage_tiles[8]) {
    static_assert(BOUND_MAX_STAGES == 8, "the signature's array");
    if (n < 0 || k < 1 || k > MMRAG_MAX_K_DEEP || !slots || !stage_tiles) return -1;
    const BoundPlan pl = make_bound_plan(n, k, cap_override, (dbg & BO_DBG_NO_BOUND) != 0u);
    *slots = pl.cap;
    for (int i = 0; i < pl.n_stages; ++i) stage_tiles[i] = pl.stage_tiles[i];
    return pl.n_stages;
}

int mmrag_boosted_topk(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                       int64_t row_offset, const uint32_t *alive_bits, const float *prior, const float *weight,
                       float *out_scores, int64_t *out_rows, float *out_boost, void *workspace, size_t workspace_bytes,
                       void *stream) {
    return mmrag_internal_boosted_topk_ex(q, rows, B, n, d, ld, dtype, k, row_offset, alive_bits, prior, weight,
                                          out_scores, out_rows, out_boost, workspace, workspace_bytes, stream, 0, 0u);
}

}  // extern "C"
