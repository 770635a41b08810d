// Document-scoped top-k (include/mmrag.h mmrag_scoped_topk): a batch of queries against the stored rows, each query
// seeing only the rows whose group ordinal (document) is in ITS scope, in one masked scan.
//
// prep launch: one union bitmap over the n_groups ordinals per tile of 128 queries, the OR of that tile's scopes
// (O(B / 128 * n_groups / 8) bytes of workspace).
//
// scan launch: Q . X^T with pair_tile.h's body, a 128-row tile of stored rows as A and a 128-query tile as B; rows past n
// and queries past B read as zero through the buffer descriptor.  Workgroups are persistent over row tiles.  Every
// wave reads the tile's 128 ordinals (two per lane, dead and out-of-range rows as -1) and tests them against each query
// tile's union bitmap with a ballot: all four waves read the same words, so the outcome is the same scalar in each and
// the workgroup branches as one without touching LDS.  A (row tile, query tile) item none of whose rows passes is never
// fetched; a row tile no query tile wants costs its ordinal reads and nothing else.  The ring runs over the K-slabs
// of the query tiles that are left without draining between them, as kmeans_assign_kernel's runs over centroid tiles.
// After a query tile's last slab a lane tests its 16 rows' ordinals against each of its 4 queries' scope lists (at most
// 64 ascending ordinals: first / last reject, then a binary search, the answer kept while the ordinal repeats) and
// appends the matches as (score, local row) through the query's counter, the append of the deep search's filter.  No
// threshold: a scope is small, every visible row is a candidate.  The K order is slab_step's, so a score's bits depend
// on the query row, the stored row and d alone.
//
// select and overflow: candidate_select.h's driver, unchanged, with `max_candidates` as its n.
#include "candidate_select.h"
#include "pair_tile.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

struct ScopedParams {
    const char *rows;
    const char *q;
    long long n;
    int B;
    unsigned row_bytes;     // ld * element size, of the rows and of the queries
    int nk;                 // K-slabs that hold the d logical columns
    int nqt;                // query tiles, <= SCAN_MAX_TILES
    const unsigned *alive;
    const int *group_of_row;
    int n_groups;
    int W;                  // words of a union bitmap
    const unsigned *bitmap; // [nqt, W]
    const int *scope_of_query;
    int S;
    const int *scope_off;
    const int *scope_groups;
    float *cand_s;
    int *cand_r;
    unsigned *cnt;
    unsigned cap;
    long long T;            // row tiles
};

// bitmap[t, :] |= the ordinals of the scopes of queries 128 t .. 128 t + 127 (the bitmap is zero on entry).  A scope
// index outside 0..S-1, offsets that do not ascend and ordinals outside 0..n_groups-1 match nothing, here and in the scan.
__global__ __launch_bounds__(PT) void scoped_union_kernel(const ScopedParams p, unsigned *bitmap) {
    const int col = blockIdx.x * PT + threadIdx.x;
    if (col >= p.B) return;
    const int s = p.scope_of_query[col];
    if ((unsigned)s >= (unsigned)p.S) return;
    const int lo = p.scope_off[s];
    int hi = p.scope_off[s + 1];
    if (lo < 0 || hi - lo > MMRAG_MAX_SCOPE_GROUPS) hi = lo;
    unsigned *bm = bitmap + (size_t)blockIdx.x * p.W;
    for (int i = lo; i < hi; ++i) {
        const int g = p.scope_groups[i];
        if ((unsigned)g < (unsigned)p.n_groups) atomicOr(bm + (g >> 5), 1u << (g & 31));
    }
}

template <int DT>
__global__ __launch_bounds__(256, 2) void scoped_scan_kernel(const ScopedParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];

    const unsigned RB = p.row_bytes;
    const PairTileCtx c = pair_tile_ctx(threadIdx.x, RB, smem);
    const int lane = c.lane, wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;
    const int nqt = p.nqt, W = p.W;

    for (long long tile = blockIdx.x; tile < p.T; tile += gridDim.x) {
        const PairRowTile rt = pair_row_tile(tile, p.T, p.T, p.n);
        const long long row0 = rt.row0;
        // ordinals of rows `lane` and `lane + 64` of the tile: -1 = past n, dead, in no group
        int ord[2];
        pair_tile_row_ordinals(row0, lane, p.n, p.alive, p.group_of_row, p.n_groups, ord);
        // rows of the tile that query tile qt's union bitmap holds: bit i of m0 = row i, of m1 = row 64 + i.  The same
        // two scalars in all four waves.
        auto wanted = [&](int qt, unsigned long long &m0, unsigned long long &m1) {
            const unsigned *bm = p.bitmap + (size_t)qt * W;
            const bool h0 = ord[0] >= 0 && ((bm[ord[0] >> 5] >> (ord[0] & 31)) & 1u);
            const bool h1 = ord[1] >= 0 && ((bm[ord[1] >> 5] >> (ord[1] & 31)) & 1u);
            m0 = __builtin_amdgcn_ballot_w64(h0);
            m1 = __builtin_amdgcn_ballot_w64(h1);
        };
        unsigned long long active = 0;      // bit qt: the item (this row tile, query tile qt) has a visible row
        if (__builtin_amdgcn_ballot_w64(ord[0] >= 0 || ord[1] >= 0) != 0ull) {
            for (int qt = 0; qt < nqt; ++qt) {
                unsigned long long m0, m1;
                wanted(qt, m0, m1);
                if ((m0 | m1) != 0ull) active |= 1ull << qt;
            }
        }
        // uniform: the whole workgroup takes this path; nothing was fetched, no LDS is touched
        if (active == 0ull) continue;

        const PairTileSrc rows_src = {p.rows + (size_t)row0 * RB, (unsigned)rt.rows * RB};
        // the ring runs over the wanted query tiles, lowest first: each callback pops its own copy of the mask
        unsigned long long i_left = active, c_left = active;
        const auto tile_src = [&](int) {
            const int qt = __builtin_ctzll(i_left);
            i_left &= i_left - 1;
            const int q_left = p.B - qt * PT;
            const PairTileSrc q_src = {p.q + (size_t)qt * PT * RB, (unsigned)(q_left < PT ? q_left : PT) * RB};
            return wave < 2 ? rows_src : q_src;
        };
        // ---- acc[a][b][r] = <row wm*64 + 16a + 4 g4 + r, query qt * 128 + wn*64 + 16b + c16>
        const auto tile_done = [&](int, const f32x4_t (&acc)[4][4]) {
            const int qt = __builtin_ctzll(c_left);
            c_left &= c_left - 1;
            unsigned long long m0, m1;
            wanted(qt, m0, m1);
            const unsigned long long mw = wm ? m1 : m0;      // this wave's 64 rows
            const int ow = wm ? ord[1] : ord[0];
            if (mw != 0ull) {
                // this lane's 16 rows: bit 4a + r of `vis` = row 16a + 4 g4 + r of the wave's 64 passed the union test
                int my_ord[16];
                unsigned vis = 0;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int src = 16 * a + 4 * g4 + r;
                        my_ord[4 * a + r] = __shfl(ow, src);
                        vis |= (unsigned)((mw >> src) & 1ull) << (4 * a + r);
                    }
                const int lrow0 = (int)row0 + wm * 64 + 4 * g4;      // n < 2^31 (the entry point's check)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int col = qt * PT + wn * 64 + 16 * b + c16;
                    if (col >= p.B || vis == 0u) continue;
                    const int s = p.scope_of_query[col];
                    if ((unsigned)s >= (unsigned)p.S) continue;
                    const int lo = p.scope_off[s], hi = p.scope_off[s + 1];
                    if (lo < 0 || hi <= lo || hi - lo > MMRAG_MAX_SCOPE_GROUPS) continue;
                    const int *list = p.scope_groups + lo;
                    const int len = hi - lo, first = list[0], last = list[len - 1];
                    unsigned hit = 0;
                    int prev = -1;
                    bool prev_hit = false;
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        if (((vis >> j) & 1u) == 0u) continue;
                        const int o = my_ord[j];
                        if (o != prev) {
                            prev = o;
                            prev_hit = false;
                            if (o >= first && o <= last) {
                                int l = 0, h = len - 1;     // list[l] <= o <= list[h]
                                while (l < h) {
                                    const int m = (l + h + 1) >> 1;
                                    if (list[m] <= o) l = m;
                                    else h = m - 1;
                                }
                                prev_hit = list[l] == o;
                            }
                        }
                        if (prev_hit) hit |= 1u << j;
                    }
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
        };
        pair_tile_ring<DT>(c, smem, p.nk, __popcll(active), tile_src, tile_done);
        __syncthreads();   // the ring's contract: every wave is done with it before the next tile's first slab lands
    }
#endif
}

template <int DT>
int launch_scan(const ScopedParams &p, hipStream_t s) {
    hipLaunchKernelGGL(scoped_scan_kernel<DT>, dim3(scan_grid(p.T)), dim3(256), 0, s, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

inline int scoped_words(int n_groups) { return (n_groups + 31) / 32; }
inline long long scoped_cap(int k, long long cap_override) {
    const long long cap = candidate_capacity(k);
    return cap_override > 0 && cap_override < cap ? cap_override : cap;
}
// the candidate driver's blocks, then the union bitmaps: one per query tile of the batch and one for a re-run
inline size_t scoped_bitmap_bytes(int B, int n_groups) {
    return align_up(((size_t)(B + PT - 1) / PT + 1) * (size_t)scoped_words(n_groups) * sizeof(unsigned), 256);
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

size_t mmrag_scoped_topk_workspace_bytes(int B, int64_t n, int k, int n_groups) {
    if (B <= 0 || n < 0 || n >= (1LL << 31) || k < 1 || k > MMRAG_MAX_K_DEEP || n_groups < 0) return 0;
    return candidate_ws_layout(B, candidate_capacity(k), n, false).total + scoped_bitmap_bytes(B, n_groups);
}

// candidate slots per query of a top-k of k: what a caller sizes max_candidates against (VectorIndex.scoped_search)
int64_t mmrag_internal_candidate_capacity(int k) { return k >= 1 && k <= MMRAG_MAX_K_DEEP ? candidate_capacity(k) : 0; }

// mmrag_scoped_topk with a smaller candidate capacity (cap > 0): the test that pins the overflow re-run.  Exported for
// it, deliberately absent from include/mmrag.h.
int mmrag_internal_scoped_topk_ex(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                                  int64_t row_offset, const uint32_t *alive_bits, const int32_t *group_of_row,
                                  int n_groups, const int32_t *scope_of_query, int S, const int32_t *scope_off,
                                  const int32_t *scope_groups, int64_t max_candidates, float *out_scores,
                                  int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream,
                                  int64_t cap_override) {
    MMRAG_CHECK_ARG(q && rows && group_of_row && scope_of_query && scope_off && scope_groups,
                    "scoped_topk: null pointer");
    MMRAG_CHECK_ARG(out_scores && out_rows, "scoped_topk: null output");
    if (int st = check_stored_rows("scoped_topk", "searched by scope", "search", ld, dtype, d, &n)) return st;
    MMRAG_CHECK_ARG(n < (1LL << 31), "scoped_topk: need n < 2^31 (n=%lld)", (long long)n);
    MMRAG_CHECK_ARG(B >= 1, "scoped_topk: need B >= 1 (B=%d)", B);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K_DEEP, "scoped_topk: k=%d outside 1..%d", k, MMRAG_MAX_K_DEEP);
    MMRAG_CHECK_ARG(n_groups >= 0, "scoped_topk: need n_groups >= 0 (n_groups=%d)", n_groups);
    MMRAG_CHECK_ARG(S >= 1, "scoped_topk: need S >= 1 scopes (S=%d)", S);
    MMRAG_CHECK_ARG(max_candidates >= 0, "scoped_topk: need max_candidates >= 0 (max_candidates=%lld)",
                    (long long)max_candidates);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0 || n_groups == 0 || max_candidates == 0)
        return candidate_fill_empty(out_scores, (long long *)out_rows, B, k, s);

    const long long cap = scoped_cap(k, cap_override);
    const CandWs wl = candidate_ws_layout(B, cap, n, false);
    const size_t need = wl.total + scoped_bitmap_bytes(B, n_groups);
    if (!workspace || workspace_bytes < need) {
        set_error("scoped_topk: workspace %zu bytes < required %zu", workspace_bytes, need);
        return MMRAG_EWORKSPACE;
    }
    MMRAG_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "scoped_topk: workspace must be 16-byte aligned");

    char *ws = (char *)workspace;
    unsigned *bitmap = (unsigned *)(ws + wl.total);
    ScopedParams p;
    p.rows = (const char *)rows;
    p.q = (const char *)q;
    p.n = n;
    p.B = B;
    p.row_bytes = stored_row_bytes(ld, dtype);
    p.nk = stored_k_slabs(d, dtype);
    p.alive = alive_bits;
    p.group_of_row = group_of_row;
    p.n_groups = n_groups;
    p.W = scoped_words(n_groups);
    p.scope_of_query = scope_of_query;
    p.S = S;
    p.scope_off = scope_off;
    p.scope_groups = scope_groups;
    p.T = (n + PT - 1) / PT;
    const int nqt_all = (B + PT - 1) / PT;

    // queries q0 .. q0 + Bq of the caller's batch into their slots: the unions into `bm`, then the scans
    const auto produce = [&](int q0, int Bq, unsigned *bm, float *cand_s, int *cand_r, unsigned *counts,
                             long long slots) -> int {
        ScopedParams pq = p;
        pq.q = p.q + (size_t)q0 * p.row_bytes;
        pq.scope_of_query = scope_of_query + q0;
        pq.B = Bq;
        pq.cap = (unsigned)slots;
        const int tiles = (Bq + PT - 1) / PT;
        MMRAG_CHECK_HIP(hipMemsetAsync(bm, 0, (size_t)tiles * p.W * sizeof(unsigned), s));
        hipLaunchKernelGGL(scoped_union_kernel, dim3((unsigned)tiles), dim3(PT), 0, s, pq, bm);
        MMRAG_CHECK_HIP(hipGetLastError());
        return for_scan_chunks(Bq, PT, [&](int first, int Bc, int nqt, int t0) -> int {
            ScopedParams pc = pq;
            pc.q = pq.q + (size_t)first * p.row_bytes;
            pc.scope_of_query = pq.scope_of_query + first;
            pc.B = Bc;
            pc.nqt = nqt;
            pc.bitmap = bm + (size_t)t0 * p.W;
            pc.cand_s = cand_s + (size_t)first * slots;
            pc.cand_r = cand_r + (size_t)first * slots;
            pc.cnt = counts + first;
            return with_elem_type(dtype, [&](auto tag) { return launch_scan<decltype(tag)::value>(pc, s); });
        });
    };
    // the driver's n: no scope holds more rows than this, so a re-run of one query fits max_candidates slots
    const long long n_sel = max_candidates < n ? max_candidates : n;
    return candidate_select(
        "scoped_topk", B, n_sel, cap, k, row_offset, out_scores, (long long *)out_rows, ws, wl, s,
        [&](float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return produce(0, B, bitmap, cand_s, cand_r, counts, slots);
        },
        [&](int qi, float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return produce(qi, 1, bitmap + (size_t)nqt_all * p.W, cand_s, cand_r, counts, slots);
        });
}

int mmrag_scoped_topk(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                      int64_t row_offset, const uint32_t *alive_bits, const int32_t *group_of_row, int n_groups,
                      const int32_t *scope_of_query, int S, const int32_t *scope_off, const int32_t *scope_groups,
                      int64_t max_candidates, float *out_scores, int64_t *out_rows, void *workspace,
                      size_t workspace_bytes, void *stream) {
    return mmrag_internal_scoped_topk_ex(q, rows, B, n, d, ld, dtype, k, row_offset, alive_bits, group_of_row, n_groups,
                                         scope_of_query, S, scope_off, scope_groups, max_candidates, out_scores,
                                         out_rows, workspace, workspace_bytes, stream, 0);
}

}  // extern "C"
