// The masked scan shared by the filtered top-k (filtered.hip) and the range scan (range.hip): Q . X^T with pair_tile.h's
// body over persistent workgroups, each query seeing only the rows of ITS bitmap, and what surrounds it on the host --
// the bitmap geometry and the union bitmaps of a query tile.  The ring is pair_tile.h's pair_tile_ring; the split of a
// batch into launches (for_scan_chunks), the grid (scan_grid) and the bounded sequence around the scan
// (bounded_scan_select) are candidate_select.h's.  The kernels keep what differs: the epilogue.  Internal, gfx950 only.
//
// The scan: a 128-row tile of stored rows as A and a 128-query tile as B; rows past n and queries past B read as zero
// through the buffer descriptor.  Before anything is fetched all four waves read the tile's four words of every query
// tile's union: the same scalar mask of wanted query tiles in each, so the workgroup branches as one and the ring's
// barriers are reached by all waves or by none.  An item (row tile, query tile) in which no query sees a row is never
// issued; a row tile nobody wants costs those words only.  The ring runs over the K-slabs of the wanted query tiles
// without draining.  After a query tile's last slab a lane reads, for each of its 4 query columns, the 8 bytes of that
// query's bitmap that cover its wave's 64 rows and hands its 16 bits and its accumulators to the epilogue.
// Without bitmaps (vis == null, uni == null) every row below n is visible to every query and every item is issued.
// The K order is slab_step's, so a score's bits depend on the query row, the stored row and d alone.
#pragma once
#include "candidate_select.h"
#include "pair_tile.h"

namespace mmrag_impl {

namespace {

// debug switches of the _ex entry points (tests only)
constexpr unsigned FI_DBG_NO_BOUND = 1u;  // no bound passes: tau stays at its start, every survivor of it is a candidate

inline long long filter_words(long long n) { return 4 * ((n + PT - 1) / PT); }

struct MaskedScanParams {
    const char *rows;
    const char *q;
    long long n;
    int B;
    unsigned row_bytes;     // ld * element size, of the rows and of the queries
    int nk;                 // K-slabs that hold the d logical columns
    int nqt;                // query tiles, <= SCAN_MAX_TILES
    const unsigned *uni;    // [nqt, W]: the union bitmaps of this launch's query tiles; null: every item is wanted
    const unsigned *vis;    // [F, W]; null: every row below n is visible to every query
    const int *filter_of_query;
    int F;
    long long W;
    long long T;            // row tiles of the collection
    long long walk;         // tiles this launch visits: tile i * T / walk for i in 0 .. walk (walk == T: every tile)
    unsigned long long *items;   // optional: += the (row tile, query tile) items this launch issues
};

static_assert(BOUND_TILE_ROWS == PT, "the bound stages are planned in this scan's tiles");

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

// the union bitmaps: one per query tile of the batch and one for a re-run
inline size_t filtered_union_bytes(int B, long long n) {
    return mmrag::align_up(((size_t)(B + PT - 1) / PT + 1) * (size_t)filter_words(n) * sizeof(unsigned), 256);
}

// the unions of Bq queries (their filters at filter_of_query[0 .. Bq)) into um[0 .. ceil(Bq / 128))
inline int launch_unions(const int *filter_of_query, int Bq, int F, const unsigned *vis, long long W, unsigned *um,
                         hipStream_t s) {
    const unsigned wblocks = (unsigned)((W + 255) / 256);
    return for_scan_chunks(Bq, PT, [&](int first, int Bc, int nt, int t0) -> int {
        hipLaunchKernelGGL(filtered_union_kernel, dim3(wblocks, (unsigned)nt), dim3(256), 0, s, filter_of_query + first, Bc,
                           F, vis, W, um + (size_t)t0 * W);
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    });
}

// The scan of one launch.  `smem`: PT_LDS bytes, 1 KiB aligned.  For every complete (row tile, query tile) and each of
// this lane's 4 query columns that is a query of the launch with a filter in range:
//   epilogue(col, vis, acc, b, lrow0)
// col: the query; vis: bit 4a + r = row lrow0 + 16a + r is below n and visible to col (may be 0); acc[a][b][r]: that
// row's score.  Lanes diverge around the call.
template <int DT, typename Epilogue>
__device__ __forceinline__ void masked_scan_body(const MaskedScanParams &p, char *smem, Epilogue &&epilogue) {
    const unsigned RB = p.row_bytes;
    const PairTileCtx c = pair_tile_ctx(threadIdx.x, RB, smem);
    const int wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;
    const int nqt = p.nqt;
    const long long W = p.W;
    const bool masked = p.uni != nullptr;      // uniform

    for (long long i = blockIdx.x; i < p.walk; i += gridDim.x) {
        const PairRowTile rt = pair_row_tile(i, p.T, p.walk, p.n);
        const long long tile = rt.tile, row0 = rt.row0;
        const int in_tile = rt.rows;
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
        if (masked) {
            for (int qt = 0; qt < nqt; ++qt) {
                const unsigned *u = uw + (size_t)qt * W;
                if (((u[0] & vm[0]) | (u[1] & vm[1]) | (u[2] & vm[2]) | (u[3] & vm[3])) != 0u) active |= 1ull << qt;
            }
        } else {
            active = nqt >= 64 ? ~0ull : (1ull << nqt) - 1ull;
        }
        active = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(active >> 32)) << 32) |
                 (unsigned)__builtin_amdgcn_readfirstlane((unsigned)active);
        // uniform: the whole workgroup takes this path; nothing was fetched, no LDS is touched
        if (active == 0ull) continue;
        if (p.items != nullptr && threadIdx.x == 0) atomicAdd(p.items, (unsigned long long)__popcll(active));

        const PairTileSrc rows_src = {p.rows + (size_t)row0 * RB, (unsigned)in_tile * RB};
        // this wave's 64 rows below n
        const unsigned long long valid = ((unsigned long long)vm[2 * wm + 1] << 32) | vm[2 * wm];
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
            unsigned long long mw = valid;
            if (masked) {
                const unsigned *const uq = uw + (size_t)qt * W + 2 * wm;
                mw &= ((unsigned long long)uq[1] << 32) | uq[0];
            }
            if (mw != 0ull) {      // some query of the tile sees one of this wave's rows
                const int lrow0 = (int)row0 + wm * 64 + 4 * g4;      // n < 2^31 (the entry point's check)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int col = qt * PT + wn * 64 + 16 * b + c16;
                    if (col >= p.B) continue;
                    unsigned long long mv = valid;
                    if (p.vis != nullptr) {
                        const int f = p.filter_of_query[col];
                        if ((unsigned)f >= (unsigned)p.F) continue;
                        const unsigned *const vq = p.vis + (size_t)f * W + 4 * tile + 2 * wm;
                        mv &= ((unsigned long long)vq[1] << 32) | vq[0];
                    }
                    // this lane's 16 rows: bit 4a + r of `vis` = row 16a + 4 g4 + r of the wave's 64 is visible
                    unsigned vis = 0;
#pragma unroll
                    for (int a = 0; a < 4; ++a) vis |= (unsigned)((mv >> (16 * a + 4 * g4)) & 15ull) << (4 * a);
                    epilogue(col, vis, acc, b, lrow0);
                }
            }
        };
        pair_tile_ring<DT>(c, smem, p.nk, __popcll(active), tile_src, tile_done);
        __syncthreads();   // the ring's contract: every wave is done with it before the next tile's first slab lands
    }
}

// bit 4a + r: acc[a][b][r] >= t
__device__ __forceinline__ unsigned scores_at_least(const f32x4_t (&acc)[4][4], int b, float t) {
    unsigned m = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) m |= (unsigned)(acc[a][b][r] >= t) << (4 * a + r);
    return m;
}

// the rows of `hit` (bit 4a + r = row lrow0 + 16a + r, score acc[a][b][r]) appended to a query's candidate slots bs / br
// through its counter: one returning atomic reserves the slots; the counter keeps the true count, slots at or past cap
// are not written
__device__ __forceinline__ void append_candidates(unsigned hit, const f32x4_t (&acc)[4][4], int b, int lrow0,
                                                  unsigned *cnt, float *bs, int *br, unsigned cap) {
    unsigned at = atomicAdd(cnt, (unsigned)__popc(hit));
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if ((hit >> (4 * a + r)) & 1u) {
                if (at < cap) {
                    bs[at] = acc[a][b][r];
                    br[at] = lrow0 + 16 * a + r;
                }
                ++at;
            }
}

}  // namespace

}  // namespace mmrag_impl
