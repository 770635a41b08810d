// Exact MaxSim retrieval over a plane of stored token rows (include/mmrag.h mmrag_maxsim_topk): each question's top-k
// ITEMS by late-interaction score, item i owning rows item_off[i] .. item_off[i + 1] of the plane.
//
//   1. plan (one workgroup): whole questions are packed greedily, in order, into 128-row A tiles -- a question never
//      straddles tiles, a bad question (length out of range, rows outside q_rows) is in no tile.  row_src[tile][r] is the
//      q_tok row behind packed row r, row_q[tile][r] the question whose FIRST token is packed row r.
//   2. pack: the A tiles as contiguous rows of the workspace (rows of no question are zero), so one buffer descriptor
//      covers a tile whatever the questions' starts are.  Four 32-token questions share one tile.
//   3. scan: grid (chunks of R plane rows) x (question tiles), pair_tile.h's body, 4 waves.  Chunk c OWNS the items whose
//      first row lies in [c R, (c + 1) R): two binary searches in item_off.  A chunk none of whose items is a candidate
//      (dead, empty, too long) returns before anything is fetched.  Otherwise the workgroup walks 128-row B tiles from
//      its first owned CANDIDATE's start to its last owned candidate's end; the ring runs over ALL (B tile, K-slab) items without
//      draining, the A tile's slabs are fetched again for each B tile (L2), as maxsim.hip does.
//      Epilogue.  After a B tile's last slab, for every item that intersects the tile: columns outside the item are set
//      to -inf by INDEX and the lane's 64 accumulators are folded into the running maxima of its 16 question rows,
//      which are carried in registers while the item stays open across tiles.  When the item closes the 16 lanes that
//      share rows are folded by an xor butterfly and the two waves that share rows through LDS; thread r, where packed
//      row r starts a question, adds that question's maxima in ascending i from 0.0f -- mmrag_maxsim_scores' sum, bit
//      for bit -- and appends (score, item) to the question's candidate slots when the score is at or above tau_q.
//      No atomics take part in the reduction (the append reserves a slot through the question's counter, as every
//      candidate producer here does) and no [Q, n_items] matrix is written.
//   4. select and overflow: candidate_select.h's driver.  When n_items exceeds the slots, tau_q is first staged from a
//      strided sample of whole chunks by deep_select_kernel's bound mode (boosted.hip's plan, counted in items).
// Every table is read on the device with its index checked: a malformed item_off gives wrong answers, never a read
// outside the tables or the plane (the B tile's descriptor ends at the walk's last row, which lies inside the plane).
#include "candidate_select.h"
#include "pair_tile.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int MS_CHUNK_ROWS = 2048;      // R: plane rows per chunk (16 B tiles; the walk runs at most 511 rows past it)
constexpr int MS_SAMPLE0_ITEMS = 12288;  // first bound sample: the select's LDS key cache
constexpr int MS_MAX_STAGES = 8;
constexpr int MS_PLAN_THREADS = 256;

constexpr unsigned MS_DBG_NO_BOUND = 1u;  // no bound passes: tau = -inf, every candidate survives the main pass

struct MsPlanParams {
    const int *q_start, *q_len;
    int Q;
    long long q_rows;
    int max_tiles;    // tiles the workspace and the grid have room for: a question past them is in no tile
    int *n_tiles;     // [1]
    int *q_tile;      // [Q]: the question's tile, -1 for a bad question
    int *row_src;     // [Q, 128], preset to -1
    int *row_q;       // [Q, 128], preset to -1
};

__global__ __launch_bounds__(MS_PLAN_THREADS) void maxsim_plan_kernel(const MsPlanParams p) {
    __shared__ short len_s[MMRAG_MAX_LATE_QUESTIONS];
    __shared__ short off_s[MMRAG_MAX_LATE_QUESTIONS];
    __shared__ short tile_s[MMRAG_MAX_LATE_QUESTIONS];
    const int tid = threadIdx.x;
    for (int q = tid; q < p.Q; q += MS_PLAN_THREADS) {
        const int s = p.q_start[q], l = p.q_len[q];
        const bool ok = l >= 1 && l <= MMRAG_MAX_LATE_QUERY_TOKENS && s >= 0 && (long long)s + l <= p.q_rows;
        len_s[q] = (short)(ok ? l : 0);
    }
    __syncthreads();
    if (tid == 0) {
        int t = -1, used = PT + 1;
        for (int q = 0; q < p.Q; ++q) {
            const int l = len_s[q];
            if (l == 0) {
                tile_s[q] = -1;
                continue;
            }
            if (used + l > PT) {
                ++t;
                used = 0;
            }
            if (t >= p.max_tiles) {     // (never with max_tiles = Q)
                tile_s[q] = -1;
                continue;
            }
            tile_s[q] = (short)t;
            off_s[q] = (short)used;
            used += l;
        }
        p.n_tiles[0] = t + 1 < p.max_tiles ? t + 1 : p.max_tiles;
    }
    __syncthreads();
    for (int q = tid; q < p.Q; q += MS_PLAN_THREADS) {
        const int t = tile_s[q];
        p.q_tile[q] = t;
        if (t < 0) continue;
        const int s = p.q_start[q], l = len_s[q], o = off_s[q];
        for (int i = 0; i < l; ++i) {
            p.row_src[t * PT + o + i] = s + i;
            p.row_q[t * PT + o + i] = i == 0 ? q : -1;
        }
    }
}

// qpack[tile * 128 + r] = q_tok row row_src[tile][r], or zero; 16 bytes per thread and step
__global__ __launch_bounds__(256) void maxsim_pack_kernel(const char *__restrict__ q_tok, unsigned q_rb,
                                                          const int *__restrict__ n_tiles,
                                                          const int *__restrict__ row_src, char *__restrict__ qpack,
                                                          unsigned pack_rb) {
    const int tile = blockIdx.x;
    if (tile >= n_tiles[0]) return;
    const int per_row = pack_rb / 16;
    for (int i = threadIdx.x; i < PT * per_row; i += 256) {
        const int r = i / per_row, ch = i % per_row;
        const int src = row_src[tile * PT + r];
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (src >= 0) v = *(const uint4 *)(q_tok + (size_t)src * q_rb + (size_t)ch * 16);
        *(uint4 *)(qpack + ((size_t)tile * PT + r) * pack_rb + (size_t)ch * 16) = v;
    }
}

struct MsScanParams {
    const char *tok;
    unsigned rb;            // row pitch of the plane in bytes
    long long T;
    const char *qpack;
    unsigned q_rb;          // row pitch of the packed A tiles
    int nk;                 // K-slabs that hold the dim columns
    const int *item_off;
    int n_items;
    const unsigned *alive;  // or null
    const int *n_tiles, *row_q, *q_len, *q_tile;
    int only_q;             // >= 0: this question alone (its tile), into slot 0
    const float *tau;       // [Q], or null: -inf
    float *cand_s;
    int *cand_r;
    unsigned *cnt;
    unsigned cap;
    int R;
    long long n_chunks;     // chunks of the plane
    long long walk;         // chunks this launch visits: chunk i * n_chunks / walk for i in 0 .. walk
};

// the first i in [0, n) with off[i] >= v, else n
__device__ inline int ms_lower_bound(const int *off, int n, long long v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((long long)off[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// DT: MMRAG_F16, or MMRAG_F8E4M3 (code rows on both sides: maxima are taken in the accumulator domain and scaled by
// 2^-16, exactly, before the ascending sum, so sums and tau are similarities as in the fp16 instantiation)
template <int DT>
__global__ __launch_bounds__(256, 2) void maxsim_scan_kernel(const MsScanParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(PT == MMRAG_MAX_LATE_QUERY_TOKENS, "a question fits one A tile");
    static_assert(PT_LDS + 2 * PT * 4 + 32 <= 80 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    __shared__ float red[2][PT];
    __shared__ int trim[2][4];

    const int tid = threadIdx.x;
    // every thread reads the same table entries: all the branches below are uniform over the workgroup
    int tile = blockIdx.y;
    if (p.only_q >= 0) tile = p.q_tile[p.only_q];
    tile = __builtin_amdgcn_readfirstlane(tile);
    if (tile < 0 || tile >= p.n_tiles[0]) return;

    const long long chunk = (long long)blockIdx.x * p.n_chunks / p.walk;
    const long long row_lo = chunk * p.R;
    const long long row_hi = row_lo + p.R < p.T ? row_lo + p.R : p.T;
    // the items this chunk owns, [o0, o1), and the rows they span
    const int o0 = __builtin_amdgcn_readfirstlane(ms_lower_bound(p.item_off, p.n_items, row_lo));
    const int o1 = __builtin_amdgcn_readfirstlane(ms_lower_bound(p.item_off, p.n_items, row_hi));
    if (o0 >= o1) return;
    const int own_s = __builtin_amdgcn_readfirstlane(p.item_off[o0]);
    const int own_e = __builtin_amdgcn_readfirstlane(p.item_off[o1]);     // o1 <= n_items: the last owned item's end
    if (own_s < 0 || own_e <= own_s || (long long)own_e > p.T) return;

    const auto candidate = [&](int i, int s, int e) -> bool {
        return e - s >= 1 && e - s <= MMRAG_MAX_LATE_DOC_TOKENS && s >= own_s && e <= own_e &&
               (p.alive == nullptr || ((p.alive[i >> 5] >> (i & 31)) & 1u) != 0u);
    };
    // The walk is trimmed to the first and the last CANDIDATE among them, [i0, i1): dead, empty and over-long items at
    // either end are not fetched, and a chunk without a candidate fetches nothing.  (Such items between two candidates
    // are still walked.)  Each thread looks at every 256th item, then the waves and the workgroup fold.
    int c_lo = 0x7fffffff, c_hi = -1;
    for (int i = o0 + tid; i < o1; i += 256)
        if (candidate(i, p.item_off[i], p.item_off[i + 1])) {
            c_lo = i < c_lo ? i : c_lo;
            c_hi = i > c_hi ? i : c_hi;
        }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int ol = __shfl_xor(c_lo, m), oh = __shfl_xor(c_hi, m);
        c_lo = ol < c_lo ? ol : c_lo;
        c_hi = oh > c_hi ? oh : c_hi;
    }
    if ((tid & 63) == 0) {
        trim[0][tid >> 6] = c_lo;
        trim[1][tid >> 6] = c_hi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        c_lo = trim[0][w] < c_lo ? trim[0][w] : c_lo;
        c_hi = trim[1][w] > c_hi ? trim[1][w] : c_hi;
    }
    if (c_hi < 0) return;     // uniform: every thread read the same four pairs; nothing was fetched
    const int i0 = __builtin_amdgcn_readfirstlane(c_lo), i1 = __builtin_amdgcn_readfirstlane(c_hi) + 1;
    const int rs = __builtin_amdgcn_readfirstlane(p.item_off[i0]);
    const int re = __builtin_amdgcn_readfirstlane(p.item_off[i1]);
    if (re <= rs) return;     // candidates lie inside [own_s, own_e): only a malformed table gets here

    // thread r < 128: the question whose first token is packed row r of this tile
    int my_q = -1, my_len = 0;
    if (tid < PT) {
        my_q = p.row_q[tile * PT + tid];
        if (p.only_q >= 0 && my_q != p.only_q) my_q = -1;
        if (my_q >= 0) my_len = p.q_len[my_q];
        if (my_len < 1 || tid + my_len > PT) my_q = -1;    // the plan never writes such a row
    }
    const int my_slot = p.only_q >= 0 ? 0 : my_q;
    const float my_tau = my_q >= 0 && p.tau != nullptr ? p.tau[my_q] : NEG_INF;

    const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);
    const PairTileCtx c = pair_tile_ctx(tid, wave_id < 2 ? p.q_rb : p.rb, smem);
    const int wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;
    const int nct = (int)(((long long)re - rs + PT - 1) / PT);
    const PairTileSrc a_src = {p.qpack + (size_t)tile * PT * p.q_rb, (unsigned)PT * p.q_rb};
    const char *const b_base = p.tok + (size_t)rs * p.rb;
    // (the question tile, B tile ct of the walk): the B side is the one that moves
    const auto tile_src = [&](int ct) {
        const int b_left = re - rs - ct * PT;
        const PairTileSrc b_src = {b_base + (size_t)ct * PT * p.rb, (unsigned)(b_left < PT ? b_left : PT) * p.rb};
        return wave < 2 ? a_src : b_src;
    };

    // running maxima of this lane's question rows wm * 64 + 16 a + 4 g4 + r over the open item's columns it has seen
    float bv[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[a][r] = NEG_INF;

    int ci = i0;     // the first item not yet closed
    // ---- acc[a][b][r] = <question row wm*64 + 16a + 4 g4 + r, plane row r0 + wn*64 + 16b + c16>
    const auto tile_done = [&](int ct, const f32x4_t (&acc)[4][4]) {
        // columns are counted from the tile's first row r0 (r0 + 128 may not fit an int): the tile holds n_in rows
        const int r0 = rs + ct * PT;
        const int n_in = re - r0 < PT ? re - r0 : PT;
        const int col0 = wn * 64 + c16;
        while (ci < i1) {
            const int s = __builtin_amdgcn_readfirstlane(p.item_off[ci]);
            if (s >= re || s - r0 >= n_in) break;
            const int e = __builtin_amdgcn_readfirstlane(p.item_off[ci + 1]);
            if (e <= s) {
                // an empty item: on to the last item that starts at s, the next one with rows (or i1)
                int nx = ms_lower_bound(p.item_off + ci + 1, i1 - ci - 1, (long long)s + 1) + ci;
                ci = __builtin_amdgcn_readfirstlane(nx > ci ? nx : ci + 1);
                continue;
            }
            const bool cand = candidate(ci, s, e);
            if (cand) {
                const int lo = s > r0 ? s - r0 : 0, hi = e - r0 < n_in ? e - r0 : n_in;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int col = col0 + 16 * b;
                    const bool in = col >= lo && col < hi;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float v = in ? acc[a][b][r] : NEG_INF;
                            if (v > bv[a][r]) bv[a][r] = v;
                        }
                }
            }
            if (e - r0 > n_in) break;      // the item stays open: its maxima are carried into the next tile
            if (cand) {
                // ---- the item closes: fold the 16 lanes that hold other columns of the same rows, then the two waves
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = bv[a][r];
#pragma unroll
                        for (int m = 1; m < 16; m <<= 1) {
                            const float ov = __shfl_xor(v, m);
                            if (ov > v) v = ov;
                        }
                        if (c16 == 0) red[wn][wm * 64 + 16 * a + 4 * g4 + r] = v;
                        bv[a][r] = NEG_INF;
                    }
                __syncthreads();
                if (my_q >= 0) {
                    float sum = 0.0f;
                    for (int i = 0; i < my_len; ++i) {      // ascending i: the sum's bits are defined
                        const float v0 = red[0][tid + i], v1 = red[1][tid + i];
                        if constexpr (DT == MMRAG_F8E4M3) sum += (v1 > v0 ? v1 : v0) * PT_ACC_SCALE<DT>;
                        else sum += v1 > v0 ? v1 : v0;
                    }
                    if (sum >= my_tau) {
                        // the counter keeps the true count; slots at or past cap are not written
                        const unsigned at = atomicAdd(p.cnt + my_slot, 1u);
                        if (at < p.cap) {
                            p.cand_s[(size_t)my_slot * p.cap + at] = sum;
                            p.cand_r[(size_t)my_slot * p.cap + at] = ci;
                        }
                    }
                }
                __syncthreads();    // red is rewritten by the next item that closes
            }
            ++ci;
        }
    };
    // one ring per workgroup: no barrier after it
    pair_tile_ring<DT>(c, smem, p.nk, nct, tile_src, tile_done);
#endif
}

struct MsPlan {
    long long cap;          // candidate slots per question
    int n_stages;
    long long stage_chunks[MS_MAX_STAGES];
};

// candidate_select.h's make_bound_plan counted in items (survivors ~ k n / m for a bound from m sampled items), then
// turned into whole chunks under the assumption that items are spread evenly over the plane.  The bound is valid
// whatever the sample holds; only the number of survivors depends on it.
MsPlan make_ms_plan(long long n_items, long long n_chunks, int k, long long cap_override, unsigned dbg) {
    MsPlan pl;
    const long long C = candidate_capacity(k);
    pl.cap = cap_override > 0 && cap_override < C ? cap_override : C;
    pl.n_stages = 0;
    if (n_items <= C || (dbg & MS_DBG_NO_BOUND)) return pl;   // every item fits: no bound needed
    const long long target = (4LL * k * n_items + C - 1) / C;
    const auto chunks_of = [&](long long items) {
        long long ch = (items * n_chunks + n_items - 1) / n_items;
        return ch < 1 ? 1 : (ch > n_chunks ? n_chunks : ch);
    };
    long long m = MS_SAMPLE0_ITEMS < n_items ? MS_SAMPLE0_ITEMS : n_items;
    for (;;) {
        pl.stage_chunks[pl.n_stages++] = chunks_of(m);
        if (m >= target || pl.n_stages == MS_MAX_STAGES) break;
        long long nm = m * C / (4LL * k);
        if (nm > target) nm = target;
        if (nm > n_items) nm = n_items;
        if (nm <= m) break;
        m = nm;
    }
    return pl;
}

struct MsWs {
    CandWs cand;
    size_t off_ntiles, off_qtile, off_rowsrc, off_rowq, off_pack, total;
};

// [candidate_select's blocks | n_tiles | q_tile [Q] | row_src [Q, 128] | row_q [Q, 128] | packed A tiles]: `tiles` packed
// tiles of 128 rows of `pack_rb` bytes (2 dim for fp16 rows, dim for codes).  The public sizes are those of tiles = Q
// at dim 1024, an upper bound of every call's
inline MsWs ms_ws_layout(int Q, long long cap, long long n_items, int tiles, int pack_rb) {
    MsWs w;
    w.cand = candidate_ws_layout(Q, cap, n_items, true);
    w.off_ntiles = w.cand.total;
    w.off_qtile = w.off_ntiles + 256;
    w.off_rowsrc = align_up(w.off_qtile + (size_t)Q * sizeof(int), 256);
    w.off_rowq = w.off_rowsrc + (size_t)Q * PT * sizeof(int);
    w.off_pack = align_up(w.off_rowq + (size_t)Q * PT * sizeof(int), 1024);
    w.total = w.off_pack + (size_t)tiles * PT * (size_t)pack_rb;
    return w;
}

// bytes of a packed question row: the slabs that hold the dim columns (fp16: 2 dim, dim % 64 == 0; codes: the padded dim)
inline int ms_pack_rb(int dim, int dtype) { return stored_k_slabs(dim, dtype) * SLAB; }

// mmrag_maxsim_topk (DT = MMRAG_F16) and mmrag_maxsim_topk_f8 (MMRAG_F8E4M3) behind their _ex entries
template <int DT>
int maxsim_topk_impl(const char *who, const void *q_tok, int64_t q_rows, int64_t q_ld, const int32_t *q_start,
                     const int32_t *q_len, int Q, const void *tok, int64_t T, int64_t ld, const int32_t *item_off,
                     int64_t n_items, const uint32_t *alive_bits, int dim, int k, float *out_scores,
                     int64_t *out_items, void *workspace, size_t workspace_bytes, void *stream, int chunk_rows,
                     int64_t cap_override, unsigned dbg, int max_tiles) {
    MMRAG_CHECK_ARG(q_tok && q_start && q_len && item_off, "%s: null pointer", who);
    MMRAG_CHECK_ARG(out_scores && out_items, "%s: null output", who);
    MMRAG_CHECK_ARG(dim > 0 && dim % 64 == 0 && dim <= 1024,
                    "%s: dim must be a multiple of 64, at most 1024 (dim=%d)", who, dim);
    for (const int64_t w : {q_ld, ld})
        if (int st = DT == MMRAG_F8E4M3 ? check_code_rows(who, w, dim)
                                        : check_stored_rows(who, "scanned", "scan", w, DT, dim))
            return st;
    MMRAG_CHECK_ARG(Q >= 1 && Q <= MMRAG_MAX_LATE_QUESTIONS, "%s: Q=%d outside 1..%d", who, Q,
                    MMRAG_MAX_LATE_QUESTIONS);
    MMRAG_CHECK_ARG(n_items >= 0 && n_items < (1LL << 31) && T >= 0 && T < (1LL << 31) && q_rows >= 1 &&
                        q_rows < (1LL << 31),
                    "%s: need 0 <= n_items < 2^31, 0 <= T < 2^31 and 1 <= q_rows < 2^31 (n_items=%lld T=%lld "
                    "q_rows=%lld)", who, (long long)n_items, (long long)T, (long long)q_rows);
    MMRAG_CHECK_ARG(tok || T == 0, "%s: null token plane", who);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K_DEEP, "%s: k=%d outside 1..%d", who, k, MMRAG_MAX_K_DEEP);
    MMRAG_CHECK_ARG(((uintptr_t)q_tok % 16) == 0 && ((uintptr_t)tok % 16) == 0,
                    "%s: token rows must be 16-byte aligned", who);
    MMRAG_CHECK_ARG(chunk_rows >= 0 && max_tiles >= 0, "%s: chunk_rows=%d or max_tiles=%d is negative", who,
                    chunk_rows, max_tiles);
    const int tiles = max_tiles > 0 && max_tiles < Q ? max_tiles : Q;
    hipStream_t s = (hipStream_t)stream;
    if (n_items == 0 || T == 0) return candidate_fill_empty(out_scores, (long long *)out_items, Q, k, s);

    const int R = chunk_rows > 0 ? chunk_rows : MS_CHUNK_ROWS;
    const long long n_chunks = (T + R - 1) / R;
    const MsPlan pl = make_ms_plan(n_items, n_chunks, k, cap_override, dbg);
    const MsWs wl = ms_ws_layout(Q, pl.cap, n_items, tiles, ms_pack_rb(dim, DT));
    const size_t need = wl.total + 1024;
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu bytes < required %zu", who, workspace_bytes, need);
        return MMRAG_EWORKSPACE;
    }
    if (((uintptr_t)workspace % 16) != 0) {
        set_error("%s: workspace must be 16-byte aligned", who);
        return MMRAG_EWORKSPACE;
    }

    char *ws = (char *)workspace;
    unsigned *cnt = (unsigned *)(ws + wl.cand.off_cnt);
    float *tau = (float *)(ws + wl.cand.off_floats);
    char *qpack = (char *)align_up((size_t)(uintptr_t)(ws + wl.off_pack), 1024);

    // 1. plan and pack the question tiles, once for every pass
    MsPlanParams pp;
    pp.q_start = q_start, pp.q_len = q_len, pp.Q = Q, pp.q_rows = q_rows, pp.max_tiles = tiles;
    pp.n_tiles = (int *)(ws + wl.off_ntiles);
    pp.q_tile = (int *)(ws + wl.off_qtile);
    pp.row_src = (int *)(ws + wl.off_rowsrc);
    pp.row_q = (int *)(ws + wl.off_rowq);
    MMRAG_CHECK_HIP(hipMemsetAsync(pp.row_src, 0xff, 2 * (size_t)Q * PT * sizeof(int), s));
    hipLaunchKernelGGL(maxsim_plan_kernel, dim3(1), dim3(MS_PLAN_THREADS), 0, s, pp);
    MMRAG_CHECK_HIP(hipGetLastError());
    const unsigned q_rb = stored_row_bytes(q_ld, DT);
    const unsigned pack_rb = ms_pack_rb(dim, DT);
    hipLaunchKernelGGL(maxsim_pack_kernel, dim3((unsigned)tiles), dim3(256), 0, s, (const char *)q_tok, q_rb,
                       (const int *)pp.n_tiles, (const int *)pp.row_src, qpack, pack_rb);
    MMRAG_CHECK_HIP(hipGetLastError());

    MsScanParams p;
    p.tok = (const char *)tok;
    p.rb = stored_row_bytes(ld, DT);
    p.T = T;
    p.qpack = qpack;
    p.q_rb = pack_rb;
    p.nk = stored_k_slabs(dim, DT);
    p.item_off = item_off;
    p.n_items = (int)n_items;
    p.alive = alive_bits;
    p.n_tiles = pp.n_tiles, p.row_q = pp.row_q, p.q_len = q_len, p.q_tile = pp.q_tile;
    p.only_q = -1;
    p.tau = nullptr;
    p.cand_s = (float *)(ws + wl.cand.off_bs);
    p.cand_r = (int *)(ws + wl.cand.off_br);
    p.cnt = cnt;
    p.cap = (unsigned)pl.cap;
    p.R = R;
    p.n_chunks = n_chunks;
    p.walk = n_chunks;

    // the scan over `walk` chunks: every question tile (only_q < 0; `tiles` of them at most, the rest return at once), or the
    // tile of one question
    const auto produce = [&](int only_q, long long walk, float *cand_s, int *cand_r, unsigned *counts,
                             long long slots) -> int {
        MsScanParams pc = p;
        pc.only_q = only_q;
        pc.walk = walk;
        pc.cand_s = cand_s, pc.cand_r = cand_r, pc.cnt = counts;
        pc.cap = (unsigned)slots;
        hipLaunchKernelGGL(maxsim_scan_kernel<DT>, dim3((unsigned)walk, only_q >= 0 ? 1u : (unsigned)tiles), dim3(256), 0, s, pc);
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    };

    // 2. bound passes (tau starts at -inf: the bit pattern 0xff800000)
    if (pl.n_stages > 0) {
        MMRAG_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)tau, (int)0xff800000u, (size_t)Q, s));
        p.tau = tau;
    }
    for (int st = 0; st < pl.n_stages; ++st) {
        MMRAG_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)Q * sizeof(unsigned), s));
        if (int e = produce(-1, pl.stage_chunks[st], p.cand_s, p.cand_r, cnt, pl.cap)) return e;
        deep_select_kernel<<<Q, SEL_THREADS, 0, s>>>(p.cand_s, p.cand_r, cnt, pl.cap, k, 0, 1, nullptr, nullptr, tau);
        MMRAG_CHECK_HIP(hipGetLastError());
    }
    // 3. main pass over every chunk, select, and each question with more survivors than slots alone, same tau_q
    return candidate_select(
        who, Q, n_items, pl.cap, k, 0, out_scores, (long long *)out_items, ws, wl.cand, s,
        [&](float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return produce(-1, n_chunks, cand_s, cand_r, counts, slots);
        },
        [&](int qi, float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return produce(qi, n_chunks, cand_s, cand_r, counts, slots);
        });
}

}  // namespace
}  // namespace mmrag_impl

using namespace mmrag_impl;

extern "C" {

size_t mmrag_maxsim_topk_workspace_bytes(int Q, int64_t n_items, int k) {
    if (Q < 1 || Q > MMRAG_MAX_LATE_QUESTIONS || n_items < 0 || n_items >= (1LL << 31) || k < 1 || k > MMRAG_MAX_K_DEEP)
        return 0;
    return ms_ws_layout(Q, candidate_capacity(k), n_items, Q, 2 * 1024).total + 1024;   // + the slack that aligns the tiles
}

size_t mmrag_maxsim_topk_f8_workspace_bytes(int Q, int64_t n_items, int k) {
    if (mmrag_maxsim_topk_workspace_bytes(Q, n_items, k) == 0) return 0;
    return ms_ws_layout(Q, candidate_capacity(k), n_items, Q, 1024).total + 1024;
}

// what a call with this dim and at most max_tiles question tiles (0: Q) needs: the wrapper, which holds the host tables
size_t mmrag_internal_maxsim_topk_workspace_bytes_ex(int Q, int64_t n_items, int k, int dim, int max_tiles) {
    if (mmrag_maxsim_topk_workspace_bytes(Q, n_items, k) == 0 || dim <= 0 || dim % 64 != 0 || dim > 1024) return 0;
    const int tiles = max_tiles > 0 && max_tiles < Q ? max_tiles : Q;
    return ms_ws_layout(Q, candidate_capacity(k), n_items, tiles, ms_pack_rb(dim, MMRAG_F16)).total + 1024;
}

size_t mmrag_internal_maxsim_topk_f8_workspace_bytes_ex(int Q, int64_t n_items, int k, int dim, int max_tiles) {
    if (mmrag_maxsim_topk_workspace_bytes(Q, n_items, k) == 0 || dim <= 0 || dim % 64 != 0 || dim > 1024) return 0;
    const int tiles = max_tiles > 0 && max_tiles < Q ? max_tiles : Q;
    return ms_ws_layout(Q, candidate_capacity(k), n_items, tiles, ms_pack_rb(dim, MMRAG_F8E4M3)).total + 1024;
}

// mmrag_maxsim_topk with a chunk size (chunk_rows > 0), a smaller candidate capacity (cap_override > 0), debug
// switches (MS_DBG_*) and an upper bound of the question tiles (max_tiles > 0; a caller that holds the host tables
// knows it: the grid and the packed tiles are then sized by it instead of by Q, and a question the bound leaves no tile
// for gets padding only): the tests that pin chunk independence, the overflow re-run and the unbounded scan, and the bench.
// Exported for them, deliberately absent from include/mmrag.h.
int mmrag_internal_maxsim_topk_ex(const void *q_tok, int64_t q_rows, int64_t q_ld, const int32_t *q_start,
                                  const int32_t *q_len, int Q, const void *tok, int64_t T, int64_t ld,
                                  const int32_t *item_off, int64_t n_items, const uint32_t *alive_bits, int dim, int k,
                                  float *out_scores, int64_t *out_items, void *workspace, size_t workspace_bytes,
                                  void *stream, int chunk_rows, int64_t cap_override, unsigned dbg, int max_tiles) {
    return maxsim_topk_impl<MMRAG_F16>("maxsim_topk", q_tok, q_rows, q_ld, q_start, q_len, Q, tok, T, ld, item_off,
                                       n_items, alive_bits, dim, k, out_scores, out_items, workspace, workspace_bytes,
                                       stream, chunk_rows, cap_override, dbg, max_tiles);
}

// the same for code rows
int mmrag_internal_maxsim_topk_f8_ex(const void *q_codes, int64_t q_rows, int64_t q_ld, const int32_t *q_start,
                                     const int32_t *q_len, int Q, const void *codes, int64_t T, int64_t ld,
                                     const int32_t *item_off, int64_t n_items, const uint32_t *alive_bits, int dim,
                                     int k, float *out_scores, int64_t *out_items, void *workspace,
                                     size_t workspace_bytes, void *stream, int chunk_rows, int64_t cap_override,
                                     unsigned dbg, int max_tiles) {
    return maxsim_topk_impl<MMRAG_F8E4M3>("maxsim_topk_f8", q_codes, q_rows, q_ld, q_start, q_len, Q, codes, T, ld,
                                          item_off, n_items, alive_bits, dim, k, out_scores, out_items, workspace,
                                          workspace_bytes, stream, chunk_rows, cap_override, dbg, max_tiles);
}

int mmrag_maxsim_topk_f8(const void *q_codes, int64_t q_rows, int64_t q_ld, const int32_t *q_start,
                         const int32_t *q_len, int Q, const void *codes, int64_t T, int64_t ld,
                         const int32_t *item_off, int64_t n_items, const uint32_t *alive_bits, int dim, int k,
                         float *out_scores, int64_t *out_items, void *workspace, size_t workspace_bytes, void *stream) {
    return mmrag_internal_maxsim_topk_f8_ex(q_codes, q_rows, q_ld, q_start, q_len, Q, codes, T, ld, item_off, n_items,
                                            alive_bits, dim, k, out_scores, out_items, workspace, workspace_bytes,
                                            stream, 0, 0, 0u, 0);
}

int mmrag_maxsim_topk(const void *q_tok, int64_t q_rows, int64_t q_ld, const int32_t *q_start, const int32_t *q_len,
                      int Q, const void *tok, int64_t T, int64_t ld, const int32_t *item_off, int64_t n_items,
                      const uint32_t *alive_bits, int dim, int k, float *out_scores, int64_t *out_items,
                      void *workspace, size_t workspace_bytes, void *stream) {
    return mmrag_internal_maxsim_topk_ex(q_tok, q_rows, q_ld, q_start, q_len, Q, tok, T, ld, item_off, n_items,
                                         alive_bits, dim, k, out_scores, out_items, workspace, workspace_bytes, stream,
                                         0, 0, 0u, 0);
}

}  // extern "C"
