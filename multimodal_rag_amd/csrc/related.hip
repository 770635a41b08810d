// Related-document retrieval (include/mmrag.h mmrag_related_groups, where the definition is): S sets of vectors (M
// columns in all) against every stored group (document) in one exact scan --
//     best[a][g] = max over the candidate rows r of g of <A_a, x_r>,   similarity[s][g] = mean over the set's a.
//
// zero fill: table[a][g], one 64-bit key per (column, group), 0 = "no candidate row".
//
// scan launch: A . X^T with pair_tile.h's body, scoped_scan_kernel's structure: a 128-row tile of stored rows as A, a
// 128-column tile of the sets as B, persistent workgroups over row tiles, the ring running over the K-slabs of all
// column tiles without a drain.  Every wave reads the tile's 128 ordinals (two per lane; past n, dead and out-of-range
// rows as -1); a row tile with no candidate row is skipped before anything is fetched.  After a column tile's last slab
// a lane walks its 16 rows in row order for each of its 4 columns, keeps the maximum key while the ordinal repeats, and
// ends each run with ONE atomicMax of
//     key = (monotone_u32(dot) << 32) | (0xFFFFFFFF - row)
// into table[a][g].  monotone_u32 (deep_select.h's map: -0 as +0, then flip all bits of a negative, set the sign bit
// of the rest) orders as the floats do, so the maximum key is the maximum dot and, among equal dots, the LOWEST row.  A
// maximum is associative and commutative: the table after the scan is a pure function of the inputs whatever the grid,
// the batch or the order the atomics arrive in.  Rows arrive in ingest order, a document's chunks are contiguous, so a
// lane's 16 rows are one or two runs.
//
// finish launch: one thread per (set, group) reads the set's columns of table[:, g] in ascending a, forms the float64
// sum and appends (similarity, ordinal) as a candidate of the set; a group with no candidate row and the set's excluded
// group append nothing.
//
// select: candidate_select.h's driver, unchanged, with the ordinals in the place of rows and n_groups slots per set
// (nothing can overflow, so it never synchronises).
//
// gather launch: the winners' ordinals as int32, their coverage counts, and best / best_row of every column for each
// winner of the column's set.
#include "candidate_select.h"
#include "pair_tile.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int RL_MAX_ROWS = MMRAG_MAX_RELATED_ROWS;
constexpr int RL_MAX_SETS = MMRAG_MAX_RELATED_SETS;
static_assert(RL_MAX_ROWS == SCAN_MAX_TILES * PT, "one scan launch holds every column tile");

struct RelatedParams {
    const char *rows;
    const char *q;          // the sets' columns [M, ld]
    long long n;
    int M;
    unsigned row_bytes;     // ld * element size, of the rows and of the columns
    int nk;                 // K-slabs that hold the d logical columns
    int nqt;                // column tiles, <= SCAN_MAX_TILES
    const unsigned *alive;
    const int *group_of_row;
    int n_groups;
    unsigned long long *table;      // [M, n_groups]
    long long T;            // row tiles
};

__device__ __forceinline__ unsigned long long related_key(float s, unsigned row) {
    unsigned u = s == 0.0f ? 0u : __float_as_uint(s);       // -0 and +0 tie (then the lower row wins)
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (0xFFFFFFFFu - row);
}

template <int DT>
__global__ __launch_bounds__(256, 2) void related_scan_kernel(const RelatedParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];

    const unsigned RB = p.row_bytes;
    const PairTileCtx c = pair_tile_ctx(threadIdx.x, RB, smem);
    const int lane = c.lane, wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;
    const size_t NG = (size_t)p.n_groups;

    for (long long tile = blockIdx.x; tile < p.T; tile += gridDim.x) {
        const PairRowTile rt = pair_row_tile(tile, p.T, p.T, p.n);
        const long long row0 = rt.row0;
        // ordinals of rows `lane` and `lane + 64` of the tile: -1 = past n, dead, in no group
        int ord[2];
        pair_tile_row_ordinals(row0, lane, p.n, p.alive, p.group_of_row, p.n_groups, ord);
        // uniform (the same two ballots in all four waves): no candidate row, nothing is fetched, no LDS is touched
        const unsigned long long m0 = __builtin_amdgcn_ballot_w64(ord[0] >= 0);
        const unsigned long long m1 = __builtin_amdgcn_ballot_w64(ord[1] >= 0);
        if ((m0 | m1) == 0ull) continue;

        const PairTileSrc rows_src = {p.rows + (size_t)row0 * RB, (unsigned)rt.rows * RB};
        // (this row tile, column tile qt)
        const auto tile_src = [&](int qt) {
            const int q_left = p.M - qt * PT;
            const PairTileSrc q_src = {p.q + (size_t)qt * PT * RB, (unsigned)(q_left < PT ? q_left : PT) * RB};
            return wave < 2 ? rows_src : q_src;
        };
        // ---- acc[a][b][r] = <row wm*64 + 16a + 4 g4 + r, column qt * 128 + wn*64 + 16b + c16>
        const auto tile_done = [&](int qt, const f32x4_t (&acc)[4][4]) {
            const unsigned long long mw = wm ? m1 : m0;      // this wave's 64 rows
            const int ow = wm ? ord[1] : ord[0];
            if (mw != 0ull) {
                // this lane's 16 rows in row order: j = 4a + r is row 16a + 4 g4 + r of the wave's 64
                int my_ord[16];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) my_ord[4 * a + r] = __shfl(ow, 16 * a + 4 * g4 + r);
                const unsigned lrow0 = (unsigned)row0 + wm * 64 + 4 * g4;      // n < 2^31 (the entry point's check)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int col = qt * PT + wn * 64 + 16 * b + c16;
                    if (col >= p.M) continue;
                    unsigned long long *const cell = p.table + (size_t)col * NG;
                    int run = -1;                   // the ordinal of the open run, -1 = none
                    unsigned long long best = 0;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int o = my_ord[4 * a + r];
                            if (o < 0) continue;
                            const unsigned long long key = related_key(acc[a][b][r], lrow0 + 16 * a + r);
                            if (o == run) {
                                best = key > best ? key : best;
                            } else {
                                if (run >= 0) atomicMax(cell + run, best);
                                run = o;
                                best = key;
                            }
                        }
                    if (run >= 0) atomicMax(cell + run, best);
                }
            }
        };
        pair_tile_ring<DT>(c, smem, p.nk, p.nqt, tile_src, tile_done);
        __syncthreads();   // the ring's contract: every wave is done with it before the next tile's first slab lands
    }
#endif
}

template <int DT>
int launch_scan(const RelatedParams &p, long long grid, hipStream_t s) {
    const unsigned g = grid > 0 ? (unsigned)(grid < p.T ? grid : p.T) : scan_grid(p.T);   // `grid`: the test's
    hipLaunchKernelGGL(related_scan_kernel<DT>, dim3(g), dim3(256), 0, s, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

__device__ __forceinline__ float related_key_score(unsigned long long key) { return deep_key_score(key); }

// set s's columns [lo, hi) or false: offsets that do not ascend inside 0..M own nothing
__device__ __forceinline__ bool related_set_range(const int *set_off, int s, int M, int &lo, int &hi) {
    lo = set_off[s];
    hi = set_off[s + 1];
    return lo >= 0 && hi > lo && hi <= M;
}

// one thread per (set, group): the set's candidate (similarity, ordinal), appended through the set's counter.  The
// slot a candidate lands in depends on the arrival order; the select's result does not (its keys are distinct).
__global__ __launch_bounds__(256) void related_finish_kernel(const unsigned long long *__restrict__ table, int M,
                                                             const int *__restrict__ set_off, int S, int n_groups,
                                                             const int *__restrict__ exclude, float *cand_s, int *cand_r,
                                                             unsigned *cnt, long long cap) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)S * n_groups) return;
    const int s = (int)(idx / n_groups), g = (int)(idx % n_groups);
    int lo, hi;
    if (!related_set_range(set_off, s, M, lo, hi) || g == exclude[s]) return;
    const unsigned long long *col = table + g;
    if (col[(size_t)lo * n_groups] == 0ull) return;      // no candidate row: every column of the table says so
    double sum = 0.0;
    for (int a = lo; a < hi; ++a) sum += (double)related_key_score(col[(size_t)a * n_groups]);
    const unsigned at = atomicAdd(cnt + s, 1u);          // < n_groups <= cap
    cand_s[(size_t)s * cap + at] = (float)(sum / (double)(hi - lo));
    cand_r[(size_t)s * cap + at] = g;
}

// threads 0 .. S k: out_group / out_covered of winner j of set s; threads S k .. S k + M k: out_best / out_best_row of
// column a for winner j of a's set
__global__ __launch_bounds__(256) void related_gather_kernel(const unsigned long long *__restrict__ table, int M,
                                                             const int *__restrict__ set_off, int S, int n_groups,
                                                             float threshold, int k, const long long *__restrict__ sel_g,
                                                             int *out_group, int *out_covered, float *out_best,
                                                             long long *out_best_row) {
    long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long heads = (long long)S * k;
    if (idx < heads) {
        const int s = (int)(idx / k);
        const int g = (int)sel_g[idx];
        int lo, hi, covered = 0;
        if (g >= 0 && related_set_range(set_off, s, M, lo, hi))
            for (int a = lo; a < hi; ++a)
                covered += related_key_score(table[(size_t)a * n_groups + g]) >= threshold ? 1 : 0;
        out_group[idx] = g;
        out_covered[idx] = covered;
        return;
    }
    idx -= heads;
    if (idx >= (long long)M * k) return;
    const int a = (int)(idx / k), j = (int)(idx % k);
    float best = NEG_INF;
    long long row = -1;
    for (int s = 0; s < S; ++s) {
        int lo, hi;
        if (!related_set_range(set_off, s, M, lo, hi) || a < lo || a >= hi) continue;
        const int g = (int)sel_g[(size_t)s * k + j];
        if (g >= 0) {
            const unsigned long long key = table[(size_t)a * n_groups + g];
            best = related_key_score(key);
            row = (long long)(0xFFFFFFFFu - (unsigned)key);
        }
        break;
    }
    out_best[idx] = best;
    out_best_row[idx] = row;
}

struct RelatedWs {
    CandWs cand;
    size_t off_sel, off_table, total;
};

// [the candidate driver's blocks | S x k winners' ordinals (int64) | table M x n_groups keys]
inline RelatedWs related_ws_layout(int M, int S, int n_groups, int k) {
    RelatedWs w;
    const long long cap = n_groups > 0 ? n_groups : 1;
    w.cand = candidate_ws_layout(S, cap, 0, false);
    w.off_sel = w.cand.total;
    w.off_table = align_up(w.off_sel + (size_t)S * k * sizeof(long long), 256);
    w.total = align_up(w.off_table + (size_t)M * n_groups * sizeof(unsigned long long), 256);
    return w;
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

size_t mmrag_related_groups_workspace_bytes(int M, int S, int64_t n, int n_groups, int k) {
    if (M < 0 || M > RL_MAX_ROWS || S < 1 || S > RL_MAX_SETS || n < 0 || n >= (1LL << 31) || n_groups < 0 || k < 1 ||
        k > MMRAG_MAX_K_DEEP)
        return 0;
    return related_ws_layout(M, S, n_groups, k).total;
}

// mmrag_related_groups with the scan's grid given (grid > 0): the test that pins "not a function of the grid".  Exported
// for it, deliberately absent from include/mmrag.h.
int mmrag_internal_related_groups_ex(const void *set_rows, int M, const int32_t *set_off, int S, const void *rows,
                                     int64_t n, int d, int64_t ld, int dtype, const uint32_t *alive_bits,
                                     const int32_t *group_of_row, int n_groups, const int32_t *exclude_group,
                                     float threshold, int k, float *out_similarity, int32_t *out_group,
                                     int32_t *out_covered, float *out_best, int64_t *out_best_row, void *workspace,
                                     size_t workspace_bytes, void *stream, int64_t grid) {
    MMRAG_CHECK_ARG(set_rows && set_off && rows && group_of_row && exclude_group, "related_groups: null pointer");
    MMRAG_CHECK_ARG(out_similarity && out_group && out_covered && out_best && out_best_row,
                    "related_groups: null output");
    if (int st = check_stored_rows("related_groups", "compared by document", "compare", ld, dtype, d, &n)) return st;
    MMRAG_CHECK_ARG(n < (1LL << 31), "related_groups: need n < 2^31 (n=%lld)", (long long)n);
    MMRAG_CHECK_ARG(M >= 0 && M <= RL_MAX_ROWS, "related_groups: M=%d outside 0..%d", M, RL_MAX_ROWS);
    MMRAG_CHECK_ARG(S >= 1 && S <= RL_MAX_SETS, "related_groups: S=%d outside 1..%d", S, RL_MAX_SETS);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K_DEEP, "related_groups: k=%d outside 1..%d", k, MMRAG_MAX_K_DEEP);
    MMRAG_CHECK_ARG(n_groups >= 0, "related_groups: need n_groups >= 0 (n_groups=%d)", n_groups);
    MMRAG_CHECK_ARG(!(threshold != threshold), "related_groups: threshold is not a number");
    const RelatedWs wl = related_ws_layout(M, S, n_groups, k);
    MMRAG_CHECK_ARG(workspace && workspace_bytes >= wl.total, "related_groups: workspace %zu bytes < required %zu",
                    workspace_bytes, wl.total);
    MMRAG_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "related_groups: workspace must be 16-byte aligned");

    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    long long *sel_g = (long long *)(ws + wl.off_sel);
    unsigned long long *table = (unsigned long long *)(ws + wl.off_table);
    const long long outs = (long long)S * k + (long long)M * k;
    const auto gather = [&]() -> int {
        hipLaunchKernelGGL(related_gather_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, table, M,
                           set_off, S, n_groups, threshold, k, sel_g, out_group, out_covered, out_best, (long long *)out_best_row);
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    };
    if (n == 0 || n_groups == 0 || M == 0) {
        // nothing can match: padding only (the gather reads no cell of the table for a winner of -1)
        if (int st = candidate_fill_empty(out_similarity, sel_g, S, k, s)) return st;
        return gather();
    }

    RelatedParams p;
    p.rows = (const char *)rows;
    p.q = (const char *)set_rows;
    p.n = n;
    p.M = M;
    p.row_bytes = stored_row_bytes(ld, dtype);
    p.nk = stored_k_slabs(d, dtype);
    p.nqt = (M + PT - 1) / PT;
    p.alive = alive_bits;
    p.group_of_row = group_of_row;
    p.n_groups = n_groups;
    p.table = table;
    p.T = (n + PT - 1) / PT;
    MMRAG_CHECK_HIP(hipMemsetAsync(table, 0, (size_t)M * n_groups * sizeof(unsigned long long), s));
    if (int st = with_elem_type(dtype, [&](auto tag) { return launch_scan<decltype(tag)::value>(p, grid, s); }))
        return st;

    const long long cells = (long long)S * n_groups;
    if (int st = candidate_select(
            "related_groups", S, n_groups, n_groups, k, 0, out_similarity, sel_g, ws, wl.cand, s,
            [&](float *cand_s, int *cand_r, unsigned *counts, long long slots) -> int {
                hipLaunchKernelGGL(related_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, table,
                                   M, set_off, S, n_groups, exclude_group, cand_s, cand_r, counts, slots);
                MMRAG_CHECK_HIP(hipGetLastError());
                return MMRAG_OK;
            },
            // never called: a set has at most n_groups candidates and n_groups slots
            [&](int, float *, int *, unsigned *, long long) -> int { return MMRAG_OK; }))
        return st;
    return gather();
}

int mmrag_related_groups(const void *set_rows, int M, const int32_t *set_off, int S, const void *rows, int64_t n, int d,
                         int64_t ld, int dtype, const uint32_t *alive_bits, const int32_t *group_of_row, int n_groups,
                         const int32_t *exclude_group, float threshold, int k, float *out_similarity, int32_t *out_group,
                         int32_t *out_covered, float *out_best, int64_t *out_best_row, void *workspace,
                         size_t workspace_bytes, void *stream) {
    return mmrag_internal_related_groups_ex(set_rows, M, set_off, S, rows, n, d, ld, dtype, alive_bits, group_of_row,
                                            n_groups, exclude_group, threshold, k, out_similarity, out_group,
                                            out_covered, out_best, out_best_row, workspace, workspace_bytes, stream, 0);
}

}  // extern "C"
