// Recommend top-k (include/mmrag.h mmrag_recommend_topk): a batch of requests against the stored rows, each request a
// group of up to 16 signed example vectors ("more like these, less like those"), ranked by
//   pos = max over the positive examples of <e, x>, neg = max over the negative ones (none: 0),
//   final = fmaf(-w, max(neg, 0), pos)
// formed INSIDE one exact scan.  With negatives the winners are often far down the positive ranking -- everything near
// the top sits next to a negative -- so the penalty cannot be applied to a finished list.
//
//   1. bound passes, only when n exceeds the candidate capacity: candidate_select.h's plan (whole 128-row tiles spread
//      evenly over the collection, stages growing), every live final >= tau_g appended; deep_select_kernel in its bound
//      mode then sets tau_g = max(tau_g, the k-th best of those).  The k-th best final of ANY subset of live rows is at
//      most the true k-th final whatever the score function is, so the argument boosted.hip gives for its prior carries
//      over to this score unchanged: tau_g stays a valid lower bound (-inf while fewer than k rows were seen).
//   2. main pass: every tile, every live final >= tau_g appended as (final, local row) through the request's counter.
//   3. select and overflow: an overflowed request is produced again alone (its 16 example rows as a batch of one)
//      with the same tau_g into n slots.  Steps 1 to 3 are candidate_select.h's bounded_scan_select; this file
//      supplies the producer.
//   4. finish: pos, neg and the slots that gave them, recomputed per winner with row_dot.h's wave_row_dot.
//
// scan kernel: boosted_scan_kernel's structure with the operands swapped.  E . X^T with pair_tile.h's body, a
// 128-EXAMPLE tile (8 requests of 16 slots) as A and a 128-row tile of stored rows as B; example rows past 16 R and
// stored rows past n read as zero through the buffer descriptor.  Workgroups are persistent over row tiles; a tile with
// no live row is skipped without a fetch; the ring runs over the K-slabs of all the example tiles without draining.
// In the accumulator acc[a][b][r] = <example 16 a + 4 g4 + r, stored row 16 b + c16> of the wave's quadrant, so a
// request is one 16-row `a` block: its max is in-lane over r, then two steps over g4 (lanes 32 apart, lanes 16 apart),
// once under the positive and once under the negative sign mask, where stored rows as A would need a 4-step reduction
// over c16 for each of a lane's 16 values.  The two steps are a reduce-scatter by v_permlane32_swap / v_permlane16_swap
// (24 swaps per wave and example tile, no LDS): lane group g4 ends with request a == g4 for its four stored-row
// columns: one final each, ONE reserving atomic per lane group (its hits counted by ballots), every surviving (request,
// row) appended exactly once.  Alive
// bits belong to columns.  Slots of sign 0 are masked by selection, never by arithmetic: whatever their rows hold does
// not reach a result.  The K order is slab_step's and max is exact, so a dot's bits depend on the example row, the
// stored row and d alone, and final's on the request's examples, signs and weight plus the stored row: not on the batch,
// the slot or tile the request sits in, the order of its examples, the grid, tau or whether bound passes ran.
#include "candidate_select.h"
#include "pair_tile.h"
#include "row_dot.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int RC_E = MMRAG_MAX_RECOMMEND_EXAMPLES;   // example slots of a request
constexpr int RC_REQ_TILE = PT / RC_E;               // requests of a 128-example tile
static_assert(RC_E == 16 && RC_REQ_TILE == 8, "a request is one 16-row MFMA block");

// debug switches of mmrag_internal_recommend_topk_ex (tests only)
constexpr unsigned RC_DBG_NO_BOUND = 1u;  // no bound passes: tau = -inf, every live row survives the main pass

struct RecommendParams {
    const char *rows;
    const char *ex;          // [16 R, ld]
    const signed char *sign; // [16 R], 4-byte aligned
    const float *negw;       // [R]
    long long n;
    int R;
    unsigned row_bytes;     // ld * element size, of the rows and of the examples
    int nk;                 // K-slabs that hold the d logical columns
    int net;                // example tiles, <= SCAN_MAX_TILES (512 requests)
    const unsigned *alive;
    const float *tau;       // [R], or null: -inf
    float *cand_s;
    int *cand_r;
    unsigned *cnt;
    unsigned cap;
    long long T;            // row tiles of the collection
    long long walk;         // tiles this launch visits: tile i * T / walk for i in 0 .. walk (walk == T: every tile)
};

static_assert(BOUND_TILE_ROWS == PT, "the bound stages are planned in this scan's tiles");

// x in the lanes below 32 and y in the lanes from 32 on, each joined with the same value of the lane 32 away:
// v_permlane32_swap trades the upper half of x with the lower half of y, so max of the pair is, in a lower lane l,
// max(x[l], x[l + 32]) and in an upper lane max(y[l - 32], y[l])
__device__ __forceinline__ float swap_max32(float x, float y) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
// the same one level down: v_permlane16_swap trades the odd 16-lane rows of x with the even rows of y, so an even row
// ends with max(x[row], x[row + 1]) and an odd row with max(y[row - 1], y[row])
__device__ __forceinline__ float swap_max16(float x, float y) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

template <int DT>
__global__ __launch_bounds__(256, 2) void recommend_scan_kernel(const RecommendParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];

    const unsigned RB = p.row_bytes;
    const PairTileCtx c = pair_tile_ctx(threadIdx.x, RB, smem);
    const int lane = c.lane, wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;
    const int net = p.net;
    const long long n_ex = (long long)p.R * RC_E;

    for (long long i = blockIdx.x; i < p.walk; i += gridDim.x) {
        const PairRowTile rt = pair_row_tile(i, p.T, p.walk, p.n);
        const long long row0 = rt.row0;
        unsigned long long m0, m1;
        pair_tile_live_rows(row0, lane, p.n, p.alive, m0, m1);
        // uniform: the whole workgroup takes this path; nothing was fetched, no LDS is touched
        if ((m0 | m1) == 0ull) continue;

        const PairTileSrc rows_src = {p.rows + (size_t)row0 * RB, (unsigned)rt.rows * RB};
        const unsigned long long mw = wn ? m1 : m0;      // this wave's 64 stored-row columns
        // bit b of `vis` = column 16 b + c16 of the wave's 64 is live
        unsigned vis = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) vis |= (unsigned)((mw >> (16 * b + c16)) & 1ull) << b;
        const int lrow0 = (int)row0 + wn * 64 + c16;     // n < 2^31 (the entry point's check)

        // what the epilogue of an example tile reads from memory, fetched a whole tile of K-slabs ahead so that it waits
        // for none of it: the signs of this lane's four slots 4 g4 .. 4 g4 + 3 of the wave's requests a = 0 .. 3 (one
        // aligned word each; a request past R has none), and weight and tau of request a == g4
        unsigned sw[4];
        float w_rq = 0.0f, t_rq = NEG_INF;
        auto fetch_requests = [&](int et_) {
            const int req_w = et_ * RC_REQ_TILE + wm * 4;
#pragma unroll
            for (int a = 0; a < 4; ++a)
                sw[a] = req_w + a < p.R ? *(const unsigned *)(p.sign + (size_t)(req_w + a) * RC_E + 4 * g4) : 0u;
            if (req_w + g4 < p.R) {
                w_rq = p.negw[req_w + g4];
                t_rq = p.tau != nullptr ? p.tau[req_w + g4] : NEG_INF;
            }
        };

        // (example tile et, this row tile): the A side is the one that moves
        const auto tile_src = [&](int et) {
            const long long e_left = n_ex - (long long)et * PT;
            const PairTileSrc ex_src = {p.ex + (size_t)et * PT * RB, (unsigned)(e_left < PT ? e_left : PT) * RB};
            return wave < 2 ? ex_src : rows_src;
        };
        // ---- acc[a][b][r] = <example et * 128 + wm*64 + 16a + 4 g4 + r, row col 16b + c16>
        const auto tile_done = [&](int et, const f32x4_t (&acc)[4][4]) {
            if (mw != 0ull) {       // wave-uniform: every lane takes part in the shuffles below
                const int req_w = et * RC_REQ_TILE + wm * 4;    // request of this wave's block a = 0
                // in-lane: the sign-masked maxima over this lane's four slots 4 g4 .. 4 g4 + 3 of request a, column b
                float pv[4][4], nv[4][4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    bool is_p[4], is_n[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int sg = (int)(signed char)(sw[a] >> (8 * r));
                        is_p[r] = sg > 0;
                        is_n[r] = sg < 0;
                    }
                    // uniform: a request without a negative ("nearest to any of these") skips that half
                    const bool any_neg = __builtin_amdgcn_ballot_w64((sw[a] & 0x80808080u) != 0u) != 0ull;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        // selection: a slot of sign 0 never reaches a result
                        pv[a][b] = fmaxf(fmaxf(is_p[0] ? acc[a][b][0] : NEG_INF, is_p[1] ? acc[a][b][1] : NEG_INF),
                                         fmaxf(is_p[2] ? acc[a][b][2] : NEG_INF, is_p[3] ? acc[a][b][3] : NEG_INF));
                        nv[a][b] = NEG_INF;
                        if (any_neg)
                            nv[a][b] = fmaxf(fmaxf(is_n[0] ? acc[a][b][0] : NEG_INF, is_n[1] ? acc[a][b][1] : NEG_INF),
                                             fmaxf(is_n[2] ? acc[a][b][2] : NEG_INF, is_n[3] ? acc[a][b][3] : NEG_INF));
                    }
                }
                // across g4, a reduce-scatter in two swaps: lanes l and l + 32 trade the halves a < 2 / a >= 2, then
                // the 16-lane rows 2j and 2j + 1 trade a even / a odd, so lane group g4 ends with the maxima of request
                // a == g4 over all 16 slots.  max is exact: the order does not reach the bits.
                float my_pos[4], my_neg[4];                    // of request req_w + g4, per column b
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float p0 = swap_max32(pv[0][b], pv[2][b]), p1 = swap_max32(pv[1][b], pv[3][b]);
                    const float n0 = swap_max32(nv[0][b], nv[2][b]), n1 = swap_max32(nv[1][b], nv[3][b]);
                    my_pos[b] = swap_max16(p0, p1);
                    my_neg[b] = swap_max16(n0, n1);
                }
                const int rq = req_w + g4;
                const float w = w_rq, t = t_rq;
                float fin[4];
                unsigned hit = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    // no negative: max(-inf, 0) = 0 and final = pos exactly; one rounding otherwise
                    const float f = __builtin_fmaf(-w, fmaxf(my_neg[b], 0.0f), my_pos[b]);
                    fin[b] = f;
                    // a request without a positive has pos = -inf: nothing is appended, its answer is padding
                    hit |= (unsigned)(f >= t && f > NEG_INF) << b;
                }
                hit &= vis;
                if (rq >= p.R) hit = 0u;
                // uniform: most waves of a main pass have no survivor at all
                if (__builtin_amdgcn_ballot_w64(hit != 0u) != 0ull) {
                    // ONE reservation per lane group: its 16 lanes share the request and so the counter, and a batch
                    // has only R counters, so a returning atomic per lane queues up 16 deep on one address (measured:
                    // the bound pass, where every live row survives, took three times the boosted scan's).  The
                    // group's hits are counted from four ballots, column block by column block; lane c16 == 0
                    // reserves them all and hands the base back.  The counter keeps the true count, slots at or past
                    // cap are not written.
                    unsigned off[4], total = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const unsigned long long m = __builtin_amdgcn_ballot_w64(((hit >> b) & 1u) != 0u);
                        const unsigned grp = (unsigned)(m >> (16 * g4)) & 0xffffu;
                        off[b] = total + (unsigned)__popc(grp & ((1u << c16) - 1u));
                        total += (unsigned)__popc(grp);
                    }
                    unsigned base = 0;
                    if (c16 == 0 && total != 0u) base = atomicAdd(p.cnt + rq, total);     // total != 0 only with rq < R
                    base = (unsigned)__shfl((int)base, lane & 48);
                    if (hit != 0u) {
                        float *bs = p.cand_s + (size_t)rq * p.cap;
                        int *br = p.cand_r + (size_t)rq * p.cap;
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const unsigned at = base + off[b];
                            if (((hit >> b) & 1u) && at < p.cap) {
                                bs[at] = fin[b];
                                br[at] = lrow0 + 16 * b;
                            }
                        }
                    }
                }
            }
            // the next example tile's request words, a whole tile of K-slabs ahead of their use
            if (et + 1 < net) fetch_requests(et + 1);
        };
        fetch_requests(0);
        pair_tile_ring<DT>(c, smem, p.nk, net, tile_src, tile_done);
        __syncthreads();   // the ring's contract: every wave is done with it before the next tile's first slab lands
    }
#endif
}

// One wave per winner i = (request g, place): the dots of the request's used slots against the winning row with
// wave_row_dot, pos / neg = the largest of each sign (the lowest slot on equal dots), neg = 0 and arg = -1 without a
// negative; padding gets 0 / -1.  Every output may be null.
template <typename T>
__global__ __launch_bounds__(256) void recommend_finish_kernel(const long long *__restrict__ out_r, const T *__restrict__ ex,
                                                              const T *__restrict__ rows,
                                                              const signed char *__restrict__ sign, long long ld, int d,
                                                              long long row_offset, long long n, int k, long long total,
                                                              float *__restrict__ out_pos, float *__restrict__ out_neg,
                                                              int *__restrict__ out_pos_arg,
                                                              int *__restrict__ out_neg_arg) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);     // wave-uniform
    if (i >= total) return;
    const long long g = i / k;
    const long long local = out_r[i] - row_offset;
    float pos = 0.0f, neg = 0.0f;
    int pa = -1, na = -1;
    if (out_r[i] >= 0 && local >= 0 && local < n) {
        const T *x = rows + (size_t)local * ld;
        for (int e = 0; e < RC_E; ++e) {
            const int sg = sign[g * RC_E + e];      // uniform
            if (sg == 0) continue;
            const float v = wave_row_dot(ex + (size_t)(g * RC_E + e) * ld, x, d, lane);
            if (sg > 0) {
                if (pa < 0 || v > pos) {
                    pos = v;
                    pa = e;
                }
            } else if (na < 0 || v > neg) {
                neg = v;
                na = e;
            }
        }
    }
    if (lane == 0) {
        if (out_pos) out_pos[i] = pos;
        if (out_neg) out_neg[i] = neg;
        if (out_pos_arg) out_pos_arg[i] = pa;
        if (out_neg_arg) out_neg_arg[i] = na;
    }
}

template <int DT>
int launch_scan(const RecommendParams &p, hipStream_t s) {
    hipLaunchKernelGGL(recommend_scan_kernel<DT>, dim3(scan_grid(p.walk)), dim3(256), 0, s, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

size_t mmrag_recommend_topk_workspace_bytes(int R, int64_t n, int k) {
    if (R <= 0 || R > (1 << 20) || n < 0 || n >= (1LL << 31) || k < 1 || k > MMRAG_MAX_K_DEEP) return 0;
    return bounded_scan_layout(R, n, k, 0, false).select_bytes;
}

// mmrag_recommend_topk with a smaller candidate capacity (cap_override > 0) and debug switches (RC_DBG_*): the tests
// that pin the overflow re-run and the unbounded scan.  Exported for them, deliberately absent from include/mmrag.h.
int mmrag_internal_recommend_topk_ex(const void *examples, const int8_t *sign, const float *neg_weight, const void *rows,
                                     int R, int64_t n, int d, int64_t ld, int dtype, int k, int64_t row_offset,
                                     const uint32_t *alive_bits, float *out_scores, int64_t *out_rows, float *out_pos,
                                     float *out_neg, int32_t *out_pos_arg, int32_t *out_neg_arg, void *workspace,
                                     size_t workspace_bytes, void *stream, int64_t cap_override, unsigned dbg) {
    MMRAG_CHECK_ARG(examples && sign && neg_weight && rows, "recommend_topk: null pointer");
    MMRAG_CHECK_ARG(out_scores && out_rows, "recommend_topk: null output");
    if (int st = check_stored_rows("recommend_topk", "searched by examples", "search", ld, dtype, d, &n)) return st;
    MMRAG_CHECK_ARG(n < (1LL << 31), "recommend_topk: need n < 2^31 (n=%lld)", (long long)n);
    // (R workgroups of the select, R * k / 4 of the finish launch: both within a grid)
    MMRAG_CHECK_ARG(R >= 1 && R <= (1 << 20), "recommend_topk: need 1 <= R <= 2^20 (R=%d)", R);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K_DEEP, "recommend_topk: k=%d outside 1..%d", k, MMRAG_MAX_K_DEEP);
    MMRAG_CHECK_ARG(((uintptr_t)sign % 4) == 0, "recommend_topk: sign must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long total_out = (long long)R * k;
    const bool explain = out_pos || out_neg || out_pos_arg || out_neg_arg;
    const auto finish = [&]() -> int {
        if (!explain) return MMRAG_OK;
        const unsigned blocks = (unsigned)((total_out + 3) / 4);
        return with_elem_type(dtype, [&](auto tag) -> int {
            using T = elem_t<decltype(tag)::value>;
            recommend_finish_kernel<T><<<blocks, 256, 0, s>>>((const long long *)out_rows, (const T *)examples,
                                                              (const T *)rows, (const signed char *)sign, ld, d,
                                                              row_offset, n, k, total_out, out_pos, out_neg, out_pos_arg,
                                                              out_neg_arg);
            MMRAG_CHECK_HIP(hipGetLastError());
            return MMRAG_OK;
        });
    };
    if (n == 0) {
        if (int st = candidate_fill_empty(out_scores, (long long *)out_rows, R, k, s)) return st;
        return finish();     // every row is -1: all padding
    }

    RecommendParams p;
    p.rows = (const char *)rows;
    p.n = n;
    p.row_bytes = stored_row_bytes(ld, dtype);
    p.nk = stored_k_slabs(d, dtype);
    p.alive = alive_bits;
    p.T = (n + PT - 1) / PT;
    // requests g0 .. g0 + Rq of the caller's batch over `walk` tiles into their slots.  A request alone is its 16
    // example rows as a batch of one.
    const auto produce = [&](ScanPass, int g0, int Rq, long long walk, const float *tau, float *cand_s, int *cand_r,
                             unsigned *counts, long long slots) -> int {
        return for_scan_chunks(Rq, RC_REQ_TILE, [&](int first, int Rc, int net, int) -> int {
            RecommendParams pc = p;
            const int c0 = g0 + first;
            pc.ex = (const char *)examples + (size_t)c0 * RC_E * p.row_bytes;
            pc.sign = (const signed char *)sign + (size_t)c0 * RC_E;
            pc.negw = neg_weight + c0;
            pc.tau = tau != nullptr ? tau + c0 : nullptr;
            pc.R = Rc;
            pc.net = net;
            pc.walk = walk;
            pc.cap = (unsigned)slots;
            pc.cand_s = cand_s + (size_t)first * slots;
            pc.cand_r = cand_r + (size_t)first * slots;
            pc.cnt = counts + first;
            return with_elem_type(dtype, [&](auto tag) { return launch_scan<decltype(tag)::value>(pc, s); });
        });
    };
    if (int st = bounded_scan_select("recommend_topk", R, n, k, cap_override, (dbg & RC_DBG_NO_BOUND) != 0u, row_offset,
                                     nullptr, out_scores, (long long *)out_rows, workspace, workspace_bytes, 0, s,
                                     [](char *) { return MMRAG_OK; }, produce))
        return st;
    return finish();
}

int mmrag_recommend_topk(const void *examples, const int8_t *sign, const float *neg_weight, const void *rows, int R,
                         int64_t n, int d, int64_t ld, int dtype, int k, int64_t row_offset, const uint32_t *alive_bits,
                         float *out_scores, int64_t *out_rows, float *out_pos, float *out_neg, int32_t *out_pos_arg,
                         int32_t *out_neg_arg, void *workspace, size_t workspace_bytes, void *stream) {
    return mmrag_internal_recommend_topk_ex(examples, sign, neg_weight, rows, R, n, d, ld, dtype, k, row_offset,
                                            alive_bits, out_scores, out_rows, out_pos, out_neg, out_pos_arg, out_neg_arg,
                                            workspace, workspace_bytes, stream, 0, 0u);
}

}  // extern "C"
