// Extractive selection by sentence centrality (include/mmrag.h mmrag_summary_select): LexRank
// centrality over the sentences of one unit, then a budgeted maximal-marginal-relevance selection.
//
// One workgroup of 256 threads per unit (at most 128 sentences).  The unit's rows are BOTH tiles of one pair of
// pair_tile.h's body: the buffer descriptor ends at the unit's last row, so rows >= n read as zero whatever follows
// them in the plane, and they are dropped by INDEX afterwards (no loop below reaches them), as maxsim.hip does.  A bias
// row is a second ring item, a one-row B tile: s_i = <x_i, q> has the arithmetic of S_ij.  The epilogue writes the 64
// accumulators of every lane into a 128 x 128 float32 matrix in LDS; nothing is read from global memory after that and
// no dot product is computed twice.
//
// LDS: the matrix (64 KiB) lies NEXT TO the ring's two stages (PT_LDS, 64 KiB) plus 2.5 KiB of per-sentence state, so
// one workgroup has a CU's 160 KiB to itself.  (Reusing the ring's stages for the matrix would fit two, at the price
// of a barrier inside the ring's epilogue; the steps below are chains of LDS round trips of two waves either way.)
//
// After the matrix thread i < n owns sentence i.  S is read column-wise, S[j * 128 + i]: the lanes of a wave read
// consecutive words of one row j, which lie in distinct banks.
//
// ORDER OF EVERY FLOAT32 SUM: ascending index j = 0 .. n - 1 in ONE thread's accumulator -- the degree (plain adds),
// the bias mass (plain adds, every thread forms the same sum), a step's sum (fmaf(W_ji, p_j * inv_j, acc)) -- and S_ij
// is the tile body's, a function of the two rows and d alone.  A unit's bits therefore do not depend on the batch, the
// grid or its place in the plane.  The maximum of p is order-free.  lambda and 1 - lambda are float32 and v is
// __fmul_rn(lambda, rel) - __fmul_rn(1 - lambda, red), as mmr.hip forms it.
//
// Selection: one step is a 128-wide arg-max (v descending, index ascending): an xor butterfly inside each of the two
// waves that own sentences, then an exchange of the two results through LDS (one barrier per step, slots alternate
// with the step's parity).  The `red` update reads row `pick` of S.
// No global atomics, no host synchronisation, nothing written but the outputs: the call can be captured into a graph.
#include <limits.h>
#include <math.h>

#include "pair_tile.h"

namespace mmrag_impl {

namespace {

constexpr int SUM_N = MMRAG_MAX_SUMMARY_SENTENCES;
static_assert(SUM_N == PT, "a unit is one tile");

struct SummaryParams {
    const char *rows;
    unsigned rb;                // row pitch in bytes (unit rows and bias rows)
    long long n_rows;
    int nk;                     // K-slabs that hold the d columns
    const int *unit_start, *unit_len, *cost, *budget;
    const char *bias;           // null: no unit has a bias row
    long long n_bias;
    const int *unit_bias;
    float t, alpha, oma;        // oma = 1 - alpha (float32)
    int iters;
    float lam, oml;             // lambda and 1 - lambda (float32)
    int k;
    int *out_pos;
    float *out_val, *out_rel;
    int *out_used;
};

// (v, i) <- the better of (v, i) and (ov, oi): an index of INT_MAX is "nothing"; the greater v, else the lower index
__device__ __forceinline__ void sum_better(float &v, int &i, float ov, int oi) {
    if (oi != INT_MAX && (i == INT_MAX || ov > v || (ov == v && oi < i))) {
        v = ov;
        i = oi;
    }
}

template <int DT>
__global__ __launch_bounds__(256) void summary_select_kernel(const SummaryParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(PT_LDS + SUM_N * SUM_N * 4 + 4 * 1024 <= 160 * 1024, "one workgroup per CU");
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    __shared__ float S[SUM_N * SUM_N];
    __shared__ float sb[SUM_N];          // <x_i, bias row>
    __shared__ float pq[2][SUM_N];       // p_j * inv_j of the step that reads it
    __shared__ float pfin[SUM_N];
    __shared__ int costs[SUM_N];
    __shared__ float ex_v[2][2];
    __shared__ int ex_i[2][2];

    const int u = blockIdx.x, tid = threadIdx.x, k = p.k;
    const float NEG_INF = -__builtin_inff();
    // every thread reads the same table entries: the checks are uniform over the workgroup
    const int start = p.unit_start[u], n = p.unit_len[u];
    const int ub = p.unit_bias != nullptr ? p.unit_bias[u] : -1;
    const bool ok = n >= 1 && n <= SUM_N && start >= 0 && (long long)start + n <= p.n_rows && ub >= -1 &&
                    (long long)ub < p.n_bias;
    if (!ok) {
        for (int t = tid; t < k; t += 256) {
            p.out_pos[(size_t)u * k + t] = -1;
            p.out_val[(size_t)u * k + t] = t == 0 ? __builtin_nanf("") : NEG_INF;
        }
        if (tid == 0) p.out_used[u] = 0;
        return;
    }
    const bool biased = ub >= 0;

    const PairTileCtx c = pair_tile_ctx(tid, p.rb, smem);
    const PairTileSrc unit_src = {p.rows + (size_t)start * p.rb, (unsigned)n * p.rb};
    const PairTileSrc bias_src = {biased ? p.bias + (size_t)ub * p.rb : nullptr, biased ? p.rb : 0u};
    pair_tile_ring<DT>(
        c, smem, p.nk, biased ? 2 : 1,
        [&](int j) { return j == 0 || c.wave < 2 ? unit_src : bias_src; },
        [&](int j, const f32x4_t (&acc)[4][4]) {
            // acc[a][b][r] = <row wm*64 + 16a + 4 g4 + r, B row wn*64 + 16b + c16>
            if (j == 0) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            S[(c.wm * 64 + 16 * a + 4 * c.g4 + r) * SUM_N + c.wn * 64 + 16 * b + c.c16] = acc[a][b][r];
            } else if (c.wn == 0 && c.c16 == 0) {   // B row 0 is the bias row
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sb[c.wm * 64 + 16 * a + 4 * c.g4 + r] = acc[a][0][r];
            }
        });
    const int i = tid;
    const bool mine = i < n;
    if (mine) costs[i] = p.cost[start + i];
    __syncthreads();

    // ---- graph and prior
    float inv = 0.0f, b = 0.0f, pi = 0.0f;
    if (mine) {
        float deg = 0.0f;
        for (int j = 0; j < n; ++j) {
            const float s = S[j * SUM_N + i];
            deg += (j != i && s >= p.t) ? s : 0.0f;
        }
        inv = deg > 0.0f ? 1.0f / deg : 0.0f;
        b = 1.0f / (float)n;
        if (biased) {
            float mass = 0.0f;
            for (int j = 0; j < n; ++j) mass += fmaxf(sb[j], 0.0f);
            if (mass > 0.0f) b = fmaxf(sb[i], 0.0f) / mass;
        }
        pi = b;
        pq[0][i] = pi * inv;
    }
    __syncthreads();

    // ---- centrality: exactly `iters` steps
    const float ab = __fmul_rn(p.alpha, b);
    for (int it = 0; it < p.iters; ++it) {
        if (mine) {
            const float *cur = pq[it & 1];
            float acc = 0.0f;
            for (int j = 0; j < n; ++j) {
                const float s = S[j * SUM_N + i];
                acc = fmaf((j != i && s >= p.t) ? s : 0.0f, cur[j], acc);
            }
            pi = fmaf(p.oma, acc, ab);
            pq[(it + 1) & 1][i] = pi * inv;
        }
        __syncthreads();
    }
    if (mine) pfin[i] = pi;
    __syncthreads();
    float rel = 0.0f;
    if (mine) {
        float top = pfin[0];
        for (int j = 1; j < n; ++j) top = fmaxf(top, pfin[j]);
        rel = pi / top;
        if (p.out_rel != nullptr) p.out_rel[(size_t)start + i] = rel;
    }

    // ---- selection
    int remaining = p.budget[u];
    const int budget = remaining;
    bool is_free = mine;
    float red = 0.0f;
    const int wave = c.wave, lane = c.lane;
    int t = 0;
    for (; t < k; ++t) {
        float v = NEG_INF;
        int arg = INT_MAX;
        if (wave < 2) {
            if (is_free && costs[i] <= remaining) {
                v = __fmul_rn(p.lam, rel) - __fmul_rn(p.oml, red);
                arg = i;
            }
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const float ov = __shfl_xor(v, m);
                const int oa = __shfl_xor(arg, m);
                sum_better(v, arg, ov, oa);
            }
            if (lane == 0) {
                ex_v[t & 1][wave] = v;
                ex_i[t & 1][wave] = arg;
            }
        }
        __syncthreads();
        v = ex_v[t & 1][0];
        arg = ex_i[t & 1][0];
        sum_better(v, arg, ex_v[t & 1][1], ex_i[t & 1][1]);
        if (arg == INT_MAX) break;      // nothing free fits what is left: the same in every thread
        if (tid == 0) {
            p.out_pos[(size_t)u * k + t] = arg;
            p.out_val[(size_t)u * k + t] = v;
        }
        remaining -= costs[arg];
        if (arg == i) is_free = false;
        if (mine) red = fmaxf(red, fmaxf(S[arg * SUM_N + i], 0.0f));
    }
    for (int r = t + tid; r < k; r += 256) {
        p.out_pos[(size_t)u * k + r] = -1;
        p.out_val[(size_t)u * k + r] = NEG_INF;
    }
    if (tid == 0) p.out_used[u] = budget - remaining;
#endif
}

}  // namespace

}  // namespace mmrag_impl

extern "C" {

int mmrag_summary_select(const void *rows, int64_t ld, int dtype, int d, int64_t n_rows, const int32_t *unit_start,
                         const int32_t *unit_len, int n_units, const int32_t *cost, const int32_t *budget,
                         const void *bias_rows, int64_t n_bias, const int32_t *unit_bias, float edge_threshold,
                         float alpha, int iterations, float lambda, int k, int32_t *out_pos, float *out_val,
                         float *out_rel, int32_t *out_used, void *stream) {
    using namespace mmrag_impl;
    MMRAG_CHECK_ARG(rows && unit_start && unit_len && cost && budget && out_pos && out_val && out_used,
                    "summary_select: null pointer");
    if (int st = check_stored_rows("summary_select", "summarised", "summarise", ld, dtype, d)) return st;
    MMRAG_CHECK_ARG(n_rows >= 1 && n_rows < (1LL << 31), "summary_select: n_rows=%lld outside 1..2^31 - 1",
                    (long long)n_rows);
    MMRAG_CHECK_ARG(n_units >= 1 && n_units <= (1 << 24), "summary_select: n_units=%d outside 1..2^24", n_units);
    MMRAG_CHECK_ARG((bias_rows != nullptr) == (unit_bias != nullptr) && (bias_rows != nullptr) == (n_bias > 0) &&
                        n_bias >= 0 && n_bias < (1LL << 31),
                    "summary_select: bias_rows, n_bias and unit_bias go together: all given (1 <= n_bias < 2^31) or "
                    "NULL, 0, NULL (n_bias=%lld)", (long long)n_bias);
    MMRAG_CHECK_ARG(edge_threshold >= 0.0f && edge_threshold < INFINITY,
                    "summary_select: edge_threshold=%g must be finite and >= 0", (double)edge_threshold);
    MMRAG_CHECK_ARG(alpha > 0.0f && alpha <= 1.0f, "summary_select: alpha=%g outside (0, 1]", (double)alpha);
    MMRAG_CHECK_ARG(iterations >= 0 && iterations <= MMRAG_MAX_SUMMARY_ITERATIONS,
                    "summary_select: iterations=%d outside 0..%d", iterations, MMRAG_MAX_SUMMARY_ITERATIONS);
    MMRAG_CHECK_ARG(lambda >= 0.0f && lambda <= 1.0f, "summary_select: lambda=%g outside [0, 1]", (double)lambda);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_SUMMARY_SENTENCES, "summary_select: k=%d outside 1..%d", k,
                    MMRAG_MAX_SUMMARY_SENTENCES);
    MMRAG_CHECK_ARG(((uintptr_t)rows % 16) == 0 && ((uintptr_t)bias_rows % 16) == 0,
                    "summary_select: rows and bias_rows must be 16-byte aligned");
    SummaryParams p;
    p.rows = (const char *)rows;
    p.rb = stored_row_bytes(ld, dtype);
    p.n_rows = n_rows;
    p.nk = stored_k_slabs(d, dtype);
    p.unit_start = unit_start, p.unit_len = unit_len, p.cost = cost, p.budget = budget;
    p.bias = (const char *)bias_rows, p.n_bias = n_bias, p.unit_bias = unit_bias;
    p.t = edge_threshold, p.alpha = alpha, p.oma = 1.0f - alpha;
    p.iters = iterations;
    p.lam = lambda, p.oml = 1.0f - lambda;
    p.k = k;
    p.out_pos = out_pos, p.out_val = out_val, p.out_rel = out_rel, p.out_used = out_used;
    mmrag::with_elem_type(dtype, [&](auto tag) {
        hipLaunchKernelGGL(summary_select_kernel<decltype(tag)::value>, dim3((unsigned)n_units), dim3(256), 0,
                           (hipStream_t)stream, p);
    });
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // extern "C"
