// Fusion of the ranked lists of several query variants on gfx950: the device half of VectorIndex.fused_search
// (the definition is in include/mmrag.h at mmrag_fuse_select).
//
// One workgroup per group (one question), one launch, no workspace, no atomics on global memory, no host
// synchronisation: the call can be captured into a graph.  A group's nl <= 16 lists of C <= 256 entries are at most
// 4096 entries; everything between the first read and the last write is in LDS.
//
//   1. Load.  All threads read the group's entries: rows, scores (kept in LDS at their (list, position)), the weights,
//      and each list's end (its first row < 0: one LDS integer atomicMin per such entry).  Entries past a list's end,
//      and the slots up to the next power of two, become sentinels that sort last.
//   2. Sort by (row, list, position): a bitonic network in LDS over (int64 row, 16-bit list << 8 | position).  The keys
//      of valid entries are distinct, so the result is one fixed permutation: a row's entries are adjacent, in ascending
//      list order -- the order the definition adds them in -- and a list's repeats of a row follow its first occurrence.
//   3. Reduce.  The lane at the first entry of a run owns the row: it walks the run (at most 16 counted entries) and
//      computes fused, best, best_list and count in registers, in the definition's order of operations.
//   4. Sort by (fused desc, best desc, row asc): a second bitonic network over (float, float, 16-bit position of the
//      run in the row-sorted order << 4 | best_list), payload (entry of the row's first occurrence << 4 | count - 1).
//      The position stands for the row: it ascends with it, so no 64-bit row is moved again, and the first sort's row
//      array is dead by now -- the second sort's arrays take its place in LDS (48 KiB over the first sort's 56 KiB).
//   5. Output.  Slot j < n takes entry j of the sorted order; its row is read back from the input through the payload.
//
// The network, not the thread count, fixes the permutation: the block is sized by the host from L and C only (half the
// largest padded group, 64..1024 threads) and the bits do not depend on it.  Stages whose pair distance is below 64 touch
// only the 128 elements one wave also wrote in the stage before, so they are separated by a wave-level fence; only the
// stages of distance >= 64 take a workgroup barrier (21 of the 78 stages of a 4096-entry sort).
#include "mmrag_internal.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int FUSE_MAX_LISTS = MMRAG_MAX_FUSE_LISTS;
constexpr int FUSE_MAX_C = MMRAG_MAX_FUSE_CANDIDATES;
constexpr int FUSE_MAX_E = FUSE_MAX_LISTS * FUSE_MAX_C;   // 4096 entries per group
constexpr int FUSE_MAX_THREADS = 1024;
constexpr int FUSE_PER = 4;                               // entries a thread owns in steps 3 and 4: E_pad <= 4 x threads
constexpr long long FUSE_ROW_SENTINEL = 0x7fffffffffffffffLL;
constexpr unsigned FUSE_NEG_INF_BITS = 0xff800000u;

static_assert(FUSE_MAX_C == 256 && FUSE_MAX_LISTS == 16, "an entry is packed as list << 8 | position in 12 bits");
static_assert(FUSE_MAX_E <= FUSE_PER * FUSE_MAX_THREADS, "every entry needs an owner lane");

struct FuseParams {
    const float *scores;         // [L, C]
    const long long *rows;       // [L, C]
    const int *list_off;         // [G + 1]
    const float *weights;        // [L] or null
    int L, C, method, rrf_k, n;
    float *out_f;                // [G, n]
    long long *out_r;
    float *out_b;
    int *out_bl, *out_cnt;
    int *out_info;               // [G, 2]
};

// ascending sort of N (a power of two) elements by `before`: thread t takes the pairs t, t + T, ... of every stage.  A
// wave's 64 pairs of a stage with distance j <= 64 lie in one aligned block of 128 elements, the same block in every
// such stage, so a stage with j < 64 reads only what its own wave wrote since the last barrier
template <typename Before, typename Swap>
__device__ __forceinline__ void bitonic_sort(int N, int tid, int T, Before before, Swap swap) {
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= 64)
                __syncthreads();
            else
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int t = tid; t < (N >> 1); t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i + j;
                const bool ascending = (i & k) == 0;
                if (ascending ? before(p, i) : before(i, p)) swap(i, p);
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(FUSE_MAX_THREADS) void fuse_select_kernel(const FuseParams p) {
    // steps 1-3: rows [4096] int64 | lp [4096] u16 | sc [4096] float      (56 KiB)
    // steps 4-5: fused [4096] float | best [4096] float | ib [4096] u16 | ec [4096] u16 over the same bytes (48 KiB)
    __shared__ __align__(16) unsigned char smem[FUSE_MAX_E * 14];
    __shared__ int len[FUSE_MAX_LISTS];
    __shared__ float wts[FUSE_MAX_LISTS];
    __shared__ int n_distinct;

    long long *rows = (long long *)smem;
    unsigned short *lp = (unsigned short *)(smem + FUSE_MAX_E * 8);
    float *sc = (float *)(smem + FUSE_MAX_E * 10);
    float *fus = (float *)smem;
    float *bst = (float *)(smem + FUSE_MAX_E * 4);
    unsigned short *ib = (unsigned short *)(smem + FUSE_MAX_E * 8);
    unsigned short *ec = (unsigned short *)(smem + FUSE_MAX_E * 10);

    const int tid = threadIdx.x, T = blockDim.x;
    const size_t g = blockIdx.x;
    const int C = p.C, n = p.n;

    // a group's lists; offsets that do not describe lists of this call are an empty group, lists past the 16th are not
    // read (the caller checks both: the offsets live on the device)
    int l0 = p.list_off[g], nl = p.list_off[g + 1] - l0;
    if (l0 < 0 || nl < 0 || (long long)l0 + nl > p.L) nl = 0;
    if (nl > FUSE_MAX_LISTS) nl = FUSE_MAX_LISTS;
    const int E = nl * C;
    int N = 1;
    while (N < E) N <<= 1;
    const long long *grows = p.rows + (size_t)l0 * C;
    const float *gscores = p.scores + (size_t)l0 * C;

    if (tid < FUSE_MAX_LISTS) {
        len[tid] = C;
        wts[tid] = (p.weights && tid < nl) ? p.weights[l0 + tid] : 1.0f;
    }
    if (tid == 0) n_distinct = 0;
    __syncthreads();

    // 1. load
    for (int e = tid; e < E; e += T) {
        const int l = e / C, pos = e - l * C;
        const long long r = grows[e];
        rows[e] = r;
        sc[(l << 8) | pos] = gscores[e];
        if (r < 0) atomicMin(&len[l], pos);   // LDS: the list ends at its first row < 0
    }
    __syncthreads();
    int V = 0;
    for (int l = 0; l < nl; ++l) V += len[l];
    for (int e = tid; e < N; e += T) {
        const int l = e < E ? e / C : 0, pos = e - l * C;
        const bool valid = e < E && pos < len[l];
        if (!valid) rows[e] = FUSE_ROW_SENTINEL;
        lp[e] = valid ? (unsigned short)((l << 8) | pos) : (unsigned short)0xffff;
    }

    // 2. by (row, list, position)
    bitonic_sort(
        N, tid, T,
        [&](int a, int b) {
            const long long ra = rows[a], rb = rows[b];
            return ra < rb || (ra == rb && lp[a] < lp[b]);
        },
        [&](int a, int b) {
            const long long r = rows[a];
            rows[a] = rows[b];
            rows[b] = r;
            const unsigned short q = lp[a];
            lp[a] = lp[b];
            lp[b] = q;
        });

    // 3. one owner lane per run of equal rows
    float o_f[FUSE_PER], o_b[FUSE_PER];
    unsigned short o_ib[FUSE_PER], o_ec[FUSE_PER];
    int owners = 0;
#pragma unroll
    for (int m = 0; m < FUSE_PER; ++m) {
        const int i = tid + m * T;
        o_f[m] = o_b[m] = __uint_as_float(FUSE_NEG_INF_BITS);
        o_ib[m] = o_ec[m] = 0xffff;
        if (i < V && (i == 0 || rows[i - 1] != rows[i])) {
            const long long row = rows[i];
            float fused = 0.0f, best = 0.0f;
            int bl = 0, cnt = 0, prev_l = -1;
            for (int j = i; j < V && rows[j] == row; ++j) {
                const int e = lp[j], l = e >> 8, pos = e & 255;
                if (l == prev_l) continue;   // the row again in one list: only its first occurrence counts
                prev_l = l;
                const float s = sc[e], w = wts[l];
                const float c = p.method == MMRAG_FUSE_RRF ? __fdiv_rn(w, (float)((long long)p.rrf_k + pos + 1))
                                                           : __fmul_rn(w, s);
                if (cnt == 0) {
                    fused = c;
                    best = s;
                    bl = l;
                } else {
                    if (p.method == MMRAG_FUSE_RRF)
                        fused = __fadd_rn(fused, c);
                    else if (c > fused)
                        fused = c;
                    if (s > best) {
                        best = s;
                        bl = l;
                    }
                }
                ++cnt;
            }
            o_f[m] = fused;
            o_b[m] = best;
            o_ib[m] = (unsigned short)((i << 4) | bl);
            o_ec[m] = (unsigned short)((lp[i] << 4) | (cnt - 1));
            ++owners;
        }
    }
    // the number of distinct rows: one LDS integer add per wave
    for (int off = 32; off > 0; off >>= 1) owners += __shfl_xor(owners, off);
    if ((tid & 63) == 0 && owners) atomicAdd(&n_distinct, owners);
    __syncthreads();   // every read of rows / lp / sc is done: their bytes become the second sort's arrays
#pragma unroll
    for (int m = 0; m < FUSE_PER; ++m) {
        const int i = tid + m * T;
        if (i < N) {
            fus[i] = o_f[m];
            bst[i] = o_b[m];
            ib[i] = o_ib[m];
            ec[i] = o_ec[m];
        }
    }

    // 4. by (fused desc, best desc, row asc); -0.0 == 0.0 falls through to the next key as the float compare has it
    bitonic_sort(
        N, tid, T,
        [&](int a, int b) {
            const float fa = fus[a], fb = fus[b];
            if (fa > fb) return true;
            if (!(fa == fb)) return false;
            const float ba = bst[a], bb = bst[b];
            return ba > bb || (ba == bb && ib[a] < ib[b]);
        },
        [&](int a, int b) {
            const float f = fus[a];
            fus[a] = fus[b];
            fus[b] = f;
            const float s = bst[a];
            bst[a] = bst[b];
            bst[b] = s;
            unsigned short q = ib[a];
            ib[a] = ib[b];
            ib[b] = q;
            q = ec[a];
            ec[a] = ec[b];
            ec[b] = q;
        });

    // 5. output
    const int D = n_distinct;
    for (int j = tid; j < n; j += T) {
        const size_t o = g * n + j;
        if (j < D) {
            const int e = ec[j] >> 4;
            p.out_f[o] = fus[j];
            p.out_r[o] = grows[(size_t)(e >> 8) * C + (e & 255)];
            p.out_b[o] = bst[j];
            p.out_bl[o] = ib[j] & 15;
            p.out_cnt[o] = (ec[j] & 15) + 1;
        } else {
            p.out_f[o] = __uint_as_float(FUSE_NEG_INF_BITS);
            p.out_r[o] = -1;
            p.out_b[o] = __uint_as_float(FUSE_NEG_INF_BITS);
            p.out_bl[o] = -1;
            p.out_cnt[o] = 0;
        }
    }
    if (tid == 0) {
        p.out_info[g * 2] = D;
        p.out_info[g * 2 + 1] = V;
    }
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

int mmrag_fuse_select(const float *scores, const int64_t *rows, int L, int C, const int32_t *list_off, int G,
                      const float *weights, int method, int rrf_k, int n, float *out_fused, int64_t *out_rows,
                      float *out_best, int32_t *out_best_list, int32_t *out_count, int32_t *out_info, void *stream) {
    MMRAG_CHECK_ARG(G >= 1, "fuse_select: G must be positive (got %d)", G);
    MMRAG_CHECK_ARG(L >= 0, "fuse_select: L must not be negative (got %d)", L);
    MMRAG_CHECK_ARG(C >= 1 && C <= MMRAG_MAX_FUSE_CANDIDATES, "fuse_select: need 1 <= C <= %d (got C=%d)",
                    MMRAG_MAX_FUSE_CANDIDATES, C);
    MMRAG_CHECK_ARG(n >= 1 && n <= MMRAG_MAX_FUSE_RESULTS, "fuse_select: need 1 <= n <= %d (got %d)",
                    MMRAG_MAX_FUSE_RESULTS, n);
    MMRAG_CHECK_ARG(rrf_k >= 0, "fuse_select: rrf_k must not be negative (got %d)", rrf_k);
    MMRAG_CHECK_ARG(method == MMRAG_FUSE_RRF || method == MMRAG_FUSE_MAX, "fuse_select: unknown method %d", method);
    MMRAG_CHECK_ARG(list_off && out_fused && out_rows && out_best && out_best_list && out_count && out_info,
                    "fuse_select: null pointer");
    MMRAG_CHECK_ARG((scores && rows) || L == 0, "fuse_select: scores / rows are null with L=%d", L);
    FuseParams p;
    p.scores = scores;
    p.rows = (const long long *)rows;
    p.list_off = list_off;
    p.weights = weights;
    p.L = L;
    p.C = C;
    p.method = method;
    p.rrf_k = rrf_k;
    p.n = n;
    p.out_f = out_fused;
    p.out_r = (long long *)out_rows;
    p.out_b = out_best;
    p.out_bl = out_best_list;
    p.out_cnt = out_count;
    p.out_info = out_info;
    // half the largest padded group this call can hold: one pair per thread and stage where that fits
    int most = (L < MMRAG_MAX_FUSE_LISTS ? L : MMRAG_MAX_FUSE_LISTS) * C, padded = 1;
    while (padded < most) padded <<= 1;
    // bitonic_sort's barrier-free stages need whole 64-lane waves that own aligned 128-element blocks: the block size
    // must be a power of two >= 64 (`padded` is a power of two, and so are both clamps)
    static_assert(FUSE_MAX_THREADS >= 64 && (FUSE_MAX_THREADS & (FUSE_MAX_THREADS - 1)) == 0,
                  "the block size must be a power of two >= 64");
    int threads = padded / 2;
    threads = threads < 64 ? 64 : (threads > FUSE_MAX_THREADS ? FUSE_MAX_THREADS : threads);
    if (threads < 64 || (threads & (threads - 1)) != 0 || threads * FUSE_PER < padded) {
        mmrag::set_error("fuse_select: internal error: block size %d for %d padded entries", threads, padded);
        return MMRAG_EINVAL;
    }
    fuse_select_kernel<<<G, threads, 0, (hipStream_t)stream>>>(p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // extern "C"
