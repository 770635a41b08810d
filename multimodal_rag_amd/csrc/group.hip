// Grouping of search hits by a per-row key on gfx950: the device half of VectorIndex.grouped_search (DESIGN.md section
// 3.1h; the definition is in include/mmrag.h at mmrag_group_select).
//
// One workgroup of 256 threads per query, one launch, no workspace, no atomics on global memory, no floating-point
// operation at all (scores are moved as bits), no host synchronisation: the call can be captured into a graph.
//
//   1. All four waves read the query's C rows, gather each row's group ordinal into LDS (`keys`; -1 = the row has no
//      key, a row outside [0, n_rows) is never used as an index) and find the end of the list (its first row < 0) with
//      one LDS integer atomicMin.
//   2. Wave 0 walks the list in chunks of 64 candidates, in order, one candidate per lane.  An LDS open-addressing table
//      maps ordinal -> group index for the groups that made the output, so it never holds more than G <= 256 entries in
//      its 1024 slots; gcount[group index] is the number of members written so far.
//        a. every keyed lane looks its ordinal up (read only: the table does not change during this step);
//        b. while fewer than G groups exist, the lanes that found nothing are taken in lane order: the lowest one opens
//           the next group index for itself and for every lane of the chunk with the same ordinal (one ballot), a row
//           without a key opens one for itself alone.  The lowest lane of each new ordinal is its ONE writer: it claims
//           a slot (integer compare-and-swap on the slot's key; which slot it gets decides nothing, the value stored
//           was fixed by the lane order) and writes the group's ordinal to out_group.  Once G groups exist, ordinals
//           that are not in the table belong to groups ranked G or worse and are skipped for good;
//        c. lanes whose group still has room rank themselves among the chunk's lanes of the same group (one ballot
//           per such group in the chunk), write their slot base + rank if it is < S, and the group's lowest lane
//           stores the new count.
//      The walk stops at the end of the list or as soon as G groups hold S members each.
//   3. All four waves pad what was not written with (-inf, -1, -1) and out_group with -2.
// Steps b and c are loops over DISTINCT ordinals of one chunk, not over pairs: b runs at most G + 63 times per query,
// c at most min(C, G * S) times, and a chunk whose lanes all belong to full or unlisted groups costs the look-up only.
//
// The slot of ordinal g is g mod 1024, linear probing.  The index layer numbers a collection's documents 0, 1, 2, ... by
// first appearance, so the low bits spread them as well as any mixing would; ordinals that agree in their low ten bits
// only lengthen the probe chains (at most G - 1 steps), never change the answer.
#include "mmrag_internal.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int GRP_THREADS = 256;
constexpr int GRP_MAX_C = MMRAG_MAX_GROUP_CANDIDATES;
constexpr int GRP_MAX_G = MMRAG_MAX_GROUPS;
constexpr int GRP_SLOTS = 1024;            // 4 x the most groups a query lists: probe chains stay short
constexpr int GRP_EMPTY = -1;              // table key of a free slot (ordinals in the table are >= 0)
constexpr int GRP_NO_KEY = -1, GRP_PAST_END = -2;   // keys[]: a row without a key, a position past the list's end
constexpr unsigned GRP_NEG_INF_BITS = 0xff800000u;

struct GroupParams {
    const unsigned *scores;      // [B, C] float32, moved as bits
    const long long *rows;       // [B, C]
    const int *group_of_row;     // [n_rows]
    long long n_rows;
    int C, G, S;
    unsigned *out_s;             // [B, G, S]
    long long *out_r;
    int *out_p;
    int *out_g;                  // [B, G]
    int *out_info;               // [B, 2]
};

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

__global__ __launch_bounds__(GRP_THREADS) void group_select_kernel(const GroupParams p) {
    __shared__ int keys[GRP_MAX_C];
    __shared__ int tkey[GRP_SLOTS], tval[GRP_SLOTS];
    __shared__ int gcount[GRP_MAX_G];
    __shared__ int n_valid, n_groups;

    const int tid = threadIdx.x, lane = tid & 63;
    const size_t q = blockIdx.x;
    const int C = p.C, G = p.G, S = p.S;
    const unsigned *sc = p.scores + q * C;
    const long long *rw = p.rows + q * C;

    if (tid == 0) {
        n_valid = C;
        n_groups = 0;
    }
    for (int i = tid; i < GRP_SLOTS; i += GRP_THREADS) tkey[i] = GRP_EMPTY;
    for (int i = tid; i < GRP_MAX_G; i += GRP_THREADS) gcount[i] = 0;
    __syncthreads();
    for (int i = tid; i < C; i += GRP_THREADS) {
        const long long r = rw[i];
        int g = GRP_NO_KEY;
        if (r < 0)
            atomicMin(&n_valid, i);   // LDS: the list ends at its first row < 0
        else if (r < p.n_rows)
            g = p.group_of_row[r];
        keys[i] = g < 0 ? GRP_NO_KEY : g;
    }
    __syncthreads();
    const int cnt = n_valid;

    if (tid < 64) {
        int ng = 0, filled = 0;   // wave-uniform: groups opened, groups holding S members
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const int i = c0 + lane;
            const bool valid = i < cnt;
            const int key = valid ? keys[i] : GRP_PAST_END;
            // a. look the ordinal up
            int gi = -1;
            {
                bool pend = key >= 0;
                unsigned h = (unsigned)key & (GRP_SLOTS - 1);
                while (pend) {
                    const int k = tkey[h];
                    if (k == key) {
                        gi = tval[h];
                        pend = false;
                    } else if (k == GRP_EMPTY) {
                        pend = false;
                    } else {
                        h = (h + 1) & (GRP_SLOTS - 1);
                    }
                }
            }
            // b. open groups for what is new, in lane order
            if (ng < G) {
                unsigned long long rem = __ballot(valid && gi < 0);
                bool lead = false;
                while (rem && ng < G) {
                    const int src = __ffsll((long long)rem) - 1;
                    const int k = __shfl(key, src);
                    const unsigned long long m = k >= 0 ? __ballot(key == k) : (1ull << src);
                    if ((m >> lane) & 1ull) gi = ng;
                    lead = lead || lane == src;
                    ++ng;
                    rem &= ~m;
                }
                if (lead) {
                    p.out_g[q * G + gi] = key;   // GRP_NO_KEY is the -1 the caller sees
                    if (key >= 0) {
                        unsigned h = (unsigned)key & (GRP_SLOTS - 1);
                        while (atomicCAS(&tkey[h], GRP_EMPTY, key) != GRP_EMPTY) h = (h + 1) & (GRP_SLOTS - 1);
                        tval[h] = gi;
                    }
                }
            }
            // c. members of groups with room: slot = members so far + rank among the chunk's lanes of the group
            const int base = gi >= 0 ? gcount[gi] : 0;
            const bool active = gi >= 0 && base < S;
            unsigned long long rem = __ballot(active);
            int rank = 0, tot = 0;
            while (rem) {
                const int src = __ffsll((long long)rem) - 1;
                const int g0 = __shfl(gi, src);
                const unsigned long long m = __ballot(active && gi == g0);
                if ((m >> lane) & 1ull) {
                    rank = __popcll(m & lanes_below(lane));
                    tot = __popcll(m);
                }
                rem &= ~m;
            }
            const int slot = base + rank;
            if (active && slot < S) {
                const size_t o = (q * G + gi) * S + slot;
                p.out_s[o] = sc[i];
                p.out_r[o] = rw[i];
                p.out_p[o] = i;
            }
            const bool closes = active && rank == 0 && base + tot >= S;
            if (active && rank == 0) gcount[gi] = base + tot < S ? base + tot : S;
            filled += __popcll(__ballot(closes));
            // the table and the counts written above are read by other lanes of this wave in the next chunk: the LDS
            // serves one wave's operations in order, the fence keeps the compiler from moving them
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (ng == G && filled == G) break;
        }
        if (lane == 0) {
            n_groups = ng;
            p.out_info[q * 2] = ng;
            p.out_info[q * 2 + 1] = cnt;
        }
    }
    __syncthreads();
    const int ng = n_groups;
    for (int t = tid; t < G * S; t += GRP_THREADS) {
        const int gi = t / S, slot = t - gi * S;
        if (gi >= ng || slot >= gcount[gi]) {
            const size_t o = q * G * S + t;
            p.out_s[o] = GRP_NEG_INF_BITS;
            p.out_r[o] = -1;
            p.out_p[o] = -1;
        }
    }
    for (int gi = ng + tid; gi < G; gi += GRP_THREADS) p.out_g[q * G + gi] = -2;
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

int mmrag_group_select(const float *scores, const int64_t *rows, int B, int C, const int32_t *group_of_row,
                       int64_t n_rows, int n_groups, int group_size, float *out_scores, int64_t *out_rows,
                       int32_t *out_pos, int32_t *out_group, int32_t *out_info, void *stream) {
    MMRAG_CHECK_ARG(B > 0, "group_select: B must be positive (got %d)", B);
    MMRAG_CHECK_ARG(C >= 1 && C <= MMRAG_MAX_GROUP_CANDIDATES, "group_select: need 1 <= C <= %d (got C=%d)",
                    MMRAG_MAX_GROUP_CANDIDATES, C);
    MMRAG_CHECK_ARG(n_groups >= 1 && n_groups <= MMRAG_MAX_GROUPS, "group_select: need 1 <= n_groups <= %d (got %d)",
                    MMRAG_MAX_GROUPS, n_groups);
    MMRAG_CHECK_ARG(group_size >= 1 && group_size <= MMRAG_MAX_GROUP_SIZE,
                    "group_select: need 1 <= group_size <= %d (got %d)", MMRAG_MAX_GROUP_SIZE, group_size);
    MMRAG_CHECK_ARG(n_rows >= 0, "group_select: n_rows must not be negative (got %lld)", (long long)n_rows);
    MMRAG_CHECK_ARG(scores && rows && out_scores && out_rows && out_pos && out_group && out_info,
                    "group_select: null pointer");
    MMRAG_CHECK_ARG(group_of_row || n_rows == 0, "group_select: group_of_row is null with n_rows=%lld",
                    (long long)n_rows);
    GroupParams p;
    p.scores = (const unsigned *)scores;
    p.rows = (const long long *)rows;
    p.group_of_row = group_of_row;
    p.n_rows = n_rows;
    p.C = C;
    p.G = n_groups;
    p.S = group_size;
    p.out_s = (unsigned *)out_scores;
    p.out_r = (long long *)out_rows;
    p.out_p = out_pos;
    p.out_g = out_group;
    p.out_info = out_info;
    group_select_kernel<<<B, GRP_THREADS, 0, (hipStream_t)stream>>>(p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // extern "C"
