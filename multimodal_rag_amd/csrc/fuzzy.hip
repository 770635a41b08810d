// Typo-tolerant term matching for the lexical leg: for every query term that BM25 would drop,
// the lexicon terms within its edit budget, best first.  gfx950 only.
//
//   fuzzy_match_kernel   grid (term tiles, pattern-tile lanes).  A workgroup stages FZ_TERMS consecutive terms' code
//                        points (one contiguous slice of the pool) into LDS; thread i owns term tile * FZ_TERMS + i.
//                        Patterns come FZ_PATTERNS at a time through LDS; the pattern index is the same in every lane,
//                        so its code points and budget are broadcast reads.  Per pair: the length filter
//                        |len_t - len_p| <= e, then the banded optimal-string-alignment recurrence, one row per
//                        pattern code point, the band's five cells of the last two rows in registers and a six code
//                        point window of the term that slides by one LDS read per row.  A wave leaves a pattern when
//                        no lane can still come in under its budget.
//   selection            a match is the 64-bit key (2 - dist) << 62 | df << 31 | (2^31 - 1 - id).  Keys go into a
//                        list of E slots by a cascade of integer maxima: slot s keeps the largest key it has ever been
//                        shown and passes the smaller one on, so whatever the order of arrival slot s ends up with the
//                        (s + 1)-th largest key.  Once per (workgroup, pattern) list in LDS, then the survivors into
//                        the [P, E] list in the workspace the same way: bounded memory, nothing to overflow, no [P, V]
//                        matrix, and a result that does not depend on scheduling.
//   fuzzy_unpack_kernel  keys -> (term id, edits), -1 padded.
#include "mmrag_internal.h"

#include <limits.h>

namespace {

constexpr int FZ_TERMS = 256;                        // terms per workgroup = threads per workgroup
constexpr int FZ_PATTERNS = 32;                      // patterns per LDS tile
constexpr int FZ_MAX_LEN = MMRAG_FUZZY_MAX_LEN;      // longest term / pattern that is matched
constexpr int FZ_MAX_E = MMRAG_FUZZY_MAX_EXPANSIONS;
constexpr int FZ_STAGE = 8192;                       // code points of a term tile held in LDS (32 per term: the rest of
                                                     // an unusually long slice is read from global memory)
constexpr int FZ_MAX_EDITS = 2;
constexpr int FZ_BAND = 2 * FZ_MAX_EDITS + 1;
constexpr int FZ_INF = 1 << 16;
constexpr int FZ_GRID_TARGET = 2048;                 // workgroups worth launching when the lexicon alone gives fewer

typedef unsigned long long u64;

// Put `key` into the descending list of E slots.  Each slot is only ever raised, and each step hands on exactly the
// smaller of (slot, key), so the final list is the E largest keys shown to slot 0 in order, whatever the interleaving.
__device__ inline void cascade_insert(u64 *list, int E, u64 key) {
    for (int s = 0; s < E && key; ++s) {
        const u64 old = atomicMax(&list[s], key);
        key = old < key ? old : key;
    }
}

__global__ __launch_bounds__(FZ_TERMS) void fuzzy_match_kernel(const int32_t *__restrict__ term_off,
                                                               const uint32_t *__restrict__ term_cps,
                                                               const int32_t *__restrict__ df, int n_terms,
                                                               const int32_t *__restrict__ pat_off,
                                                               const uint32_t *__restrict__ pat_cps,
                                                               const int32_t *__restrict__ pat_edits, int n_patterns,
                                                               int E, u64 *__restrict__ lists) {
    __shared__ uint32_t s_terms[FZ_STAGE];
    __shared__ uint32_t s_pat[FZ_PATTERNS * FZ_MAX_LEN];
    __shared__ int s_plen[FZ_PATTERNS], s_pedits[FZ_PATTERNS];
    __shared__ u64 s_list[FZ_PATTERNS * FZ_MAX_E];

    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * FZ_TERMS;
    const int nt = min(FZ_TERMS, n_terms - t0);
    const int base = term_off[t0];
    const int staged = min(term_off[t0 + nt] - base, FZ_STAGE);
    for (int i = tid; i < staged; i += FZ_TERMS) s_terms[i] = term_cps[(size_t)base + i];

    int lt = 0, lo = 0;
    bool cand = false, in_lds = false;
    u64 key_low = 0;
    if (tid < nt) {
        const int a = term_off[t0 + tid], b = term_off[t0 + tid + 1];
        const int d = df[t0 + tid];
        lt = b - a;
        lo = a - base;
        in_lds = b - base <= staged;
        cand = lt >= 1 && lt <= FZ_MAX_LEN && d >= 1;
        key_low = ((u64)(uint32_t)d << 31) | (u64)(0x7fffffff - (t0 + tid));
    }
    const uint32_t *g_term = term_cps + (size_t)base + lo;
    // code point idx of this thread's term (clamped into the term, so every read is of the term's own code points)
    auto term_cp = [&](int idx) -> uint32_t {
        idx = min(idx, lt - 1);
        return in_lds ? s_terms[lo + idx] : g_term[idx];
    };

    for (int pt = blockIdx.y; pt * FZ_PATTERNS < n_patterns; pt += gridDim.y) {
        const int p0 = pt * FZ_PATTERNS;
        const int np = min(FZ_PATTERNS, n_patterns - p0);
        __syncthreads();   // the previous tile's lists and patterns are done with (and s_terms is written)
        for (int i = tid; i < FZ_PATTERNS * FZ_MAX_E; i += FZ_TERMS) s_list[i] = 0;
        if (tid < np) {
            const int len = pat_off[p0 + tid + 1] - pat_off[p0 + tid];
            const int e = pat_edits[p0 + tid];
            s_plen[tid] = len;
            s_pedits[tid] = (len >= 0 && len <= FZ_MAX_LEN && e >= 0 && e <= FZ_MAX_EDITS) ? e : -1;
        }
        for (int i = tid; i < np * FZ_MAX_LEN; i += FZ_TERMS) {
            const int p = i / FZ_MAX_LEN, c = i % FZ_MAX_LEN;
            const int a = pat_off[p0 + p], len = pat_off[p0 + p + 1] - a;
            if (len <= FZ_MAX_LEN && c < len) s_pat[i] = pat_cps[(size_t)a + c];
        }
        __syncthreads();

        for (int p = 0; p < np; ++p) {
            const int e = s_pedits[p], lp = s_plen[p];
            if (e < 0) continue;
            const int dl = lt - lp;
            bool alive = cand && dl >= -e && dl <= e;
            if (!__ballot(alive)) continue;   // no lane of this wave passes the length filter
            const bool mine = alive;          // this lane's term may be read

            // Row i of the recurrence holds d[i][j] for j = i - 2 + k, k = 0..4.  w[m] is term code point i - 4 + m
            // (0-based), so cell k compares pattern[i-1] with w[k+1] = term[j-1] and, for a transposition,
            // pattern[i-2] with it and pattern[i-1] with w[k] = term[j-2].
            int prev[FZ_BAND], prev2[FZ_BAND], cur[FZ_BAND];
            uint32_t w[FZ_BAND + 1];
#pragma unroll
            for (int k = 0; k < FZ_BAND; ++k) {
                const int j = k - FZ_MAX_EDITS;
                prev[k] = (j >= 0 && j <= lt) ? j : FZ_INF;
                prev2[k] = FZ_INF;
            }
            w[0] = w[1] = w[2] = 0;
            w[3] = mine ? term_cp(0) : 0;
            w[4] = mine ? term_cp(1) : 0;
            w[5] = mine ? term_cp(2) : 0;
            uint32_t ppc = 0;
            for (int i = 1; i <= lp; ++i) {
                const uint32_t pc = s_pat[p * FZ_MAX_LEN + i - 1];
                if (i > 1) {
#pragma unroll
                    for (int m = 0; m < FZ_BAND; ++m) w[m] = w[m + 1];
                    w[FZ_BAND] = mine ? term_cp(i + 1) : 0;
                }
                int rowmin = FZ_INF;
#pragma unroll
                for (int k = 0; k < FZ_BAND; ++k) {
                    const int j = i - FZ_MAX_EDITS + k;
                    const uint32_t tc = w[k + 1], tpc = w[k];
                    int v = prev[k] + (tc != pc ? 1 : 0);                       // substitute / match: d[i-1][j-1]
                    if (k + 1 < FZ_BAND) v = min(v, prev[k + 1] + 1);           // d[i-1][j] + 1
                    if (k > 0) v = min(v, cur[k - 1] + 1);                      // d[i][j-1] + 1
                    if (i >= 2 && j >= 2 && pc == tpc && ppc == tc) v = min(v, prev2[k] + 1);   // d[i-2][j-2] + 1
                    if (j == 0) v = i;
                    if (j < 0 || j > lt) v = FZ_INF;
                    cur[k] = v;
                    rowmin = min(rowmin, v);
                }
                alive = alive && rowmin <= e;
                if (!__ballot(alive)) break;   // the whole band of every lane is over budget
#pragma unroll
                for (int k = 0; k < FZ_BAND; ++k) {
                    prev2[k] = prev[k];
                    prev[k] = cur[k];
                }
                ppc = pc;
            }
            if (alive) {
                // d[lp][lt] sits at k = lt - lp + 2 of the last row (in 0..4 by the length filter)
                int dist = prev[0];
#pragma unroll
                for (int k = 1; k < FZ_BAND; ++k) dist = (dl + FZ_MAX_EDITS == k) ? prev[k] : dist;
                if (dist <= e) cascade_insert(&s_list[p * FZ_MAX_E], E, ((u64)(FZ_MAX_EDITS - dist) << 62) | key_low);
            }
        }
        __syncthreads();
        // this workgroup's survivors into the global lists; a key below the list's last slot can never enter it
        for (int i = tid; i < np * E; i += FZ_TERMS) {
            const int p = i / E, s = i % E;
            const u64 key = s_list[p * FZ_MAX_E + s];
            if (!key) continue;
            u64 *g = lists + (size_t)(p0 + p) * E;
            if (key < __hip_atomic_load(&g[E - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) continue;
            cascade_insert(g, E, key);
        }
    }
}

__global__ void fuzzy_unpack_kernel(const u64 *__restrict__ lists, int n, int32_t *__restrict__ out_terms,
                                    int32_t *__restrict__ out_edits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 key = lists[i];
    out_terms[i] = key ? (int32_t)(0x7fffffff - (uint32_t)(key & 0x7fffffffu)) : -1;
    out_edits[i] = key ? FZ_MAX_EDITS - (int32_t)(key >> 62) : -1;
}

}  // namespace

extern "C" {

size_t mmrag_fuzzy_terms_workspace_bytes(int n_terms, int n_patterns, int max_expansions) {
    if (n_terms < 0 || n_patterns < 0 || max_expansions < 1 || max_expansions > FZ_MAX_E) return 0;
    return mmrag::align_up((size_t)(n_patterns > 0 ? n_patterns : 1) * max_expansions * sizeof(u64), 16);
}

int mmrag_fuzzy_terms(const int32_t *term_off, const uint32_t *term_cps, const int32_t *df, int n_terms,
                      const int32_t *pat_off, const uint32_t *pat_cps, const int32_t *pat_edits, int n_patterns,
                      int max_expansions, int32_t *out_terms, int32_t *out_edits, void *workspace,
                      size_t workspace_bytes, void *stream) {
    MMRAG_CHECK_ARG(n_terms >= 0 && n_patterns >= 0, "fuzzy_terms: bad shape n_terms=%d n_patterns=%d", n_terms,
                    n_patterns);
    MMRAG_CHECK_ARG(max_expansions >= 1 && max_expansions <= FZ_MAX_E, "fuzzy_terms: max_expansions=%d outside 1..%d",
                    max_expansions, FZ_MAX_E);
    if (n_patterns == 0) return MMRAG_OK;
    MMRAG_CHECK_ARG(pat_off && pat_cps && pat_edits && out_terms && out_edits, "fuzzy_terms: null pointer");
    MMRAG_CHECK_ARG(n_terms == 0 || (term_off && term_cps && df), "fuzzy_terms: null term plane");
    MMRAG_CHECK_ARG((int64_t)n_patterns * max_expansions < INT_MAX, "fuzzy_terms: n_patterns=%d too large", n_patterns);
    const size_t need = mmrag_fuzzy_terms_workspace_bytes(n_terms, n_patterns, max_expansions);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace % 16) != 0) {
        mmrag::set_error("fuzzy_terms: workspace of %zu bytes, 16-byte aligned, needed (got %zu)", need, workspace_bytes);
        return MMRAG_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    u64 *lists = (u64 *)workspace;
    const int cells = n_patterns * max_expansions;
    MMRAG_CHECK_HIP(hipMemsetAsync(lists, 0, (size_t)cells * sizeof(u64), s));
    if (n_terms > 0) {
        const int gx = (n_terms + FZ_TERMS - 1) / FZ_TERMS;
        const int p_tiles = (n_patterns + FZ_PATTERNS - 1) / FZ_PATTERNS;
        int gy = (FZ_GRID_TARGET + gx - 1) / gx;   // few term tiles: spread the pattern tiles over more workgroups
        gy = gy < 1 ? 1 : (gy > p_tiles ? p_tiles : gy);
        gy = gy > 65535 ? 65535 : gy;
        fuzzy_match_kernel<<<dim3(gx, gy), FZ_TERMS, 0, s>>>(term_off, term_cps, df, n_terms, pat_off, pat_cps,
                                                              pat_edits, n_patterns, max_expansions, lists);
        MMRAG_CHECK_HIP(hipGetLastError());
    }
    fuzzy_unpack_kernel<<<(cells + 255) / 256, 256, 0, s>>>(lists, cells, out_terms, out_edits);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

// test-only export (not in include/mmrag.h): the sizes the tests put their seams on
int mmrag_internal_fuzzy_limits(int *term_tile, int *pattern_tile, int *max_len, int *max_expansions, int *stage_cps) {
    if (!term_tile || !pattern_tile || !max_len || !max_expansions || !stage_cps) return MMRAG_EINVAL;
    *term_tile = FZ_TERMS;
    *pattern_tile = FZ_PATTERNS;
    *max_len = FZ_MAX_LEN;
    *max_expansions = FZ_MAX_E;
    *stage_cps = FZ_STAGE;
    return MMRAG_OK;
}

}  // extern "C"
