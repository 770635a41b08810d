// Phrase queries on gfx950: the positional half of the lexical leg (multimodal_rag_amd/lexical.py; DESIGN.md 3.1e,
// "Phrase queries").
//
// Layout beside lexical.hip's forward log and CSR (all device memory owned by the caller):
//   positions plane  forward posting i (row r, term t) stands at the token positions pos[pos_off[i] .. pos_off[i+1]),
//                    ascending; pos_off is the prefix sum of fwd_tf
//   phrase tables    phrase p = ph_terms[ph_off[p] .. ph_off[p+1]), its driver term ph_driver[p] (-1: occurs nowhere)
//   ptf              per phrase, aligned with the driver's CSR list: tf_p of that posting's row
//
// Match (mmrag_phrase_match): a workgroup takes PH_BLOCK consecutive postings of one phrase's driver list, a lane per
// posting.  The lane finds each phrase term in its row's forward postings (sorted by term id: one binary search per term)
// and parks the term's position range in LDS; a row that lacks a term is done.  Then every position of the phrase's
// FIRST term is a start: from it the lane takes, term by term, the earliest position behind the previous one (a binary
// search in that term's range) and stops as soon as the gaps exceed the slop -- the greedy choice decides existence.
// A lane walks up to PH_LANE_STARTS starts alone; a row with more (a stop word leading a phrase) is shared by its
// wave afterwards, 64 starts at a time, so one long row does not hold a whole workgroup on one lane.  ptf stays aligned
// with the driver's list, so it is row-sorted like the list and needs no compaction.
//
// Score (mmrag_bm25_phrase_topk): bm25_score_kernel's twin.  The loose terms are scored by the same statements in the
// same order; each phrase is one more clause over the block's slice of its driver's list with tf from ptf, and an LDS
// counter per row says how many phrases it holds.  candidate_select.h's driver runs after it as it does for bm25_topk.
#include "candidate_select.h"

#include <math.h>

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int PH_THREADS = 256;
constexpr int PH_BLOCK = 256;          // driver postings per match workgroup: one per lane
constexpr int PH_LANE_STARTS = 64;     // starts one lane walks alone; a row with more is shared by the wave
constexpr int PH_SCORE_R = 2048;       // rows per scoring workgroup: lexical.hip's SCORE_R
constexpr int PH_SCORE_TERMS = 128;    // lexical.hip's SCORE_TERMS
constexpr int PH_MAX_TERMS = MMRAG_MAX_PHRASE_TERMS;
constexpr int PH_MAX_PHRASES = MMRAG_MAX_QUERY_PHRASES;
constexpr int PH_GRID_Y = 32768;       // phrases (or queries) per launch

__device__ inline long long ph_lower_bound_rows(const int *__restrict__ rows, long long lo, long long hi, int x) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (rows[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// ---- match -----------------------------------------------------------------------------------------------------------
struct MatchParams {
    const long long *fwd_off;
    const int *fwd_term;
    const long long *pos_off;
    const int *pos;
    const long long *term_off;
    const int *post_row;
    const int *ph_off, *ph_terms, *ph_driver;
    const long long *ptf_off;
    const uint32_t *alive_bits;
    int slop, ph_base;
    int *ptf, *ph_rows;
};

// does the phrase occur at start `s` (an index into its first term's positions) of the row parked in LDS slot `slot`?
__device__ inline int occurs_at(const int *__restrict__ pos, const long long (*plo)[PH_BLOCK],
                                const int (*plen)[PH_BLOCK], int slot, int m, int s, int slop) {
    const int p0 = pos[plo[0][slot] + s];
    int prev = p0;
    for (int j = 1; j < m; ++j) {
        const long long base = plo[j][slot];
        int lo = 0, hi = plen[j][slot];
        const int len = hi;
        while (lo < hi) {   // the first position of term j behind `prev`
            const int mid = (lo + hi) >> 1;
            if (pos[base + mid] <= prev)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo == len) return 0;
        prev = pos[base + lo];
        if (prev - p0 - j > slop) return 0;   // later terms only widen the span
    }
    return 1;
}

__global__ __launch_bounds__(PH_THREADS) void phrase_match_kernel(MatchParams p) {
    __shared__ long long plo[PH_MAX_TERMS][PH_BLOCK];
    __shared__ int plen[PH_MAX_TERMS][PH_BLOCK];
    __shared__ int terms[PH_MAX_TERMS];
    const int tid = threadIdx.x, lane = tid & 63, ph = p.ph_base + blockIdx.y;
    const int drv = p.ph_driver[ph];
    if (drv < 0) return;
    const long long d0 = p.term_off[drv], dn = p.term_off[drv + 1] - d0;
    const long long i0 = (long long)blockIdx.x * PH_BLOCK;
    if (i0 >= dn) return;
    const int t0 = p.ph_off[ph];
    int m = p.ph_off[ph + 1] - t0;
    if (m > PH_MAX_TERMS) m = PH_MAX_TERMS;
    if (tid < m) terms[tid] = p.ph_terms[t0 + tid];
    __syncthreads();
    const long long i = i0 + tid;
    const bool mine = i < dn;
    bool ok = mine && m > 0;
    if (ok) {
        const int r = p.post_row[d0 + i];
        if (p.alive_bits) ok = (p.alive_bits[r >> 5] >> (r & 31)) & 1u;
        if (ok) {
            const long long f0 = p.fwd_off[r], f1 = p.fwd_off[r + 1];
            for (int j = 0; j < m && ok; ++j) {
                const int t = terms[j];
                long long lo = f0, hi = f1;
                while (lo < hi) {
                    const long long mid = (lo + hi) >> 1;
                    if (p.fwd_term[mid] < t)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (lo < f1 && p.fwd_term[lo] == t) {
                    const long long a = p.pos_off[lo];
                    plo[j][tid] = a;
                    plen[j][tid] = (int)(p.pos_off[lo + 1] - a);
                } else {
                    ok = false;
                }
            }
        }
    }
    __syncthreads();   // the ranges of a long row are read by its whole wave below
    const int starts = ok ? plen[0][tid] : 0;
    const bool heavy = starts > PH_LANE_STARTS;
    int count = 0;
    if (!heavy)
        for (int s = 0; s < starts; ++s) count += occurs_at(p.pos, plo, plen, tid, m, s, p.slop);
    unsigned long long hm = __builtin_amdgcn_ballot_w64(heavy);
    while (hm) {   // wave-uniform: every lane takes a share of each long row of its wave
        const int src = __builtin_ctzll(hm);
        hm &= hm - 1;
        const int slot = (tid & ~63) + src;
        const int ns = plen[0][slot];
        int c = 0;
        for (int s = lane; s < ns; s += 64) c += occurs_at(p.pos, plo, plen, slot, m, s, p.slop);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
        if (lane == src) count = c;
    }
    if (mine) p.ptf[p.ptf_off[ph] + i] = count;
    const unsigned long long hit = __builtin_amdgcn_ballot_w64(count > 0);
    if (hit && lane == __builtin_ctzll(hit)) atomicAdd(&p.ph_rows[ph], __popcll(hit));
}

// ---- per-query bitmaps: the rows that hold every phrase of the query ---------------------------------------------------
struct BitmapParams {
    const long long *term_off;
    const int *post_row;
    const int *ph_driver;
    const long long *ptf_off;
    const int *ptf;
    const int *q_ph_off, *q_ph;
    long long n, words;
    int q_base;
    uint32_t *out;   // [B, words]
};

__global__ __launch_bounds__(PH_THREADS) void phrase_bitmap_kernel(BitmapParams p) {
    __shared__ int matched[PH_SCORE_R];
    __shared__ long long slice[2];
    const int tid = threadIdx.x, q = p.q_base + blockIdx.y;
    const long long r0 = (long long)blockIdx.x * PH_SCORE_R;
    const long long r1 = r0 + PH_SCORE_R < p.n ? r0 + PH_SCORE_R : p.n;
    const long long w0 = r0 >> 5;
    uint32_t *out = p.out + (size_t)q * p.words;
    const int ph0 = p.q_ph_off[q];
    int nph = p.q_ph_off[q + 1] - ph0;
    if (nph > PH_MAX_PHRASES) nph = PH_MAX_PHRASES;
    if (nph <= 0) {   // no phrase: every row below n
        for (int w = tid; w < PH_SCORE_R / 32; w += PH_THREADS) {
            if (w0 + w >= p.words) continue;
            const long long base = (w0 + w) * 32;
            out[w0 + w] = base + 32 <= p.n ? 0xffffffffu : base >= p.n ? 0u : (1u << (int)(p.n - base)) - 1u;
        }
        return;
    }
    for (int i = tid; i < PH_SCORE_R; i += PH_THREADS) matched[i] = 0;
    __syncthreads();
    for (int j = 0; j < nph; ++j) {
        const int ph = p.q_ph[ph0 + j];
        const int drv = p.ph_driver[ph];
        if (drv < 0) continue;   // occurs nowhere: no row reaches nph
        const long long lo = p.term_off[drv], hi = p.term_off[drv + 1];
        if (tid < 2) slice[tid] = ph_lower_bound_rows(p.post_row, lo, hi, (int)(tid ? r1 : r0));
        __syncthreads();
        const long long a = slice[0], b = slice[1], base = p.ptf_off[ph] - lo;
        for (long long i = a + tid; i < b; i += PH_THREADS)
            if (p.ptf[base + i] > 0) matched[p.post_row[i] - r0] += 1;   // a phrase's rows are distinct
        __syncthreads();   // the next phrase rewrites slice and adds to the same rows
    }
    for (int w = tid; w < PH_SCORE_R / 32; w += PH_THREADS) {
        if (w0 + w >= p.words) continue;
        uint32_t bits = 0u;
        for (int b = 0; b < 32; ++b)
            if (matched[w * 32 + b] == nph) bits |= 1u << b;
        out[w0 + w] = bits;
    }
}

// ---- scoring -----------------------------------------------------------------------------------------------------------
struct PhraseScoreParams {
    const long long *term_off;
    const int *post_row, *post_tf, *dl, *df;
    const int *q_off, *q_terms;
    const int *q_ph_off, *q_ph, *ph_off, *ph_terms, *ph_driver;
    const long long *ptf_off;
    const int *ptf;
    const uint32_t *alive_bits;
    long long n;
    float k1, b, avgdl;
    double n_live;
    int require;
    int q_base;            // query of blockIdx.y = 0
    long long cap;         // candidate slots per query
    unsigned *cnt;         // [grid.y] match counts (the true count; appends past cap are dropped)
    float *cand_s;         // [grid.y, cap]
    int *cand_r;
};

__global__ __launch_bounds__(PH_THREADS) void bm25_phrase_score_kernel(PhraseScoreParams p) {
    __shared__ float acc[PH_SCORE_R];
    __shared__ int matched[PH_SCORE_R];
    __shared__ long long rlo[PH_SCORE_TERMS], rhi[PH_SCORE_TERMS];
    __shared__ float idf[PH_SCORE_TERMS];
    __shared__ int any;
    __shared__ long long plo[PH_MAX_PHRASES], phi[PH_MAX_PHRASES], pbase[PH_MAX_PHRASES];
    __shared__ float pidf[PH_MAX_PHRASES];
    const int tid = threadIdx.x, slot = blockIdx.y, q = p.q_base + slot;
    const long long r0 = (long long)blockIdx.x * PH_SCORE_R;
    const long long r1 = r0 + PH_SCORE_R < p.n ? r0 + PH_SCORE_R : p.n;
    const int t0 = p.q_off[q], nt = p.q_off[q + 1] - t0;
    const float kp1 = p.k1 + 1.0f;
    bool zeroed = false;
    // the loose terms: bm25_score_kernel's statements, in its order
    for (int c0 = 0; c0 < nt; c0 += PH_SCORE_TERMS) {
        const int cn = nt - c0 < PH_SCORE_TERMS ? nt - c0 : PH_SCORE_TERMS;
        if (tid == 0) any = 0;
        __syncthreads();
        for (int i = tid; i < 2 * cn; i += PH_THREADS) {
            const int t = p.q_terms[t0 + c0 + (i >> 1)];
            const long long lo = p.term_off[t], hi = p.term_off[t + 1];
            const long long at = ph_lower_bound_rows(p.post_row, lo, hi, (int)((i & 1) ? r1 : r0));
            if (i & 1) {
                rhi[i >> 1] = at;
            } else {
                rlo[i >> 1] = at;
                const double df = (double)p.df[t];
                idf[i >> 1] = (float)log1p((p.n_live - df + 0.5) / (df + 0.5));
            }
        }
        __syncthreads();
        if (tid < cn && rhi[tid] > rlo[tid]) any = 1;
        __syncthreads();
        if (!any) continue;
        if (!zeroed) {
            for (int i = tid; i < PH_SCORE_R; i += PH_THREADS) acc[i] = 0.0f;
            zeroed = true;
            __syncthreads();
        }
        for (int j = 0; j < cn; ++j) {
            const float w = idf[j];
            for (long long i = rlo[j] + tid; i < rhi[j]; i += PH_THREADS) {
                const int r = p.post_row[i];
                const float tf = (float)p.post_tf[i];
                const float norm = p.k1 * (1.0f - p.b + p.b * ((float)p.dl[r] / p.avgdl));
                acc[r - r0] += w * (tf * kp1 / (tf + norm));
            }
            __syncthreads();   // the next term may add to the same rows
        }
    }
    // the phrases: one clause each, over the block's slice of the driver's list with tf from ptf
    const int ph0 = p.q_ph_off[q];
    int nph = p.q_ph_off[q + 1] - ph0;
    if (nph > PH_MAX_PHRASES) nph = PH_MAX_PHRASES;
    const bool need_all = p.require && nph > 0;
    if (nph > 0) {
        __syncthreads();
        if (tid < nph) {
            const int ph = p.q_ph[ph0 + tid];
            const int drv = p.ph_driver[ph];
            long long a = 0, b = 0, base = 0;
            float w = 0.0f;
            if (drv >= 0) {
                const long long lo = p.term_off[drv], hi = p.term_off[drv + 1];
                a = ph_lower_bound_rows(p.post_row, lo, hi, (int)r0);
                b = ph_lower_bound_rows(p.post_row, lo, hi, (int)r1);
                base = p.ptf_off[ph] - lo;
                int j1 = p.ph_off[ph + 1];
                if (j1 - p.ph_off[ph] > PH_MAX_TERMS) j1 = p.ph_off[ph] + PH_MAX_TERMS;
                for (int j = p.ph_off[ph]; j < j1; ++j) {
                    const double df = (double)p.df[p.ph_terms[j]];
                    w += (float)log1p((p.n_live - df + 0.5) / (df + 0.5));
                }
            }
            plo[tid] = a;
            phi[tid] = b;
            pbase[tid] = base;
            pidf[tid] = w;
        }
        __syncthreads();
        bool some = false;
        for (int j = 0; j < nph; ++j) some |= phi[j] > plo[j];
        if (some) {
            for (int i = tid; i < PH_SCORE_R; i += PH_THREADS) {
                if (!zeroed) acc[i] = 0.0f;
                matched[i] = 0;
            }
            zeroed = true;
            __syncthreads();
            for (int j = 0; j < nph; ++j) {
                const float w = pidf[j];
                for (long long i = plo[j] + tid; i < phi[j]; i += PH_THREADS) {
                    const int tfi = p.ptf[pbase[j] + i];
                    if (tfi == 0) continue;
                    const int r = p.post_row[i];
                    const float tf = (float)tfi;
                    const float norm = p.k1 * (1.0f - p.b + p.b * ((float)p.dl[r] / p.avgdl));
                    acc[r - r0] += w * (tf * kp1 / (tf + norm));
                    matched[r - r0] += 1;
                }
                __syncthreads();   // the next phrase may add to the same rows
            }
        } else if (need_all) {
            return;   // no posting of any phrase in this block: no row can hold them all
        }
    }
    if (!zeroed) return;   // no posting of any clause in this block
    const int lane = tid & 63;
    for (int i0 = 0; i0 < PH_SCORE_R; i0 += PH_THREADS) {
        const long long r = r0 + i0 + tid;
        const float s = acc[i0 + tid];
        bool hit = r < r1 && (need_all ? matched[i0 + tid] == nph : s > 0.0f);
        if (hit && p.alive_bits) hit = (p.alive_bits[r >> 5] >> (r & 31)) & 1u;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
        if (!m) continue;
        unsigned base = 0;
        const int leader = __builtin_ctzll(m);
        if (lane == leader) base = atomicAdd(&p.cnt[slot], (unsigned)__popcll(m));
        base = __shfl(base, leader);
        if (hit) {
            const unsigned at = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            if (at < p.cap) {
                p.cand_s[(size_t)slot * p.cap + at] = s;
                p.cand_r[(size_t)slot * p.cap + at] = (int)r;
            }
        }
    }
}

// lexical.hip's capacity and layout: no more than n slots in whole 256s
long long phrase_capacity(long long n, int k) {
    const long long c = candidate_capacity(k), nn = (long long)align_up((size_t)(n > 0 ? n : 1), 256);
    return c < nn ? c : nn;
}

CandWs phrase_ws_layout(int B, long long n, int k) {
    return candidate_ws_layout(B, phrase_capacity(n, k), n > 0 ? n : 1, false);
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

int mmrag_phrase_match(const int64_t *fwd_off, const int32_t *fwd_term, const int64_t *pos_off, const int32_t *pos,
                       int64_t n, const int64_t *term_off, const int32_t *post_row, const int32_t *ph_off,
                       const int32_t *ph_terms, const int32_t *ph_driver, const int64_t *ptf_off, int n_phrases,
                       int max_terms, int64_t max_driver_postings, int slop, const uint32_t *alive_bits, int32_t *ptf,
                       int32_t *ph_rows, const int32_t *q_ph_off, const int32_t *q_ph, int B, int max_phrases,
                       uint32_t *bitmaps, void *stream) {
    MMRAG_CHECK_ARG(n >= 0 && n < (int64_t)INT_MAX - PH_SCORE_R, "phrase_match: n=%lld out of range", (long long)n);
    MMRAG_CHECK_ARG(n_phrases >= 0 && B >= 0 && max_driver_postings >= 0 && max_driver_postings < INT_MAX,
                    "phrase_match: negative count");
    MMRAG_CHECK_ARG(slop >= 0 && slop <= MMRAG_MAX_PHRASE_SLOP, "phrase_match: slop=%d outside 0..%d", slop,
                    MMRAG_MAX_PHRASE_SLOP);
    MMRAG_CHECK_ARG(max_terms >= 0 && max_terms <= MMRAG_MAX_PHRASE_TERMS, "phrase_match: %d terms in a phrase, at most %d",
                    max_terms, MMRAG_MAX_PHRASE_TERMS);
    MMRAG_CHECK_ARG(max_phrases >= 0 && max_phrases <= MMRAG_MAX_QUERY_PHRASES,
                    "phrase_match: %d phrases in a query, at most %d", max_phrases, MMRAG_MAX_QUERY_PHRASES);
    MMRAG_CHECK_ARG(n_phrases == 0 || (ph_off && ph_terms && ph_driver && ptf_off && ph_rows),
                    "phrase_match: null phrase table");
    MMRAG_CHECK_ARG(!bitmaps || B == 0 || (q_ph_off && (n_phrases == 0 || q_ph)), "phrase_match: null query table");
    const bool match = n_phrases > 0 && max_driver_postings > 0, maps = bitmaps && B > 0 && n > 0;
    MMRAG_CHECK_ARG(!match || (fwd_off && fwd_term && pos_off && pos && term_off && post_row && ptf),
                    "phrase_match: null pointer");
    MMRAG_CHECK_ARG(!maps || n_phrases == 0 || (term_off && post_row && ptf), "phrase_match: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_phrases > 0) MMRAG_CHECK_HIP(hipMemsetAsync(ph_rows, 0, (size_t)n_phrases * sizeof(int32_t), s));
    if (match) {
        MatchParams p = {};
        p.fwd_off = (const long long *)fwd_off;
        p.fwd_term = fwd_term;
        p.pos_off = (const long long *)pos_off;
        p.pos = pos;
        p.term_off = (const long long *)term_off;
        p.post_row = post_row;
        p.ph_off = ph_off;
        p.ph_terms = ph_terms;
        p.ph_driver = ph_driver;
        p.ptf_off = (const long long *)ptf_off;
        p.alive_bits = alive_bits;
        p.slop = slop;
        p.ptf = ptf;
        p.ph_rows = ph_rows;
        const unsigned gx = (unsigned)((max_driver_postings + PH_BLOCK - 1) / PH_BLOCK);
        for (int base = 0; base < n_phrases; base += PH_GRID_Y) {
            p.ph_base = base;
            const int gy = n_phrases - base < PH_GRID_Y ? n_phrases - base : PH_GRID_Y;
            phrase_match_kernel<<<dim3(gx, (unsigned)gy), PH_THREADS, 0, s>>>(p);
            MMRAG_CHECK_HIP(hipGetLastError());
        }
    }
    if (maps) {
        BitmapParams bp = {};
        bp.term_off = (const long long *)term_off;
        bp.post_row = post_row;
        bp.ph_driver = ph_driver;
        bp.ptf_off = (const long long *)ptf_off;
        bp.ptf = ptf;
        bp.q_ph_off = q_ph_off;
        bp.q_ph = q_ph;
        bp.n = n;
        bp.words = 4 * ((n + 127) / 128);   // mmrag_filter_words(n)
        bp.out = bitmaps;
        const unsigned gx = (unsigned)((n + PH_SCORE_R - 1) / PH_SCORE_R);
        for (int base = 0; base < B; base += PH_GRID_Y) {
            bp.q_base = base;
            const int gy = B - base < PH_GRID_Y ? B - base : PH_GRID_Y;
            phrase_bitmap_kernel<<<dim3(gx, (unsigned)gy), PH_THREADS, 0, s>>>(bp);
            MMRAG_CHECK_HIP(hipGetLastError());
        }
    }
    return MMRAG_OK;
}

size_t mmrag_bm25_phrase_topk_workspace_bytes(int B, int64_t n, int k) {
    if (B <= 0 || n < 0 || k < 1 || k > MMRAG_MAX_K_DEEP) return 0;
    return phrase_ws_layout(B, n, k).total;
}

int mmrag_bm25_phrase_topk(const int64_t *term_off, const int32_t *post_row, const int32_t *post_tf, const int32_t *dl,
                           const int32_t *df, int n_terms, int64_t n, const int32_t *q_off, const int32_t *q_terms,
                           int B, const int32_t *q_ph_off, const int32_t *q_ph, const int32_t *ph_off,
                           const int32_t *ph_terms, const int32_t *ph_driver, const int64_t *ptf_off,
                           const int32_t *ptf, int n_phrases, int max_terms, int max_phrases, int require,
                           int64_t n_live, int64_t sum_dl, float k1, float b, int k, const uint32_t *alive_bits,
                           float *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream) {
    MMRAG_CHECK_ARG(B > 0, "bm25_phrase_topk: B must be positive (got %d)", B);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K_DEEP, "bm25_phrase_topk: k=%d outside 1..%d", k, MMRAG_MAX_K_DEEP);
    MMRAG_CHECK_ARG(n >= 0 && n < (int64_t)INT_MAX - PH_SCORE_R, "bm25_phrase_topk: n=%lld out of range", (long long)n);
    MMRAG_CHECK_ARG(n_terms >= 0 && n_live >= 0 && n_live <= n && sum_dl >= 0, "bm25_phrase_topk: bad statistics");
    MMRAG_CHECK_ARG(k1 >= 0.0f && b >= 0.0f && b <= 1.0f, "bm25_phrase_topk: need k1 >= 0 and 0 <= b <= 1");
    MMRAG_CHECK_ARG(n_phrases >= 0, "bm25_phrase_topk: n_phrases=%d", n_phrases);
    MMRAG_CHECK_ARG(max_terms >= 0 && max_terms <= MMRAG_MAX_PHRASE_TERMS,
                    "bm25_phrase_topk: %d terms in a phrase, at most %d", max_terms, MMRAG_MAX_PHRASE_TERMS);
    MMRAG_CHECK_ARG(max_phrases >= 0 && max_phrases <= MMRAG_MAX_QUERY_PHRASES,
                    "bm25_phrase_topk: %d phrases in a query, at most %d", max_phrases, MMRAG_MAX_QUERY_PHRASES);
    MMRAG_CHECK_ARG(out_scores && out_rows && q_off && q_ph_off, "bm25_phrase_topk: null pointer");
    MMRAG_CHECK_ARG(n_phrases == 0 || (q_ph && ph_off && ph_terms && ph_driver && ptf_off && ptf),
                    "bm25_phrase_topk: null phrase table");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0 || n_live == 0 || n_terms == 0)   // nothing can match
        return candidate_fill_empty(out_scores, (long long *)out_rows, B, k, s);
    MMRAG_CHECK_ARG(term_off && post_row && post_tf && dl && df && q_terms, "bm25_phrase_topk: null pointer");
    const CandWs wl = phrase_ws_layout(B, n, k);
    if (!workspace || workspace_bytes < wl.total) {
        set_error("bm25_phrase_topk: workspace %zu bytes < required %zu", workspace_bytes, wl.total);
        return MMRAG_EWORKSPACE;
    }
    MMRAG_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "bm25_phrase_topk: workspace must be 16-byte aligned");
    PhraseScoreParams p = {};
    p.term_off = (const long long *)term_off;
    p.post_row = post_row;
    p.post_tf = post_tf;
    p.dl = dl;
    p.df = df;
    p.q_off = q_off;
    p.q_terms = q_terms;
    p.q_ph_off = q_ph_off;
    p.q_ph = q_ph;
    p.ph_off = ph_off;
    p.ph_terms = ph_terms;
    p.ph_driver = ph_driver;
    p.ptf_off = (const long long *)ptf_off;
    p.ptf = ptf;
    p.alive_bits = alive_bits;
    p.n = n;
    p.k1 = k1;
    p.b = b;
    p.avgdl = sum_dl > 0 ? (float)((double)sum_dl / (double)n_live) : 1.0f;
    p.n_live = (double)n_live;
    p.require = require != 0;
    const unsigned blocks = (unsigned)((n + PH_SCORE_R - 1) / PH_SCORE_R);
    const auto score_into = [&](int q_base, unsigned n_queries, float *cand_s, int *cand_r, unsigned *counts,
                                long long slots) -> int {
        PhraseScoreParams pq = p;
        pq.q_base = q_base;
        pq.cap = slots;
        pq.cnt = counts;
        pq.cand_s = cand_s;
        pq.cand_r = cand_r;
        bm25_phrase_score_kernel<<<dim3(blocks, n_queries), PH_THREADS, 0, s>>>(pq);
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    };
    return candidate_select(
        "bm25_phrase_topk", B, n, phrase_capacity(n, k), k, 0, out_scores, (long long *)out_rows, (char *)workspace, wl,
        s,
        [&](float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return score_into(0, (unsigned)B, cand_s, cand_r, counts, slots);
        },
        [&](int qi, float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return score_into(qi, 1u, cand_s, cand_r, counts, slots);
        });
}

// The sizes at which the kernels above change path: driver postings per match workgroup, the starts a lane walks alone
// (a row with more is shared by its wave), the wave's lanes, rows per scoring workgroup.  Exported for the tests,
// deliberately absent from include/mmrag.h.  Host code, no device needed.
int mmrag_internal_phrase_limits(int *match_block, int *lane_starts, int *wave_lanes, int *score_rows) {
    if (!match_block || !lane_starts || !wave_lanes || !score_rows) return -1;
    *match_block = PH_BLOCK;
    *lane_starts = PH_LANE_STARTS;
    *wave_lanes = 64;
    *score_rows = PH_SCORE_R;
    return 0;
}

}  // extern "C"
