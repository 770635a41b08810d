// BM25 lexical search on gfx950: the device half of multimodal_rag_amd/lexical.py.
//
// Layout (all device memory owned by the caller):
//   forward log   row r's postings (term id, tf) at fwd_off[r] .. fwd_off[r+1), sorted by term id; dl[r] its token count
//   df            [n_terms] live rows holding each term (integer atomics on add / delete: order-free)
//   inverted CSR  term t's postings (row, tf) at term_off[t] .. term_off[t+1), sorted by row
//
// CSR build (mmrag_lexical_csr_build): histogram of term ids, one-workgroup exclusive scan, scatter through per-term
// cursors (atomic, so a term's rows land in arrival order), then one pass per term that puts its rows in order -- a
// bitonic sort in LDS for up to SORT_LDS postings, else a bitmap over the rows (set a bit per posting, read the words
// back in order) -- and fills in each posting's tf from the row's forward postings.  The result depends only on the
// forward log.
//
// Search (mmrag_bm25_topk): one workgroup per (query, block of SCORE_R rows) with an LDS accumulator of SCORE_R floats.
// The query's terms are taken in query order; for each, the block's slice of the term's postings is found by binary
// search and every posting adds one contribution.  Rows within a term are distinct, so no two lanes add to the same
// slot between the barriers of consecutive terms, and every score is summed in the same order whatever the batch, the
// grid or the run.  Rows with a positive score, alive and passing `where`, are appended to the query's candidate buffer
// and the deep top-k's select (deep_select.h) sorts them; a query whose matches overflow the buffer is re-run alone
// into n slots after one read of the counters: the driver of candidate_select.h, which search_deep.hip runs too.
#include "candidate_select.h"
#include "row_dot.h"

#include <math.h>

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int LEX_THREADS = 256;
constexpr int SCORE_R = 2048;           // rows per scoring workgroup (8 KiB LDS accumulator)
constexpr int SCORE_TERMS = 128;        // query terms whose postings ranges are looked up together
constexpr int SORT_LDS = 8192;          // postings a term sorts in LDS (32 KiB); longer lists use the row bitmap
constexpr int SORT_GRID = 256;          // workgroups of the per-term sort (each owns one row bitmap)
constexpr int SCAN_TERMS = 1024;        // terms the one-workgroup scan takes per step (one per thread)

__device__ inline long long lower_bound_rows(const int *__restrict__ rows, long long lo, long long hi, int x) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (rows[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// ---- forward log -> df ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LEX_THREADS) void df_update_kernel(const long long *__restrict__ fwd_off,
                                                                const int *__restrict__ fwd_term,
                                                                const long long *__restrict__ rows, long long row0,
                                                                long long n_rows, int sign, int *__restrict__ df) {
    const long long i = (long long)blockIdx.x * (LEX_THREADS / 64) + threadIdx.x / 64;   // one wave per row
    if (i >= n_rows) return;
    const long long r = rows ? rows[i] : row0 + i;
    for (long long p = fwd_off[r] + (threadIdx.x & 63); p < fwd_off[r + 1]; p += 64) atomicAdd(&df[fwd_term[p]], sign);
}

// ---- CSR build -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LEX_THREADS) void csr_hist_kernel(const int *__restrict__ fwd_term, long long P,
                                                               unsigned *__restrict__ cnt) {
    for (long long p = (long long)blockIdx.x * LEX_THREADS + threadIdx.x; p < P; p += (long long)gridDim.x * LEX_THREADS)
        atomicAdd(&cnt[fwd_term[p]], 1u);
}

// term_off = exclusive scan of cnt (term_off[V] = P), cursor = term_off[0 .. V): one workgroup of SCAN_TERMS threads
__global__ __launch_bounds__(SCAN_TERMS) void csr_scan_kernel(const unsigned *__restrict__ cnt, int V,
                                                              long long *__restrict__ term_off,
                                                              unsigned long long *__restrict__ cursor) {
    __shared__ long long wsum[SCAN_TERMS / 64];
    __shared__ long long carry;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < V; base += SCAN_TERMS) {
        const int t = base + tid;
        const long long v = t < V ? cnt[t] : 0;
        long long incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        long long before = carry;
        for (int j = 0; j < w; ++j) before += wsum[j];
        if (t < V) {
            term_off[t] = before + incl - v;
            cursor[t] = (unsigned long long)(before + incl - v);
        }
        __syncthreads();
        if (tid == SCAN_TERMS - 1) carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) term_off[V] = carry;
}

__global__ __launch_bounds__(LEX_THREADS) void csr_scatter_kernel(const long long *__restrict__ fwd_off,
                                                                  const int *__restrict__ fwd_term, long long n,
                                                                  unsigned long long *__restrict__ cursor,
                                                                  int *__restrict__ post_row) {
    const long long r = (long long)blockIdx.x * (LEX_THREADS / 64) + threadIdx.x / 64;   // one wave per row
    if (r >= n) return;
    for (long long p = fwd_off[r] + (threadIdx.x & 63); p < fwd_off[r + 1]; p += 64)
        post_row[atomicAdd(&cursor[fwd_term[p]], 1ull)] = (int)r;
}

// tf of (row r, term t): binary search of r's forward postings (sorted by term id)
__device__ inline int forward_tf(const long long *__restrict__ fwd_off, const int *__restrict__ fwd_term,
                                 const int *__restrict__ fwd_tf, int r, int t) {
    long long lo = fwd_off[r], hi = fwd_off[r + 1];
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (fwd_term[mid] < t)
            lo = mid + 1;
        else
            hi = mid;
    }
    return fwd_tf[lo];   // the term is there: the posting was scattered from this row
}

__global__ __launch_bounds__(LEX_THREADS) void csr_sort_kernel(const long long *__restrict__ fwd_off,
                                                               const int *__restrict__ fwd_term,
                                                               const int *__restrict__ fwd_tf, long long n, int V,
                                                               const long long *__restrict__ term_off,
                                                               int *__restrict__ post_row, int *__restrict__ post_tf,
                                                               unsigned *__restrict__ bitmaps) {
    __shared__ int buf[SORT_LDS];
    __shared__ int wcount[LEX_THREADS / 64];
    const int tid = threadIdx.x;
    const long long words = (n + 31) / 32;
    unsigned *bits = bitmaps + (size_t)blockIdx.x * words;
    for (int t = blockIdx.x; t < V; t += gridDim.x) {
        const long long lo = term_off[t], s = term_off[t + 1] - lo;
        if (s == 0) continue;
        if (s <= SORT_LDS) {
            int P = 1;
            while (P < s) P <<= 1;
            for (int i = tid; i < P; i += LEX_THREADS) buf[i] = i < s ? post_row[lo + i] : INT_MAX;
            __syncthreads();
            for (int size = 2; size <= P; size <<= 1) {
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int i = tid; i < P; i += LEX_THREADS) {
                        const int j = i ^ stride;
                        if (j > i) {
                            const int a = buf[i], b = buf[j];
                            if ((a > b) == ((i & size) == 0)) {
                                buf[i] = b;
                                buf[j] = a;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            for (int i = tid; i < s; i += LEX_THREADS) {
                const int r = buf[i];
                post_row[lo + i] = r;
                post_tf[lo + i] = forward_tf(fwd_off, fwd_term, fwd_tf, r, t);
            }
            __syncthreads();   // buf is reused by the next term
        } else {
            for (long long w = tid; w < words; w += LEX_THREADS) bits[w] = 0u;
            __threadfence();
            __syncthreads();
            for (long long i = tid; i < s; i += LEX_THREADS) {
                const int r = post_row[lo + i];
                atomicOr(&bits[r >> 5], 1u << (r & 31));
            }
            __threadfence();
            __syncthreads();
            long long run = 0;   // rows written so far
            for (long long base = 0; base < words; base += LEX_THREADS) {
                const long long w = base + tid;
                const unsigned word =
                    w < words ? __hip_atomic_load(&bits[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                const int c = __popc(word);
                int incl = c;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int o = __shfl_up(incl, off);
                    if ((tid & 63) >= off) incl += o;
                }
                if ((tid & 63) == 63) wcount[tid >> 6] = incl;
                __syncthreads();
                long long at = run + incl - c;
                long long total = 0;
                for (int j = 0; j < LEX_THREADS / 64; ++j) {
                    if (j < (tid >> 6)) at += wcount[j];
                    total += wcount[j];
                }
                for (unsigned m = word; m; m &= m - 1) {
                    const int r = (int)(w * 32 + __builtin_ctz(m));
                    post_row[lo + at] = r;
                    post_tf[lo + at] = forward_tf(fwd_off, fwd_term, fwd_tf, r, t);
                    ++at;
                }
                run += total;
                __syncthreads();   // wcount is rewritten by the next chunk
            }
        }
    }
}

// ---- scoring -------------------------------------------------------------------------------------------------------
struct Bm25Params {
    const long long *term_off;
    const int *post_row, *post_tf, *dl, *df;
    const int *q_off, *q_terms;
    const uint32_t *alive_bits;
    long long n;
    float k1, b, avgdl;
    double n_live;
    int q_base;            // query of blockIdx.y = 0
    long long cap;         // candidate slots per query
    unsigned *cnt;         // [grid.y] match counts (the true count; appends past cap are dropped)
    float *cand_s;         // [grid.y, cap]
    int *cand_r;
};

__global__ __launch_bounds__(LEX_THREADS) void bm25_score_kernel(Bm25Params p) {
    __shared__ float acc[SCORE_R];
    __shared__ long long rlo[SCORE_TERMS], rhi[SCORE_TERMS];
    __shared__ float idf[SCORE_TERMS];
    __shared__ int any;
    const int tid = threadIdx.x, slot = blockIdx.y, q = p.q_base + slot;
    const long long r0 = (long long)blockIdx.x * SCORE_R;
    const long long r1 = r0 + SCORE_R < p.n ? r0 + SCORE_R : p.n;
    const int t0 = p.q_off[q], nt = p.q_off[q + 1] - t0;
    const float kp1 = p.k1 + 1.0f;
    bool zeroed = false;
    for (int c0 = 0; c0 < nt; c0 += SCORE_TERMS) {
        const int cn = nt - c0 < SCORE_TERMS ? nt - c0 : SCORE_TERMS;
        if (tid == 0) any = 0;
        __syncthreads();
        // the block's slice of each term's postings (two searches per term, one per lane) and the term's idf
        for (int i = tid; i < 2 * cn; i += LEX_THREADS) {
            const int t = p.q_terms[t0 + c0 + (i >> 1)];
            const long long lo = p.term_off[t], hi = p.term_off[t + 1];
            const long long at = lower_bound_rows(p.post_row, lo, hi, (int)((i & 1) ? r1 : r0));
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
            for (int i = tid; i < SCORE_R; i += LEX_THREADS) acc[i] = 0.0f;
            zeroed = true;
            __syncthreads();
        }
        for (int j = 0; j < cn; ++j) {
            const float w = idf[j];
            for (long long i = rlo[j] + tid; i < rhi[j]; i += LEX_THREADS) {
                const int r = p.post_row[i];
                const float tf = (float)p.post_tf[i];
                const float norm = p.k1 * (1.0f - p.b + p.b * ((float)p.dl[r] / p.avgdl));
                acc[r - r0] += w * (tf * kp1 / (tf + norm));
            }
            __syncthreads();   // the next term may add to the same rows
        }
    }
    if (!zeroed) return;   // no posting of any query term in this block
    const int lane = tid & 63;
    for (int i0 = 0; i0 < SCORE_R; i0 += LEX_THREADS) {
        const long long r = r0 + i0 + tid;
        const float s = acc[i0 + tid];
        bool hit = r < r1 && s > 0.0f;
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

// candidate slots per query: no more than n in whole 256s (with >= n slots nothing can overflow)
long long bm25_capacity(long long n, int k) {
    const long long c = candidate_capacity(k), nn = (long long)align_up((size_t)(n > 0 ? n : 1), 256);
    return c < nn ? c : nn;
}

CandWs bm25_ws_layout(int B, long long n, int k) {
    return candidate_ws_layout(B, bm25_capacity(n, k), n > 0 ? n : 1, false);
}

// ---- row dot products ----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LEX_THREADS) void rows_dot_kernel(const T *__restrict__ q, const T *__restrict__ corpus,
                                                               long long ld, int d, const int *__restrict__ qi,
                                                               const long long *__restrict__ rows, long long m,
                                                               float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * (LEX_THREADS / 64) + threadIdx.x / 64;   // one wave per pair
    if (i >= m) return;
    const int lane = threadIdx.x & 63;
    const float s = wave_row_dot(q + (size_t)qi[i] * ld, corpus + (size_t)rows[i] * ld, d, lane);
    if (lane == 0) out[i] = s;
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

int mmrag_lexical_df_update(const int64_t *fwd_off, const int32_t *fwd_term, const int64_t *rows, int64_t row0,
                            int64_t n_rows, int sign, int32_t *df, void *stream) {
    MMRAG_CHECK_ARG(sign == 1 || sign == -1, "lexical_df_update: sign must be +-1 (got %d)", sign);
    MMRAG_CHECK_ARG(n_rows >= 0 && row0 >= 0, "lexical_df_update: bad row range");
    if (n_rows == 0) return MMRAG_OK;
    MMRAG_CHECK_ARG(fwd_off && fwd_term && df, "lexical_df_update: null pointer");
    const long long per = LEX_THREADS / 64;
    df_update_kernel<<<(unsigned)((n_rows + per - 1) / per), LEX_THREADS, 0, (hipStream_t)stream>>>(
        (const long long *)fwd_off, fwd_term, (const long long *)rows, row0, n_rows, sign, df);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

size_t mmrag_lexical_csr_build_workspace_bytes(int64_t n, int n_terms) {
    if (n < 0 || n_terms < 0) return 0;
    return align_up((size_t)n_terms * 4, 256) + align_up((size_t)n_terms * 8, 256) +
           align_up((size_t)SORT_GRID * ((n + 31) / 32) * 4, 256) + 256;
}

int mmrag_lexical_csr_build(const int64_t *fwd_off, const int32_t *fwd_term, const int32_t *fwd_tf, int64_t n,
                            int64_t n_postings, int n_terms, int64_t *term_off, int32_t *post_row, int32_t *post_tf,
                            void *workspace, size_t workspace_bytes, void *stream) {
    MMRAG_CHECK_ARG(n >= 0 && n < INT_MAX && n_terms >= 0 && n_postings >= 0 && n_postings < INT_MAX,
                    "lexical_csr_build: bad sizes n=%lld n_terms=%d n_postings=%lld", (long long)n, n_terms,
                    (long long)n_postings);
    MMRAG_CHECK_ARG(term_off, "lexical_csr_build: null term_off");
    MMRAG_CHECK_ARG(n_postings == 0 || (fwd_off && fwd_term && fwd_tf && post_row && post_tf),
                    "lexical_csr_build: null pointer");
    const size_t need = mmrag_lexical_csr_build_workspace_bytes(n, n_terms);
    if (!workspace || workspace_bytes < need) {
        set_error("lexical_csr_build: workspace %zu bytes < required %zu", workspace_bytes, need);
        return MMRAG_EWORKSPACE;
    }
    MMRAG_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "lexical_csr_build: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    unsigned *cnt = (unsigned *)ws;
    unsigned long long *cursor = (unsigned long long *)(ws + align_up((size_t)n_terms * 4, 256));
    unsigned *bitmaps = (unsigned *)(ws + align_up((size_t)n_terms * 4, 256) + align_up((size_t)n_terms * 8, 256));
    if (n_terms > 0) MMRAG_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)n_terms * 4, s));
    if (n_postings > 0) {
        long long g = (n_postings + LEX_THREADS - 1) / LEX_THREADS;
        csr_hist_kernel<<<(unsigned)(g < 8192 ? g : 8192), LEX_THREADS, 0, s>>>(fwd_term, n_postings, cnt);
        MMRAG_CHECK_HIP(hipGetLastError());
    }
    csr_scan_kernel<<<1, SCAN_TERMS, 0, s>>>(cnt, n_terms, (long long *)term_off, cursor);
    MMRAG_CHECK_HIP(hipGetLastError());
    if (n_postings == 0) return MMRAG_OK;
    const long long per = LEX_THREADS / 64;
    csr_scatter_kernel<<<(unsigned)((n + per - 1) / per), LEX_THREADS, 0, s>>>((const long long *)fwd_off, fwd_term, n,
                                                                                cursor, post_row);
    MMRAG_CHECK_HIP(hipGetLastError());
    const int grid = n_terms < SORT_GRID ? n_terms : SORT_GRID;
    csr_sort_kernel<<<grid, LEX_THREADS, 0, s>>>((const long long *)fwd_off, fwd_term, fwd_tf, n, n_terms,
                                                 (const long long *)term_off, post_row, post_tf, bitmaps);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

size_t mmrag_bm25_topk_workspace_bytes(int B, int64_t n, int k) {
    if (B <= 0 || n < 0 || k < 1 || k > MMRAG_MAX_K_DEEP) return 0;
    return bm25_ws_layout(B, n, k).total;
}

int mmrag_bm25_topk(const int64_t *term_off, const int32_t *post_row, const int32_t *post_tf, const int32_t *dl,
                    const int32_t *df, int n_terms, int64_t n, const int32_t *q_off, const int32_t *q_terms, int B,
                    int64_t n_live, int64_t sum_dl, float k1, float b, int k, const uint32_t *alive_bits,
                    float *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream) {
    MMRAG_CHECK_ARG(B > 0, "bm25_topk: B must be positive (got %d)", B);
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_K_DEEP, "bm25_topk: k=%d outside 1..%d", k, MMRAG_MAX_K_DEEP);
    MMRAG_CHECK_ARG(n >= 0 && n < (int64_t)INT_MAX - SCORE_R, "bm25_topk: n=%lld out of range", (long long)n);
    MMRAG_CHECK_ARG(n_terms >= 0 && n_live >= 0 && n_live <= n && sum_dl >= 0, "bm25_topk: bad statistics");
    MMRAG_CHECK_ARG(k1 >= 0.0f && b >= 0.0f && b <= 1.0f, "bm25_topk: need k1 >= 0 and 0 <= b <= 1");
    MMRAG_CHECK_ARG(out_scores && out_rows && q_off, "bm25_topk: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0 || n_live == 0 || n_terms == 0)   // nothing can match
        return candidate_fill_empty(out_scores, (long long *)out_rows, B, k, s);
    MMRAG_CHECK_ARG(term_off && post_row && post_tf && dl && df && q_terms, "bm25_topk: null pointer");
    const CandWs wl = bm25_ws_layout(B, n, k);
    if (!workspace || workspace_bytes < wl.total) {
        set_error("bm25_topk: workspace %zu bytes < required %zu", workspace_bytes, wl.total);
        return MMRAG_EWORKSPACE;
    }
    MMRAG_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "bm25_topk: workspace must be 16-byte aligned");
    Bm25Params p = {};
    p.term_off = (const long long *)term_off;
    p.post_row = post_row;
    p.post_tf = post_tf;
    p.dl = dl;
    p.df = df;
    p.q_off = q_off;
    p.q_terms = q_terms;
    p.alive_bits = alive_bits;
    p.n = n;
    p.k1 = k1;
    p.b = b;
    p.avgdl = sum_dl > 0 ? (float)((double)sum_dl / (double)n_live) : 1.0f;
    p.n_live = (double)n_live;
    const unsigned blocks = (unsigned)((n + SCORE_R - 1) / SCORE_R);
    const auto score_into = [&](int q_base, unsigned n_queries, float *cand_s, int *cand_r, unsigned *counts,
                                long long slots) -> int {
        Bm25Params pq = p;
        pq.q_base = q_base;
        pq.cap = slots;
        pq.cnt = counts;
        pq.cand_s = cand_s;
        pq.cand_r = cand_r;
        bm25_score_kernel<<<dim3(blocks, n_queries), LEX_THREADS, 0, s>>>(pq);
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    };
    return candidate_select(
        "bm25_topk", B, n, bm25_capacity(n, k), k, 0, out_scores, (long long *)out_rows, (char *)workspace, wl, s,
        [&](float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return score_into(0, (unsigned)B, cand_s, cand_r, counts, slots);
        },
        [&](int qi, float *cand_s, int *cand_r, unsigned *counts, long long slots) {
            return score_into(qi, 1u, cand_s, cand_r, counts, slots);
        });
}

int mmrag_rows_dot(const void *q, const void *corpus, int64_t ld, int dtype, int d, const int32_t *qi,
                   const int64_t *rows, int64_t m, float *out, void *stream) {
    MMRAG_CHECK_ARG(dtype >= 0 && dtype <= 2, "rows_dot: bad dtype %d", dtype);
    MMRAG_CHECK_ARG(d > 0 && ld >= d && m >= 0, "rows_dot: bad shape d=%d ld=%lld m=%lld", d, (long long)ld,
                    (long long)m);
    if (m == 0) return MMRAG_OK;
    MMRAG_CHECK_ARG(q && corpus && qi && rows && out, "rows_dot: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long long per = LEX_THREADS / 64;
    const unsigned grid = (unsigned)((m + per - 1) / per);
    with_elem_type(dtype, [&](auto tag) {
        using T = elem_t<decltype(tag)::value>;
        rows_dot_kernel<T><<<grid, LEX_THREADS, 0, s>>>((const T *)q, (const T *)corpus, ld, d, qi,
                                                        (const long long *)rows, m, out);
    });
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

// The sizes at which the kernels above change path: rows per scoring workgroup, query terms per lookup chunk, the longest
// postings list sorted in LDS, the sort's grid and the scan's terms per step.  The tests restate them to place their
// cases on the edges and compare (candidate_select.h's capacity has mmrag_internal_candidate_capacity).  Exported for
// them, deliberately absent from include/mmrag.h.  Host code, no device needed.
int mmrag_internal_lexical_limits(int *score_rows, int *score_terms, int *sort_lds, int *sort_grid, int *scan_terms) {
    if (!score_rows || !score_terms || !sort_lds || !sort_grid || !scan_terms) return -1;
    *score_rows = SCORE_R;
    *score_terms = SCORE_TERMS;
    *sort_lds = SORT_LDS;
    *sort_grid = SORT_GRID;
    *scan_terms = SCAN_TERMS;
    return 0;
}

}  // extern "C"
