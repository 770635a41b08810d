// Significant terms on gfx950: which terms set a group of rows apart from the rest of the collection.  The device half of
// LexicalIndex.group_terms (multimodal_rag_amd/lexical.py); tests/terms_ref.py restates it.
//
// Rows carry a label group[r] in 0 .. G-1, or -1 for "in no group" (dead rows are -1).  For group g and term t, with
//   fg = rows of g holding t,  size = group_size[g],  bg = df[t],  N = n_live,  fgp = fg / size,  bgp = bg / N
// the pair qualifies when size > 0, bg > 0, fg >= min_count, t's bit is set in the optional term mask and fgp > bgp; its
// score is the JLH measure (fgp - bgp) * (fgp / bgp), float32 with every operation rounded once.  Group g's result is
// its `top` qualifying terms, score descending, ties to the lower term id.
//
// The counting kernel is term-major over the inverted CSR of lexical.hip and serves one window of at most GT_GROUPS
// consecutive groups per launch: a workgroup takes GT_BLOCK_TERMS consecutive term ids, drops every term whose df is
// below min_count (df bounds every fg) or whose mask bit is clear without touching its postings, and counts the others
// into a histogram of GT_GROUPS LDS counters -- a list of at most GT_WAVE_LIMIT postings by one wave with a histogram of
// its own, a longer one by the whole workgroup.  The sweep of a histogram clears it and appends every qualifying bin as a
// candidate (score, term) to its group's slots under the contract of candidate_select.h (a true per-group counter,
// appends past cap dropped); the shared select sorts each group's top and a group whose candidates overflowed is counted
// again alone into n_terms slots by the same kernel with a window of that one group.  The only global atomics are the
// slot counters.  A second kernel walks the list of every returned (group, term) once more for its integer count.
#include "candidate_select.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int GT_THREADS = 256;
constexpr int GT_WAVES = GT_THREADS / 64;
constexpr int GT_GROUPS = 256;          // groups of one launch: the LDS histogram's counters (1 KiB)
// consecutive term ids of one workgroup.  Few: under Zipf's law the lowest ids hold the longest lists, and the workgroup
// that gets them is the launch's tail.  Measured over 116 M postings (DESIGN.md 3.1e "Significant terms"): 62 ms a pass
// with 64 ids and one posting in flight per thread, 12 ms with 8 ids and GT_LONG_UNROLL in flight
constexpr int GT_BLOCK_TERMS = 8;
constexpr int GT_WAVE_LIMIT = 1024;     // the longest postings list one wave takes alone (16 steps of 64)
constexpr int GT_LONG_UNROLL = 4;       // postings a thread of the workgroup's walk has in flight
constexpr int GT_COUNT_GRID = 65536;    // workgroups of the count kernel (it strides over the outputs)

struct TermsParams {
    const long long *term_off;
    const int *post_row, *df, *group, *group_size;
    const uint32_t *term_bits;
    int n_terms, n_groups;
    int g0, gw;             // the launch's window: groups g0 .. g0 + gw, gw <= GT_GROUPS
    int min_count;
    float n_live;
    long long cap;          // candidate slots per group
    unsigned *cnt;          // [gw] qualifying pairs per group (the true count; appends past cap are dropped)
    float *cand_s;          // [gw, cap]
    int *cand_t;
};

// bin `rel` of a swept histogram held `fg` rows of term t: append the pair when it qualifies
__device__ inline void terms_emit(const TermsParams &p, int rel, int fg, int t, int bg) {
    if (fg < p.min_count) return;
    const int size = p.group_size[p.g0 + rel];
    if (size <= 0) return;
    const float fgp = __fdiv_rn((float)fg, (float)size), bgp = __fdiv_rn((float)bg, p.n_live);
    if (!(fgp > bgp)) return;
    const float s = __fmul_rn(__fsub_rn(fgp, bgp), __fdiv_rn(fgp, bgp));
    const unsigned at = atomicAdd(&p.cnt[rel], 1u);
    if (at < p.cap) {
        p.cand_s[(size_t)rel * p.cap + at] = s;
        p.cand_t[(size_t)rel * p.cap + at] = t;
    }
}

__global__ __launch_bounds__(GT_THREADS) void group_terms_kernel(TermsParams p) {
    __shared__ unsigned hist[GT_WAVES][GT_GROUPS];   // hist[w]: wave w's; hist[0] also serves the workgroup's lists
    __shared__ long long t_lo[GT_BLOCK_TERMS];
    __shared__ int t_len[GT_BLOCK_TERMS];            // 0: the term is skipped
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int t0 = blockIdx.x * GT_BLOCK_TERMS;
    for (int i = tid; i < GT_WAVES * GT_GROUPS; i += GT_THREADS) (&hist[0][0])[i] = 0u;
    if (tid < GT_BLOCK_TERMS) {
        const int t = t0 + tid;
        long long lo = 0;
        int len = 0;
        if (t < p.n_terms) {
            const int bg = p.df[t];
            const bool masked = p.term_bits && !((p.term_bits[t >> 5] >> (t & 31)) & 1u);
            if (bg >= p.min_count && bg > 0 && !masked) {
                lo = p.term_off[t];
                len = (int)(p.term_off[t + 1] - lo);
            }
        }
        t_lo[tid] = lo;
        t_len[tid] = len;
    }
    __syncthreads();

    // the short lists: wave w takes the block's terms w, w + GT_WAVES, .. with its own histogram
    unsigned *mine = hist[w];
    for (int j = w; j < GT_BLOCK_TERMS; j += GT_WAVES) {
        const int len = t_len[j];
        if (len == 0 || len > GT_WAVE_LIMIT) continue;
        const long long lo = t_lo[j];
        bool hit = false;
        for (int i = lane; i < len; i += 64) {
            const unsigned rel = (unsigned)(p.group[p.post_row[lo + i]] - p.g0);
            if (rel < (unsigned)p.gw) {
                atomicAdd(&mine[rel], 1u);
                hit = true;
            }
        }
        if (!__builtin_amdgcn_ballot_w64(hit)) continue;   // no row of the window: the histogram is still clear
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int t = t0 + j, bg = p.df[t];
        for (int rel = lane; rel < p.gw; rel += 64) {
            const int fg = (int)mine[rel];
            if (fg) {
                mine[rel] = 0u;
                terms_emit(p, rel, fg, t, bg);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();

    // the long lists: the whole workgroup strides over one list at a time
    unsigned *all = hist[0];
    for (int j = 0; j < GT_BLOCK_TERMS; ++j) {
        const int len = t_len[j];
        if (len <= GT_WAVE_LIMIT) continue;   // the same in every thread
        const long long lo = t_lo[j];
        // GT_LONG_UNROLL independent (row, label) load pairs per thread and step: the walk is bound by their latency
        for (int i0 = tid; i0 < len; i0 += GT_LONG_UNROLL * GT_THREADS) {
            int row[GT_LONG_UNROLL];
            unsigned rel[GT_LONG_UNROLL];
#pragma unroll
            for (int u = 0; u < GT_LONG_UNROLL; ++u) {
                const int i = i0 + u * GT_THREADS;
                row[u] = i < len ? p.post_row[lo + i] : -1;
            }
#pragma unroll
            for (int u = 0; u < GT_LONG_UNROLL; ++u)
                rel[u] = row[u] >= 0 ? (unsigned)(p.group[row[u]] - p.g0) : ~0u;
#pragma unroll
            for (int u = 0; u < GT_LONG_UNROLL; ++u)
                if (rel[u] < (unsigned)p.gw) atomicAdd(&all[rel[u]], 1u);
        }
        __syncthreads();
        if (tid < p.gw) {       // GT_GROUPS == GT_THREADS: one bin per thread
            const int fg = (int)all[tid];
            if (fg) {
                all[tid] = 0u;
                terms_emit(p, tid, fg, t0 + j, p.df[t0 + j]);
            }
        }
        __syncthreads();
    }
}
static_assert(GT_GROUPS == MMRAG_TERM_GROUP_WINDOW, "include/mmrag.h states the launch window");
static_assert(GT_GROUPS <= GT_THREADS, "the workgroup's sweep takes one bin per thread");
static_assert(GT_BLOCK_TERMS <= GT_THREADS, "one thread per term reads the block's list bounds");

// out_counts[g, j] = rows of group g holding out_terms[g, j] (0 on padding): one workgroup per output at a time
__global__ __launch_bounds__(GT_THREADS) void group_term_counts_kernel(const long long *__restrict__ term_off,
                                                                       const int *__restrict__ post_row,
                                                                       const int *__restrict__ group,
                                                                       const long long *__restrict__ out_terms,
                                                                       long long total, int top,
                                                                       int *__restrict__ out_counts) {
    __shared__ int wsum[GT_WAVES];
    const int tid = threadIdx.x;
    for (long long e = blockIdx.x; e < total; e += gridDim.x) {
        const long long t = out_terms[e];
        if (t < 0) {   // the same in every thread
            if (tid == 0) out_counts[e] = 0;
            continue;
        }
        const int g = (int)(e / top);
        const long long lo = term_off[t], hi = term_off[t + 1];
        int c = 0;
        for (long long i = lo + tid; i < hi; i += GT_THREADS) c += group[post_row[i]] == g;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
        if ((tid & 63) == 0) wsum[tid >> 6] = c;
        __syncthreads();
        if (tid == 0) {
            int sum = 0;
            for (int j = 0; j < GT_WAVES; ++j) sum += wsum[j];
            out_counts[e] = sum;
        }
        __syncthreads();   // wsum is rewritten by the next output
    }
}

int terms_window(int n_groups) { return n_groups < GT_GROUPS ? n_groups : GT_GROUPS; }

// candidate slots per group: no more than n_terms in whole 256s (with >= n_terms slots nothing can overflow)
long long terms_capacity(int n_terms, int top) {
    const long long c = candidate_capacity(top), nn = (long long)align_up((size_t)(n_terms > 0 ? n_terms : 1), 256);
    return c < nn ? c : nn;
}

CandWs terms_ws_layout(int n_groups, int n_terms, int top) {
    return candidate_ws_layout(terms_window(n_groups), terms_capacity(n_terms, top), n_terms > 0 ? n_terms : 1, false);
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

size_t mmrag_group_terms_workspace_bytes(int n_groups, int n_terms, int top) {
    if (n_groups < 1 || n_groups > MMRAG_MAX_TERM_GROUPS || n_terms < 0 || top < 1 || top > MMRAG_MAX_K_DEEP) return 0;
    return terms_ws_layout(n_groups, n_terms, top).total;
}

int mmrag_group_terms(const int64_t *term_off, const int32_t *post_row, const int32_t *df, int n_terms, int64_t n,
                      const int32_t *group, const int32_t *group_size, int n_groups, int64_t n_live,
                      const uint32_t *term_bits, int min_count, int top, float *out_scores, int64_t *out_terms,
                      int32_t *out_counts, void *workspace, size_t workspace_bytes, void *stream) {
    MMRAG_CHECK_ARG(n_groups >= 1 && n_groups <= MMRAG_MAX_TERM_GROUPS, "group_terms: n_groups=%d outside 1..%d",
                    n_groups, MMRAG_MAX_TERM_GROUPS);
    MMRAG_CHECK_ARG(top >= 1 && top <= MMRAG_MAX_K_DEEP, "group_terms: top=%d outside 1..%d", top, MMRAG_MAX_K_DEEP);
    MMRAG_CHECK_ARG(min_count >= 1, "group_terms: min_count must be at least 1 (got %d)", min_count);
    // (a walk steps past a list's end by less than two of its strides before it stops)
    MMRAG_CHECK_ARG(n >= 0 && n < (int64_t)INT_MAX - 2 * GT_LONG_UNROLL * GT_THREADS && n_terms >= 0 && n_live >= 0 &&
                        n_live <= n,
                    "group_terms: bad sizes n=%lld n_terms=%d n_live=%lld", (long long)n, n_terms, (long long)n_live);
    MMRAG_CHECK_ARG(term_off && post_row && df && group && group_size && out_scores && out_terms && out_counts,
                    "group_terms: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0 || n_live == 0 || n_terms == 0) {   // no pair can qualify
        MMRAG_CHECK_HIP(hipMemsetAsync(out_counts, 0, (size_t)n_groups * top * sizeof(int32_t), s));
        return candidate_fill_empty(out_scores, (long long *)out_terms, n_groups, top, s);
    }
    const CandWs wl = terms_ws_layout(n_groups, n_terms, top);
    if (!workspace || workspace_bytes < wl.total) {
        set_error("group_terms: workspace %zu bytes < required %zu", workspace_bytes, wl.total);
        return MMRAG_EWORKSPACE;
    }
    MMRAG_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "group_terms: workspace must be 16-byte aligned");
    TermsParams p = {};
    p.term_off = (const long long *)term_off;
    p.post_row = post_row;
    p.df = df;
    p.group = group;
    p.group_size = group_size;
    p.term_bits = term_bits;
    p.n_terms = n_terms;
    p.n_groups = n_groups;
    p.min_count = min_count;
    p.n_live = (float)n_live;
    const unsigned blocks = (unsigned)((n_terms + GT_BLOCK_TERMS - 1) / GT_BLOCK_TERMS);
    const auto count_into = [&](int g0, int gw, float *cand_s, int *cand_t, unsigned *counts, long long slots) -> int {
        TermsParams pw = p;
        pw.g0 = g0;
        pw.gw = gw;
        pw.cap = slots;
        pw.cnt = counts;
        pw.cand_s = cand_s;
        pw.cand_t = cand_t;
        group_terms_kernel<<<blocks, GT_THREADS, 0, s>>>(pw);
        MMRAG_CHECK_HIP(hipGetLastError());
        return MMRAG_OK;
    };
    const long long cap = terms_capacity(n_terms, top);
    // windows of GT_GROUPS groups over the same CSR, cut as for_scan_chunks cuts a batch into launches
    for (int g0 = 0; g0 < n_groups; g0 += GT_GROUPS) {
        const int gw = n_groups - g0 < GT_GROUPS ? n_groups - g0 : GT_GROUPS;
        const int st = candidate_select(
            "group_terms", gw, n_terms, cap, top, 0, out_scores + (size_t)g0 * top,
            (long long *)out_terms + (size_t)g0 * top, (char *)workspace, wl, s,
            [&](float *cand_s, int *cand_t, unsigned *counts, long long slots) {
                return count_into(g0, gw, cand_s, cand_t, counts, slots);
            },
            [&](int gi, float *cand_s, int *cand_t, unsigned *counts, long long slots) {
                return count_into(g0 + gi, 1, cand_s, cand_t, counts, slots);
            });
        if (st) return st;
    }
    const long long total = (long long)n_groups * top;
    group_term_counts_kernel<<<(unsigned)(total < GT_COUNT_GRID ? total : GT_COUNT_GRID), GT_THREADS, 0, s>>>(
        (const long long *)term_off, post_row, group, (const long long *)out_terms, total, top, out_counts);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

// The sizes at which the kernels above change path: groups per launch, term ids per workgroup, the longest list one wave
// takes alone and the workgroup's stride over a longer one.  The tests place their cases on the edges.  Exported for
// them, deliberately absent from include/mmrag.h.  Host code, no device needed.
int mmrag_internal_terms_limits(int *groups, int *block_terms, int *wave_limit, int *block_stride) {
    if (!groups || !block_terms || !wave_limit || !block_stride) return -1;
    *groups = GT_GROUPS;
    *block_terms = GT_BLOCK_TERMS;
    *wave_limit = GT_WAVE_LIMIT;
    *block_stride = GT_THREADS;
    return 0;
}

}  // extern "C"
