// Learned sparse expansion (SPLADE-style) on gfx950: the device half of multimodal_rag_amd/sparse.py between the MLM
// transform (encoder.hip, mmrag_sparse_expand_forward) and the forward log of the impact index (sparse_score.hip).
//
//   mmrag_sparse_pool     pooled[c][v] = max over the tokens t of chunk c of <tok_t, E_v>: the vocabulary projection of a
//                         masked-LM head and the per-chunk max in one kernel.  The [T, V] logits never exist.
//   mmrag_sparse_select   per chunk: w = log1p(relu(pooled + bias)), an 8-bit impact, the m terms of highest impact in
//                         ascending term id -- the forward-log form mmrag_lexical_csr_build takes.
//
// Pool.  pair_tile.h's body with a 128-row tile of the token plane as A and 128 decoder rows as B; the token plane is
// walked in PLAIN 128-row tiles (grid.x), whatever the chunks are, and a workgroup takes a run of vocabulary tiles
// (grid.y) through pair_tile_ring, the token tile fetched again for each (L2).  Short chunks therefore share A tiles:
// sixteen 8-token queries are one tile.  The epilogue is segmented by chunk piece (the rows of one chunk inside the
// tile): with acc[a][b][r] = <token wm*64 + 16a + 4 g4 + r, term wn*64 + 16b + c16> a lane holds 16 tokens of 4 terms,
// and the maximum over the piece's tokens goes
//     in-lane over a, r (tokens outside the piece masked by INDEX, never by value)
//  -> two cross-lane steps over g4 (lanes 16 and 32 apart)
//  -> one LDS step over wm (red[piece][wm][term]; SP_BATCH pieces per pair of barriers)
//  -> across the token tiles a chunk spans (at most five for 512 tokens): an integer atomicMax on the order-preserving
//     key of the float, into the output itself.
// A maximum does not depend on arrival order and every logit's bits depend on its two rows and dim alone (slab_step's
// fixed K order), so the output is a pure function of the inputs: the same bits for every grid, batch and packing.
// `pooled` holds keys between the memset (key 0 lies below every float's) and the finish kernel, which turns them into
// floats in place and writes -inf rows for chunks the kernel refuses.  Nothing of size T x V is written, no workspace,
// no host synchronisation.
//
// Bounds.  Token rows past T and decoder rows past V read as zero through the buffer descriptors and are excluded by
// index; every store is to pooled[c][v] with c < n_chunks and v < V checked at the store.  `cu` is read on the device
// with every index below n_chunks + 1: a malformed table gives wrong maxima, never an access outside the buffers.
#include "pair_tile.h"

#include <math.h>

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int SP_BATCH = 8;          // chunk pieces folded per pair of barriers
constexpr int SP_VRUN = 16;          // vocabulary tiles per workgroup at most
constexpr int SEL_T = 256;           // threads of a select workgroup
constexpr float NEG_INF_F = -__builtin_inff();

// order-preserving key of a float: a < b  <=>  key(a) < key(b) as unsigned; no float has key 0
__device__ __forceinline__ unsigned sp_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sp_unkey(unsigned k) {
    return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}

struct SpPoolParams {
    const char *tok;
    unsigned tok_rb;        // row pitch of the token plane in bytes
    long long T;
    const char *E;
    unsigned e_rb;          // row pitch of the decoder rows
    int V;
    int nk;                 // K-slabs that hold the dim columns
    const int *cu;
    int n_chunks;
    unsigned *keys;         // [n_chunks, V]: pooled, as keys
    int vt, vrun;           // vocabulary tiles, and how many of them a workgroup takes
};

__device__ __forceinline__ bool sp_chunk_ok(int s, int e, long long T) {
    return s >= 0 && e > s && e - s <= MMRAG_MAX_SPARSE_CHUNK_TOKENS && (long long)e <= T;
}

__global__ __launch_bounds__(256, 2) void sparse_pool_kernel(const SpPoolParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(PT_LDS + SP_BATCH * 2 * PT * 4 + 64 <= 80 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    __shared__ float red[SP_BATCH][2][PT];
    __shared__ int piece_chunk[SP_BATCH];

    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * PT;                 // < T: the grid has ceil(T / 128) tiles
    const int rows = (int)(p.T - r0 < PT ? p.T - r0 : PT);
    const int vt0 = blockIdx.y * p.vrun;
    const int nvt = p.vt - vt0 < p.vrun ? p.vt - vt0 : p.vrun;      // >= 1

    // the first chunk that ends past r0: the first i with cu[i + 1] > r0
    int c_first;
    {
        int lo = 0, hi = p.n_chunks;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((long long)p.cu[mid + 1] <= r0) lo = mid + 1;
            else hi = mid;
        }
        c_first = __builtin_amdgcn_readfirstlane(lo);
    }

    const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);
    const PairTileCtx c = pair_tile_ctx(tid, wave_id < 2 ? p.tok_rb : p.e_rb, smem);
    const int wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;
    const PairTileSrc a_src = {p.tok + (size_t)r0 * p.tok_rb, (unsigned)rows * p.tok_rb};
    const auto tile_src = [&](int j) {
        const int v0 = (vt0 + j) * PT;
        const int vrows = p.V - v0 < PT ? p.V - v0 : PT;
        const PairTileSrc b_src = {p.E + (size_t)v0 * p.e_rb, (unsigned)vrows * p.e_rb};
        return wave < 2 ? a_src : b_src;
    };

    const auto tile_done = [&](int j, const f32x4_t (&acc)[4][4]) {
        const int v0 = (vt0 + j) * PT;
        int ci = c_first;
        bool more = true;
        while (more) {
            // ---- up to SP_BATCH pieces: every wave folds its 64 x 64 quadrant, both halves of the tokens write
            int nb = 0;
            while (nb < SP_BATCH) {
                if (ci >= p.n_chunks) {
                    more = false;
                    break;
                }
                const int s = __builtin_amdgcn_readfirstlane(p.cu[ci]);
                if ((long long)s >= r0 + rows) {
                    more = false;
                    break;
                }
                const int e = __builtin_amdgcn_readfirstlane(p.cu[ci + 1]);
                const int lo = (long long)s > r0 ? (int)(s - r0) : 0;
                const int hi = (long long)e - r0 < rows ? (int)(e - r0) : rows;
                if (sp_chunk_ok(s, e, p.T) && hi > lo) {
                    float m[4] = {NEG_INF_F, NEG_INF_F, NEG_INF_F, NEG_INF_F};
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const int blk = wm * 64 + 16 * a;       // the 16 tokens of this MFMA block row
                        if (blk + 16 <= lo || blk >= hi) continue;
                        if (blk >= lo && blk + 16 <= hi) {
#pragma unroll
                            for (int b = 0; b < 4; ++b)
#pragma unroll
                                for (int r = 0; r < 4; ++r) m[b] = acc[a][b][r] > m[b] ? acc[a][b][r] : m[b];
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int row = blk + 4 * g4 + r;
                                const bool in = row >= lo && row < hi;
#pragma unroll
                                for (int b = 0; b < 4; ++b) {
                                    const float v = in ? acc[a][b][r] : NEG_INF_F;
                                    m[b] = v > m[b] ? v : m[b];
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        float v = m[b];
                        const float o1 = __shfl_xor(v, 16);
                        v = o1 > v ? o1 : v;
                        const float o2 = __shfl_xor(v, 32);
                        v = o2 > v ? o2 : v;
                        if (g4 == 0) red[nb][wm][wn * 64 + 16 * b + c16] = v;
                    }
                    if (tid == 0) piece_chunk[nb] = ci;
                    ++nb;
                }
                ++ci;
            }
            if (nb == 0) break;      // uniform: nb and `more` come from scalar reads
            __syncthreads();
            for (int i = tid; i < nb * PT; i += 256) {
                const int pc = i >> 7, t = i & (PT - 1), v = v0 + t;
                if (v < p.V) {
                    const float x0 = red[pc][0][t], x1 = red[pc][1][t];
                    atomicMax(p.keys + (size_t)piece_chunk[pc] * p.V + v, sp_key(x1 > x0 ? x1 : x0));
                }
            }
            __syncthreads();         // red is rewritten by the next batch, or by the next tile
        }
    };
    // one ring per workgroup: no barrier after it
    pair_tile_ring<MMRAG_F16>(c, smem, p.nk, nvt, tile_src, tile_done);
#endif
}

// keys -> floats in place; a chunk the pool refuses (rows outside 0 .. T, length outside 1 .. 512) gets -inf
__global__ __launch_bounds__(256) void sparse_pool_finish_kernel(unsigned *__restrict__ keys, const int *__restrict__ cu,
                                                                 long long T, int V) {
    const int ch = blockIdx.x;
    const bool ok = sp_chunk_ok(cu[ch], cu[ch + 1], T);
    unsigned *row = keys + (size_t)ch * V;
    for (int v = blockIdx.y * 256 + threadIdx.x; v < V; v += gridDim.y * 256) {
        const unsigned k = row[v];
        const float f = ok && k != 0u ? sp_unkey(k) : NEG_INF_F;
        row[v] = __float_as_uint(f);
    }
}

// ---- select ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int sp_impact(float pooled, float bias, float scale) {
    const float w = log1pf(fmaxf(pooled + bias, 0.0f));
    const int q = (int)rintf(w * scale);
    return q > 255 ? 255 : q;
}

// One workgroup per chunk.  Pass 1: a histogram of the impacts >= 1 of the terms that are not skipped (256 bins, LDS).
// The cut: the lowest impact c with at least m terms at or above it (1 when fewer than m terms are positive); terms
// above the cut are all kept, of the terms AT the cut the `need` lowest ids.  Pass 2: the terms in ascending id, 256 at
// a time, kept terms written at (kept before) -- two prefix counts per step, wave ballots and one LDS step over the
// four waves -- so the pairs come out sorted by term id.
__global__ __launch_bounds__(SEL_T) void sparse_select_kernel(const float *__restrict__ pooled,
                                                              const float *__restrict__ bias,
                                                              const unsigned *__restrict__ skip, int V, float scale,
                                                              int m, int *__restrict__ out_cnt,
                                                              int *__restrict__ out_terms, int *__restrict__ out_imp) {
    __shared__ int hist[256];
    __shared__ int cut_s, need_s;
    __shared__ int wkeep[SEL_T / 64], wtie[SEL_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, ch = blockIdx.x;
    const float *row = pooled + (size_t)ch * V;
    const auto impact_of = [&](int v) -> int {
        if (skip != nullptr && ((skip[v >> 5] >> (v & 31)) & 1u)) return 0;
        return sp_impact(row[v], bias[v], scale);
    };
    hist[tid] = 0;
    __syncthreads();
    for (int v = tid; v < V; v += SEL_T) {
        const int q = impact_of(v);
        if (q >= 1) atomicAdd(&hist[q], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int above = 0, cut = 1, need = 0;
        for (int q = 255; q >= 1; --q) {
            if (above + hist[q] >= m) {
                cut = q;
                need = m - above;
                break;
            }
            above += hist[q];
            if (q == 1) need = hist[1];      // fewer than m positive terms: all of them (cut = 1)
        }
        cut_s = cut;
        need_s = need;
    }
    __syncthreads();
    const int cut = cut_s, need = need_s;
    int kept = 0, ties = 0;      // before this step: terms written, terms at the cut seen
    for (int base = 0; base < V; base += SEL_T) {
        const int v = base + tid;
        const int q = v < V ? impact_of(v) : 0;
        const bool tie = q == cut;
        const unsigned long long tm = __builtin_amdgcn_ballot_w64(tie);
        if (lane == 0) wtie[w] = __popcll(tm);
        __syncthreads();
        int tie_before = ties + __popcll(tm & ((1ull << lane) - 1ull)), tie_total = 0;
        for (int j = 0; j < SEL_T / 64; ++j) {
            if (j < w) tie_before += wtie[j];
            tie_total += wtie[j];
        }
        const bool keep = q > cut || (tie && tie_before < need);
        const unsigned long long km = __builtin_amdgcn_ballot_w64(keep);
        if (lane == 0) wkeep[w] = __popcll(km);
        __syncthreads();
        int at = kept + __popcll(km & ((1ull << lane) - 1ull)), keep_total = 0;
        for (int j = 0; j < SEL_T / 64; ++j) {
            if (j < w) at += wkeep[j];
            keep_total += wkeep[j];
        }
        if (keep && at < m) {
            out_terms[(size_t)ch * m + at] = v;
            out_imp[(size_t)ch * m + at] = q;
        }
        kept += keep_total;
        ties += tie_total;
        // wtie / wkeep are rewritten only after the next step's first barrier, which every read above precedes
    }
    for (int i = kept + tid; i < m; i += SEL_T) {      // kept <= m
        out_terms[(size_t)ch * m + i] = -1;
        out_imp[(size_t)ch * m + i] = 0;
    }
    if (tid == 0) out_cnt[ch] = kept;
}

}  // namespace

}  // namespace mmrag_impl
using namespace mmrag_impl;

extern "C" {

size_t mmrag_sparse_pool_workspace_bytes(int64_t T, int n_chunks, int V) {
    (void)T, (void)n_chunks, (void)V;
    return 0;      // the maxima are merged in `pooled` itself
}

// mmrag_sparse_pool with the run of vocabulary tiles a workgroup takes given (vrun > 0; 0: chosen from the grid as
// below): the bench that compares runs, and the tests that pin the output's independence of it.  Exported for them,
// deliberately absent from include/mmrag.h.
int mmrag_internal_sparse_pool_ex(const void *tok, int64_t T, int64_t tok_ld, const int32_t *cu, int n_chunks,
                                  const void *E, int V, int64_t e_ld, int dim, float *pooled, void *stream,
                                  int vrun_override) {
    MMRAG_CHECK_ARG(vrun_override >= 0, "sparse_pool: negative run of vocabulary tiles");
    MMRAG_CHECK_ARG(tok && cu && E && pooled, "sparse_pool: null pointer");
    MMRAG_CHECK_ARG(dim > 0 && dim % 64 == 0 && dim <= 1024,
                    "sparse_pool: dim must be a multiple of 64, at most 1024 (dim=%d)", dim);
    MMRAG_CHECK_ARG(V >= 1 && V <= MMRAG_MAX_SPARSE_VOCAB, "sparse_pool: V=%d outside 1..%d", V, MMRAG_MAX_SPARSE_VOCAB);
    MMRAG_CHECK_ARG(n_chunks >= 1 && n_chunks <= MMRAG_MAX_SPARSE_CHUNKS, "sparse_pool: n_chunks=%d outside 1..%d",
                    n_chunks, MMRAG_MAX_SPARSE_CHUNKS);
    MMRAG_CHECK_ARG(T >= 1 && T < (1LL << 31) - PT, "sparse_pool: T=%lld out of range", (long long)T);
    for (const int64_t w : {tok_ld, e_ld})
        if (int st = check_stored_rows("sparse_pool", "projected", "project", w, MMRAG_F16, dim)) return st;
    MMRAG_CHECK_ARG(((uintptr_t)tok % 16) == 0 && ((uintptr_t)E % 16) == 0 && ((uintptr_t)pooled % 4) == 0,
                    "sparse_pool: token and decoder rows must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    SpPoolParams p;
    p.tok = (const char *)tok;
    p.tok_rb = stored_row_bytes(tok_ld, MMRAG_F16);
    p.T = T;
    p.E = (const char *)E;
    p.e_rb = stored_row_bytes(e_ld, MMRAG_F16);
    p.V = V;
    p.nk = stored_k_slabs(dim, MMRAG_F16);
    p.cu = cu;
    p.n_chunks = n_chunks;
    p.keys = (unsigned *)pooled;
    p.vt = (V + PT - 1) / PT;
    const long long tt = (T + PT - 1) / PT;
    // a run of vocabulary tiles per workgroup, shortened until the grid has four workgroups per CU (the output's bits
    // do not depend on it)
    long long vrun = tt * p.vt / (4LL * num_cus());
    p.vrun = (int)(vrun < 1 ? 1 : (vrun > SP_VRUN ? SP_VRUN : vrun));
    if (vrun_override > 0) p.vrun = vrun_override < p.vt ? vrun_override : p.vt;
    MMRAG_CHECK_HIP(hipMemsetAsync(pooled, 0, (size_t)n_chunks * V * sizeof(float), s));
    hipLaunchKernelGGL(sparse_pool_kernel, dim3((unsigned)tt, (unsigned)((p.vt + p.vrun - 1) / p.vrun)), dim3(256), 0, s,
                       p);
    MMRAG_CHECK_HIP(hipGetLastError());
    const unsigned fy = (unsigned)((V + 1023) / 1024);
    hipLaunchKernelGGL(sparse_pool_finish_kernel, dim3((unsigned)n_chunks, fy), dim3(256), 0, s, p.keys, cu,
                       (long long)T, V);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

int mmrag_sparse_pool(const void *tok, int64_t T, int64_t tok_ld, const int32_t *cu, int n_chunks, const void *E, int V,
                      int64_t e_ld, int dim, float *pooled, void *workspace, size_t workspace_bytes, void *stream) {
    (void)workspace, (void)workspace_bytes;
    return mmrag_internal_sparse_pool_ex(tok, T, tok_ld, cu, n_chunks, E, V, e_ld, dim, pooled, stream, 0);
}

int mmrag_sparse_select(const float *pooled, const float *bias, const uint32_t *skip_bits, int n_chunks, int V,
                        float scale, int m, int32_t *out_cnt, int32_t *out_terms, int32_t *out_imp, void *stream) {
    MMRAG_CHECK_ARG(pooled && bias && out_cnt && out_terms && out_imp, "sparse_select: null pointer");
    MMRAG_CHECK_ARG(V >= 1 && V <= MMRAG_MAX_SPARSE_VOCAB, "sparse_select: V=%d outside 1..%d", V,
                    MMRAG_MAX_SPARSE_VOCAB);
    MMRAG_CHECK_ARG(n_chunks >= 1 && n_chunks <= MMRAG_MAX_SPARSE_CHUNKS, "sparse_select: n_chunks=%d outside 1..%d",
                    n_chunks, MMRAG_MAX_SPARSE_CHUNKS);
    MMRAG_CHECK_ARG(m >= 1 && m <= MMRAG_MAX_SPARSE_TERMS, "sparse_select: m=%d outside 1..%d", m,
                    MMRAG_MAX_SPARSE_TERMS);
    MMRAG_CHECK_ARG(scale > 0.0f && scale <= 1024.0f, "sparse_select: scale must be in (0, 1024] (scale=%g)",
                    (double)scale);
    hipLaunchKernelGGL(sparse_select_kernel, dim3((unsigned)n_chunks), dim3(SEL_T), 0, (hipStream_t)stream, pooled, bias,
                       (const unsigned *)skip_bits, V, scale, m, out_cnt, out_terms, out_imp);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

// The sizes at which the sparse kernels change path: rows per impact scoring workgroup, chunk pieces per pair of
// barriers and the longest run of vocabulary tiles in the pool, terms per step of the select, rows of the pair tile.
// The tests restate them to place their cases on the edges and compare.  Exported for them, deliberately absent from
// include/mmrag.h.  Host code, no device needed.
int mmrag_internal_sparse_limits(int *impact_rows, int *pool_batch, int *pool_vrun, int *select_terms, int *tile_rows) {
    if (!impact_rows || !pool_batch || !pool_vrun || !select_terms || !tile_rows) return -1;
    *impact_rows = impact_block_rows();
    *pool_batch = SP_BATCH;
    *pool_vrun = SP_VRUN;
    *select_terms = SEL_T;
    *tile_rows = PT;
    return 0;
}

}  // extern "C"
