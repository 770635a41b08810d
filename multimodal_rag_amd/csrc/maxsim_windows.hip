// Windowed MaxSim of (query, passage) pairs: which contiguous window of a passage keeps the most of the pair's MaxSim
// (include/mmrag.h mmrag_maxsim_windows).
//
// One workgroup per pair, the ring of maxsim.hip's maxsim_kernel: the query's tokens are the A tile, the passage is
// walked in 128-token B tiles, buffer descriptors per SEQUENCE.  What differs is the epilogue.  A 16 x 16 MFMA output
// tile holds 16 passage columns of one row across the 16 lanes `lane & 15`, one DPP row: after a passage tile's last
// slab the four registers of a row are folded over that DPP row (columns j >= d_len set to -inf by INDEX first), each
// quad of lanes ending up with one of the four blocks, and one lane per quad writes the block maximum bm[row][block]
// into a 128 x 32 float32 LDS table (16 KiB beside the 64 KiB ring).
// A maximum is order-free, so nothing here depends on which lane or wave came first.
//
// Tail, behind a barrier (the ring's LDS is free then and holds every temporary):
//   1. thread i < 128 reads row i of bm, forms the row's full maximum (out_sum's addend) and the maxima of runs of
//      2^k blocks by doubling, 2^k the largest power of two <= the window width; a window's maximum for row i is the
//      max of two such runs: rowmax[s][i] for the valid s (all 256 threads, behind a barrier), values scaled where
//      they leave the accumulator domain;
//   2. one thread per window s adds rowmax[s][0 .. q_len) in ascending i from 0.0f, one more adds the full maxima:
//      maxsim_kernel's sum, same addends, same order, same bits;
//   3. every thread picks the lowest s of the largest sum; thread i < q_len finds the lowest block of that window that
//      attains row i's window maximum; min and max over i by wave shuffles and two LDS slots.
#include <math.h>

#include "f8_codec.h"
#include "pair_tile.h"

namespace mmrag_impl {

constexpr int MW_BLOCK = MMRAG_LATE_WINDOW_TOKENS;     // passage tokens per block
constexpr int MW_NB = MMRAG_MAX_LATE_WINDOWS;          // blocks of the longest passage = window slots
static_assert(MW_BLOCK == 16, "a block is the 16 columns of one MFMA output tile");
static_assert(MW_NB * MW_BLOCK == MMRAG_MAX_LATE_DOC_TOKENS && MW_NB == 32, "32 blocks cover the longest passage");

struct MaxSimWindowsParams {
    const char *q_tok, *d_tok;
    unsigned q_rb, d_rb;            // row pitch in bytes
    long long q_rows, d_rows;       // rows the two buffers hold
    int nk;                         // K-slabs that hold the dim columns
    const int *q_start, *q_len, *d_start, *d_len;
    int n_q, n_d;                   // entries of the two sequence tables
    const int *pair_q, *pair_d;
    int w;                          // window width in blocks, 1..32
    float *out_sum, *out_win;
    int *out_best;
};

// Where blocks 4 c .. 4 c + 3 of row `row` live in a 128 x 32 float table (float index): the row's eight 16-byte
// chunks are permuted by the row, so the threads of a wave, which read the same chunk of consecutive rows, spread
// over the banks
__device__ __forceinline__ int mw_chunk(int row, int c) { return row * MW_NB + ((c ^ (row >> 1)) & 7) * 4; }
__device__ __forceinline__ int mw_at(int row, int g) { return mw_chunk(row, g >> 2) + (g & 3); }

// max(a, b) of two numbers as ONE instruction: the median of (a, b, top), top = +inf.  fmaxf would first quiet a
// signalling NaN in each operand (a v_max of the value with itself), which triples a fold step; similarities are
// numbers.  `top` comes from mw_top(): a constant the compiler can see would turn the median back into fmaxf.
__device__ __forceinline__ float mw_max(float a, float b, float top) { return __builtin_amdgcn_fmed3f(a, b, top); }
__device__ __forceinline__ float mw_top() {
    float top = __builtin_inff();
    asm volatile("" : "+v"(top));
    return top;
}

// `v` as another lane of the caller's DPP row (16 lanes) holds it; CTRL: the DPP control
template <int CTRL>
__device__ __forceinline__ float mw_dpp(float v) {
    const int x = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(x, x, CTRL, 0xf, 0xf, false));
}
constexpr int MW_XOR1 = 0xb1, MW_XOR2 = 0x4e;       // quad_perm [1, 0, 3, 2] and [2, 3, 0, 1]
constexpr int MW_HALF_MIRROR = 0x141;               // lane i <-> 7 - i of its half: the other quad of the half
constexpr int MW_ROR8 = 0x128;                      // row_ror:8, lane i <-> i ^ 8

// m[b] = one row's value at column c16 of blocks b = 0 .. 3 (the 16 lanes of a DPP row are a block's 16 columns).
// Returns, in every lane, the maximum over the 16 lanes of block c16 >> 2: the fold hands each quad of lanes one block.
// Lanes i and i ^ 8 first split the blocks (the lower half keeps 0, 1 and receives the partner's, the upper 2, 3), the
// two quads of a half then split the remaining two, and each quad folds its own block: 5 lane exchanges where four
// separate folds take 16.
__device__ __forceinline__ float mw_fold_blocks(const f32x4_t m, bool hi8, bool hi4, float top) {
    const float k0 = mw_max(hi8 ? m[2] : m[0], mw_dpp<MW_ROR8>(hi8 ? m[0] : m[2]), top);
    const float k1 = mw_max(hi8 ? m[3] : m[1], mw_dpp<MW_ROR8>(hi8 ? m[1] : m[3]), top);
    float v = mw_max(hi4 ? k1 : k0, mw_dpp<MW_HALF_MIRROR>(hi4 ? k0 : k1), top);
    v = mw_max(v, mw_dpp<MW_XOR1>(v), top);
    return mw_max(v, mw_dpp<MW_XOR2>(v), top);
}

template <int DT>
__global__ __launch_bounds__(256, 2) void maxsim_windows_kernel(const MaxSimWindowsParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(PT == MMRAG_MAX_LATE_QUERY_TOKENS, "the query is one A tile");
    static_assert(PT_LDS + PT * MW_NB * 4 <= 80 * 1024, "two workgroups per CU");
    static_assert((PT * MW_NB + (MW_NB + 1) * PT + MW_NB + 4) * 4 <= PT_LDS, "the tail's temporaries fit the ring");
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    __shared__ __attribute__((aligned(16))) float bm[PT * MW_NB];

    const int pair = blockIdx.x;
    const float NEG_INF = -__builtin_inff();
    // every thread reads the same table entries: the checks below are uniform over the workgroup
    const int pq = p.pair_q[pair], pd = p.pair_d[pair];
    bool ok = pq >= 0 && pq < p.n_q && pd >= 0 && pd < p.n_d;
    int qs = 0, ql = 0, ds = 0, dl = 0;
    if (ok) {
        qs = p.q_start[pq], ql = p.q_len[pq], ds = p.d_start[pd], dl = p.d_len[pd];
        ok = ql >= 1 && ql <= MMRAG_MAX_LATE_QUERY_TOKENS && dl >= 1 && dl <= MMRAG_MAX_LATE_DOC_TOKENS && qs >= 0 &&
             ds >= 0 && (long long)qs + ql <= p.q_rows && (long long)ds + dl <= p.d_rows;
    }
    if (!ok) {
        if (threadIdx.x == 0) p.out_sum[pair] = __builtin_nanf("");
        if (threadIdx.x < 3) p.out_best[(size_t)pair * 3 + threadIdx.x] = -1;
        return;
    }

    const int wave_id = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const PairTileCtx c = pair_tile_ctx(threadIdx.x, wave_id < 2 ? p.q_rb : p.d_rb, smem);
    const int wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;
    const int nct = (dl + PT - 1) / PT;
    const PairTileSrc q_src = {p.q_tok + (size_t)qs * p.q_rb, (unsigned)ql * p.q_rb};
    const char *const d_base = p.d_tok + (size_t)ds * p.d_rb;
    const float top = mw_top();

    pair_tile_ring<DT>(
        c, smem, p.nk, nct,
        [&](int ct) {      // (the query tile, passage tile ct): the B side is the one that moves
            const int d_left = dl - ct * PT;
            const PairTileSrc d_src = {d_base + (size_t)ct * PT * p.d_rb, (unsigned)(d_left < PT ? d_left : PT) * p.d_rb};
            return wave < 2 ? q_src : d_src;
        },
        [&](int ct, const f32x4_t (&acc)[4][4]) {
            // ---- acc[a][b][r] = <query row wm*64 + 16a + 4 g4 + r, passage token ct * 128 + wn*64 + 16b + c16>:
            // the 16 lanes c16 of a register are block ct * 8 + wn * 4 + b of that row
            const int col0 = ct * PT + wn * 64 + c16;
            const bool ragged = (ct + 1) * PT > dl;     // uniform: only the last passage tile can hold columns >= d_len
            const bool hi8 = (c16 & 8) != 0, hi4 = (c16 & 4) != 0;
            const int blk = ct * 8 + wn * 4 + (c16 >> 2);       // the block this lane's quad ends up with
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    f32x4_t m;
#pragma unroll
                    for (int b = 0; b < 4; ++b) m[b] = ragged && col0 + 16 * b >= dl ? NEG_INF : acc[a][b][r];
                    const float v = mw_fold_blocks(m, hi8, hi4, top);
                    if ((c16 & 3) == 0) bm[mw_at(wm * 64 + 16 * a + 4 * g4 + r, blk)] = v;
                }
        });
    __syncthreads();        // bm is whole, the ring's LDS is free

    // ---- the tail's temporaries, in the ring's LDS
    float *const runs = (float *)smem;                 // [128][32] as bm: maxima of runs of `run` blocks
    float *const rowmax = runs + PT * MW_NB;           // [33][128]: window s < 32, slot 32 the whole passage
    float *const win = rowmax + (MW_NB + 1) * PT;      // [32]
    int *const span = (int *)(win + MW_NB);            // [2][2]: (first, last) of waves 0 and 1

    const int t = threadIdx.x;
    const int nb = (dl + MW_BLOCK - 1) / MW_BLOCK;     // 1..32
    const int w = p.w < nb ? p.w : nb;                 // every window is w blocks wide: a clipped one is the only one
    const int ns = nb - w + 1;                         // windows
    int lg = 0;
    while ((2 << lg) <= w) ++lg;
    const int run = 1 << lg;                           // the largest power of two <= w
    if (t < PT) {
        float x[MW_NB];
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) {
            const f32x4_t v = *(const f32x4_t *)&bm[mw_chunk(t, ch)];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[4 * ch + e] = 4 * ch + e < nb ? v[e] : NEG_INF;   // tiles not walked: by index
        }
        float full = x[0];
#pragma unroll
        for (int g = 1; g < MW_NB; ++g) full = fmaxf(full, x[g]);
        rowmax[MW_NB * PT + t] = full * PT_ACC_SCALE<DT>;
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (k < lg) {       // uniform.  Ascending g reads x[g + step] before this level overwrites it
#pragma unroll
                for (int g = 0; g < MW_NB; ++g) x[g] = fmaxf(x[g], g + (1 << k) < MW_NB ? x[g + (1 << k)] : NEG_INF);
            }
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) {
            f32x4_t v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = x[4 * ch + e];
            *(f32x4_t *)&runs[mw_chunk(t, ch)] = v;
        }
    }
    __syncthreads();
    for (int s = t >> 7, i = t & (PT - 1); s < ns; s += 2)
        rowmax[s * PT + i] = fmaxf(runs[mw_at(i, s)], runs[mw_at(i, s + w - run)]) * PT_ACC_SCALE<DT>;
    __syncthreads();

    // ---- the sums: summer s = lane s >> 2 of wave s & 3, slot 32 the whole passage
    {
        const int s = (t & 63) * 4 + (t >> 6);
        if (s < ns || s == MW_NB) {
            const float *src = rowmax + s * PT;
            float sum = 0.0f;
            for (int i = 0; i < ql; ++i) sum += src[i];      // ascending i: the sum's bits are defined
            if (s == MW_NB) p.out_sum[pair] = sum;
            else {
                win[s] = sum;
                p.out_win[(size_t)pair * MW_NB + s] = sum;
            }
        } else if (s < MW_NB)
            p.out_win[(size_t)pair * MW_NB + s] = NEG_INF;
    }
    __syncthreads();

    // ---- the best window (every thread, the same reads), then its tight span
    int start = 0;
    float most = win[0];
    for (int s = 1; s < ns; ++s) {
        const float v = win[s];
        if (v > most) most = v, start = s;     // strictly greater: the lowest s of the largest sum
    }
    int first = MW_NB, last = -1;
    if (t < ql) {
        float m = bm[mw_at(t, start)];
        int arg = start;
        for (int g = start + 1; g < start + w; ++g) {
            const float v = bm[mw_at(t, g)];
            if (v > m) m = v, arg = g;      // strictly greater: the lowest block of the maximum
        }
        first = last = arg;
    }
    if (wave < 2) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int of = __shfl_xor(first, m), ol = __shfl_xor(last, m);
            first = of < first ? of : first;
            last = ol > last ? ol : last;
        }
        if (c.lane == 0) span[2 * wave] = first, span[2 * wave + 1] = last;
    }
    __syncthreads();
    if (t == 0) {
        const int f0 = span[0], f1 = span[2], l0 = span[1], l1 = span[3];
        p.out_best[(size_t)pair * 3 + 0] = start;
        p.out_best[(size_t)pair * 3 + 1] = f0 < f1 ? f0 : f1;
        p.out_best[(size_t)pair * 3 + 2] = l0 > l1 ? l0 : l1;
    }
#endif
}

template <int DT>
static int maxsim_windows_impl(const char *who, const void *q_tok, int64_t q_rows, int64_t q_ld, const void *d_tok,
                               int64_t d_rows, int64_t d_ld, int dim, const int32_t *q_start, const int32_t *q_len,
                               int n_q, const int32_t *d_start, const int32_t *d_len, int n_d, const int32_t *pair_q,
                               const int32_t *pair_d, int P, int window_blocks, float *out_sum, float *out_win,
                               int32_t *out_best, void *stream) {
    MMRAG_CHECK_ARG(q_tok && d_tok && q_start && q_len && d_start && d_len && pair_q && pair_d && out_sum && out_win &&
                        out_best, "%s: null pointer", who);
    MMRAG_CHECK_ARG(window_blocks >= 1 && window_blocks <= MMRAG_MAX_LATE_WINDOWS,
                    "%s: window_blocks=%d outside 1..%d", who, window_blocks, MMRAG_MAX_LATE_WINDOWS);
    MMRAG_CHECK_ARG(dim > 0 && dim % 64 == 0 && dim <= 1024,
                    "%s: dim must be a multiple of 64, at most 1024 (dim=%d)", who, dim);
    for (const int64_t ld : {q_ld, d_ld}) {
        const int st = DT == MMRAG_F8E4M3 ? check_code_rows(who, ld, dim)
                                          : check_stored_rows(who, "scored", "score", ld, DT, dim);
        if (st != MMRAG_OK) return st;
    }
    MMRAG_CHECK_ARG(P >= 1 && P <= 65535, "%s: P=%d outside 1..65535", who, P);
    MMRAG_CHECK_ARG(n_q >= 1 && n_d >= 1 && q_rows >= 1 && d_rows >= 1 && q_rows < (1LL << 31) && d_rows < (1LL << 31),
                    "%s: need at least one sequence and one row on each side, fewer than 2^31 rows "
                    "(n_q=%d n_d=%d q_rows=%lld d_rows=%lld)", who, n_q, n_d, (long long)q_rows, (long long)d_rows);
    MMRAG_CHECK_ARG(((uintptr_t)q_tok % 16) == 0 && ((uintptr_t)d_tok % 16) == 0,
                    "%s: token rows must be 16-byte aligned", who);
    MaxSimWindowsParams p;
    p.q_tok = (const char *)q_tok, p.d_tok = (const char *)d_tok;
    p.q_rb = stored_row_bytes(q_ld, DT), p.d_rb = stored_row_bytes(d_ld, DT);
    p.q_rows = q_rows, p.d_rows = d_rows;
    p.nk = stored_k_slabs(dim, DT);
    p.q_start = q_start, p.q_len = q_len, p.d_start = d_start, p.d_len = d_len;
    p.n_q = n_q, p.n_d = n_d;
    p.pair_q = pair_q, p.pair_d = pair_d;
    p.w = window_blocks;
    p.out_sum = out_sum, p.out_win = out_win, p.out_best = out_best;
    hipLaunchKernelGGL(maxsim_windows_kernel<DT>, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // namespace mmrag_impl

extern "C" {

int mmrag_maxsim_windows(const void *q_tok, int64_t q_rows, int64_t q_ld, const void *d_tok, int64_t d_rows,
                         int64_t d_ld, int dim, const int32_t *q_start, const int32_t *q_len, int n_q,
                         const int32_t *d_start, const int32_t *d_len, int n_d, const int32_t *pair_q,
                         const int32_t *pair_d, int P, int window_blocks, float *out_sum, float *out_win,
                         int32_t *out_best, void *stream) {
    return mmrag_impl::maxsim_windows_impl<MMRAG_F16>("maxsim_windows", q_tok, q_rows, q_ld, d_tok, d_rows, d_ld, dim,
                                                      q_start, q_len, n_q, d_start, d_len, n_d, pair_q, pair_d, P,
                                                      window_blocks, out_sum, out_win, out_best, stream);
}

int mmrag_maxsim_windows_f8(const void *q_codes, int64_t q_rows, int64_t q_ld, const void *d_codes, int64_t d_rows,
                            int64_t d_ld, int dim, const int32_t *q_start, const int32_t *q_len, int n_q,
                            const int32_t *d_start, const int32_t *d_len, int n_d, const int32_t *pair_q,
                            const int32_t *pair_d, int P, int window_blocks, float *out_sum, float *out_win,
                            int32_t *out_best, void *stream) {
    return mmrag_impl::maxsim_windows_impl<MMRAG_F8E4M3>("maxsim_windows_f8", q_codes, q_rows, q_ld, d_codes, d_rows,
                                                         d_ld, dim, q_start, q_len, n_q, d_start, d_len, n_d, pair_q,
                                                         pair_d, P, window_blocks, out_sum, out_win, out_best, stream);
}

}  // extern "C"
