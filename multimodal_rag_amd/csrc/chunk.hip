// Semantic chunking (include/mmrag.h mmrag_chunk_boundaries): the partition of a document's
// sentences into admissible chunks of greatest total gain, by dynamic programming over the band of all-pairs
// similarities at distance < 64.
//
// One workgroup of 256 threads per document, documents of any length.  The workgroup walks its document in steps of 64
// sentences: step t forms the self-pair tile of rows [64 t, 64 t + 128) of the document with pair_tile.h's body (A and
// B the same source; the buffer descriptor ends at the document's last row, so rows past it read as zero whatever
// follows them in the plane, and they are dropped by INDEX afterwards, as summarize.hip does) and writes its 64
// accumulators per lane into a 128 x 128 float32 matrix S in LDS.  That tile holds every pair at distance < 64 whose
// later member lies in [64 (t + 1), 64 (t + 2)), i.e. all of DP block t + 1 (chunk ends b in (64 (t + 1), 64 (t + 2)]);
// step 0 also serves block 0.  A document of n sentences takes max(1, ceil(n / 64) - 1) steps.
//
// A block k (b = 64 k + 1 + bb, bb < 64; candidate a = b - 1 - l, l < W) is three phases with a barrier after each:
//   A  thread a (128 of them) runs R_a(b) = sum_{j = a+1}^{b-1} (S_aj - tau) over ascending j in one accumulator and
//      leaves R_a(b) at band[bb][l];
//   B  thread bb (64) runs G(a, b) = G(a + 1, b) + R_a(b) over descending a, i.e. ascending l, in place;
//   C  wave 0 runs the block's sequential DP steps: lane l holds best[a] and the exact 64-bit cost sum of [a, b) in
//      registers (both move up one lane per step), v = best[a] + (G(a, b) - beta) where [a, b) is admissible, and an
//      xor butterfly takes the arg-max (v descending, a ascending).  Lane bb keeps step bb's result; the block's
//      results leave in one store per output.
// best[] of the last 64 positions lives in wave 0's registers from block to block (lane l: best[b - 1 - l]): the one
// wave that writes it is the one that reads it, so it needs no LDS slot and no barrier of its own.
//
// tau: `threshold`, or with auto_scale > 0 the document's own auto_scale * mean adjacent similarity.  That mean needs
// every S_{i,i+1} before the first DP step, so a document of more than one step walks its tiles twice: the first walk
// forms the same tiles and thread 0 adds S_{i,i+1} in ascending i to one accumulator (tile t owns i in [64 t, 64 t +
// 64), the last tile the rest).  A one-step document forms its tile once.  wave_row_dot (row_dot.h) is NOT used for
// it: its sum is 64 fmaf chains and a butterfly, not the tile body's order, and tau must be the mean of the S the
// gains are made of.
//
// LDS: the ring's two stages (PT_LDS, 64 KiB) + S (64 KiB) + the band (64 x 65 floats: the pad keeps phase A's stores,
// which run down a column, on distinct banks) + tau: one workgroup has a CU to itself.  Phase A reads S[a][a + 1 + s]
// (address 129 a + const: distinct banks), phases B and C read band[bb][l] along bb resp. l (pitch 65 resp. 1).
//
// ORDER OF EVERY FLOAT32 SUM is the definition's (mmrag.h), S_ij is the tile body's (a function of the two rows and d
// alone) and always taken with i < j as (A row i, B row j): a document's bits do not depend on the batch, the grid or
// its place in the plane.  No global atomics, no host synchronisation, nothing written but the outputs: the call can
// be captured into a graph.
#include <limits.h>
#include <math.h>

#include "pair_tile.h"

namespace mmrag_impl {

namespace {

constexpr int CH_W = MMRAG_MAX_CHUNK_SENTENCES;     // the band: candidates per chunk end, and the walk's step
constexpr int CH_PITCH = CH_W + 1;
static_assert(2 * CH_W == PT, "a tile is two steps");

struct ChunkParams {
    const char *rows;
    unsigned rb;                // row pitch in bytes
    long long n_rows;
    int nk;                     // K-slabs that hold the d columns
    const int *doc_start, *doc_len, *cost;
    int max_cost, W;
    float threshold, auto_scale, beta;
    int *out_prev;
    float *out_best, *out_tau, *out_score;
};

template <int DT>
__global__ __launch_bounds__(256) void chunk_boundaries_kernel(const ChunkParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(PT_LDS + PT * PT * 4 + CH_W * CH_PITCH * 4 + 1024 <= 160 * 1024, "one workgroup per CU");
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    __shared__ float S[PT * PT];
    __shared__ float band[CH_W * CH_PITCH];     // R_a(b), then G(a, b), at [bb][l]
    __shared__ float tau_s;

    const int u = blockIdx.x, tid = threadIdx.x;
    // every thread reads the same table entries: the checks are uniform over the workgroup
    const int start = p.doc_start[u], n = p.doc_len[u];
    if (!(n >= 1 && start >= 0 && (long long)start + n <= p.n_rows)) {
        if (tid == 0) p.out_score[u] = __builtin_nanf("");
        return;
    }
    const int blocks = (n - 1) / CH_W + 1;              // DP blocks
    const int steps = blocks > 1 ? blocks - 1 : 1;      // tiles

    const PairTileCtx c = pair_tile_ctx(tid, p.rb, smem);
    int have = -1;      // the tile S holds
    // S <- the self-pair tile of rows [64 t, 64 t + 128) of the document; ends with a barrier
    auto form_tile = [&](int t) {
        if (have == t) return;
        have = t;
        const int left = n - CH_W * t;      // >= 1
        const PairTileSrc src = {p.rows + ((size_t)start + (size_t)CH_W * t) * p.rb,
                                 (unsigned)(left < PT ? left : PT) * p.rb};
        pair_tile_ring<DT>(
            c, smem, p.nk, 1, [&](int) { return src; },
            [&](int, const f32x4_t (&acc)[4][4]) {
                // acc[a][b][r] = <row wm*64 + 16a + 4 g4 + r, row wn*64 + 16b + c16>
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            S[(c.wm * 64 + 16 * a + 4 * c.g4 + r) * PT + c.wn * 64 + 16 * b + c.c16] = acc[a][b][r];
            });
        __syncthreads();
    };

    // ---- tau
    float tau = p.threshold;
    if (p.auto_scale > 0.0f) {
        tau = 0.0f;
        if (n >= 2) {
            float sum = 0.0f;
            for (int t = 0; t < steps; ++t) {
                form_tile(t);
                if (tid == 0) {
                    const int row0 = CH_W * t, hi = t == steps - 1 ? n - 1 : row0 + CH_W;
                    for (int i = row0; i < hi; ++i) sum += S[(i - row0) * PT + (i - row0) + 1];
                }
                if (t + 1 < steps) __syncthreads();     // S is overwritten next
            }
            if (tid == 0) tau_s = __fmul_rn(p.auto_scale, __fdiv_rn(sum, (float)(n - 1)));
            __syncthreads();
            tau = tau_s;
        }
    }
    if (tid == 0) p.out_tau[u] = tau;

    // ---- the walk
    const int lane = c.lane, W = p.W;
    float best = 0.0f;          // wave 0, lane l: best[b - 1 - l] of the step at hand (lane 0 starts as best[0] = 0)
    long long csum = 0;         // wave 0, lane l: cost of [b - 1 - l, b)
    auto dp_block = [&](int k, int row0) {
        const int jlo = CH_W * k, jhi = n - 1 < jlo + CH_W - 1 ? n - 1 : jlo + CH_W - 1;    // the block's later members
        // A: thread a, sentence row0 + a
        if (tid < PT) {
            const int a = row0 + tid;
            int last = a + W - 1 < jhi ? a + W - 1 : jhi;
            if (a < n && last >= jlo) {
                float r = 0.0f;
                for (int j = a + 1; j <= last; ++j) {
                    r += __fsub_rn(S[tid * PT + (j - row0)], tau);
                    if (j >= jlo) band[(j - jlo) * CH_PITCH + (j - a)] = r;
                }
            }
        }
        __syncthreads();
        // B: thread bb, chunk end b = jlo + 1 + bb
        if (tid < CH_W && jlo + tid <= jhi) {
            const int b = jlo + 1 + tid;
            const int lmax = (W < b ? W : b) - 1;
            float g = 0.0f;
            band[tid * CH_PITCH] = g;
            for (int l = 1; l <= lmax; ++l) {
                g += band[tid * CH_PITCH + l];
                band[tid * CH_PITCH + l] = g;
            }
        }
        __syncthreads();
        // C: wave 0
        if (c.wave == 0) {
            const int nb = jhi - jlo + 1;
            const int cl = lane < nb ? p.cost[(size_t)start + jlo + lane] : 0;
            int my_prev = 0;
            float my_best = 0.0f;
            for (int bb = 0; bb < nb; ++bb) {
                const int b = jlo + 1 + bb;
                const long long up = __shfl_up(csum, 1);
                csum = (lane == 0 ? 0ll : up) + (long long)__shfl(cl, bb);
                const int a = b - 1 - lane;
                float v = -__builtin_inff();
                int arg = INT_MAX;
                if (a >= 0 && lane < W && (lane == 0 || csum <= (long long)p.max_cost)) {
                    v = __fadd_rn(best, __fsub_rn(band[bb * CH_PITCH + lane], p.beta));
                    arg = a;
                }
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) {
                    const float ov = __shfl_xor(v, m);
                    const int oa = __shfl_xor(arg, m);
                    if (ov > v || (ov == v && oa < arg)) {
                        v = ov;
                        arg = oa;
                    }
                }
                v = __shfl(v, 0);       // lane 0's candidate is always admissible: arg is a position
                arg = __shfl(arg, 0);
                if (lane == bb) {
                    my_prev = arg;
                    my_best = v;
                }
                const float upb = __shfl_up(best, 1);
                best = lane == 0 ? v : upb;
            }
            if (lane < nb) {
                p.out_prev[(size_t)start + jlo + lane] = my_prev;
                p.out_best[(size_t)start + jlo + lane] = my_best;
                if (jlo + lane == n - 1) p.out_score[u] = my_best;
            }
        }
        __syncthreads();        // the band, and then S, are written again
    };
    for (int t = 0; t < steps; ++t) {
        form_tile(t);
        if (t == 0) dp_block(0, 0);
        if (t + 1 < blocks) dp_block(t + 1, CH_W * t);
    }
#endif
}

}  // namespace

}  // namespace mmrag_impl

extern "C" {

int mmrag_chunk_boundaries(const void *rows, int64_t ld, int dtype, int d, int64_t n_rows, const int32_t *doc_start,
                           const int32_t *doc_len, int n_docs, const int32_t *cost, int32_t max_cost,
                           int max_sentences, float threshold, float auto_scale, float penalty, int32_t *out_prev,
                           float *out_best, float *out_tau, float *out_score, void *stream) {
    using namespace mmrag_impl;
    MMRAG_CHECK_ARG(rows && doc_start && doc_len && cost && out_prev && out_best && out_tau && out_score,
                    "chunk_boundaries: null pointer");
    MMRAG_CHECK_ARG(dtype != MMRAG_F8E4M3, "chunk_boundaries: float8_e4m3 rows are not segmented; pass the rows in a "
                    "full-precision dtype");
    if (int st = check_stored_rows("chunk_boundaries", "segmented", "segment", ld, dtype, d)) return st;
    MMRAG_CHECK_ARG(n_rows >= 1 && n_rows < (1LL << 31), "chunk_boundaries: n_rows=%lld outside 1..2^31 - 1",
                    (long long)n_rows);
    MMRAG_CHECK_ARG(n_docs >= 1 && n_docs <= (1 << 24), "chunk_boundaries: n_docs=%d outside 1..2^24", n_docs);
    MMRAG_CHECK_ARG(max_cost >= 1, "chunk_boundaries: max_cost=%d must be >= 1", (int)max_cost);
    MMRAG_CHECK_ARG(max_sentences >= 1 && max_sentences <= MMRAG_MAX_CHUNK_SENTENCES,
                    "chunk_boundaries: max_sentences=%d outside 1..%d", max_sentences, MMRAG_MAX_CHUNK_SENTENCES);
    MMRAG_CHECK_ARG(isfinite(threshold), "chunk_boundaries: threshold=%g must be finite", (double)threshold);
    MMRAG_CHECK_ARG(auto_scale >= 0.0f && auto_scale < INFINITY,
                    "chunk_boundaries: auto_scale=%g must be finite and >= 0", (double)auto_scale);
    MMRAG_CHECK_ARG(penalty >= 0.0f && penalty < INFINITY, "chunk_boundaries: penalty=%g must be finite and >= 0",
                    (double)penalty);
    MMRAG_CHECK_ARG(((uintptr_t)rows % 16) == 0, "chunk_boundaries: rows must be 16-byte aligned");
    ChunkParams p;
    p.rows = (const char *)rows;
    p.rb = stored_row_bytes(ld, dtype);
    p.n_rows = n_rows;
    p.nk = stored_k_slabs(d, dtype);
    p.doc_start = doc_start, p.doc_len = doc_len, p.cost = cost;
    p.max_cost = max_cost, p.W = max_sentences;
    p.threshold = threshold, p.auto_scale = auto_scale, p.beta = penalty;
    p.out_prev = out_prev, p.out_best = out_best, p.out_tau = out_tau, p.out_score = out_score;
    mmrag::with_elem_type(dtype, [&](auto tag) {
        hipLaunchKernelGGL(chunk_boundaries_kernel<decltype(tag)::value>, dim3((unsigned)n_docs), dim3(256), 0,
                           (hipStream_t)stream, p);
    });
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // extern "C"
