// Answer citations: sentence-to-source attribution (include/mmrag.h mmrag_attribute).  For
// every sentence of an answer (a claim) and every source, the best-supporting evidence sentence of that source; then
// per claim the m best sources.
//
// One workgroup of 256 threads per unit (at most 128 claims, at most 4096 evidence rows).  The claims are the A tile
// of pair_tile.h's body and stay; the evidence moves through the ring in 128-row B tiles.  Both buffer descriptors end
// at the last row of their side, so rows past it read as zero whatever follows them in the plane, and they are dropped
// by INDEX in the epilogue (claim >= C, evidence >= E), as summarize.hip does.
//
// LDS: a 128 x 64 table of packed 64-bit keys, one per (claim, source), 64 KiB NEXT TO the ring's two stages (PT_LDS,
// 64 KiB): one workgroup has a CU's 160 KiB to itself, summarize.hip's layout.  A key is
//     (order-preserving bits of S_ij) << 32 | ~j
// so an unsigned maximum over the keys of one (claim, source) is the greatest score and, among equal scores, the
// LOWEST j.  A maximum does not depend on the order of its operands: whichever wave, lane or evidence tile gets to an
// entry first, the entry ends the same.  That is why an LDS atomic is allowed here (ds_max_u64; the read in front of
// it only skips an operand that cannot win: entries never decrease).  Key 0 is "no evidence": every real key has a
// non-zero low word (j <= 4095).  Scores are taken as acc + 0.0f, so a zero is +0 and orders as one value.
//
// S_ij is the tile body's, a function of the two rows and d alone, and nothing else is summed: a unit's bits do not
// depend on the batch, the grid or its place in the plane.
//
// The select: wave w owns claims w, w + 4, ...; lane s holds source s.  A lane's rank is the number of lanes whose
// (score bits, 63 - s) is greater -- distinct for sources with evidence -- and rank r < m writes slot r.
// No workspace, no global atomics, no host synchronisation, nothing written but the outputs: the call can be captured
// into a graph.
#include <limits.h>
#include <math.h>

#include "pair_tile.h"

namespace mmrag_impl {

namespace {

constexpr int ATT_C = MMRAG_MAX_CLAIMS;
constexpr int ATT_S = MMRAG_MAX_ATTR_SOURCES;
static_assert(ATT_C == PT, "the claims are one tile");
static_assert(ATT_S == 64, "a source per lane");
static_assert(MMRAG_MAX_EVIDENCE % PT == 0 && MMRAG_MAX_EVIDENCE <= (1 << 16), "whole tiles; ~j keeps a low word");

struct AttributeParams {
    const char *rows;
    unsigned rb;                // row pitch in bytes
    long long n_rows;
    int nk;                     // K-slabs that hold the d columns
    const int *claim_start, *claim_len, *ev_start, *ev_len, *ev_source;
    int n_sources, m, max_claims;
    int *out_src, *out_ev;
    float *out_score, *out_support;
};

// float32 bits -> unsigned in the order of the numbers (-inf lowest, +inf highest) and back
__device__ __forceinline__ unsigned att_ordered(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float att_score(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

template <int DT>
__global__ __launch_bounds__(256) void attribute_kernel(const AttributeParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(PT_LDS + ATT_C * ATT_S * 8 + 4 * 1024 <= 160 * 1024, "one workgroup per CU");
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    __shared__ unsigned long long key[ATT_C * ATT_S];

    const int u = blockIdx.x, tid = threadIdx.x, m = p.m, ns = p.n_sources;
    const float NEG_INF = -__builtin_inff();
    const size_t cite0 = (size_t)u * p.max_claims * m;
    // every thread reads the same table entries: the checks are uniform over the workgroup
    const int cs = p.claim_start[u], C = p.claim_len[u], es = p.ev_start[u], E = p.ev_len[u];
    const int most = p.max_claims < ATT_C ? p.max_claims : ATT_C;
    const bool ok = C >= 1 && C <= most && E >= 0 && E <= MMRAG_MAX_EVIDENCE && cs >= 0 && es >= 0 &&
                    (long long)cs + C <= p.n_rows && (long long)es + E <= p.n_rows;
    if (!ok) {
        for (int t = tid; t < p.max_claims * m; t += 256) {
            p.out_src[cite0 + t] = -1;
            p.out_ev[cite0 + t] = -1;
            p.out_score[cite0 + t] = t == 0 ? __builtin_nanf("") : NEG_INF;
        }
        return;
    }
    for (int t = tid; t < C * ATT_S; t += 256) key[t] = 0ull;
    __syncthreads();

    const PairTileCtx c = pair_tile_ctx(tid, p.rb, smem);
    const PairTileSrc claim_src = {p.rows + (size_t)cs * p.rb, (unsigned)C * p.rb};
    const char *ev_rows = p.rows + (size_t)es * p.rb;
    const int *ev_ord = p.ev_source + es;
    pair_tile_ring<DT>(
        c, smem, p.nk, (E + PT - 1) / PT,
        [&](int j) {
            if (c.wave < 2) return claim_src;
            const int left = E - j * PT;        // >= 1
            return PairTileSrc{ev_rows + (size_t)j * PT * p.rb, (unsigned)(left < PT ? left : PT) * p.rb};
        },
        [&](int j, const f32x4_t (&acc)[4][4]) {
            // acc[a][b][r] = <claim wm*64 + 16a + 4 g4 + r, evidence j*128 + wn*64 + 16b + c16>
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int e = j * PT + c.wn * 64 + 16 * b + c.c16;
                const int s = e < E ? ev_ord[e] : -1;
                if ((unsigned)s >= (unsigned)ns) continue;      // past E, or a row that counts for nothing
                const unsigned low = ~(unsigned)e;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = c.wm * 64 + 16 * a + 4 * c.g4 + r;
                        if (i >= C) continue;
                        const unsigned long long k =
                            ((unsigned long long)att_ordered(acc[a][b][r] + 0.0f) << 32) | low;
                        unsigned long long *at = &key[i * ATT_S + s];
                        if (k > *at) atomicMax(at, k);
                    }
            }
        });
    __syncthreads();

    // ---- per claim: the whole row of M, then the m best sources
    const int lane = c.lane;
    for (int i = c.wave; i < C; i += 4) {
        const unsigned long long k = lane < ns ? key[i * ATT_S + lane] : 0ull;
        const bool has = k != 0ull;
        const unsigned hi = (unsigned)(k >> 32);
        const float score = has ? att_score(hi) : NEG_INF;
        if (p.out_support != nullptr && lane < ns)
            p.out_support[((size_t)u * p.max_claims + i) * ns + lane] = score;
        // greater score first, then the lower source: distinct among the lanes that have evidence
        const unsigned long long sel = has ? ((unsigned long long)hi << 6) | (unsigned)(63 - lane) : 0ull;
        const unsigned sel_lo = (unsigned)sel, sel_hi = (unsigned)(sel >> 32);
        int rank = 0;
#pragma unroll
        for (int t = 0; t < ATT_S; ++t) {       // lane t's value as a scalar: no LDS round trip
            const unsigned long long other =
                ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)sel_hi, t) << 32) |
                (unsigned)__builtin_amdgcn_readlane((int)sel_lo, t);
            rank += other > sel ? 1 : 0;
        }
        const int found = __popcll(__builtin_amdgcn_ballot_w64(has));
        const size_t at = cite0 + (size_t)i * m;
        if (has && rank < m) {
            p.out_src[at + rank] = lane;
            p.out_ev[at + rank] = (int)~(unsigned)k;
            p.out_score[at + rank] = score;
        }
        if (lane >= found && lane < m) {
            p.out_src[at + lane] = -1;
            p.out_ev[at + lane] = -1;
            p.out_score[at + lane] = NEG_INF;
        }
    }
    for (int t = C * m + tid; t < p.max_claims * m; t += 256) {
        p.out_src[cite0 + t] = -1;
        p.out_ev[cite0 + t] = -1;
        p.out_score[cite0 + t] = NEG_INF;
    }
#endif
}

}  // namespace

}  // namespace mmrag_impl

extern "C" {

int mmrag_attribute(const void *rows, int64_t ld, int dtype, int d, int64_t n_rows, const int32_t *claim_start,
                    const int32_t *claim_len, const int32_t *ev_start, const int32_t *ev_len, int n_units,
                    const int32_t *ev_source, int n_sources, int m, int max_claims, int32_t *out_src, int32_t *out_ev,
                    float *out_score, float *out_support, void *stream) {
    using namespace mmrag_impl;
    MMRAG_CHECK_ARG(rows && claim_start && claim_len && ev_start && ev_len && ev_source && out_src && out_ev &&
                        out_score, "attribute: null pointer");
    if (int st = check_stored_rows("attribute", "attributed", "attribute against", ld, dtype, d)) return st;
    MMRAG_CHECK_ARG(n_rows >= 1 && n_rows < (1LL << 31), "attribute: n_rows=%lld outside 1..2^31 - 1",
                    (long long)n_rows);
    MMRAG_CHECK_ARG(n_units >= 1 && n_units <= (1 << 24), "attribute: n_units=%d outside 1..2^24", n_units);
    MMRAG_CHECK_ARG(n_sources >= 1 && n_sources <= MMRAG_MAX_ATTR_SOURCES, "attribute: n_sources=%d outside 1..%d",
                    n_sources, MMRAG_MAX_ATTR_SOURCES);
    MMRAG_CHECK_ARG(m >= 1 && m <= MMRAG_MAX_CITATIONS, "attribute: m=%d outside 1..%d", m, MMRAG_MAX_CITATIONS);
    MMRAG_CHECK_ARG(max_claims >= 1 && max_claims <= MMRAG_MAX_CLAIMS, "attribute: max_claims=%d outside 1..%d",
                    max_claims, MMRAG_MAX_CLAIMS);
    MMRAG_CHECK_ARG(((uintptr_t)rows % 16) == 0, "attribute: rows must be 16-byte aligned");
    AttributeParams p;
    p.rows = (const char *)rows;
    p.rb = stored_row_bytes(ld, dtype);
    p.n_rows = n_rows;
    p.nk = stored_k_slabs(d, dtype);
    p.claim_start = claim_start, p.claim_len = claim_len, p.ev_start = ev_start, p.ev_len = ev_len;
    p.ev_source = ev_source;
    p.n_sources = n_sources, p.m = m, p.max_claims = max_claims;
    p.out_src = out_src, p.out_ev = out_ev, p.out_score = out_score, p.out_support = out_support;
    mmrag::with_elem_type(dtype, [&](auto tag) {
        hipLaunchKernelGGL(attribute_kernel<decltype(tag)::value>, dim3((unsigned)n_units), dim3(256), 0,
                           (hipStream_t)stream, p);
    });
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // extern "C"
