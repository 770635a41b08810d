// Topic clustering (spherical k-means over the stored unit rows): the two device steps of a Lloyd iteration
// (include/mmrag.h mmrag_kmeans_assign, mmrag_cluster_sums).
//
// mmrag_kmeans_assign: X . C^T with an arg-max epilogue, the [n, k] scores never written.  The tile body (LDS ring, DMA
// split, MFMA fragments, K order) is pair_tile.h's, the one the similarity join runs, with a 128-row tile as A and a
// 128-centroid tile as B; rows past n and centroids past k read as zero through the buffer descriptor.
// Workgroups are persistent over row tiles.  Inside a row tile the ring runs over ALL (centroid tile, K-slab) items
// without draining between centroid tiles; the row tile's slabs are fetched again for each centroid tile (L2).  After a
// centroid tile's last slab every lane folds its 64 accumulators into a running (best, arg) for its 16 rows: columns
// ascend with the centroid tile and inside the lane and only a strictly greater score replaces, so the lowest index
// wins a tie; columns >= k are set to -inf by INDEX first (a zero column can win a row whose scores are all negative).
// After the last centroid tile the 16 lanes that share rows are folded by an xor butterfly, the two waves that share
// rows through LDS, both with "greater score, else lower index"; 128 threads store the tile's results coalesced.
// The K order and the tile edges are fixed, so a row's outputs depend on the row, the centroids and d alone.
//
// mmrag_cluster_sums: one workgroup per (cluster, 128-byte column slab).  Thread (row lane j of 32, chunk c of 8) adds
// the 16-byte chunk c of the segment's members j, j + 32, j + 64, ... in that order; the 32 partial sums of a column
// are added by the fixed tree of strides 16, 8, 4, 2, 1.  No atomics, no workspace: a cluster's bits depend on its own
// member list alone.
#include <math.h>

#include "pair_tile.h"

namespace mmrag_impl {

struct AssignParams {
    const char *rows;
    const char *centroids;
    long long n;
    int k;
    unsigned row_bytes;     // ld * element size
    int nk;                 // K-slabs that hold the d logical columns
    int nct;                // centroid tiles
    const unsigned *alive;
    int *out_assign;
    float *out_score;
    long long T;            // row tiles
};

// (v, i) <- the better of (v, i) and (ov, oi): the greater score, else the lower index
__device__ inline void km_better(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

template <int DT>
__global__ __launch_bounds__(256, 2) void kmeans_assign_kernel(const AssignParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(PT_LDS + 2 * PT * 8 <= 80 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    __shared__ float red_v[2][PT];
    __shared__ int red_a[2][PT];

    const unsigned RB = p.row_bytes;
    const PairTileCtx c = pair_tile_ctx(threadIdx.x, RB, smem);
    const int wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;
    const float NEG_INF = -__builtin_inff();

    for (long long tile = blockIdx.x; tile < p.T; tile += gridDim.x) {
        const PairRowTile rt = pair_row_tile(tile, p.T, p.T, p.n);
        const long long row0 = rt.row0;
        const int in_tile = rt.rows;

        unsigned any = 1u;
        if (p.alive != nullptr) {
            any = 0u;
#pragma unroll
            for (int w = 0; w < PT / 32; ++w)
                if (32 * w < in_tile) any |= p.alive[(row0 >> 5) + w];
        }
        if (any == 0u) {
            // a tile of dead rows (uniform: the whole workgroup takes this path; no LDS is touched)
            if ((int)threadIdx.x < in_tile) {
                p.out_assign[row0 + threadIdx.x] = -1;
                p.out_score[row0 + threadIdx.x] = NEG_INF;
            }
            continue;
        }

        // running best of this lane's rows wm * 64 + 16 a + 4 g4 + r over the columns it has seen
        float bv[4][4];
        int ba[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bv[a][r] = NEG_INF;
                ba[a][r] = 0;
            }

        const PairTileSrc rows_src = {p.rows + (size_t)row0 * RB, (unsigned)in_tile * RB};
        pair_tile_ring<DT>(
            c, smem, p.nk, p.nct,
            [&](int ct) {      // (this row tile, centroid tile ct)
                const int c_left = p.k - ct * PT;
                const PairTileSrc c_src = {p.centroids + (size_t)ct * PT * RB, (unsigned)(c_left < PT ? c_left : PT) * RB};
                return wave < 2 ? rows_src : c_src;
            },
            [&](int ct, const f32x4_t (&acc)[4][4]) {
                // ---- acc[a][b][r] = <row wm*64 + 16a + 4 g4 + r, centroid ct * 128 + wn*64 + 16b + c16>
                const int col0 = ct * PT + wn * 64 + c16;
                const bool ragged = (ct + 1) * PT > p.k;     // uniform: only the last centroid tile can hold columns >= k
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int col = col0 + 16 * b;
                    const bool pad = ragged && col >= p.k;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float v = pad ? NEG_INF : acc[a][b][r];
                            if (v > bv[a][r]) {
                                bv[a][r] = v;
                                ba[a][r] = col;
                            }
                        }
                }
            });

        // ---- fold the 16 lanes that hold other columns of the same rows, then the two waves wn = 0, 1
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) {
                    const float ov = __shfl_xor(bv[a][r], m);
                    const int oa = __shfl_xor(ba[a][r], m);
                    km_better(bv[a][r], ba[a][r], ov, oa);
                }
                if (c16 == 0) {
                    red_v[wn][wm * 64 + 16 * a + 4 * g4 + r] = bv[a][r];
                    red_a[wn][wm * 64 + 16 * a + 4 * g4 + r] = ba[a][r];
                }
            }
        __syncthreads();   // also the ring's: every wave is done with it before the next tile's first slab lands
        if ((int)threadIdx.x < in_tile) {
            const int t = threadIdx.x;
            float v = red_v[0][t];
            int arg = red_a[0][t];
            km_better(v, arg, red_v[1][t], red_a[1][t]);
            const long long row = row0 + t;
            if (p.alive != nullptr && ((p.alive[row >> 5] >> (row & 31)) & 1u) == 0u) {
                v = NEG_INF;
                arg = -1;
            }
            p.out_assign[row] = arg;
            p.out_score[row] = v;
        }
        // the next tile writes red_* only after its item loop's barriers, which every thread reaches after these reads
    }
#endif
}

template <int DT>
static int launch_assign(const AssignParams &p, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_assign_kernel<DT>, dim3(scan_grid(p.T)), dim3(256), 0, s, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

// ---- cluster sums ------------------------------------------------------------------------------------------------
constexpr int CS_LANES = 32;    // row lanes of a workgroup: member i of the segment belongs to lane i % 32

struct SumsParams {
    const char *rows;
    unsigned row_bytes;
    int d;
    const int *order;
    const long long *seg_off;
    float *out_sums;
};

template <int DT>
__global__ __launch_bounds__(256) void cluster_sums_kernel(const SumsParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int PER = DT == MMRAG_F32 ? 4 : 8;     // elements of a 16-byte chunk
    constexpr int COLS = 8 * PER;                    // columns of a 128-byte slab
    __shared__ float part[CS_LANES][COLS + 1];
    const int chunk = threadIdx.x & 7, rl = threadIdx.x >> 3;
    const int slab = blockIdx.x, c = blockIdx.y;   // k <= 4096 fits grid.y; a row holds up to 2^17 slabs
    const long long lo = p.seg_off[c], hi = p.seg_off[c + 1];
    const char *const col_base = p.rows + (size_t)slab * SLAB + chunk * 16;

    float acc[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) acc[e] = 0.0f;
    auto add = [&](int row) {
        const char *src = col_base + (size_t)row * p.row_bytes;
        if constexpr (DT == MMRAG_F32) {
            const f32x4_t v = *(const f32x4_t *)src;
#pragma unroll
            for (int e = 0; e < PER; ++e) acc[e] += v[e];
        } else if constexpr (DT == MMRAG_F16) {
            const half8_t v = *(const half8_t *)src;
#pragma unroll
            for (int e = 0; e < PER; ++e) acc[e] += (float)v[e];
        } else {
            const bf16x8_t v = *(const bf16x8_t *)src;
#pragma unroll
            for (int e = 0; e < PER; ++e) acc[e] += (float)v[e];
        }
    };
    // members rl, rl + 32, ... in order; four row numbers are fetched ahead so their loads overlap
    long long i = lo + rl;
    for (; i + 3 * CS_LANES < hi; i += 4 * CS_LANES) {
        const int r0 = p.order[i], r1 = p.order[i + CS_LANES], r2 = p.order[i + 2 * CS_LANES], r3 = p.order[i + 3 * CS_LANES];
        add(r0);
        add(r1);
        add(r2);
        add(r3);
    }
    for (; i < hi; i += CS_LANES) add(p.order[i]);

#pragma unroll
    for (int e = 0; e < PER; ++e) part[rl][chunk * PER + e] = acc[e];
    __syncthreads();
    if ((int)threadIdx.x < COLS) {
        float s[CS_LANES];
#pragma unroll
        for (int j = 0; j < CS_LANES; ++j) s[j] = part[j][threadIdx.x];
#pragma unroll
        for (int stride = CS_LANES / 2; stride >= 1; stride >>= 1)
#pragma unroll
            for (int j = 0; j < stride; ++j) s[j] += s[j + stride];
        const int col = slab * COLS + threadIdx.x;
        if (col < p.d) p.out_sums[(size_t)c * p.d + col] = s[0];
    }
#endif
}

template <int DT>
static int launch_sums(const SumsParams &p, int k, int slabs, hipStream_t s) {
    hipLaunchKernelGGL(cluster_sums_kernel<DT>, dim3((unsigned)slabs, (unsigned)k), dim3(256), 0, s, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

// the checks the two entry points share
static int check_rows(const char *who, int64_t ld, int dtype, int d, int k) {
    const int st = check_stored_rows(who, "clustered", "cluster", ld, dtype, d);
    if (st != MMRAG_OK) return st;
    MMRAG_CHECK_ARG(k >= 1 && k <= MMRAG_MAX_CLUSTERS, "%s: k=%d outside 1..%d", who, k, MMRAG_MAX_CLUSTERS);
    return MMRAG_OK;
}

}  // namespace mmrag_impl

extern "C" {

int mmrag_kmeans_assign(const void *rows, int64_t n, int64_t ld, int dtype, int d, const void *centroids, int k,
                        const uint32_t *alive, int32_t *out_assign, float *out_score, void *stream) {
    using namespace mmrag_impl;
    MMRAG_CHECK_ARG(rows && centroids && out_assign && out_score, "kmeans_assign: null pointer");
    MMRAG_CHECK_ARG(n >= 0 && n < (1LL << 31), "kmeans_assign: need 0 <= n < 2^31 (n=%lld)", (long long)n);
    const int st = check_rows("kmeans_assign", ld, dtype, d, k);
    if (st != MMRAG_OK) return st;
    if (n == 0) return MMRAG_OK;
    AssignParams p;
    p.rows = (const char *)rows;
    p.centroids = (const char *)centroids;
    p.n = n;
    p.k = k;
    p.row_bytes = stored_row_bytes(ld, dtype);
    p.nk = stored_k_slabs(d, dtype);
    p.nct = (k + PT - 1) / PT;
    p.alive = alive;
    p.out_assign = out_assign;
    p.out_score = out_score;
    p.T = (n + PT - 1) / PT;
    hipStream_t s = (hipStream_t)stream;
    return mmrag::with_elem_type(dtype, [&](auto tag) { return launch_assign<decltype(tag)::value>(p, s); });
}

int mmrag_cluster_sums(const void *rows, int64_t ld, int dtype, int d, const int32_t *order, const int64_t *seg_off,
                       int k, float *out_sums, void *stream) {
    using namespace mmrag_impl;
    MMRAG_CHECK_ARG(rows && order && seg_off && out_sums, "cluster_sums: null pointer");
    const int st = check_rows("cluster_sums", ld, dtype, d, k);
    if (st != MMRAG_OK) return st;
    SumsParams p;
    p.rows = (const char *)rows;
    p.row_bytes = stored_row_bytes(ld, dtype);
    p.d = d;
    p.order = order;
    p.seg_off = (const long long *)seg_off;
    p.out_sums = out_sums;
    const int slabs = stored_k_slabs(d, dtype);
    hipStream_t s = (hipStream_t)stream;
    return mmrag::with_elem_type(dtype, [&](auto tag) { return launch_sums<decltype(tag)::value>(p, k, slabs, s); });
}

}  // extern "C"
