// Near-duplicate detection: the exact all-pairs threshold self-join of a row matrix (include/mmrag.h mmrag_sim_join).
//
// X . X^T over the upper triangle, 128 x 128 output tiles, the N x N matrix never written.  The tile body (LDS ring,
// DMA split, MFMA fragments, K order) is pair_tile.h's, with the i-tile as A and the j-tile as B; rows past n read as
// zero through the buffer descriptor.  Tile edges are fixed multiples of 128 and the K order is fixed, so a pair's
// score bits depend on its two rows and d alone.
//
// Nearly every tile has no hit: its exit is one wave-wide "any accumulator >= threshold" test.  A wave with survivors
// applies the alive bits, i < j and the range check, reserves its slots with ONE returning atomic add by one lane and
// writes its pairs with 16-byte stores.
//
// Tile order.  Workgroups are persistent.  The triangle is cut into bands of JOIN_BAND tile rows; inside a band the
// tile pairs run column by column (all the band's i-tiles against one j-tile, then the next j-tile), so the band's
// i-tiles stay in L2 and a j-tile is fetched once per band and XCD.  Workgroup w of G runs the slots
// (t * 8 + w % 8) * (G / 8) + w / 8, t = 0, 1, ...: the workgroups of one XCD (ids 8 apart) hold a contiguous run of
// slots, i.e. a few columns of one band.
#include <math.h>

#include "pair_tile.h"

namespace mmrag_impl {

constexpr int JOIN_BAND = 8;     // tile rows per band

// ---- workgroup id -> tile pair -----------------------------------------------------------------------------------
// first id of tile row r in the row-major order of the triangle (ti <= tj) of a T x T tile grid
__host__ __device__ inline long long join_row_start(long long T, long long r) { return r * (2 * T - r + 1) / 2; }

// id in [0, T (T + 1) / 2) -> (ti, tj), row-major over the triangle.  Exact for T up to 2^16: (2T + 1)^2 < 2^35 is
// exact in a double, the root is off by less than one row, and the integer steps below settle it.
__host__ __device__ inline void join_tile_rowmajor(long long T, long long id, long long &ti, long long &tj) {
    const double b = 2.0 * (double)T + 1.0;
    long long r = (long long)((b - sqrt(b * b - 8.0 * (double)id)) * 0.5);
    r = r < 0 ? 0 : (r > T - 1 ? T - 1 : r);
    while (join_row_start(T, r) > id) --r;
    while (r + 1 < T && join_row_start(T, r + 1) <= id) ++r;
    ti = r;
    tj = r + (id - join_row_start(T, r));
}

// slot in [0, T (T + 1) / 2) -> (ti, tj) in the order the kernel runs: bands of JOIN_BAND tile rows, column-major
// inside a band.  A band holds the same ids as its rows do in the row-major order, so the map is one to one.
__host__ __device__ inline void join_tile_banded(long long T, long long slot, long long &ti, long long &tj) {
    long long r, unused;
    join_tile_rowmajor(T, slot, r, unused);
    const long long b0 = r / JOIN_BAND * JOIN_BAND;
    const long long h = T - b0 < JOIN_BAND ? T - b0 : JOIN_BAND;   // tile rows of this band
    long long k = slot - join_row_start(T, b0);
    const long long tri = h * (h + 1) / 2;                         // columns 0 .. h-1 hold 1 .. h tiles
    long long c = 0;
    if (k < tri) {
        while (k > c) {
            k -= c + 1;
            ++c;
        }
    } else {
        k -= tri;
        c = h + k / h;
        k = k % h;
    }
    ti = b0 + k;
    tj = b0 + c;
}

struct JoinParams {
    const char *rows;
    long long n;
    unsigned row_bytes;     // ld * element size
    int nk;                 // K-slabs that hold the d logical columns
    const unsigned *alive;
    float thr;
    long long *out_pairs;
    float *out_scores;
    unsigned long long capacity;
    unsigned long long *count;
    long long T, total;     // tile rows, tile pairs
};

typedef long long i64x2_t __attribute__((ext_vector_type(2)));

template <int DT>
__global__ __launch_bounds__(256, 2) void sim_join_kernel(const JoinParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(1024))) char smem[PT_LDS];
    const unsigned RB = p.row_bytes;
    const int nk = p.nk;
    const PairTileCtx c = pair_tile_ctx(threadIdx.x, RB, smem);
    const int lane = c.lane, wave = c.wave, wm = c.wm, wn = c.wn, c16 = c.c16, g4 = c.g4;

    const long long G8 = (long long)(gridDim.x >> 3);
    for (long long t = 0;; ++t) {
        const long long slot = (t * 8 + (blockIdx.x & 7)) * G8 + (blockIdx.x >> 3);
        if (slot >= p.total) break;
        long long ti, tj;
        join_tile_banded(p.T, slot, ti, tj);
        const long long i_row0 = ti * PT, j_row0 = tj * PT;

        if (p.alive != nullptr) {
            // a tile whose 128 i-rows or 128 j-rows are all dead has nothing to emit (uniform: the whole workgroup leaves)
            unsigned any_i = 0, any_j = 0;
#pragma unroll
            for (int w = 0; w < PT / 32; ++w) {
                if (i_row0 + 32 * w < p.n) any_i |= p.alive[(i_row0 >> 5) + w];
                if (j_row0 + 32 * w < p.n) any_j |= p.alive[(j_row0 >> 5) + w];
            }
            if (any_i == 0 || any_j == 0) continue;
        }

        const long long my_row0 = wave < 2 ? i_row0 : j_row0;
        const long long left = p.n - my_row0;
        const __amdgpu_buffer_rsrc_t rsrc =
            make_rsrc(p.rows + (size_t)my_row0 * RB, (unsigned)((left < PT ? left : (long long)PT) * (long long)RB));
        auto issue = [&](int item) { pair_tile_issue(c, rsrc, item % PT_NSTAGE, item); };   // ring item = K-slab

        // the one-pair ring, kept here and not pair_tile_ring's: the epilogue below must stay outside the slab loop
        // (pair_tile.h's header has the figures)
        f32x4_t acc[4][4];
        pair_tile_clear(acc);

        int issued = 0;
        for (; issued < PT_NSTAGE - 1 && issued < nk; ++issued) issue(issued);
        for (int it = 0; it < nk; ++it) {
            wait_vmcnt<0>();     // two stages: item `it` is the only one in flight
            __builtin_amdgcn_s_barrier();
            if (issued < nk) {
                issue(issued);
                ++issued;
            }
            slab_step<DT>(smem + (it % PT_NSTAGE) * PT_STAGE, c, acc);
        }

        // ---- epilogue: acc[a][b][r] = <row i, row j>, i = i_row0 + wm*64 + 16a + 4 g4 + r, j = j_row0 + wn*64 + 16b + c16
        float mx = acc[0][0][0];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, acc[a][b][r]);
        if (__builtin_amdgcn_ballot_w64(mx >= p.thr) != 0ull) {
            // rows fit an int: n <= 2^23 (the launcher's check)
            const int n = (int)p.n;
            const int gi0 = (int)i_row0 + wm * 64 + 4 * g4, gj0 = (int)j_row0 + wn * 64 + c16;
            unsigned ok_i = 0, ok_j = 0;    // bit 4a + r / bit b: the row is in range and alive
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                // the four rows 16a + 4 g4 .. + 3 sit in one bitmap word
                const int gi = gi0 + 16 * a;
                unsigned word = 0xffffffffu;
                if (p.alive != nullptr && gi < n) word = p.alive[gi >> 5];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (gi + r < n && ((word >> ((gi + r) & 31)) & 1u)) ok_i |= 1u << (4 * a + r);
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int gj = gj0 + 16 * b;
                unsigned word = 0xffffffffu;
                if (p.alive != nullptr && gj < n) word = p.alive[gj >> 5];
                if (gj < n && ((word >> (gj & 31)) & 1u)) ok_j |= 1u << b;
            }
            // bit 16a + 4b + r of this lane's mask: the element qualifies (score, both rows alive and in range, i < j)
            unsigned long long mask = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool ok = acc[a][b][r] >= p.thr && ((ok_i >> (4 * a + r)) & 1u) && ((ok_j >> b) & 1u) &&
                                        gi0 + 16 * a + r < gj0 + 16 * b;
                        mask |= (unsigned long long)(ok ? 1 : 0) << (16 * a + 4 * b + r);
                    }
            const int n_pass = __popcll(mask);
            // inclusive prefix sum over the wave, then one returning atomic by lane 63 (it holds the wave's total)
            int incl = n_pass;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            const int total = __shfl(incl, 63);
            if (total > 0) {
                unsigned lo = 0, hi = 0;
                if (lane == 63) {
                    const unsigned long long base = atomicAdd(p.count, (unsigned long long)total);
                    lo = (unsigned)base;
                    hi = (unsigned)(base >> 32);
                }
                lo = (unsigned)__shfl((int)lo, 63);
                hi = (unsigned)__shfl((int)hi, 63);
                unsigned long long at = (((unsigned long long)hi << 32) | lo) + (unsigned long long)(incl - n_pass);
                if (n_pass > 0) {
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if ((mask >> (16 * a + 4 * b + r)) & 1ull) {
                                    if (at < p.capacity) {
                                        i64x2_t pr;
                                        pr[0] = gi0 + 16 * a + r;
                                        pr[1] = gj0 + 16 * b;
                                        *(i64x2_t *)(p.out_pairs + 2 * at) = pr;
                                        p.out_scores[at] = acc[a][b][r];
                                    }
                                    ++at;
                                }
                }
            }
        }
        __syncthreads();   // every wave is done with the ring before the next tile's first slab lands
    }
#endif
}

template <int DT>
static int launch_join(const JoinParams &p, hipStream_t s) {
    // persistent grid: two workgroups per CU (the LDS allows two), a multiple of 8 so every XCD runs whole slot runs
    const unsigned g = (scan_grid(p.total) + 7) / 8 * 8;
    hipLaunchKernelGGL(sim_join_kernel<DT>, dim3(g), dim3(256), 0, s, p);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // namespace mmrag_impl

extern "C" {

int mmrag_internal_join_tile(int64_t T, int64_t id, int64_t *ti, int64_t *tj) {
    MMRAG_CHECK_ARG(ti && tj, "join_tile: null pointer");
    MMRAG_CHECK_ARG(T >= 1 && T <= 65536 && id >= 0 && id < T * (T + 1) / 2, "join_tile: need 1 <= T <= 65536 and "
                    "0 <= id < T (T + 1) / 2 (T=%lld id=%lld)", (long long)T, (long long)id);
    long long a, b;
    mmrag_impl::join_tile_rowmajor(T, id, a, b);
    *ti = a;
    *tj = b;
    return MMRAG_OK;
}

int mmrag_internal_join_slot_tile(int64_t T, int64_t slot, int64_t *ti, int64_t *tj) {
    MMRAG_CHECK_ARG(ti && tj, "join_slot_tile: null pointer");
    MMRAG_CHECK_ARG(T >= 1 && T <= 65536 && slot >= 0 && slot < T * (T + 1) / 2, "join_slot_tile: need 1 <= T <= 65536 "
                    "and 0 <= slot < T (T + 1) / 2 (T=%lld slot=%lld)", (long long)T, (long long)slot);
    long long a, b;
    mmrag_impl::join_tile_banded(T, slot, a, b);
    *ti = a;
    *tj = b;
    return MMRAG_OK;
}

int mmrag_sim_join(const void *rows, int64_t n, int64_t ld, int dtype, int d, const uint32_t *alive, float threshold,
                   int64_t *out_pairs, float *out_scores, int64_t capacity, unsigned long long *count, void *stream) {
    using namespace mmrag_impl;
    MMRAG_CHECK_ARG(rows && out_pairs && out_scores && count, "sim_join: null pointer");
    const int st = check_stored_rows("sim_join", "joined", "join", ld, dtype, d, &n);
    if (st != MMRAG_OK) return st;
    MMRAG_CHECK_ARG(capacity >= 0 && capacity <= MMRAG_MAX_JOIN_PAIRS, "sim_join: capacity %lld outside 0..%d",
                    (long long)capacity, MMRAG_MAX_JOIN_PAIRS);
    MMRAG_CHECK_ARG(threshold > 0.0f, "sim_join: the threshold must be a number above 0");   // false for NaN too
    MMRAG_CHECK_ARG((n + PT - 1) / PT <= 65536, "sim_join: at most 2^23 rows (n=%lld)", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    MMRAG_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long), s));
    if (n < 2) return MMRAG_OK;
    JoinParams p;
    p.rows = (const char *)rows;
    p.n = n;
    p.row_bytes = stored_row_bytes(ld, dtype);
    p.nk = stored_k_slabs(d, dtype);
    p.alive = alive;
    p.thr = threshold;
    p.out_pairs = (long long *)out_pairs;
    p.out_scores = out_scores;
    p.capacity = (unsigned long long)capacity;
    p.count = count;
    p.T = (n + PT - 1) / PT;
    p.total = p.T * (p.T + 1) / 2;
    return mmrag::with_elem_type(dtype, [&](auto tag) { return launch_join<decltype(tag)::value>(p, s); });
}

}  // extern "C"
