// The 128 x 128 "rows against rows" tile body of every kernel that scores stored rows against a batch of rows: the
// similarity join (simjoin.hip), the k-means assign step (kmeans.hip), the scoped, filtered, range, boosted, recommend
// and related scans (scoped.hip, masked_scan.h, boosted.hip, recommend.hip, related.hip) and the two MaxSim kernels
// (maxsim.hip, maxsim_scan.hip): A . B^T of a 128-row A tile and a 128-row B tile, float32 accumulators in registers.
//
// A workgroup is 4 waves in a 2 x 2 grid, 64 x 64 outputs per wave as 4 x 4 MFMA tiles of 16 x 16
// (v_mfma_f32_16x16x32_f16 / _bf16; float32 rows: v_mfma_f32_16x16x4_f32, the exact float32 matrix instruction).  Both
// operand tiles arrive by the tile_dma.h ring in 128-byte K-slabs: a stage is the A tile's slab then the B tile's
// (2 x 16 KiB), two stages, so two workgroups share a CU.  Waves 0, 1 fetch the A tile, waves 2, 3 the B tile; rows
// past the buffer descriptor's range read as zero.
//
// The ring loop is here too, once: pair_tile_ring runs a sequence of (A tile, B tile) pairs through the two stages
// without draining between them and hands each finished pair's accumulators to the kernel.  Every kernel named above
// but one calls it and has no wait, barrier or stage index of its own; they keep what differs: which tiles (the `src`
// callback) and the epilogue (`done`).  The deliberate exception is sim_join_kernel, whose ring is one pair long: as
// `done` its epilogue (64 accumulators tested and packed at once, 204 VGPRs) would sit inside the slab loop, and the
// compiler then spills (256 VGPRs, 792 bytes of scratch per lane).  It keeps the one-pair loop it had.
// The prologue the row-walking scans repeat -- a tile's geometry, which of its 128 rows are live, their group ordinals
// -- is pair_row_tile / pair_tile_live_rows / pair_tile_row_ordinals.
#pragma once
#include "mmrag_internal.h"
#include "tile_dma.h"

namespace mmrag_impl {

constexpr int PT = 128;                      // tile edge (rows of A and of B per workgroup)
constexpr int PT_NSTAGE = 2;
constexpr int PT_STAGE = 2 * PT * SLAB;      // A tile then B tile, one K-slab each
constexpr int PT_LDS = PT_NSTAGE * PT_STAGE;
constexpr int PT_LOADS = 2 * PT / 8 / 4;     // 1 KiB DMA instructions per wave per ring item: 32 pieces over 4 waves
static_assert(PT_LDS <= 80 * 1024, "two workgroups per CU");

struct PairTileCtx {
    int lane, wave;         // wave: uniform (a scalar register)
    int wm, wn;             // this wave's 64 x 64 quadrant: A rows wm * 64 .., B rows wn * 64 ..
    int c16, g4;            // lane & 15, lane >> 4
    int sw;                 // the fragment reads' chunk swizzle
    int a_base, b_base;     // byte offset in a stage of row c16 of the quadrant's first 16-row block
    unsigned src_off[PT_LOADS];
    char *dst;              // where this wave's DMA pieces land in stage 0
};

// `smem`: PT_LDS bytes, 1 KiB aligned; `row_bytes`: the pitch of both operands' rows
__device__ __forceinline__ PairTileCtx pair_tile_ctx(unsigned tid, unsigned row_bytes, char *smem) {
    PairTileCtx c;
    c.lane = tid & 63;
    c.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    c.wm = c.wave >> 1;
    c.wn = c.wave & 1;
    c.c16 = c.lane & 15;
    c.g4 = c.lane >> 4;
    // this wave's DMA pieces: 8 consecutive 8-row pieces of the stage (waves 0, 1: the A tile; waves 2, 3: the B tile)
#pragma unroll
    for (int i = 0; i < PT_LOADS; ++i) c.src_off[i] = dma_src_offset((c.wave & 1) * PT_LOADS + i, c.lane, row_bytes);
    c.dst = smem + c.wave * PT_LOADS * 1024;
    c.sw = (c.c16 >> 1) & 7;
    c.a_base = (c.wm * 64 + c.c16) * SLAB;
    c.b_base = PT * SLAB + (c.wn * 64 + c.c16) * SLAB;
    return c;
}

// this wave's share of K-slab `kslab` of the tile behind `rsrc` (waves 0, 1: the A tile's; waves 2, 3: the B tile's)
__device__ __forceinline__ void pair_tile_issue(const PairTileCtx &c, __amdgpu_buffer_rsrc_t rsrc, int stage, int kslab) {
    char *dst = c.dst + stage * PT_STAGE;
    const unsigned koff = (unsigned)kslab * SLAB;
#pragma unroll
    for (int i = 0; i < PT_LOADS; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)(dst + i * 1024), 16, c.src_off[i] + koff, 0, 0, 0);
}

__device__ __forceinline__ void pair_tile_clear(f32x4_t (&acc)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.0f;
}

// acc[a][b][r] += <A row wm*64 + 16a + 4 g4 + r, B row wn*64 + 16b + c16> over the K-slab in `stage`.
// A 128-byte slab is two k-steps (one for E4M3 codes); lane (c16, g4) reads chunk 4 s + g4 of row c16 of every 16-row
// block.  One fixed K order for every pair of rows: the score bits depend on the two rows and d alone, not on the tile, the grid or the
// kernel.
__device__ __forceinline__ void slab_step_codes(const char *stage, const PairTileCtx &c, f32x4_t (&acc)[4][4]);
template <int DT>
__device__ __forceinline__ void slab_step(const char *stage, const PairTileCtx &c, f32x4_t (&acc)[4][4]) {
    if constexpr (DT == MMRAG_F8E4M3) slab_step_codes(stage, c, acc);
    else
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int off = ((4 * s + c.g4) ^ c.sw) * 16;
        if constexpr (DT == MMRAG_F32) {
            // exact float32: chunk 4 s + g4 holds four consecutive floats of the row; MFMA e takes element e of
            // every lane's chunk, i.e. k = 4 (4 s + g4) + e for g4 = 0 .. 3 -- the same k for both operands
            f32x4_t fa[4], fb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) fa[a] = *(const f32x4_t *)(stage + c.a_base + a * (16 * SLAB) + off);
#pragma unroll
            for (int b = 0; b < 4; ++b) fb[b] = *(const f32x4_t *)(stage + c.b_base + b * (16 * SLAB) + off);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a][e], fb[b][e], acc[a][b], 0, 0, 0);
        } else {
            using Frag = FragType<DT>;
            typename Frag::T fa[4], fb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) fa[a] = *(const typename Frag::T *)(stage + c.a_base + a * (16 * SLAB) + off);
#pragma unroll
            for (int b = 0; b < 4; ++b) fb[b] = *(const typename Frag::T *)(stage + c.b_base + b * (16 * SLAB) + off);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = Frag::mfma_16x16x32(fa[a], fb[b], acc[a][b]);
        }
    }
}

// The same for rows of E4M3 codes: a 128-byte slab is 128 K-elements of a row, ONE block-scaled
// v_mfma_scale_f32_16x16x128_f8f6f4 per (a, b) block pair (format 0 = E4M3 on both sides, every scale byte 127 = 1.0).
// A lane supplies 32 bytes of its row per block: chunks g4 and 4 + g4, i.e. the two reads of slab_step's 16-bit branch
// (t for s), so the LDS reads and their banks are that branch's, conflict-free under the same swizzle.  (Chunks 2 g4,
// 2 g4 + 1 would put lanes g4 = 0 and g4 = 1 of one ds_read_b128 lane group on the same bank slots.)  A and B use the
// same lane-to-k map, so which 32 of the 128 k a lane holds is the hardware's business.  The C/D layout is the 16 x 16
// one of the other forms: acc holds 2^16 times the similarity.
__device__ __forceinline__ void slab_step_codes(const char *stage, const PairTileCtx &c, f32x4_t (&acc)[4][4]) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    typedef int i32x8 __attribute__((ext_vector_type(8)));
    const int o0 = (c.g4 ^ c.sw) * 16, o1 = ((4 + c.g4) ^ c.sw) * 16;
    i32x8 fa[4], fb[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const i32x4 lo = *(const i32x4 *)(stage + c.a_base + a * (16 * SLAB) + o0);
        const i32x4 hi = *(const i32x4 *)(stage + c.a_base + a * (16 * SLAB) + o1);
        fa[a] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const i32x4 lo = *(const i32x4 *)(stage + c.b_base + b * (16 * SLAB) + o0);
        const i32x4 hi = *(const i32x4 *)(stage + c.b_base + b * (16 * SLAB) + o1);
        fb[b] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[a], fb[b], acc[a][b], 0, 0, 0,
                                                                         0x7f7f7f7f, 0, 0x7f7f7f7f);
}

// Between a tile's last slab_step and the first read of its accumulators.  For E4M3 codes: slab_ring_body.inc's
// stop-gap for the suspected wait-state shortfall after a block-scaled MFMA (the account is there), once per B tile;
// nothing for the other types.
template <int DT>
__device__ __forceinline__ void pair_tile_settle() {
    if constexpr (DT == MMRAG_F8E4M3) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The calling wave's operand of one (A tile, B tile) pair: waves 0, 1 name the A tile, waves 2, 3 the B tile.  `bytes`
// end the buffer descriptor: rows at and past it read as zero.
struct PairTileSrc {
    const char *base;
    unsigned bytes;
};

// The ring: `n_tiles` pairs of `nk` K-slabs each through the two stages, no drain between pairs.  `smem` and `c` are
// pair_tile_ctx's.  For pair j = 0 .. n_tiles - 1
//   src(j)         -> PairTileSrc, wave-uniform; called exactly once per pair, in order, before done(j) -- but a whole
//                     slab ahead of the MFMAs, so src(j + 1) may be (with nk == 1: is) called before done(j);
//   done(j, acc)   after pair j's last slab_step and pair_tile_settle: acc[a][b][r] = <A row wm*64 + 16a + 4 g4 + r,
//                     B row wn*64 + 16b + c16> of pair j; the ring clears acc afterwards.
// Either side may be the one that moves from pair to pair; the tile that stays is fetched again for each pair (L2).
// Callbacks may keep state (a bitmask of wanted tiles popped once in each, a prefetch of pair j + 1 in done(j)) and may
// diverge inside, but every wave of the workgroup must call the ring with the same nk and n_tiles: its barriers are
// reached by all four waves or by none.  n_tiles == 0 does nothing.
// THE CALLER'S: one workgroup barrier (__syncthreads) between the return and the next call's first slab, which would
// otherwise land on a stage another wave is still reading.  A kernel that ends, or that has a barrier of its own on
// that path, needs no second one.
template <int DT, typename Src, typename Done>
__device__ __forceinline__ void pair_tile_ring(const PairTileCtx &c, const char *smem, int nk, int n_tiles, Src &&src,
                                               Done &&done) {
    const int total = nk * n_tiles;
    if (total <= 0) return;
    int issued = 0, i_ks = 0, i_j = 0;
    PairTileSrc from = {nullptr, 0u};
    auto issue = [&]() {
        // ring item `issued` = K-slab i_ks of pair i_j
        if (i_ks == 0) from = src(i_j);
        pair_tile_issue(c, make_rsrc(from.base, from.bytes), issued % PT_NSTAGE, i_ks);
        ++issued;
        if (++i_ks == nk) {
            i_ks = 0;
            ++i_j;
        }
    };

    f32x4_t acc[4][4];
    pair_tile_clear(acc);
    issue();
    int ks = 0, j = 0;
    for (int it = 0; it < total; ++it) {
        wait_vmcnt<0>();     // two stages: item `it` is the only one in flight
        __builtin_amdgcn_s_barrier();
        if (issued < total) issue();
        slab_step<DT>(smem + (it % PT_NSTAGE) * PT_STAGE, c, acc);
        if (++ks < nk) continue;
        ks = 0;
        pair_tile_settle<DT>();
        done(j, acc);
        ++j;
        pair_tile_clear(acc);
    }
}

// ---- the prologue of the kernels that walk 128-row tiles of the stored rows ----------------------------------------
struct PairRowTile {
    long long tile, row0;   // the tile and its first row
    int rows;               // its rows below n: 1 .. 128
};
// step i of a walk over `walk` of the collection's T tiles, spread evenly: tile i * T / walk (walk == T: tile i)
__device__ __forceinline__ PairRowTile pair_row_tile(long long i, long long T, long long walk, long long n) {
    PairRowTile t;
    t.tile = i * T / walk;           // < T
    t.row0 = t.tile * PT;
    const long long left = n - t.row0;      // >= 1
    t.rows = left < PT ? (int)left : PT;
    return t;
}

// Which of the tile's 128 rows are candidates (below n, alive; `alive` null: every row): each lane looks at rows
// `lane` and `lane + 64`.  Bit i of m0 = row row0 + i is live, of m1 = row row0 + 64 + i: the same two scalars in
// all four waves, so a branch on them is the workgroup's.
__device__ __forceinline__ void pair_tile_live_rows(long long row0, int lane, long long n, const unsigned *alive,
                                                    unsigned long long &m0, unsigned long long &m1) {
    bool live[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long long r = row0 + lane + 64 * h;
        live[h] = r < n && (alive == nullptr || ((alive[r >> 5] >> (r & 31)) & 1u) != 0u);
    }
    m0 = __builtin_amdgcn_ballot_w64(live[0]);
    m1 = __builtin_amdgcn_ballot_w64(live[1]);
}

// The ordinal-flavoured twin: ord[h] = the group ordinal of row row0 + lane + 64 h, -1 for a row past n, a dead row
// and a row in no group (an ordinal outside 0 .. n_groups - 1)
__device__ __forceinline__ void pair_tile_row_ordinals(long long row0, int lane, long long n, const unsigned *alive,
                                                       const int *group_of_row, int n_groups, int (&ord)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long long r = row0 + lane + 64 * h;
        int o = -1;
        if (r < n) {
            o = group_of_row[r];
            if (alive != nullptr && ((alive[r >> 5] >> (r & 31)) & 1u) == 0u) o = -1;
            if ((unsigned)o >= (unsigned)n_groups) o = -1;
        }
        ord[h] = o;
    }
}

// what an accumulator of DT operands is worth: E4M3 codes hold x * 256 on both sides
template <int DT>
constexpr float PT_ACC_SCALE = DT == MMRAG_F8E4M3 ? 0x1p-16f : 1.0f;

// ---- host side ---------------------------------------------------------------------------------------------------
// the persistent grid of a kernel that walks `walk` tiles: two workgroups per CU (PT_LDS allows two), at most one per
// visited tile
inline unsigned scan_grid(long long walk) {
    long long g = 2LL * mmrag::num_cus();
    if (g > walk) g = walk;
    return (unsigned)g;
}

inline unsigned stored_row_bytes(int64_t ld, int dtype) { return (unsigned)(ld * mmrag::esize(dtype)); }
// K-slabs that hold the d logical columns
inline int stored_k_slabs(int d, int dtype) { return (int)(((long long)d * mmrag::esize(dtype) + SLAB - 1) / SLAB); }

// Stored rows the tile body (and mmrag_cluster_sums) can read: a full-precision dtype, 0 < d <= ld, rows of whole
// 128-byte slabs and at most 16 MiB.  FP8 is reported, not read: "... rows are not `done`; `verb` the collection's
// re-scoring plane".  `n`: the row count of a caller that reports it with d and ld (null: the caller checks its own).
inline int check_stored_rows(const char *who, const char *done, const char *verb, int64_t ld, int dtype, int d,
                             const int64_t *n = nullptr) {
    MMRAG_CHECK_ARG(dtype >= 0 && dtype <= MMRAG_F8E4M3, "%s: bad dtype %d", who, dtype);
    if (n != nullptr)
        MMRAG_CHECK_ARG(*n >= 0 && d > 0 && ld >= d, "%s: need n >= 0 and 0 < d <= ld (n=%lld d=%d ld=%lld)", who,
                        (long long)*n, d, (long long)ld);
    MMRAG_CHECK_ARG(d > 0 && ld >= d, "%s: need 0 < d <= ld (d=%d ld=%lld)", who, d, (long long)ld);
    if (dtype == MMRAG_F8E4M3) {
        mmrag::set_error("%s: float8_e4m3 rows are not %s; %s the collection's re-scoring plane", who, done, verb);
        return MMRAG_EUNSUPPORTED;
    }
    MMRAG_CHECK_ARG(ld * mmrag::esize(dtype) % SLAB == 0 && ld * mmrag::esize(dtype) <= (1LL << 24),
                    "%s: ld must cover whole 128-byte slabs (mmrag_padded_dim), rows of at most 16 MiB (ld=%lld)", who,
                    (long long)ld);
    return MMRAG_OK;
}

// Rows of E4M3 codes that slab_step<MMRAG_F8E4M3> reads (the FP8 MaxSim entries alone): 0 < d <= ld, ld bytes of
// whole 128-byte slabs (mmrag_padded_dim(d, MMRAG_F8E4M3) or larger), rows of at most 16 MiB.
inline int check_code_rows(const char *who, int64_t ld, int d) {
    MMRAG_CHECK_ARG(d > 0 && ld >= d, "%s: need 0 < d <= ld (d=%d ld=%lld)", who, d, (long long)ld);
    MMRAG_CHECK_ARG(ld % SLAB == 0 && ld <= (1LL << 24),
                    "%s: ld must cover whole 128-byte slabs of codes (mmrag_padded_dim(d, MMRAG_F8E4M3)), rows of at "
                    "most 16 MiB (ld=%lld)", who, (long long)ld);
    return MMRAG_OK;
}

}  // namespace mmrag_impl
