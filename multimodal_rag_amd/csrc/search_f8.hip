// FP8 (MMRAG_F8E4M3) scan for gfx950: the slab-ring plan of cosine_topk_kernel (search.hip) on the block-scaled FP8
// matrix instruction.
//
// Same persistent grid, 256-row tiles, 128-byte slabs through the LDS-DMA ring with the same XOR swizzle, query on the
// lane, same TopList selection, same candidate-list workspace layout (merge_topk_kernel / mmrag_cosine_topk_select and
// the deep search's select reduce its output unchanged), same filter mode (K = 0).  What differs:
//   * an element is one byte, so a row has half the slabs of an fp16 row: half the DMA pieces, barriers and bytes;
//   * the slab body is two v_mfma_scale_f32_32x32x64_f8f6f4 per 32-row block (E4M3 x E4M3, scales 1.0), which does
//     twice the bf16 work per clock;
//   * stored values carry the constant scale 2^8 on both operands, so the accumulator is 2^16 x the score.  Selection
//     runs in accumulator units; a score is scaled by 2^-16 (exact) where it leaves the kernel, and thresholds handed in
//     (sample pre-pass, deep search's tau) are scaled by 2^16 where they enter.
// The kernel body is slab_ring_body.inc, the one cosine_topk_kernel includes too: these differences sit there behind
// `if constexpr (DT == MMRAG_F8E4M3)`.  The instruction streams of both families are pinned by hash
// (tests/test_deep_topk_cpu.py for search.hip, tests/test_f8_cpu.py for this file).
#include "slab_ring.h"

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int NW = 8;             // waves per workgroup, 2 per SIMD (256 registers each)

template <int WN, int K, int NSTAGE>
__global__ __launch_bounds__(64 * NW, NW / 4) void cosine_topk_f8_kernel(const KParams p) {
#if defined(__HIP_DEVICE_COMPILE__)  // amdgcn builtins below: the host pass only needs the launch stub
    constexpr int DT = MMRAG_F8E4M3;
    constexpr bool SEEDED = false;
#include "slab_ring_body.inc"
#endif  // __HIP_DEVICE_COMPILE__
}

// The 256-query plan (WN = 8) of search.hip runs here as 128-query groups of the WN = 4 kernel: an FP8 fragment is
// 8 registers, and next to the 128 accumulator registers of a wave that owns 8 row blocks (or the 128-register budget
// of a 16-wave shape) the compiler spills inside the tile loop, where a reload drains the DMA ring.  The plan's
// grid_x x grid_y workgroups were sized so that all of them are resident (144 KiB of LDS: one per CU); with `groups`
// 128-query groups instead of grid_y 256-query groups the walkers are cut to grid_x * grid_y / groups (whole XCD
// rounds), so the grid stays co-resident and the groups of a walker stream the same tiles together, one HBM fetch and
// L2 hits for the siblings, as the fp16 kernel's query groups do.  The candidate lists are indexed by (global query,
// walker): the layout and the merge do not change, and the list slots of the walkers left out are filled empty.
__global__ void fill_f8_lists_empty_kernel(float *s, int *r, int n_lists, int K, int slot_lo, int slot_hi, int B) {
    const int per = (slot_hi - slot_lo) * K;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * per) return;
    const size_t at = ((size_t)(i / per) * n_lists + slot_lo) * K + (size_t)(i % per);
    s[at] = NEG_INF;
    r[at] = INT_MAX;
}

template <int WN, int K>
void launch_f8(const KParams &p, int walkers, int groups, hipStream_t s) {
    KParams kp = p;
    kp.walkers = walkers;
    kp.share_l2 = groups > 1;
    cosine_topk_f8_kernel<WN, K, 3><<<walkers * groups, 64 * NW, 0, s>>>(kp);
}

template <int K>
int dispatch_f8(int WN, const KParams &p, int grid_x, int grid_y, hipStream_t s) {
    if (WN == 2) launch_f8<2, K>(p, grid_x, grid_y, s);
    else if (WN == 4) launch_f8<4, K>(p, grid_x, grid_y, s);
    else {
        const int groups = (p.B + 127) / 128;
        int w = (int)((long long)grid_x * grid_y / groups);
        if (w >= 8) w = w / 8 * 8;
        if (w < 1) w = 1;
        if (w > grid_x) w = grid_x;
        if (K > 0 && w < grid_x) {
            const long long total = (long long)p.B * (grid_x - w) * K;
            fill_f8_lists_empty_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(p.cand_s, p.cand_r, p.n_lists,
                                                                                        K, w, grid_x, p.B);
        }
        launch_f8<4, K>(p, w, groups, s);
    }
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

}  // namespace

// the list search's dispatch (search.hip dispatch_main) for dtype MMRAG_F8E4M3: list depth K = 5 / 10 / 20, the plan's WN
int f8_lists_launch(int K, int WN, const KParams &p, int grid_x, int grid_y, hipStream_t s) {
    if (K == 5) return dispatch_f8<5>(WN, p, grid_x, grid_y, s);
    if (K == 10) return dispatch_f8<10>(WN, p, grid_x, grid_y, s);
    return dispatch_f8<20>(WN, p, grid_x, grid_y, s);
}

// filter mode (K = 0) for search_deep.hip
int f8_filter_launch(int WN, const KParams &p, int grid_x, int grid_y, hipStream_t s) {
    return dispatch_f8<0>(WN, p, grid_x, grid_y, s);
}

}  // namespace mmrag_impl
