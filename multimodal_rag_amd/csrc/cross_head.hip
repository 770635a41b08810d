// Sequence-pair classification head of the cross-encoder (BertForSequenceClassification), float32, for gfx950.
//
// The reference's EmbeddingManager.rerank_results (app/utils/embedder.py:834-859) is a placeholder whose docstring names
// a cross-encoder as the missing piece.  After the encoder body has left the [CLS] rows in float32 ([B, H]), this one
// launch computes
//     pooled = tanh(W_p . cls + b_p)          (BertPooler)
//     logits = W_c . pooled + b_c             (the classifier, n_labels <= 16)
// The head is ~2 B H^2 flops, nothing next to the layers; what it must not do is make one workgroup stream all of W_p
// (H^2 floats) per tile of sequences, or spend its time in cross-lane reductions.  So the grid is (16-feature slices of
// W_p) x (16-sequence tiles): a workgroup stages its 16 rows of W_p and its 16 [CLS] rows in LDS (one round of loads),
// each thread computes ONE pooled feature of one sequence as a plain k-ordered fmaf chain, and the workgroup writes
// its slice's contribution to the logits to `part`.  The last workgroup of a sequence tile to finish (an arrival
// counter, zeroed earlier in the same stream) adds the slices' contributions in slice order, so the logits are
// bit-identical from call to call and do not depend on which other sequences share the batch.
#include "mmrag_internal.h"
#include "tile_dma.h"

#include <math.h>

using namespace mmrag;

namespace mmrag_impl {

namespace {

constexpr int HEAD_FT = 16;    // pooled features per workgroup
constexpr int HEAD_TB = 16;    // sequences per workgroup
constexpr int HEAD_S = 1028;   // LDS row stride (floats): H <= 1024, +4 spreads the 16 rows over all 64 banks

// cls [B, H], wp [H, H], bp [H], wc [NL, H], bc [NL] -> out [B, NL]; part [n_ft, B, NL]; cnt [n_st] (zero on entry,
// zero again on exit).  H % 16 == 0, H <= 1024, NL <= 16.
__global__ __launch_bounds__(256) void cls_head_f32_kernel(const float *__restrict__ cls, const float *__restrict__ wp,
                                                           const float *__restrict__ bp, const float *__restrict__ wc,
                                                           const float *__restrict__ bc, float *__restrict__ out,
                                                           float *__restrict__ part, int *__restrict__ cnt, int B, int H,
                                                           int NL) {
    __shared__ __attribute__((aligned(16))) float w_lds[HEAD_FT * HEAD_S];
    __shared__ __attribute__((aligned(16))) float x_lds[HEAD_TB * HEAD_S];
    __shared__ float pooled[HEAD_TB][HEAD_FT + 1];
    __shared__ int last;
    const int ft = blockIdx.x, n_ft = gridDim.x, st = blockIdx.y;
    const int b0 = st * HEAD_TB, f0 = ft * HEAD_FT;
    const int nb = B - b0 < HEAD_TB ? B - b0 : HEAD_TB;
    const int h4 = H >> 2, n4 = HEAD_FT * h4;   // float4s of the W_p slice (= of the [CLS] tile)
    // one round of loads: the slice's rows of W_p and the tile's [CLS] rows (rows past the batch: zero)
    f32x4_t buf[2 * HEAD_FT * 1024 / 4 / 256];
#pragma unroll
    for (int u = 0; u < 2 * HEAD_FT * 1024 / 4 / 256; ++u) {
        const int i = threadIdx.x + 256 * u;
        buf[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (i < n4) {
            buf[u] = ((const f32x4_t *)(wp + (size_t)(f0 + i / h4) * H))[i % h4];
        } else if (i < 2 * n4) {
            const int r = (i - n4) / h4;
            if (r < nb) buf[u] = ((const f32x4_t *)(cls + (size_t)(b0 + r) * H))[(i - n4) % h4];
        }
    }
#pragma unroll
    for (int u = 0; u < 2 * HEAD_FT * 1024 / 4 / 256; ++u) {
        const int i = threadIdx.x + 256 * u;
        if (i < n4) *(f32x4_t *)(w_lds + (i / h4) * HEAD_S + 4 * (i % h4)) = buf[u];
        else if (i < 2 * n4) *(f32x4_t *)(x_lds + ((i - n4) / h4) * HEAD_S + 4 * ((i - n4) % h4)) = buf[u];
    }
    __syncthreads();
    // pooler: thread (t, j) = sequence b0 + t, feature f0 + j
    {
        const int j = threadIdx.x & (HEAD_FT - 1), t = threadIdx.x / HEAD_FT;
        const float *wr = w_lds + j * HEAD_S, *xr = x_lds + t * HEAD_S;
        float acc = 0.f;
        for (int k = 0; k < H; k += 4) {
            const f32x4_t w4 = *(const f32x4_t *)(wr + k), x4 = *(const f32x4_t *)(xr + k);
            acc = fmaf(w4[0], x4[0], acc);
            acc = fmaf(w4[1], x4[1], acc);
            acc = fmaf(w4[2], x4[2], acc);
            acc = fmaf(w4[3], x4[3], acc);
        }
        pooled[t][j] = tanhf(acc + bp[f0 + j]);
    }
    __syncthreads();
    // this slice's contribution to the logits of the tile's sequences
    const int t = threadIdx.x / NL, c = threadIdx.x - t * NL;
    const bool mine = threadIdx.x < HEAD_TB * NL && t < nb;
    if (mine) {
        const float *wrow = wc + (size_t)c * H + f0;
        float s = 0.f;
#pragma unroll
        for (int jl = 0; jl < HEAD_FT; ++jl) s = fmaf(wrow[jl], pooled[t][jl], s);
        part[((size_t)ft * B + b0 + t) * NL + c] = s;
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(cnt + st, 1) == n_ft - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();
    if (mine) {
        float s = 0.f;
        for (int f = 0; f < n_ft; ++f)
            s += __hip_atomic_load(part + ((size_t)f * B + b0 + t) * NL + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[(size_t)(b0 + t) * NL + c] = s + bc[c];
    }
    if (threadIdx.x == 0) atomicExch(cnt + st, 0);
}

}  // namespace

size_t cls_head_workspace_bytes(int B, int H, int NL) {
    const size_t n_ft = (size_t)((H + HEAD_FT - 1) / HEAD_FT), n_st = (size_t)((B + HEAD_TB - 1) / HEAD_TB);
    return (n_ft * (size_t)B * (size_t)NL * 4 + 255) / 256 * 256 + (n_st * 4 + 255) / 256 * 256;
}

int cls_head_counters(int B) { return (B + HEAD_TB - 1) / HEAD_TB; }

// `ws` (cls_head_workspace_bytes, 256-byte aligned): partial logits, then the arrival counters, which must be zero
// when the kernel starts (the cross-encoder forward's embedding kernel zeroes them)
int launch_cls_head_f32(const float *cls, const float *wp, const float *bp, const float *wc, const float *bc, float *out,
                        int B, int H, int NL, void *ws, hipStream_t s) {
    MMRAG_CHECK_ARG(cls && wp && bp && wc && bc && out && ws, "cls_head: null pointer");
    MMRAG_CHECK_ARG(B > 0 && H > 0 && H % HEAD_FT == 0 && H <= 1024, "cls_head: bad shape B=%d H=%d", B, H);
    MMRAG_CHECK_ARG(NL >= 1 && NL <= 16, "cls_head: n_labels = %d (1..16)", NL);
    MMRAG_CHECK_ARG(((uintptr_t)cls % 16) == 0 && ((uintptr_t)wp % 16) == 0 && ((uintptr_t)ws % 256) == 0,
                    "cls_head: misaligned pointer");
    const int n_ft = (H + HEAD_FT - 1) / HEAD_FT, n_st = cls_head_counters(B);
    float *part = (float *)ws;
    int *cnt = (int *)((char *)ws + ((size_t)n_ft * B * NL * 4 + 255) / 256 * 256);
    cls_head_f32_kernel<<<dim3((unsigned)n_ft, (unsigned)n_st), 256, 0, s>>>(cls, wp, bp, wc, bc, out, part, cnt, B, H, NL);
    MMRAG_CHECK_HIP(hipGetLastError());
    return MMRAG_OK;
}

int *cls_head_counter_ptr(void *ws, int B, int H, int NL) {
    const int n_ft = (H + HEAD_FT - 1) / HEAD_FT;
    return (int *)((char *)ws + ((size_t)n_ft * B * NL * 4 + 255) / 256 * 256);
}

}  // namespace mmrag_impl

extern "C" {

// (tests only, not in mmrag.h) the head on its own: zeroes its counters, then the one launch
int mmrag_internal_cls_head_f32(const float *cls, const float *wp, const float *bp, const float *wc, const float *bc,
                                float *out, int B, int H, int NL, void *ws, size_t ws_bytes, void *stream) {
    MMRAG_CHECK_ARG(B > 0 && H > 0 && NL > 0, "cls_head: bad shape");
    if (!ws || ws_bytes < mmrag_impl::cls_head_workspace_bytes(B, H, NL)) {
        mmrag::set_error("cls_head: workspace too small");
        return MMRAG_EWORKSPACE;
    }
    MMRAG_CHECK_ARG(((uintptr_t)ws % 256) == 0, "cls_head: workspace must be 256-byte aligned");
    MMRAG_CHECK_HIP(hipMemsetAsync(mmrag_impl::cls_head_counter_ptr(ws, B, H, NL), 0,
                                   (size_t)mmrag_impl::cls_head_counters(B) * 4, (hipStream_t)stream));
    return mmrag_impl::launch_cls_head_f32(cls, wp, bp, wc, bc, out, B, H, NL, ws, (hipStream_t)stream);
}

size_t mmrag_internal_cls_head_workspace_bytes(int B, int H, int NL) {
    return mmrag_impl::cls_head_workspace_bytes(B, H, NL);
}

}  // extern "C"
