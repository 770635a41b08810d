// Internal helpers shared by the libmmrag.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/mmrag.h"

namespace mmrag {

void set_error(const char *fmt, ...);

inline int esize(int dtype) { return dtype == MMRAG_F32 ? 4 : (dtype == MMRAG_F8E4M3 ? 1 : 2); }

constexpr size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// f(tag) for the full-precision storage type of `dtype` (checked by the caller; FP8 is dispatched before this):
// decltype(tag)::value is MMRAG_F32 / MMRAG_F16 / MMRAG_BF16 as a compile-time constant, for kernels templated on the
// integer; row_dot.h's elem_t<> turns it into float / __half / __hip_bfloat16 for those templated on the element
template <int DT>
struct ElemTag {
    static constexpr int value = DT;
};
template <typename F>
inline auto with_elem_type(int dtype, F &&f) {
    if (dtype == MMRAG_F32) return f(ElemTag<MMRAG_F32>{});
    if (dtype == MMRAG_F16) return f(ElemTag<MMRAG_F16>{});
    return f(ElemTag<MMRAG_BF16>{});
}

#define MMRAG_CHECK_ARG(cond, ...)            \
    do {                                      \
        if (!(cond)) {                        \
            mmrag::set_error(__VA_ARGS__);    \
            return MMRAG_EINVAL;              \
        }                                     \
    } while (0)

#define MMRAG_CHECK_HIP(expr)                                                     \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            mmrag::set_error("%s failed: %s", #expr, hipGetErrorString(e_));      \
            return MMRAG_EHIP;                                                    \
        }                                                                         \
    } while (0)

// number of CUs of the current device (cached per device id)
int num_cus();

// developer switches (set through mmrag_internal_set_debug by A/B tools only)
unsigned debug_flags();
constexpr unsigned DBG_LINEAR_PLAIN = 1u, DBG_LINEAR_NO_SMALL = 2u, DBG_LINEAR_NO_PERSIST = 4u;
// timing-only ablations of the persistent linear kernel (results are wrong): stores dropped by the buffer unit, no epilogue at all
constexpr unsigned DBG_LINEAR_DROP_STORES = 8u, DBG_LINEAR_SKIP_EPILOGUE = 16u;
constexpr unsigned DBG_LINEAR_X_SAME = 128u;
constexpr unsigned DBG_LINEAR_MFMA32 = 8192u;   // persistent GEMM on v_mfma_f32_32x32x16_f16 instead of 16x16x32 (A/B of the MFMA shape)
constexpr unsigned DBG_LINEAR_SMALL32 = 256u;
constexpr unsigned DBG_ENCODER_LN_PASSES = 512u;
constexpr unsigned DBG_ATTENTION_STREAMED = 4096u;   // attention: the double-buffered key-tile loop also for short sequences (A/B)
constexpr unsigned DBG_LINEAR_TILE64 = 1024u, DBG_LINEAR_TILE128 = 2048u;   // mid-size M: force 64x64 / 128x128 tiles (A/B)   // BERT single-query forward with LayerNorm launches (A/B, tests)   // M <= 64: the 32-feature workgroups for every K (A/B)   // timing only: every tile reads the first token tile

}  // namespace mmrag

// test-only exports of the similarity join (simjoin.hip): the tile pair (ti <= tj) of id / slot in [0, T (T + 1) / 2),
// T = ceil(n / 128) <= 65536.  join_tile: row-major over the triangle; join_slot_tile: the order the kernel runs
// (bands of tile rows, column by column inside a band).  Host code, no device needed.
extern "C" {
int mmrag_internal_join_tile(int64_t T, int64_t id, int64_t *ti, int64_t *tj);
int mmrag_internal_join_slot_tile(int64_t T, int64_t slot, int64_t *ti, int64_t *tj);
}

// test-only export of the lexical leg's path thresholds (lexical.hip): SCORE_R, SCORE_TERMS, SORT_LDS, SORT_GRID and the
// scan's terms per step.  Host code, no device needed.
extern "C" {
int mmrag_internal_lexical_limits(int *score_rows, int *score_terms, int *sort_lds, int *sort_grid, int *scan_terms);
}

// test-only export of the significant-terms kernel's sizes (terms.hip): groups per launch, term ids per workgroup, the
// longest postings list one wave takes alone and the workgroup's stride over a longer one.  Host code, no device needed.
extern "C" {
int mmrag_internal_terms_limits(int *groups, int *block_terms, int *wave_limit, int *block_stride);
}

// test-only export of the fuzzy term matcher's sizes (fuzzy.hip): terms per workgroup, patterns per LDS tile, the
// longest matched term, the most expansions and the code points of a term tile kept in LDS.  Host code, no device needed.
extern "C" {
int mmrag_internal_fuzzy_limits(int *term_tile, int *pattern_tile, int *max_len, int *max_expansions, int *stage_cps);
}

// test-only export of the learned sparse leg's path sizes (sparse_expand.hip): rows per impact scoring workgroup
// (sparse_score.hip), chunk pieces the pool folds per pair of barriers, the longest run of vocabulary tiles a pool
// workgroup takes, threads (terms per step) of a select workgroup and the pair tile's rows.  Host code, no device needed.
extern "C" {
int mmrag_internal_sparse_limits(int *impact_rows, int *pool_batch, int *pool_vrun, int *select_terms, int *tile_rows);
}
namespace mmrag_impl {
int impact_block_rows();   // sparse_score.hip's IMP_R
}

// the cross-encoder's classification head (cross_head.hip), shared by the fp16 and fp32 forwards
namespace mmrag_impl {
size_t cls_head_workspace_bytes(int B, int H, int NL);
int cls_head_counters(int B);
int *cls_head_counter_ptr(void *ws, int B, int H, int NL);
int launch_cls_head_f32(const float *cls, const float *wp, const float *bp, const float *wc, const float *bc, float *out,
                        int B, int H, int NL, void *ws, hipStream_t s);
}  // namespace mmrag_impl

// the extractive reader's span head (span_head.hip): mmrag_span_select's checks and launch, also the tail of
// mmrag_reader_forward (encoder.hip)
namespace mmrag_impl {
int launch_span_select(const void *hidden, int ld, int H, const float *qa_w, const float *qa_b, const int32_t *cu_seqlens,
                       const int32_t *ctx_start, const int32_t *ctx_len, int64_t T, int B, int max_answer_tokens,
                       int n_best, int32_t *out_span, float *out_score, float *out_null, float *out_lse,
                       float *out_logits, hipStream_t s);
}  // namespace mmrag_impl
