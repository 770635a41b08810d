// What the two translation units of the slab-ring kernel (search.hip: fp32 / fp16 / bf16; search_f8.hip: FP8) need
// around its one body, slab_ring_body.inc.  Internal, gfx950 only.
#pragma once
#include "search_shared.h"

namespace mmrag_impl {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));

constexpr int TM = 256;            // corpus rows per tile
constexpr int CORPUS_STAGE = TM * SLAB;  // 32 KiB

// FP8 (MMRAG_F8E4M3): both operands carry the constant scale 2^8, so an accumulator is 2^16 x the score
constexpr float SCORE_PER_ACC = 0x1p-16f, ACC_PER_SCORE = 0x1p16f;

}  // namespace mmrag_impl
