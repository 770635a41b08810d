// The body of the slab-ring kernel (shape of the computation: search.hip's header), once.  Included textually inside
// the __HIP_DEVICE_COMPILE__ block of cosine_topk_kernel (search.hip) and cosine_topk_f8_kernel (search_f8.hip), with
// the compile-time names DT, WN, K, NSTAGE, NW, SEEDED and the parameter `const KParams p` in scope.  Textual on
// purpose: the instruction streams of both families are pinned by hash (tests/test_deep_topk_cpu.py,
// tests/test_f8_cpu.py), and a function template around this body moved them (DESIGN.md 3.1).
//
// What DT == MMRAG_F8E4M3 changes, each behind `if constexpr`: the k-step body (block-scaled FP8 MFMA); selection runs
// in accumulator units (2^16 x the score), so thr0 is scaled by 2^16 where it enters and a score by 2^-16 (exact)
// where it leaves; a wait between a tile's last MFMA and the epilogue; no WN == 8 shape.
    constexpr int WM = NW / WN;          // waves along corpus rows
    constexpr int RM = 8 / WM;           // 32-row blocks per wave  (== WN)
    constexpr int QROWS = 32 * WN;
    constexpr int STAGE = CORPUS_STAGE + QROWS * SLAB;
    constexpr int CLOADS = 32 / NW;      // 1 KiB DMA instructions per wave for the corpus slab
    constexpr int QLOADS = (4 * WN) / NW; // ... and for the Q slab
    constexpr int LOADS = CLOADS + QLOADS;  // per wave per ring item
    static_assert(CLOADS >= 1 && QLOADS >= 1 && CLOADS * NW == 32 && QLOADS * NW == 4 * WN, "piece split");
    static_assert(WN == 2 || WN == 4 || (WN == 8 && DT != MMRAG_F8E4M3), "WN");  // FP8 has no WN == 8 shape
    static_assert(NSTAGE >= 2 && NSTAGE <= 4, "NSTAGE");
    static_assert(NSTAGE * STAGE <= 160 * 1024, "LDS");

    __shared__ __attribute__((aligned(1024))) char smem[NSTAGE * STAGE];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WN;
    const int wn = wave % WN;
    const int r32 = lane & 31;
    const int h = lane >> 5;

    const unsigned RB = p.row_bytes;
    const int nk = (int)(RB / SLAB);
    // 1-D grid of walkers * query_groups workgroups, query group major: the query groups of one walker sit
    // walkers (a multiple of 8) ids apart, i.e. on the SAME XCD, and stream the same corpus tiles at about
    // the same time -- one HBM fetch, the other groups hit that XCD's L2 (batches above 256 queries)
    const int walkers = p.walkers;
    const int bx = (int)blockIdx.x % walkers;
    const int by = (int)blockIdx.x / walkers;
    const int q0 = by * QROWS;
    const int my_tiles = (p.n_tiles - bx + walkers - 1) / walkers;
    const int n_items = my_tiles * nk;
    // corpus tile of walk position i: tile0 + bx + i * walkers (filter mode: times tile_stride, a strided sample).
    // Written out at each use: a helper lambda changes the register allocation of the list kernels.

    // ---- DMA descriptors ------------------------------------------------------------------
    const long long q_rows_left = (long long)p.B - q0;
    const unsigned q_bytes = (unsigned)((q_rows_left < QROWS ? q_rows_left : QROWS) * (long long)RB);
    const __amdgpu_buffer_rsrc_t rsrc_q =
        __builtin_amdgcn_make_buffer_rsrc((void *)(p.q + (size_t)q0 * RB), 0, q_bytes, 0x00020000);

    // per-lane source offsets (row * RB + swizzled chunk * 16) for this wave's DMA instructions
    const int dma_row = lane >> 3;        // row inside an 8-row (1 KiB) LDS piece
    const int dma_slot = lane & 7;        // 16-byte slot inside the 128-byte LDS row
    unsigned c_off[CLOADS];
#pragma unroll
    for (int i = 0; i < CLOADS; ++i) {
        const int row = (wave * CLOADS + i) * 8 + dma_row;
        c_off[i] = (unsigned)row * RB + (unsigned)((dma_slot ^ ((row >> 1) & 7)) * 16);
    }
    unsigned q_off[QLOADS];
#pragma unroll
    for (int i = 0; i < QLOADS; ++i) {
        const int row = (wave * QLOADS + i) * 8 + dma_row;
        q_off[i] = (unsigned)row * RB + (unsigned)((dma_slot ^ ((row >> 1) & 7)) * 16);
    }

    int is_tile = 0, is_k = 0;  // issue cursor: (index among my tiles, k slab)
    auto issue = [&](int stage_idx) {
        const long long tile = K == 0 ? (long long)p.tile0 + (long long)(bx + is_tile * walkers) * p.tile_stride
                                      : (long long)p.tile0 + bx + (long long)is_tile * walkers;
        const long long row0 = tile * TM;
        const long long rows_left = p.n - row0;
        const unsigned c_bytes = (unsigned)((rows_left < TM ? rows_left : (long long)TM) * (long long)RB);
        const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(p.corpus + (size_t)row0 * RB), 0, c_bytes, 0x00020000);
        char *st = smem + stage_idx * STAGE;
        const unsigned koff = (unsigned)is_k * SLAB;
        // corpus rows are read exactly once, by this CU only: non-temporal (aux = 2) keeps them from
        // displacing the query slab that every workgroup re-reads from L2 (A/B: -2 % at B=256, -5 % at B<=128)
        if (p.share_l2) {
#pragma unroll
            for (int i = 0; i < CLOADS; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_c, (lds_ptr_t)(st + (wave * CLOADS + i) * 1024), 16,
                                                         c_off[i] + koff, 0, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < CLOADS; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_c, (lds_ptr_t)(st + (wave * CLOADS + i) * 1024), 16,
                                                         c_off[i] + koff, 0, 0, 2);
        }
#pragma unroll
        for (int i = 0; i < QLOADS; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsrc_q, (lds_ptr_t)(st + CORPUS_STAGE + (wave * QLOADS + i) * 1024), 16, q_off[i] + koff, 0,
                0, 0);
        if (++is_k == nk) {
            is_k = 0;
            ++is_tile;
        }
    };

    // ---- accumulators, lists ---------------------------------------------------------------
    f32x16_t acc[RM];
    auto init_acc = [&](int tile_idx) {
        const long long tile = K == 0 ? (long long)p.tile0 + (long long)(bx + tile_idx * walkers) * p.tile_stride
                                      : (long long)p.tile0 + bx + (long long)tile_idx * walkers;
        const long long row0 = tile * TM + (long long)wm * (RM * 32);
        const bool ragged = row0 + RM * 32 > p.n;
        if (!ragged && p.alive_bits == nullptr) {
#pragma unroll
            for (int b = 0; b < RM; ++b)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[b][j] = 0.0f;
            return;
        }
#pragma unroll
        for (int b = 0; b < RM; ++b) {
            const long long brow = row0 + b * 32;
            unsigned bits = 0xffffffffu;
            if (p.alive_bits != nullptr && brow < p.n) bits = p.alive_bits[brow >> 5];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int rr = (j & 3) + 8 * (j >> 2) + 4 * h;
                const bool ok = (brow + rr < p.n) && ((bits >> rr) & 1u);
                acc[b][j] = ok ? 0.0f : NEG_INF;
            }
        }
    };

    TopList<(K > 0 ? K : 1)> best;
    best.init();
    float thr = NEG_INF;
    if (q0 + wn * 32 + r32 >= p.B)
        thr = INFINITY;  // padding query slot: its all-zero scores must never open the insertion path
    else if (p.thr0 != nullptr) {
        thr = p.thr0[q0 + wn * 32 + r32];
        if constexpr (DT == MMRAG_F8E4M3) thr *= ACC_PER_SCORE;  // thresholds arrive in score units, exact scaling
    }
    if constexpr (K == 0) thr = fmaxf(thr, -__FLT_MAX__);  // masked rows (-inf) never pass the filter

    // ---- fragment addresses (bytes inside a stage) ------------------------------------------
    const int sw = (r32 >> 1) & 7;
    const int a_base = (wm * RM * 32 + r32) * SLAB;
    const int b_base = CORPUS_STAGE + (wn * 32 + r32) * SLAB;

    // ---- prologue ---------------------------------------------------------------------------
    int issued = 0;
    for (; issued < NSTAGE - 1 && issued < n_items; ++issued) issue(issued);
    init_acc(0);

    int tile_idx = 0, ks = 0;
    for (int it = 0; it < n_items; ++it) {
        wait_items<LOADS, NSTAGE - 2>(issued - it - 1);
        __builtin_amdgcn_s_barrier();
        if (issued < n_items) {
            issue(issued % NSTAGE);
            ++issued;
        }
        const char *st = smem + (it % NSTAGE) * STAGE;

        if constexpr (DT == MMRAG_F8E4M3) {
            // one 128-byte slab = 128 E4M3 elements of K = two 32x32x64 block-scaled MFMAs (format 0 = E4M3, every
            // scale byte 127 = 1.0).  Per MFMA a lane holds 32 bytes of its row: the chunk pair (4m + 2h, 4m + 2h + 1).
            // A and B use the same lane-to-k map, so which 32 of the 64 k a half-wave holds is the hardware's business.
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int o0 = ((4 * m + 2 * h) ^ sw) * 16, o1 = ((4 * m + 2 * h + 1) ^ sw) * 16;
                const i32x4_t q0v = *(const i32x4_t *)(st + b_base + o0), q1v = *(const i32x4_t *)(st + b_base + o1);
                const i32x8_t bq = __builtin_shufflevector(q0v, q1v, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int b = 0; b < RM; ++b) {
                    const i32x4_t c0v = *(const i32x4_t *)(st + a_base + b * (32 * SLAB) + o0);
                    const i32x4_t c1v = *(const i32x4_t *)(st + a_base + b * (32 * SLAB) + o1);
                    const i32x8_t ac = __builtin_shufflevector(c0v, c1v, 0, 1, 2, 3, 4, 5, 6, 7);
                    acc[b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ac, bq, acc[b], 0, 0, 0, 0x7f7f7f7f, 0,
                                                                             0x7f7f7f7f);
                }
            }
        } else if constexpr (DT == MMRAG_F32 && WN >= 4) {
            // fp32 storage, more than 64 queries (BASELINE config 2 at B = 256): the exact f32 MFMA runs at 1/16 of
            // the bf16 rate and this shape is matrix-bound, so every operand fragment is split on the fly into two
            // bf16 terms (x = hi + lo up to 2^-17 |x|) and the product is taken as hi*hi + hi*lo + lo*hi in fp32
            // accumulators: |score error| <= 3 * 2^-17 * sum|q_i c_i| + 2^-16 <= 4e-5 for unit vectors, inside the
            // 1e-4 parity bound (tests/test_search_gpu.py::test_fp32_split_*), at 3/16 of the f32-MFMA cost.
            // Batches of <= 64 queries are HBM- / launch-bound and keep the exact f32 MFMA below.
            auto split = [&](const char *at0, const char *at1, bf16x8_t &hi, bf16x8_t &lo) {
                const f32x4_t x0 = *(const f32x4_t *)at0, x1 = *(const f32x4_t *)at1;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float x = i < 4 ? x0[i] : x1[i - 4];
                    const __bf16 hb = (__bf16)x;
                    hi[i] = hb;
                    lo[i] = (__bf16)(x - (float)hb);
                }
            };
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {          // two 16-deep bf16 k-steps per 128-byte fp32 slab
                const int o0 = ((4 * s2 + 2 * h) ^ sw) * 16, o1 = ((4 * s2 + 2 * h + 1) ^ sw) * 16;
                bf16x8_t qh, ql;
                split(st + b_base + o0, st + b_base + o1, qh, ql);
#pragma unroll
                for (int b = 0; b < RM; ++b) {
                    bf16x8_t ch, cl;
                    split(st + a_base + b * (32 * SLAB) + o0, st + a_base + b * (32 * SLAB) + o1, ch, cl);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cl, qh, acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch, ql, acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch, qh, acc[b], 0, 0, 0);
                }
            }
        } else if constexpr (DT == MMRAG_F32) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int off = ((2 * m + h) ^ sw) * 16;
                const f32x4_t bq = *(const f32x4_t *)(st + b_base + off);
#pragma unroll
                for (int b = 0; b < RM; ++b) {
                    const f32x4_t ac = *(const f32x4_t *)(st + a_base + b * (32 * SLAB) + off);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[i], bq[i], acc[b], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int off = ((2 * m + h) ^ sw) * 16;
                if constexpr (DT == MMRAG_F16) {
                    const half8_t bq = *(const half8_t *)(st + b_base + off);
#pragma unroll
                    for (int b = 0; b < RM; ++b) {
                        const half8_t ac = *(const half8_t *)(st + a_base + b * (32 * SLAB) + off);
                        acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ac, bq, acc[b], 0, 0, 0);
                    }
                } else {
                    const bf16x8_t bq = *(const bf16x8_t *)(st + b_base + off);
#pragma unroll
                    for (int b = 0; b < RM; ++b) {
                        const bf16x8_t ac = *(const bf16x8_t *)(st + a_base + b * (32 * SLAB) + off);
                        acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ac, bq, acc[b], 0, 0, 0);
                    }
                }
            }
        }

        if (++ks == nk) {
            if constexpr (DT == MMRAG_F8E4M3) {
                // STOP-GAP for a suspected compiler wait-state shortfall (hipcc of ROCm 7.2.0, AMD clang 22.0.0git
                // roc-7.2.0 7b800a19): it spaces the epilogue's first accumulator reads 18 wait states after the last
                // v_mfma_scale_f32_32x32x64_f8f6f4 (s_nop 15, s_nop 0, one VALU), the figure for a 16-pass non-XDL
                // result; a 16-pass XDL result needs 19.  Observed on the MI355X: the LAST accumulator register of the
                // LAST row block, which the generated filter epilogue happens to read second, came back stale and the
                // row was dropped (exact-data deep search, 64-query plan: only in-block rows 27 / 31 of a wave's last
                // block went missing; gone with this wait).  The diagnosis is inferred from that pattern, not confirmed
                // by the vendor.  s_nop would be counted by the hazard recogniser and taken off its own padding, so the
                // wave sleeps instead (s_sleep 1, about 64 clocks: far more than the one missing state, though not an
                // architectural guarantee): once per 256-row tile.  tests/test_f8_cpu.py checks that it stays between
                // the tile's last MFMA and the first accumulator read; test_exact_data_bounded_deep_two_block_waves
                // pins the behaviour.
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_sleep(1);
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---- epilogue: lane-local top-K over this wave's 32*RM rows of the tile ----------
            ks = 0;
            const long long tile = K == 0 ? (long long)p.tile0 + (long long)(bx + tile_idx * walkers) * p.tile_stride
                                          : (long long)p.tile0 + bx + (long long)tile_idx * walkers;
            const int row_base = (int)(tile * TM) + wm * (RM * 32) + 4 * h;
            if constexpr (K == 0) {
                // filter mode: count this lane's survivors, reserve their slots with one returning atomic, append.
                // The counter keeps the true count; slots at or past deep_cap are not written.
                int n_pass = 0;
#pragma unroll
                for (int b = 0; b < RM; ++b)
#pragma unroll
                    for (int j = 0; j < 16; ++j) n_pass += acc[b][j] >= thr ? 1 : 0;
                if (__builtin_amdgcn_ballot_w64(n_pass > 0) != 0ull) {
                    const int qg = q0 + wn * 32 + r32;  // n_pass > 0 only for real queries (padding: thr = +inf)
                    unsigned at = 0;
                    if (n_pass > 0) at = atomicAdd(p.deep_cnt + qg, (unsigned)n_pass);
                    float *bs = p.cand_s + (size_t)qg * p.deep_cap;
                    int *br = p.cand_r + (size_t)qg * p.deep_cap;
                    const unsigned cap = (unsigned)p.deep_cap;
#pragma unroll
                    for (int b = 0; b < RM; ++b) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const float m4 = fmaxf(fmaxf(acc[b][4 * g], acc[b][4 * g + 1]),
                                                   fmaxf(acc[b][4 * g + 2], acc[b][4 * g + 3]));
                            if (__builtin_amdgcn_ballot_w64(m4 >= thr) != 0ull) {
#pragma unroll
                                for (int i = 0; i < 4; ++i) {
                                    const float s = acc[b][4 * g + i];
                                    if (s >= thr) {
                                        if (at < cap) {
                                            if constexpr (DT == MMRAG_F8E4M3) bs[at] = s * SCORE_PER_ACC;
                                            else bs[at] = s;
                                            br[at] = row_base + b * 32 + i + 8 * g;
                                        }
                                        ++at;
                                    }
                                }
                            }
                        }
                    }
                }
            } else if constexpr (K > 5) {
                // deep lists: one (not unrolled) insertion body per 4-row group keeps the code small
                // (a K=20 insertion is ~100 instructions; 128 unrolled copies would not fit the I-cache)
#pragma unroll
                for (int b = 0; b < RM; ++b) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float a0 = acc[b][4 * g], a1 = acc[b][4 * g + 1];
                        const float a2 = acc[b][4 * g + 2], a3 = acc[b][4 * g + 3];
                        if (__builtin_amdgcn_ballot_w64(fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)) >= thr) != 0ull) {
#pragma clang loop unroll(disable)
                            for (int i = 0; i < 4; ++i) {
                                const float s = i == 0 ? a0 : (i == 1 ? a1 : (i == 2 ? a2 : a3));
                                const bool pass = s >= thr;
                                if (__builtin_amdgcn_ballot_w64(pass) != 0ull) {
                                    best.insert_strict(pass ? s : NEG_INF, row_base + b * 32 + i + 8 * g);
                                    thr = fmaxf(thr, best.v[K - 1]);
                                }
                            }
                        }
                    }
                }
            } else if constexpr (SEEDED) {
                // thresholds are warm from the first element (sample pre-pass): test 4 rows at a time
#pragma unroll
                for (int b = 0; b < RM; ++b) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float m4 = fmaxf(fmaxf(acc[b][4 * g], acc[b][4 * g + 1]),
                                               fmaxf(acc[b][4 * g + 2], acc[b][4 * g + 3]));
                        if (__builtin_amdgcn_ballot_w64(m4 >= thr) != 0ull) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const float s = acc[b][4 * g + i];
                                const bool pass = s >= thr;
                                if (__builtin_amdgcn_ballot_w64(pass) != 0ull) {
                                    best.insert_strict(pass ? s : NEG_INF, row_base + b * 32 + i + 8 * g);
                                    thr = fmaxf(thr, best.v[K - 1]);
                                }
                            }
                        }
                    }
                }
            } else {
#pragma unroll
                for (int b = 0; b < RM; ++b) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const float s = acc[b][j];
                        const bool pass = s >= thr;
                        if (__builtin_amdgcn_ballot_w64(pass) != 0ull) {
                            best.insert_strict(pass ? s : NEG_INF, row_base + b * 32 + (j & 3) + 8 * (j >> 2));
                            thr = fmaxf(thr, best.v[K - 1]);
                        }
                    }
                }
            }
            if constexpr (K > 0) {
                // k-th best of the union of the two half-wave lists of this query: a lower bound
                // on the final k-th score, shared by both lanes
                float u = fmaxf(best.v[K - 1], __shfl_xor(best.v[K - 1], 32));
#pragma unroll
                for (int i = 0; i + 1 < K; ++i) u = fmaxf(u, fminf(best.v[i], __shfl_xor(best.v[K - 2 - i], 32)));
                thr = fmaxf(thr, u);
            }
            ++tile_idx;
            if (tile_idx < my_tiles) init_acc(tile_idx);
        }
    }

    // ---- merge the workgroup's WM*2 lists per query through LDS, write ONE list per query -------
    if constexpr (K > 0) {
        constexpr int NL = WM * 2;  // lists per query inside this workgroup
        static_assert(QROWS * NL * K * 8 <= NSTAGE * STAGE, "list merge scratch must fit in the ring");
        __builtin_amdgcn_s_barrier();  // every wave is done reading the ring
        float *ls = (float *)smem;
        int *lr = (int *)(smem + QROWS * NL * K * 4);
        const int ql = wn * 32 + r32;
        const int slot = (ql * NL + wm * 2 + h) * K;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if constexpr (DT == MMRAG_F8E4M3) ls[slot + i] = best.v[i] * SCORE_PER_ACC;  // -inf stays -inf
            else ls[slot + i] = best.v[i];
            lr[slot + i] = best.r[i];
        }
        __syncthreads();
        const int t = threadIdx.x;
        if (t < QROWS && q0 + t < p.B) {
            // every list is sorted (score desc, row asc) with its empty slots last: list 0 is taken as
            // it stands, and a list is left at its first entry that does not make the merged top-K
            TopList<K> m;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                m.v[i] = ls[t * NL * K + i];
                m.r[i] = lr[t * NL * K + i];
            }
            for (int l = 1; l < NL; ++l) {
                for (int i = 0; i < K; ++i) {
                    const float x = ls[(t * NL + l) * K + i];
                    const int xr = lr[(t * NL + l) * K + i];
                    if (xr == INT_MAX || !better(x, xr, m.v[K - 1], m.r[K - 1])) break;
                    m.insert_ordered(x, xr);
                }
            }
            const size_t base = ((size_t)(q0 + t) * p.n_lists + bx) * K;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                p.cand_s[base + i] = m.v[i];
                p.cand_r[base + i] = m.r[i];
            }
        }
    }
