"""ctypes binding of libmmrag.so (include/mmrag.h) -- the only way the package computes.

There is no CPU / PyTorch-eager fallback: if the shared library is missing or a call
returns a non-zero status this module raises.  torch is used for device memory and the
current HIP stream only.
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p
from typing import Optional, Tuple

import numpy as np
import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libmmrag.so")

F32, F16, BF16, F8E4M3 = 0, 1, 2, 3
MAX_K = 20
MAX_K_DEEP = 4096   # mmrag_cosine_topk_deep
MAX_MMR_CANDIDATES = 1024   # mmrag_mmr_select (MMRAG_MAX_MMR_CANDIDATES)
MAX_RESCORE_CANDIDATES = 4096   # mmrag_rescore_topk (MMRAG_MAX_RESCORE_CANDIDATES)
# mmrag_group_select (MMRAG_MAX_GROUP_CANDIDATES, MMRAG_MAX_GROUPS, MMRAG_MAX_GROUP_SIZE)
MAX_GROUP_CANDIDATES, MAX_GROUPS, MAX_GROUP_SIZE = 4096, 256, 16
# mmrag_fuse_select (MMRAG_MAX_FUSE_LISTS, MMRAG_MAX_FUSE_CANDIDATES, MMRAG_MAX_FUSE_RESULTS, MMRAG_FUSE_RRF / _MAX)
MAX_FUSE_LISTS, MAX_FUSE_CANDIDATES, MAX_FUSE_RESULTS = 16, 256, 4096
FUSE_METHODS = {"rrf": 0, "max": 1}
MAX_JOIN_PAIRS = 1 << 26   # mmrag_sim_join (MMRAG_MAX_JOIN_PAIRS)
MAX_CLUSTERS = 4096   # mmrag_kmeans_assign / mmrag_cluster_sums (MMRAG_MAX_CLUSTERS)
MAX_SCOPE_GROUPS = 64   # mmrag_scoped_topk (MMRAG_MAX_SCOPE_GROUPS)
# mmrag_filter_eval (MMRAG_MAX_FILTER_OPS, MMRAG_MAX_FILTER_SET, MMRAG_MAX_FILTER_COLUMNS)
MAX_FILTER_OPS, MAX_FILTER_SET, MAX_FILTER_COLUMNS = 32, 64, 16
MAX_FACET_COLUMNS = 4   # mmrag_range_scan (MMRAG_MAX_FACET_COLUMNS)
MAX_RELATED_ROWS, MAX_RELATED_SETS = 8192, 64   # mmrag_related_groups (MMRAG_MAX_RELATED_ROWS, MMRAG_MAX_RELATED_SETS)
MAX_RECOMMEND_EXAMPLES = 16  # mmrag_recommend_topk (MMRAG_MAX_RECOMMEND_EXAMPLES)
# mmrag_maxsim_scores (MMRAG_MAX_LATE_QUERY_TOKENS, MMRAG_MAX_LATE_DOC_TOKENS)
MAX_LATE_QUERY_TOKENS, MAX_LATE_DOC_TOKENS = 128, 512
MAX_LATE_PAIRS = 65535
MAX_LATE_QUESTIONS = 4096   # mmrag_maxsim_topk (MMRAG_MAX_LATE_QUESTIONS)
# mmrag_maxsim_windows (MMRAG_LATE_WINDOW_TOKENS, MMRAG_MAX_LATE_WINDOWS)
LATE_WINDOW_TOKENS, MAX_LATE_WINDOWS = 16, 32
# mmrag_summary_select (MMRAG_MAX_SUMMARY_SENTENCES, MMRAG_MAX_SUMMARY_ITERATIONS)
MAX_SUMMARY_SENTENCES, MAX_SUMMARY_ITERATIONS = 128, 64
MAX_CHUNK_SENTENCES = 64   # mmrag_chunk_boundaries (MMRAG_MAX_CHUNK_SENTENCES)
# mmrag_attribute (MMRAG_MAX_CLAIMS, MMRAG_MAX_EVIDENCE, MMRAG_MAX_ATTR_SOURCES, MMRAG_MAX_CITATIONS)
MAX_CLAIMS, MAX_EVIDENCE, MAX_ATTR_SOURCES, MAX_CITATIONS = 128, 4096, 64, 8
# mmrag_span_select / mmrag_reader_forward (MMRAG_MAX_READER_TOKENS, MMRAG_MAX_ANSWER_TOKENS, MMRAG_MAX_READER_SPANS)
MAX_READER_TOKENS, MAX_ANSWER_TOKENS, MAX_READER_SPANS = 512, 64, 8
_DT2TORCH = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16, F8E4M3: torch.float8_e4m3fn}
_TORCH2DT = {v: k for k, v in _DT2TORCH.items()}

_lib = None
_lock = threading.Lock()


class MMRagNativeError(RuntimeError):
    pass


def _declare(lib):
    lib.mmrag_abi_version.restype = c_int
    lib.mmrag_last_error.restype = c_char_p
    lib.mmrag_padded_dim.restype = c_int64
    lib.mmrag_padded_dim.argtypes = [c_int, c_int]
    lib.mmrag_cosine_topk_workspace_bytes.restype = c_size_t
    lib.mmrag_cosine_topk_workspace_bytes.argtypes = [c_int, c_int64, c_int]
    lib.mmrag_cosine_topk.restype = c_int
    lib.mmrag_cosine_topk.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int, c_int,
                                      c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_cosine_topk_lists.restype = c_int
    lib.mmrag_cosine_topk_lists.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int, c_int,
                                            c_void_p, c_void_p, c_size_t, c_void_p]
    # debug form of mmrag_cosine_topk_lists (kernel-shape switches; csrc/search.hip, not in include/mmrag.h)
    lib.mmrag_internal_search_uses_qs.restype = c_int
    lib.mmrag_internal_search_uses_qs.argtypes = [c_int, c_int64, c_int64, c_int, c_int]
    lib.mmrag_internal_cosine_topk_lists_ex.restype = c_int
    lib.mmrag_internal_cosine_topk_lists_ex.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int,
                                                        c_int, c_void_p, c_void_p, c_size_t, c_void_p, ctypes.c_uint]
    lib.mmrag_cosine_topk_select.restype = c_int
    lib.mmrag_cosine_topk_select.argtypes = [c_int, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.mmrag_cosine_topk_deep_workspace_bytes.restype = c_size_t
    lib.mmrag_cosine_topk_deep_workspace_bytes.argtypes = [c_int, c_int64, c_int]
    lib.mmrag_cosine_topk_deep.restype = c_int
    lib.mmrag_cosine_topk_deep.argtypes = lib.mmrag_cosine_topk.argtypes
    # debug form of mmrag_cosine_topk_deep (csrc/search_deep.hip, not in include/mmrag.h): switches + candidate capacity
    lib.mmrag_internal_cosine_topk_deep_ex.restype = c_int
    lib.mmrag_internal_cosine_topk_deep_ex.argtypes = lib.mmrag_cosine_topk.argtypes + [ctypes.c_uint, c_int64]
    lib.mmrag_rescore_topk.restype = c_int
    lib.mmrag_rescore_topk.argtypes = [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p]
    lib.mmrag_merge_topk.restype = c_int
    lib.mmrag_merge_topk.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.mmrag_merge_topk_host.restype = c_int
    lib.mmrag_merge_topk_host.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.mmrag_merge_topk_host_packed.restype = c_int
    lib.mmrag_merge_topk_host_packed.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.mmrag_append_rows.restype = c_int
    lib.mmrag_append_rows.argtypes = [c_void_p, c_int64, c_int64, c_int, c_int64, c_void_p, c_int64, c_int, c_void_p]
    lib.mmrag_gather_rows.restype = c_int
    lib.mmrag_gather_rows.argtypes = [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]
    lib.mmrag_fetch_rows_f32.restype = c_int
    lib.mmrag_fetch_rows_f32.argtypes = [c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p]
    lib.mmrag_device_info.restype = c_int
    lib.mmrag_device_info.argtypes = [ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int64)]
    lib.mmrag_bench_stream_copy.restype = c_int
    lib.mmrag_bench_stream_copy.argtypes = [c_void_p, c_void_p, c_int64, c_void_p]
    lib.mmrag_bench_mfma_f16.restype = c_int
    lib.mmrag_bench_mfma_f16.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(c_int64), c_void_p]
    lib.mmrag_bench_mfma_f16_16x16x32.restype = c_int
    lib.mmrag_bench_mfma_f16_16x16x32.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(c_int64), c_void_p]
    lib.mmrag_bench_stream_read.restype = c_int
    lib.mmrag_bench_stream_read.argtypes = [c_void_p, c_int64, c_void_p, c_void_p]
    lib.mmrag_bench_stream_write.restype = c_int
    lib.mmrag_bench_stream_write.argtypes = [c_void_p, c_int64, c_void_p]
    lib.mmrag_copy_to_host_async.restype = c_int
    lib.mmrag_copy_to_host_async.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_encoder_workspace_bytes.restype = c_size_t
    lib.mmrag_encoder_workspace_bytes.argtypes = [c_void_p, c_int64, c_int]
    lib.mmrag_encoder_forward.restype = c_int
    lib.mmrag_encoder_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int,
                                          c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_encoder_f32_workspace_bytes.restype = c_size_t
    lib.mmrag_encoder_f32_workspace_bytes.argtypes = [c_void_p, c_int64, c_int]
    lib.mmrag_encoder_forward_f32.restype = c_int
    lib.mmrag_encoder_forward_f32.argtypes = lib.mmrag_encoder_forward.argtypes
    lib.mmrag_linear_f32.restype = c_int
    lib.mmrag_linear_f32.argtypes = [c_void_p, c_int64, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    lib.mmrag_vit_forward.restype = c_int
    lib.mmrag_vit_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                      c_void_p]
    lib.mmrag_wordpiece_create.restype = c_void_p
    lib.mmrag_wordpiece_create.argtypes = [c_void_p, c_void_p, c_int, c_int]
    lib.mmrag_wordpiece_destroy.restype = None
    lib.mmrag_wordpiece_destroy.argtypes = [c_void_p]
    lib.mmrag_wordpiece_encode_batch.restype = c_int
    lib.mmrag_wordpiece_encode_batch.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int]
    lib.mmrag_clip_bpe_create.restype = c_void_p
    lib.mmrag_clip_bpe_create.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int]
    lib.mmrag_clip_bpe_destroy.restype = None
    lib.mmrag_clip_bpe_destroy.argtypes = [c_void_p]
    lib.mmrag_clip_bpe_encode_batch.restype = c_int
    lib.mmrag_clip_bpe_encode_batch.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int]
    lib.mmrag_resample_ksize.restype = c_int
    lib.mmrag_resample_ksize.argtypes = [c_int, c_int]
    lib.mmrag_resample_coeffs.restype = c_int
    lib.mmrag_resample_coeffs.argtypes = [c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.mmrag_resize_crop_u8.restype = c_int
    lib.mmrag_resize_crop_u8.argtypes = [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                         c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.mmrag_linear_f16.restype = c_int
    lib.mmrag_linear_f16.argtypes = [c_void_p, c_int64, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                     c_void_p]
    lib.mmrag_layernorm_f16.restype = c_int
    lib.mmrag_layernorm_f16.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p]
    lib.mmrag_embed_ln_f16.restype = c_int
    lib.mmrag_embed_ln_f16.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int64, c_int, c_int, c_int, c_float, c_void_p]
    lib.mmrag_attention_f16.restype = c_int
    lib.mmrag_attention_f16.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]
    lib.mmrag_pool_normalize_f16.restype = c_int
    lib.mmrag_pool_normalize_f16.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                             c_void_p]
    # test-only entry points (not in include/mmrag.h): single kernels of the folded-LayerNorm and fp32 forwards
    lib.mmrag_internal_linear_f16_norms.restype = c_int
    lib.mmrag_internal_linear_f16_norms.argtypes = [c_void_p, c_int64, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                                    c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_void_p]
    lib.mmrag_internal_attention_f32.restype = c_int
    lib.mmrag_internal_attention_f32.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]
    lib.mmrag_internal_layernorm_f32.restype = c_int
    lib.mmrag_internal_layernorm_f32.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p]
    lib.mmrag_internal_pool_norm_f32.restype = c_int
    lib.mmrag_internal_pool_norm_f32.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                                 c_void_p]
    # test-only entry points of the CLIP towers' own kernels (csrc/encoder.hip, not in include/mmrag.h)
    lib.mmrag_internal_patchify.restype = c_int
    lib.mmrag_internal_patchify.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]
    lib.mmrag_internal_vit_assemble_ln.restype = c_int
    lib.mmrag_internal_vit_assemble_ln.argtypes = [c_void_p] * 6 + [c_int, c_int, c_int, c_float, c_void_p]
    lib.mmrag_internal_normalize_rows.restype = c_int
    lib.mmrag_internal_normalize_rows.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p]
    lib.mmrag_internal_pool_f16.restype = c_int
    lib.mmrag_internal_pool_f16.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]
    # cross-encoder (include/mmrag.h) and its test-only exports
    lib.mmrag_cross_encoder_workspace_bytes.restype = c_size_t
    lib.mmrag_cross_encoder_workspace_bytes.argtypes = [c_void_p, c_int64, c_int]
    lib.mmrag_cross_encoder_f32_workspace_bytes.restype = c_size_t
    lib.mmrag_cross_encoder_f32_workspace_bytes.argtypes = [c_void_p, c_int64, c_int]
    lib.mmrag_cross_encoder_forward.restype = c_int
    lib.mmrag_cross_encoder_forward.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_int64, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_cross_encoder_forward_f32.restype = c_int
    lib.mmrag_cross_encoder_forward_f32.argtypes = lib.mmrag_cross_encoder_forward.argtypes
    lib.mmrag_span_select.restype = c_int
    lib.mmrag_span_select.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                      c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.mmrag_reader_workspace_bytes.restype = c_size_t
    lib.mmrag_reader_workspace_bytes.argtypes = [c_void_p, c_int64, c_int]
    lib.mmrag_reader_forward.restype = c_int
    lib.mmrag_reader_forward.argtypes = [c_void_p] * 8 + [c_int64, c_int, c_int, c_int, c_int] + [c_void_p] * 6 + \
        [c_size_t, c_void_p]
    lib.mmrag_wordpiece_encode_pairs.restype = c_int
    lib.mmrag_wordpiece_encode_pairs.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                                 c_void_p, c_void_p, c_int]
    lib.mmrag_internal_embed_types_ln_f16.restype = c_int
    lib.mmrag_internal_embed_types_ln_f16.argtypes = [c_void_p] * 9 + [c_int64, c_int, c_int, c_int, c_int, c_float,
                                                                       c_void_p]
    lib.mmrag_internal_embed_types_ln_f32.restype = c_int
    lib.mmrag_internal_embed_types_ln_f32.argtypes = lib.mmrag_internal_embed_types_ln_f16.argtypes
    lib.mmrag_internal_cls_head_f32.restype = c_int
    lib.mmrag_internal_cls_head_f32.argtypes = [c_void_p] * 6 + [c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]
    lib.mmrag_internal_cls_head_workspace_bytes.restype = c_size_t
    lib.mmrag_internal_cls_head_workspace_bytes.argtypes = [c_int, c_int, c_int]
    # MMR selection (csrc/mmr.hip); the _ex form is its debug entry (not in include/mmrag.h)
    lib.mmrag_mmr_select_workspace_bytes.restype = c_size_t
    lib.mmrag_mmr_select_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int]
    lib.mmrag_mmr_select.restype = c_int
    lib.mmrag_mmr_select.argtypes = [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_internal_mmr_select_ex.restype = c_int
    lib.mmrag_internal_mmr_select_ex.argtypes = lib.mmrag_mmr_select.argtypes + [ctypes.c_uint]
    # grouping of hits by a per-row key (csrc/group.hip)
    lib.mmrag_group_select.restype = c_int
    lib.mmrag_group_select.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int64, c_int, c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    # fusion of the ranked lists of query variants (csrc/fuse.hip)
    lib.mmrag_fuse_select.restype = c_int
    lib.mmrag_fuse_select.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    # near-duplicate join (csrc/simjoin.hip); the join_*tile entries are its test-only exports (csrc/mmrag_internal.h)
    lib.mmrag_sim_join.restype = c_int
    lib.mmrag_sim_join.argtypes = [c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p,
                                   c_int64, c_void_p, c_void_p]
    for name in ("mmrag_internal_join_tile", "mmrag_internal_join_slot_tile"):
        getattr(lib, name).restype = c_int
        getattr(lib, name).argtypes = [c_int64, c_int64, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]
    # topic clustering (csrc/kmeans.hip)
    lib.mmrag_kmeans_assign.restype = c_int
    lib.mmrag_kmeans_assign.argtypes = [c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                        c_void_p, c_void_p]
    lib.mmrag_cluster_sums.restype = c_int
    lib.mmrag_cluster_sums.argtypes = [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    # document-scoped top-k (csrc/scoped.hip); the _ex entry adds a candidate capacity (tests, not in include/mmrag.h)
    lib.mmrag_scoped_topk_workspace_bytes.restype = c_size_t
    lib.mmrag_scoped_topk_workspace_bytes.argtypes = [c_int, c_int64, c_int, c_int]
    lib.mmrag_scoped_topk.restype = c_int
    lib.mmrag_scoped_topk.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int, c_int, c_int64,
                                      c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int64,
                                      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_internal_scoped_topk_ex.restype = c_int
    lib.mmrag_internal_scoped_topk_ex.argtypes = lib.mmrag_scoped_topk.argtypes + [c_int64]
    # filtered retrieval (csrc/filtered.hip); the _ex entry adds a candidate capacity, debug switches and the counter of
    # issued items (tests and tools, not in include/mmrag.h)
    lib.mmrag_filter_words.restype = c_int64
    lib.mmrag_filter_words.argtypes = [c_int64]
    lib.mmrag_filter_eval.restype = c_int
    lib.mmrag_filter_eval.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                      c_int64, c_void_p, c_void_p, c_void_p]
    lib.mmrag_filtered_topk_workspace_bytes.restype = c_size_t
    lib.mmrag_filtered_topk_workspace_bytes.argtypes = [c_int, c_int64, c_int]
    lib.mmrag_filtered_topk.restype = c_int
    lib.mmrag_filtered_topk.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int, c_int, c_int64,
                                        c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_internal_filtered_topk_ex.restype = c_int
    lib.mmrag_internal_filtered_topk_ex.argtypes = lib.mmrag_filtered_topk.argtypes + [c_int64, ctypes.c_uint, c_void_p]
    # range scan (csrc/range.hip); the _ex entry adds a candidate capacity and debug switches (tests, not in
    # include/mmrag.h)
    lib.mmrag_range_scan_workspace_bytes.restype = c_size_t
    lib.mmrag_range_scan_workspace_bytes.argtypes = [c_int, c_int64, c_int, c_int]
    lib.mmrag_range_scan.restype = c_int
    lib.mmrag_range_scan.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int, c_void_p, c_int, c_int64,
                                     c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_internal_range_scan_ex.restype = c_int
    lib.mmrag_internal_range_scan_ex.argtypes = lib.mmrag_range_scan.argtypes + [c_int64, ctypes.c_uint]
    # related groups (csrc/related.hip); the _ex entry adds the scan's grid (tests, not in include/mmrag.h)
    lib.mmrag_related_groups_workspace_bytes.restype = c_size_t
    lib.mmrag_related_groups_workspace_bytes.argtypes = [c_int, c_int, c_int64, c_int, c_int]
    lib.mmrag_related_groups.restype = c_int
    lib.mmrag_related_groups.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_int, c_int64, c_int,
                                         c_void_p, c_void_p, c_int, c_void_p, c_float, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_internal_related_groups_ex.restype = c_int
    lib.mmrag_internal_related_groups_ex.argtypes = lib.mmrag_related_groups.argtypes + [c_int64]
    lib.mmrag_internal_candidate_capacity.restype = c_int64
    lib.mmrag_internal_candidate_capacity.argtypes = [c_int]
    lib.mmrag_internal_bound_plan.restype = c_int
    lib.mmrag_internal_bound_plan.argtypes = [c_int64, c_int, c_int64, ctypes.c_uint, c_void_p, c_void_p]
    # boosted top-k (csrc/boosted.hip); the _ex entry adds a candidate capacity and debug switches (tests, not in
    # include/mmrag.h)
    lib.mmrag_boosted_topk_workspace_bytes.restype = c_size_t
    lib.mmrag_boosted_topk_workspace_bytes.argtypes = [c_int, c_int64, c_int]
    lib.mmrag_boosted_topk.restype = c_int
    lib.mmrag_boosted_topk.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int, c_int, c_int64,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                       c_void_p]
    lib.mmrag_internal_boosted_topk_ex.restype = c_int
    lib.mmrag_internal_boosted_topk_ex.argtypes = lib.mmrag_boosted_topk.argtypes + [c_int64, ctypes.c_uint]
    # recommend top-k (csrc/recommend.hip); the _ex entry as the boosted one's
    lib.mmrag_recommend_topk_workspace_bytes.restype = c_size_t
    lib.mmrag_recommend_topk_workspace_bytes.argtypes = [c_int, c_int64, c_int]
    lib.mmrag_recommend_topk.restype = c_int
    lib.mmrag_recommend_topk.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int,
                                         c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_internal_recommend_topk_ex.restype = c_int
    lib.mmrag_internal_recommend_topk_ex.argtypes = lib.mmrag_recommend_topk.argtypes + [c_int64, ctypes.c_uint]
    # late interaction (csrc/encoder.hip token rows, csrc/maxsim.hip)
    lib.mmrag_encoder_tokens_workspace_bytes.restype = c_size_t
    lib.mmrag_encoder_tokens_workspace_bytes.argtypes = [c_void_p, c_int64, c_int, c_int]
    lib.mmrag_encoder_forward_tokens.restype = c_int
    lib.mmrag_encoder_forward_tokens.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int,
                                                 c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_maxsim_scores.restype = c_int
    lib.mmrag_maxsim_scores.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p,
                                        c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                        c_void_p, c_void_p]
    # token store (csrc/maxsim_scan.hip)
    lib.mmrag_maxsim_topk_workspace_bytes.restype = c_size_t
    lib.mmrag_maxsim_topk_workspace_bytes.argtypes = [c_int, c_int64, c_int]
    lib.mmrag_maxsim_topk.restype = c_int
    lib.mmrag_maxsim_topk.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int64,
                                      c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p]
    lib.mmrag_internal_maxsim_topk_ex.restype = c_int
    lib.mmrag_internal_maxsim_topk_ex.argtypes = lib.mmrag_maxsim_topk.argtypes + [c_int, c_int64, ctypes.c_uint, c_int]
    lib.mmrag_internal_maxsim_topk_workspace_bytes_ex.restype = c_size_t
    lib.mmrag_internal_maxsim_topk_workspace_bytes_ex.argtypes = [c_int, c_int64, c_int, c_int, c_int]
    # FP8 token rows: the same entries over E4M3 code rows, and the row encoder (csrc/maxsim.hip, csrc/maxsim_scan.hip)
    lib.mmrag_f8_encode_rows.restype = c_int
    lib.mmrag_f8_encode_rows.argtypes = [c_void_p, c_int, c_int64, c_int, c_int64, c_void_p, c_int64, c_void_p]
    lib.mmrag_maxsim_scores_f8.restype = c_int
    lib.mmrag_maxsim_scores_f8.argtypes = lib.mmrag_maxsim_scores.argtypes
    lib.mmrag_maxsim_topk_f8_workspace_bytes.restype = c_size_t
    lib.mmrag_maxsim_topk_f8_workspace_bytes.argtypes = [c_int, c_int64, c_int]
    lib.mmrag_maxsim_topk_f8.restype = c_int
    lib.mmrag_maxsim_topk_f8.argtypes = lib.mmrag_maxsim_topk.argtypes
    lib.mmrag_internal_maxsim_topk_f8_ex.restype = c_int
    lib.mmrag_internal_maxsim_topk_f8_ex.argtypes = lib.mmrag_internal_maxsim_topk_ex.argtypes
    lib.mmrag_internal_maxsim_topk_f8_workspace_bytes_ex.restype = c_size_t
    lib.mmrag_internal_maxsim_topk_f8_workspace_bytes_ex.argtypes = [c_int, c_int64, c_int, c_int, c_int]
    # answer passages: windowed MaxSim (csrc/maxsim_windows.hip)
    lib.mmrag_maxsim_windows.restype = c_int
    lib.mmrag_maxsim_windows.argtypes = lib.mmrag_maxsim_scores.argtypes[:16] + [c_int, c_void_p, c_void_p, c_void_p,
                                                                                 c_void_p]
    lib.mmrag_maxsim_windows_f8.restype = c_int
    lib.mmrag_maxsim_windows_f8.argtypes = lib.mmrag_maxsim_windows.argtypes
    # learned sparse retrieval (csrc/encoder.hip, csrc/sparse_expand.hip, csrc/sparse_score.hip)
    lib.mmrag_sparse_expand_forward_workspace_bytes.restype = c_size_t
    lib.mmrag_sparse_expand_forward_workspace_bytes.argtypes = [c_void_p, c_int64, c_int]
    lib.mmrag_sparse_expand_forward.restype = c_int
    lib.mmrag_sparse_expand_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                                c_void_p]
    lib.mmrag_sparse_pool_workspace_bytes.restype = c_size_t
    lib.mmrag_sparse_pool_workspace_bytes.argtypes = [c_int64, c_int, c_int]
    lib.mmrag_sparse_pool.restype = c_int
    lib.mmrag_sparse_pool.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_int, c_void_p, c_int, c_int64, c_int,
                                      c_void_p, c_void_p, c_size_t, c_void_p]
    # debug form (not in include/mmrag.h): the run of vocabulary tiles per workgroup
    lib.mmrag_internal_sparse_pool_ex.restype = c_int
    lib.mmrag_internal_sparse_pool_ex.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_int, c_void_p, c_int, c_int64,
                                                  c_int, c_void_p, c_void_p, c_int]
    lib.mmrag_sparse_select.restype = c_int
    lib.mmrag_sparse_select.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_void_p, c_void_p,
                                        c_void_p, c_void_p]
    lib.mmrag_impact_topk_workspace_bytes.restype = c_size_t
    lib.mmrag_impact_topk_workspace_bytes.argtypes = [c_int, c_int64, c_int]
    lib.mmrag_impact_topk.restype = c_int
    lib.mmrag_impact_topk.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_int,
                                      c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    # debug form (not in include/mmrag.h): candidate capacity, switches (1 = no bound stages)
    lib.mmrag_internal_impact_topk_ex.restype = c_int
    lib.mmrag_internal_impact_topk_ex.argtypes = lib.mmrag_impact_topk.argtypes + [c_int64, ctypes.c_uint]
    # test-only export (not in include/mmrag.h): the sizes at which the sparse kernels change path
    lib.mmrag_internal_sparse_limits.restype = c_int
    lib.mmrag_internal_sparse_limits.argtypes = [c_void_p] * 5
    lib.mmrag_summary_select.restype = c_int
    lib.mmrag_summary_select.argtypes = [c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_void_p, c_int, c_void_p,
                                         c_void_p, c_void_p, c_int64, c_void_p, c_float, c_float, c_int, c_float, c_int,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.mmrag_chunk_boundaries.restype = c_int
    lib.mmrag_chunk_boundaries.argtypes = [c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_void_p, c_int,
                                           c_void_p, ctypes.c_int32, c_int, c_float, c_float, c_float, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p]
    lib.mmrag_attribute.restype = c_int
    lib.mmrag_attribute.argtypes = [c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]
    lib.mmrag_group_terms_workspace_bytes.restype = c_size_t
    lib.mmrag_group_terms_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.mmrag_group_terms.restype = c_int
    lib.mmrag_group_terms.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int, c_int64,
                                      c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    # test-only export (not in include/mmrag.h): the sizes at which the significant-terms kernel changes path
    lib.mmrag_internal_terms_limits.restype = c_int
    lib.mmrag_internal_terms_limits.argtypes = [c_void_p] * 4
    from .lexical import declare as declare_lexical  # BM25 analyzer, device index and search (csrc/lexical.hip)

    declare_lexical(lib)


def lib():
    """Load libmmrag.so once (after torch, so both share one HIP runtime)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise MMRagNativeError(
                        f"{LIB_PATH} is missing: build it with `python -m multimodal_rag_amd.build` "
                        "(hipcc, gfx950).  There is no CPU fallback.")
                handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
                _declare(handle)
                _lib = handle
    return _lib


def _check(status: int, what: str):
    if status != 0:
        msg = lib().mmrag_last_error().decode("utf-8", "replace")
        raise MMRagNativeError(f"{what} failed (status {status}): {msg}")


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _dev_check(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise MMRagNativeError("libmmrag entry points take device (HIP) tensors only; got a CPU tensor")


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def _check_q_rows(who: str, q: torch.Tensor, rows: torch.Tensor, n: Optional[int] = None, other: str = "corpus"):
    """q [B, ld] against stored rows [capacity, ld] (`other`: what `who` calls them): contiguous 2-D, one dtype, one
    padded width, and n rows within the capacity"""
    if q.dim() != 2 or rows.dim() != 2 or not q.is_contiguous() or not rows.is_contiguous():
        raise MMRagNativeError(f"{who}: q and {other} must be contiguous 2-D tensors")
    if q.dtype != rows.dtype or q.shape[1] != rows.shape[1]:
        raise MMRagNativeError(f"{who}: q and {other} must share dtype and padded width")
    if n is not None and n > rows.shape[0]:
        raise MMRagNativeError(f"{who}: n={n} exceeds corpus capacity {rows.shape[0]}")


def _topk_out(B: int, k: int, device, packed: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores [B, k] float32, rows [B, k] int64) to be written by a kernel.  `packed`: both in ONE buffer
    [rows B*k int64 | scores B*k float32], so a caller that wants both on the host copies once (VectorIndex._collect
    recognises the pair by its shared `_base`)"""
    if not packed:
        return (torch.empty((B, k), dtype=torch.float32, device=device),
                torch.empty((B, k), dtype=torch.int64, device=device))
    buf = torch.empty(B * k * 12, dtype=torch.uint8, device=device)
    return buf[B * k * 8:].view(torch.float32).view(B, k), buf[: B * k * 8].view(torch.int64).view(B, k)


def search_uses_query_stationary(B: int, n: int, d: int, k: int, dtype: torch.dtype) -> bool:
    """which kernel a search of this shape runs on (True: a query-stationary kernel, False: the slab-ring cosine_topk_kernel)"""
    return bool(lib().mmrag_internal_search_uses_qs(B, n, padded_dim(d, dtype), _TORCH2DT[dtype], k))


def search_kernel_name(B: int, n: int, d: int, k: int, dtype: torch.dtype) -> str:
    """name of the dominant kernel of a search of this shape (for the bench's roofline label)"""
    v = lib().mmrag_internal_search_uses_qs(B, n, padded_dim(d, dtype), _TORCH2DT[dtype], k)
    return {0: "cosine_topk_kernel (slab-ring)", 1: "cosine_topk_qs_kernel", 2: "cosine_topk_walk_kernel"}[v]


def padded_dim(d: int, dtype: torch.dtype) -> int:
    v = lib().mmrag_padded_dim(int(d), _TORCH2DT[dtype])
    if v < 0:
        raise MMRagNativeError(f"padded_dim: bad arguments d={d} dtype={dtype}")
    return int(v)


# kernel-shape switches of the debug entry point (tests / A-B tools; the product always passes 0)
DBG_NO_PREPASS, DBG_8_WAVES, DBG_NO_QS, DBG_FORCE_QS = 1, 2, 4, 8
# query-stationary shapes: three-launch plan instead of the single-launch walk; the walk's MFMA shape forced; static tile
# assignment only; no in-kernel threshold seeding (A/B tools and the tests that pin every code path)
DBG_OLD_QS, DBG_MFMA32, DBG_MFMA16, DBG_NO_DYN, DBG_NO_SEED = 0x10000, 0x20000, 0x40000, 0x80000, 0x100000


def cosine_topk(q: torch.Tensor, corpus: torch.Tensor, n: int, d: int, k: int, row_offset: int = 0,
                alive_bits: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None, dbg: int = 0,
                packed_out: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact cosine top-k of q [B, ld] against the first n rows of corpus [cap, ld].

    Returns (scores [B, k] float32 descending, rows [B, k] int64 global).  Both inputs must be
    contiguous, same dtype, same padded leading dimension (pad columns zero).
    """
    _dev_check(q, corpus, alive_bits)
    _check_q_rows("cosine_topk", q, corpus, n)
    B, ld = q.shape
    L = lib()
    need = L.mmrag_cosine_topk_workspace_bytes(B, n, k)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)
    out_s, out_r = _topk_out(B, k, q.device, packed_out)
    if dbg:
        cosine_topk_lists(q, corpus, n, d, k, workspace, alive_bits=alive_bits, dbg=dbg)
        return cosine_topk_select(B, n, k, row_offset, workspace, out_s, out_r)
    with torch.cuda.device(q.device):
        st = L.mmrag_cosine_topk(q.data_ptr(), corpus.data_ptr(), B, n, d, ld, _TORCH2DT[q.dtype], k, row_offset,
                                 alive_bits.data_ptr() if alive_bits is not None else None,
                                 out_s.data_ptr(), out_r.data_ptr(), workspace.data_ptr(), _nbytes(workspace),
                                 _stream_ptr(q.device))
    _check(st, "mmrag_cosine_topk")
    return out_s, out_r


# debug switch of the deep search (tests only): no bound passes, every live row is a candidate of the main pass
DEEP_DBG_NO_BOUND = 1


def cosine_topk_deep(q: torch.Tensor, corpus: torch.Tensor, n: int, d: int, k: int, row_offset: int = 0,
                     alive_bits: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                     dbg: int = 0, cap: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact cosine top-k for any k in 1..MAX_K_DEEP (include/mmrag.h mmrag_cosine_topk_deep): the same arguments and
    results as cosine_topk, scores bit-identical to it.  Synchronises the current stream once (the survivor counts).
    `dbg` / `cap` (tests only): DEEP_DBG_NO_BOUND, and a candidate capacity smaller than the library's."""
    _dev_check(q, corpus, alive_bits)
    _check_q_rows("cosine_topk_deep", q, corpus, n)
    B, ld = q.shape
    L = lib()
    need = cosine_topk_deep_workspace_bytes(B, n, k)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)
    out_s, out_r = _topk_out(B, k, q.device)
    with torch.cuda.device(q.device):
        st = L.mmrag_internal_cosine_topk_deep_ex(
            q.data_ptr(), corpus.data_ptr(), B, n, d, ld, _TORCH2DT[q.dtype], k, row_offset,
            alive_bits.data_ptr() if alive_bits is not None else None, out_s.data_ptr(), out_r.data_ptr(),
            workspace.data_ptr(), _nbytes(workspace), _stream_ptr(q.device), dbg, cap)
    _check(st, "mmrag_cosine_topk_deep")
    return out_s, out_r


def cosine_topk_deep_workspace_bytes(B: int, n: int, k: int) -> int:
    return int(lib().mmrag_cosine_topk_deep_workspace_bytes(B, n, k))


def rescore_topk(q: torch.Tensor, plane: torch.Tensor, d: int, cand_rows: torch.Tensor, k: int,
                 packed_out: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact re-scoring of candidate lists (include/mmrag.h mmrag_rescore_topk): q [B, ld] and plane [cap, ld] in one
    full-precision dtype, cand_rows [B, C] int64 (a negative row ends a list).  Returns (scores [B, k] float32, rows
    [B, k] int64) ordered by (score desc, row asc), (-inf, -1) padded; scores are mmrag_rows_dot's, bit for bit.  One
    launch on the current stream, no host sync."""
    _dev_check(q, plane, cand_rows)
    _check_q_rows("rescore_topk", q, plane, other="plane")
    if cand_rows.dim() != 2 or cand_rows.dtype != torch.int64 or not cand_rows.is_contiguous() \
            or cand_rows.shape[0] != q.shape[0]:
        raise MMRagNativeError("rescore_topk: cand_rows must be a contiguous [B, C] int64 tensor")
    B, C = cand_rows.shape
    out_s, out_r = _topk_out(B, k, q.device, packed_out)
    with torch.cuda.device(q.device):
        st = lib().mmrag_rescore_topk(q.data_ptr(), plane.data_ptr(), plane.shape[1], _TORCH2DT[plane.dtype], d,
                                      cand_rows.data_ptr(), B, C, k, out_s.data_ptr(), out_r.data_ptr(),
                                      _stream_ptr(q.device))
    _check(st, "mmrag_rescore_topk")
    return out_s, out_r


# debug switch of the MMR selection (tests, tools/mmr_bench.py): the streamed form also where the staged one fits
MMR_DBG_STREAM = 1


def mmr_select_workspace_bytes(B: int, C: int, d: int, dtype: torch.dtype) -> int:
    return int(lib().mmrag_mmr_select_workspace_bytes(B, C, d, _TORCH2DT[dtype]))


def mmr_select(corpus: torch.Tensor, d: int, cand_scores: torch.Tensor, cand_rows: torch.Tensor, k: int,
               lambda_mult: float, dbg: int = 0):
    """Maximal-marginal-relevance selection (include/mmrag.h mmrag_mmr_select) of k of each query's C candidates:
    cand_scores [B, C] float32 and cand_rows [B, C] int64 in the search's order, (-inf, -1) padded tails allowed.
    Returns device tensors in pick order: (scores [B, k] float32, rows [B, k] int64, positions [B, k] int32,
    mmr values [B, k] float32), unused slots (-inf, -1, -1, -inf).  One launch on the current stream, no host sync."""
    _dev_check(corpus, cand_scores, cand_rows)
    if corpus.dim() != 2 or not corpus.is_contiguous() or corpus.dtype not in _TORCH2DT:
        raise MMRagNativeError("mmr_select: corpus must be a contiguous 2-D tensor of a storage dtype")
    if (cand_scores.dim() != 2 or cand_scores.shape != cand_rows.shape or cand_scores.dtype != torch.float32
            or cand_rows.dtype != torch.int64 or not cand_scores.is_contiguous() or not cand_rows.is_contiguous()):
        raise MMRagNativeError("mmr_select: cand_scores [B, C] float32 and cand_rows [B, C] int64 must be contiguous "
                               "and of one shape")
    if cand_scores.device != corpus.device or cand_rows.device != corpus.device:
        raise MMRagNativeError("mmr_select: candidates and corpus must be on one device")
    B, C = cand_scores.shape
    dev = corpus.device
    out_s = torch.empty((B, k), dtype=torch.float32, device=dev)
    out_r = torch.empty((B, k), dtype=torch.int64, device=dev)
    out_p = torch.empty((B, k), dtype=torch.int32, device=dev)
    out_v = torch.empty((B, k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = lib().mmrag_internal_mmr_select_ex(corpus.data_ptr(), corpus.shape[1], _TORCH2DT[corpus.dtype], d,
                                                cand_scores.data_ptr(), cand_rows.data_ptr(), B, C, k,
                                                float(lambda_mult), out_s.data_ptr(), out_r.data_ptr(),
                                                out_p.data_ptr(), out_v.data_ptr(), None, 0, _stream_ptr(dev), int(dbg))
    _check(st, "mmrag_mmr_select")
    return out_s, out_r, out_p, out_v


def group_select(scores: torch.Tensor, rows: torch.Tensor, group_of_row: torch.Tensor, n_rows: int, n_groups: int,
                 group_size: int):
    """Group each query's candidates by group_of_row[row] (include/mmrag.h mmrag_group_select): scores [B, C] float32
    and rows [B, C] int64 in the search's order, (-inf, -1) padded tails allowed; group_of_row [>= n_rows] int32.
    Returns device tensors (scores [B, G, S] float32 = the input's bits, rows [B, G, S] int64, positions [B, G, S]
    int32, group ordinals [B, G] int32, info [B, 2] int32 = (groups found, valid candidates)), unused slots
    (-inf, -1, -1) and -2.  One launch on the current stream, no host sync."""
    _dev_check(scores, rows, group_of_row)
    if (scores.dim() != 2 or scores.shape != rows.shape or scores.dtype != torch.float32 or rows.dtype != torch.int64
            or not scores.is_contiguous() or not rows.is_contiguous()):
        raise MMRagNativeError("group_select: scores [B, C] float32 and rows [B, C] int64 must be contiguous and of "
                               "one shape")
    if group_of_row.dim() != 1 or group_of_row.dtype != torch.int32 or not group_of_row.is_contiguous():
        raise MMRagNativeError("group_select: group_of_row must be a contiguous 1-D int32 tensor")
    if rows.device != scores.device or group_of_row.device != scores.device:
        raise MMRagNativeError("group_select: candidates and group_of_row must be on one device")
    n_rows, G, S = int(n_rows), int(n_groups), int(group_size)
    if n_rows > group_of_row.numel():
        raise MMRagNativeError(f"group_select: n_rows={n_rows} but group_of_row holds {group_of_row.numel()} entries")
    B, C = scores.shape
    dev = scores.device
    shape = (B, max(G, 0), max(S, 0))
    out_s = torch.empty(shape, dtype=torch.float32, device=dev)
    out_r = torch.empty(shape, dtype=torch.int64, device=dev)
    out_p = torch.empty(shape, dtype=torch.int32, device=dev)
    out_g = torch.empty(shape[:2], dtype=torch.int32, device=dev)
    out_i = torch.empty((B, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = lib().mmrag_group_select(scores.data_ptr(), rows.data_ptr(), B, C, group_of_row.data_ptr(), n_rows, G, S,
                                      out_s.data_ptr(), out_r.data_ptr(), out_p.data_ptr(), out_g.data_ptr(),
                                      out_i.data_ptr(), _stream_ptr(dev))
    _check(st, "mmrag_group_select")
    return out_s, out_r, out_p, out_g, out_i


def _pinned_to_device(host: torch.Tensor, device) -> torch.Tensor:
    """a small host tensor on `device` through pinned memory: the copy is enqueued on the current stream and the
    caller does not wait for what the stream already holds (a copy from pageable memory may)"""
    return host.contiguous().pin_memory().to(device, non_blocking=True)


def fuse_offsets(list_off, L: int, device) -> torch.Tensor:
    """the device int32 list_off of fuse_select from a host sequence, checked (the one place the rule lives): ascending
    from 0 to L over at least one group, at most MAX_FUSE_LISTS lists per group"""
    host = torch.as_tensor(list_off).to(torch.int64).reshape(-1)
    steps = host[1:] - host[:-1]
    if host.numel() < 2 or int(host[0]) != 0 or int(host[-1]) != L or bool((steps < 0).any()):
        raise MMRagNativeError(f"fuse_select: list_off must ascend from 0 to L={L} over at least one group")
    if int(steps.max()) > MAX_FUSE_LISTS:
        raise MMRagNativeError(f"fuse_select: a group owns {int(steps.max())} lists, at most {MAX_FUSE_LISTS} "
                               "are fused")
    return _pinned_to_device(host.to(torch.int32), device)


def fuse_select(scores: torch.Tensor, rows: torch.Tensor, list_off, n: int, weights: Optional[torch.Tensor] = None,
                method: str = "rrf", rrf_k: int = 60):
    """Fuse the ranked lists of query variants (include/mmrag.h mmrag_fuse_select): scores [L, C] float32 and rows
    [L, C] int64 in the search's order, (-inf, -1) padded tails allowed; group g owns the lists list_off[g] ..
    list_off[g + 1] - 1 (ascending, from 0 to L; a group may own none, at most MAX_FUSE_LISTS = 16); weights [L]
    float32 or None = all 1.0; method "rrf" (weight / (rrf_k + rank), summed) or "max" (largest weight * score).
    `list_off` is a HOST sequence or int32 tensor (checked and copied by fuse_offsets through pinned memory), or a
    device int32 tensor the caller vouches for (fuse_offsets made it, or the caller's own).  Returns device tensors (fused [G, n] float32,
    rows [G, n] int64, best [G, n] float32 = the row's largest input score, best list [G, n] int32 local to the group,
    count [G, n] int32 lists that returned the row, info [G, 2] int32 = (distinct rows, valid entries)), unused slots
    (-inf, -1, -inf, -1, 0).  One launch on the current stream, no host sync."""
    _dev_check(scores, rows, weights)
    if (scores.dim() != 2 or scores.shape != rows.shape or scores.dtype != torch.float32 or rows.dtype != torch.int64
            or not scores.is_contiguous() or not rows.is_contiguous()):
        raise MMRagNativeError("fuse_select: scores [L, C] float32 and rows [L, C] int64 must be contiguous and of "
                               "one shape")
    L, C = scores.shape
    dev = scores.device
    if rows.device != dev:
        raise MMRagNativeError("fuse_select: scores and rows must be on one device")
    if weights is not None and (weights.dim() != 1 or weights.numel() != L or weights.dtype != torch.float32
                                or not weights.is_contiguous() or weights.device != dev):
        raise MMRagNativeError("fuse_select: weights must be a contiguous float32 tensor [L] on the lists' device")
    if method not in FUSE_METHODS:
        raise MMRagNativeError(f"fuse_select: unknown method {method!r} (one of {sorted(FUSE_METHODS)})")
    if isinstance(list_off, torch.Tensor) and list_off.is_cuda:
        if list_off.dim() != 1 or list_off.dtype != torch.int32 or not list_off.is_contiguous() or list_off.device != dev:
            raise MMRagNativeError("fuse_select: list_off must be a contiguous 1-D int32 tensor on the lists' device")
        off_dev = list_off
    else:
        off_dev = fuse_offsets(list_off, L, dev)
    G, n = off_dev.numel() - 1, int(n)
    shape = (max(G, 0), max(n, 0))
    out_f = torch.empty(shape, dtype=torch.float32, device=dev)
    out_r = torch.empty(shape, dtype=torch.int64, device=dev)
    out_b = torch.empty(shape, dtype=torch.float32, device=dev)
    out_l = torch.empty(shape, dtype=torch.int32, device=dev)
    out_c = torch.empty(shape, dtype=torch.int32, device=dev)
    out_i = torch.empty((shape[0], 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = lib().mmrag_fuse_select(scores.data_ptr(), rows.data_ptr(), L, C, off_dev.data_ptr(), G,
                                     weights.data_ptr() if weights is not None else None, FUSE_METHODS[method],
                                     int(rrf_k), n, out_f.data_ptr(), out_r.data_ptr(), out_b.data_ptr(),
                                     out_l.data_ptr(), out_c.data_ptr(), out_i.data_ptr(), _stream_ptr(dev))
    _check(st, "mmrag_fuse_select")
    return out_f, out_r, out_b, out_l, out_c, out_i


def _check_stored_rows(who: str, rows: torch.Tensor):
    if rows.dim() != 2 or not rows.is_contiguous() or rows.dtype not in _TORCH2DT:
        raise MMRagNativeError(f"{who}: rows must be a contiguous 2-D tensor of a storage dtype")


def _check_alive(who: str, alive: Optional[torch.Tensor], n: int, rows: torch.Tensor):
    """the first n of `rows` are given, and `alive` (None = every row) is the index's bitmap of at least n bits"""
    if n > rows.shape[0]:
        raise MMRagNativeError(f"{who}: n={n} exceeds the {rows.shape[0]} rows given")
    if alive is not None and (alive.dim() != 1 or alive.dtype != torch.int32 or not alive.is_contiguous()
                              or alive.numel() * 32 < n or alive.device != rows.device):
        raise MMRagNativeError(f"{who}: alive must be a contiguous int32 bitmap of at least n bits on the rows' device")


def sim_join(rows: torch.Tensor, n: int, d: int, threshold: float, alive: Optional[torch.Tensor] = None,
             capacity: int = 1 << 20) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """Exact threshold self-join of the first n rows of `rows` [cap, ld] (include/mmrag.h mmrag_sim_join): every pair
    i < j of alive rows whose dot product is >= threshold.  `alive`: the index's bitmap (int32 words, bit r & 31 of word
    r >> 5), None = every row.  Returns (pairs [m, 2] int64, scores [m] float32, total): total is the exact number of
    qualifying pairs, m = min(total, capacity) of them are returned, sorted on the device by (i, j).  One launch on the
    current stream, then ONE synchronisation to read the count."""
    _dev_check(rows, alive)
    _check_stored_rows("sim_join", rows)
    n, cap = int(n), int(capacity)
    _check_alive("sim_join", alive, n, rows)
    dev = rows.device
    pairs = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=dev)
    scores = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = lib().mmrag_sim_join(rows.data_ptr(), n, rows.shape[1], _TORCH2DT[rows.dtype], int(d),
                                  alive.data_ptr() if alive is not None else None, float(threshold), pairs.data_ptr(),
                                  scores.data_ptr(), cap, count.data_ptr(), _stream_ptr(dev))
    _check(st, "mmrag_sim_join")
    total = int(count.item())
    m = min(total, cap)
    pairs, scores = pairs[:m], scores[:m]
    if m > 1:
        order = torch.argsort(pairs[:, 0] * max(n, 1) + pairs[:, 1])   # n <= 2^23: the key is below 2^46
        pairs, scores = pairs[order], scores[order]
    return pairs, scores, total


def kmeans_assign(rows: torch.Tensor, n: int, d: int, centroids: torch.Tensor,
                  alive: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Nearest centroid of each of the first n rows of `rows` [cap, ld] (include/mmrag.h mmrag_kmeans_assign):
    `centroids` [k, ld] in the rows' dtype and padded width, pad columns zero.  `alive`: the index's bitmap (int32 words,
    bit r & 31 of word r >> 5), None = every row.  Returns device tensors (assign [n] int32 = the lowest centroid at the
    row's maximum dot product, score [n] float32 = that maximum); a dead row holds (-1, -inf).  One launch on the
    current stream, no host sync."""
    _dev_check(rows, centroids, alive)
    _check_stored_rows("kmeans_assign", rows)
    if (centroids.dim() != 2 or not centroids.is_contiguous() or centroids.dtype != rows.dtype
            or centroids.shape[1] != rows.shape[1] or centroids.device != rows.device):
        raise MMRagNativeError("kmeans_assign: centroids must be a contiguous [k, ld] tensor of the rows' dtype, padded "
                               "width and device")
    n = int(n)
    _check_alive("kmeans_assign", alive, n, rows)
    dev = rows.device
    # one spare element: the pointers are real at n == 0 too (an empty tensor's data_ptr() is null)
    assign = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    score = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = lib().mmrag_kmeans_assign(rows.data_ptr(), n, rows.shape[1], _TORCH2DT[rows.dtype], int(d),
                                       centroids.data_ptr(), centroids.shape[0],
                                       alive.data_ptr() if alive is not None else None,
                                       assign.data_ptr(), score.data_ptr(), _stream_ptr(dev))
    _check(st, "mmrag_kmeans_assign")
    return assign[: max(n, 0)], score[: max(n, 0)]


def cluster_sums(rows: torch.Tensor, d: int, order: torch.Tensor, seg_off: torch.Tensor, k: int) -> torch.Tensor:
    """Float32 sum of each cluster's member rows (include/mmrag.h mmrag_cluster_sums): `order` [m] int32 row numbers of
    `rows` [cap, ld] sorted by cluster (the caller guarantees they are rows of it), `seg_off` [k + 1] int64 offsets of
    the clusters' segments in `order`.  Returns sums [k, d] float32 on the device, zeros for an empty segment; identical
    bits run to run.  One launch on the current stream, no host sync."""
    _dev_check(rows, order, seg_off)
    _check_stored_rows("cluster_sums", rows)
    k = int(k)
    if order.dim() != 1 or order.dtype != torch.int32 or not order.is_contiguous() or order.device != rows.device:
        raise MMRagNativeError("cluster_sums: order must be a contiguous 1-D int32 tensor on the rows' device")
    if (seg_off.dim() != 1 or seg_off.dtype != torch.int64 or not seg_off.is_contiguous()
            or seg_off.numel() != k + 1 or seg_off.device != rows.device):
        raise MMRagNativeError("cluster_sums: seg_off must be a contiguous int64 tensor of k + 1 offsets on the rows' "
                               "device")
    dev = rows.device
    sums = torch.empty((max(k, 1), max(int(d), 1)), dtype=torch.float32, device=dev)
    order_ptr = order.data_ptr() if order.numel() else seg_off.data_ptr()    # no members: never read
    with torch.cuda.device(dev):
        st = lib().mmrag_cluster_sums(rows.data_ptr(), rows.shape[1], _TORCH2DT[rows.dtype], int(d),
                                      order_ptr, seg_off.data_ptr(), k, sums.data_ptr(), _stream_ptr(dev))
    _check(st, "mmrag_cluster_sums")
    return sums


def scoped_topk_workspace_bytes(B: int, n: int, k: int, n_groups: int) -> int:
    return int(lib().mmrag_scoped_topk_workspace_bytes(int(B), int(n), int(k), int(n_groups)))


def candidate_capacity(k: int) -> int:
    """candidate slots a query of scoped_topk has for a top-k of k (csrc/candidate_select.h): with max_candidates at or
    below it the call cannot overflow and does not synchronise"""
    return int(lib().mmrag_internal_candidate_capacity(int(k)))


def bound_plan(n: int, k: int, cap: int = 0, dbg: int = 0) -> Tuple[int, list]:
    """(candidate slots per query, 128-row tiles of each bound stage) of boosted_topk, filtered_topk, range_scan
    (k = limit) and recommend_topk at n rows (csrc/candidate_select.h make_bound_plan); `cap`, `dbg` as those take them"""
    slots = ctypes.c_int64(0)
    stages = (ctypes.c_int64 * 8)()
    m = int(lib().mmrag_internal_bound_plan(int(n), int(k), int(cap), int(dbg), ctypes.byref(slots), stages))
    if m < 0:
        raise MMRagNativeError(f"bound_plan: n={n}, k={k} outside the range of the scans")
    return int(slots.value), [int(stages[i]) for i in range(m)]


def check_scopes(B: int, n_groups: int, scope_of_query, scope_off, scope_groups) -> int:
    """The scope tables of scoped_topk as HOST integer sequences, checked the way the device cannot report: returns S.
    Raises MMRagNativeError for a scope of more than MAX_SCOPE_GROUPS ordinals, a query whose scope index is outside
    0..S-1, offsets that do not ascend from 0 to len(scope_groups), and ordinals that are not ascending inside a scope
    or outside 0..n_groups-1."""
    soq = [int(v) for v in scope_of_query]
    off = [int(v) for v in scope_off]
    grp = [int(v) for v in scope_groups]
    S = len(off) - 1
    if len(soq) != B:
        raise MMRagNativeError(f"scoped_topk: scope_of_query holds {len(soq)} entries for {B} queries")
    if S < 1 or off[0] != 0 or off[-1] != len(grp) or any(b < a for a, b in zip(off, off[1:])):
        raise MMRagNativeError("scoped_topk: scope_off must hold S + 1 >= 2 ascending offsets from 0 to "
                               "len(scope_groups)")
    for s in range(S):
        mine = grp[off[s]: off[s + 1]]
        if len(mine) > MAX_SCOPE_GROUPS:
            raise MMRagNativeError(f"scoped_topk: scope {s} holds {len(mine)} groups, at most {MAX_SCOPE_GROUPS}")
        if any(b <= a for a, b in zip(mine, mine[1:])) or (mine and (mine[0] < 0 or mine[-1] >= n_groups)):
            raise MMRagNativeError(f"scoped_topk: scope {s} must hold ascending ordinals in 0..{n_groups - 1}")
    bad = [v for v in soq if not 0 <= v < S]
    if bad:
        raise MMRagNativeError(f"scoped_topk: scope_of_query {bad[0]} outside 0..{S - 1}")
    return S


def scoped_topk(q: torch.Tensor, rows: torch.Tensor, n: int, d: int, k: int, group_col: torch.Tensor, n_groups: int,
                scope_of_query, scope_off, scope_groups, max_candidates: int,
                alive_bits: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                row_offset: int = 0, cap: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k of each query of q [B, ld] over the rows of ITS scope among the first n of `rows` [cap, ld]
    (include/mmrag.h mmrag_scoped_topk): query b sees row r iff r is alive and group_col[r] (int32 ordinal, -1 = none)
    is one of scope_groups[scope_off[s] : scope_off[s + 1]] for s = scope_of_query[b].  The three scope tables are HOST
    integer tensors or sequences: they are checked here (check_scopes; the device cannot report a malformed table) and
    copied to the device in one transfer.  `max_candidates`: an upper bound on the rows one scope holds (n if unknown).
    Returns (scores [B, k] float32 descending, rows [B, k] int64 + row_offset), (-inf, -1) padded.  No host
    synchronisation unless max_candidates exceeds the candidate slots of a query.  `cap` (tests only): fewer slots."""
    _dev_check(q, rows, alive_bits, group_col)
    _check_q_rows("scoped_topk", q, rows, n, other="rows")
    _check_stored_rows("scoped_topk", rows)
    B, ld = q.shape
    n, k, n_groups = int(n), int(k), int(n_groups)
    _check_alive("scoped_topk", alive_bits, n, rows)
    dev = q.device
    if (group_col.dim() != 1 or group_col.dtype != torch.int32 or not group_col.is_contiguous()
            or group_col.numel() < n or group_col.device != dev):
        raise MMRagNativeError("scoped_topk: group_col must be a contiguous int32 tensor of at least n ordinals on the "
                               "rows' device")
    tables = [torch.as_tensor(t, dtype=torch.int32).reshape(-1).cpu()
              for t in (scope_of_query, scope_off, scope_groups)]
    S = check_scopes(B, n_groups, *(t.tolist() for t in tables))
    at = [0, B, B + S + 1]
    # one pinned copy; a spare element keeps the ordinals' pointer real when no scope holds any
    packed = _pinned_to_device(torch.cat(tables + [torch.zeros(1, dtype=torch.int32)]), dev)
    soq, off, grp = (packed[lo:] for lo in at)
    need = scoped_topk_workspace_bytes(B, n, k, n_groups)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    out_s, out_r = _topk_out(B, k, dev)
    with torch.cuda.device(dev):
        st = lib().mmrag_internal_scoped_topk_ex(
            q.data_ptr(), rows.data_ptr(), B, n, int(d), ld, _TORCH2DT[q.dtype], k, int(row_offset),
            alive_bits.data_ptr() if alive_bits is not None else None, group_col.data_ptr(), n_groups,
            soq.data_ptr(), S, off.data_ptr(), grp.data_ptr(), int(max_candidates), out_s.data_ptr(), out_r.data_ptr(),
            workspace.data_ptr(), _nbytes(workspace), _stream_ptr(dev), int(cap))
    _check(st, "mmrag_scoped_topk")
    return out_s, out_r


def filter_words(n: int) -> int:
    """words of a row bitmap of n rows (mmrag_filter_words): 4 per 128-row tile; 0 for n outside 0..2^31-1"""
    return int(lib().mmrag_filter_words(int(n)))


def filtered_topk_workspace_bytes(B: int, n: int, k: int) -> int:
    return int(lib().mmrag_filtered_topk_workspace_bytes(int(B), int(n), int(k)))


def check_filter_programs(ops: np.ndarray, prog_off, set_values, n_columns: int) -> int:
    """The program tables of filter_eval as HOST arrays (filters.pack_programs), checked the way the device cannot
    report: returns F.  Raises MMRagNativeError for offsets that do not ascend from 0 to len(ops), a program of 0 or
    more than MAX_FILTER_OPS instructions, an unknown code, a column index outside 0..n_columns-1, a set range outside
    set_values or longer than MAX_FILTER_SET, a constant that is not finite, and a program that does not leave exactly
    one value on a stack that never underflows."""
    off = [int(v) for v in np.asarray(prog_off).reshape(-1)]
    F, n_ops, n_set = len(off) - 1, len(ops), len(set_values)
    if F < 1 or off[0] != 0 or off[-1] != n_ops or any(b < a for a, b in zip(off, off[1:])):
        raise MMRagNativeError("filter_eval: prog_off must hold F + 1 >= 2 ascending offsets from 0 to len(ops)")
    if n_set and not np.isfinite(np.asarray(set_values, dtype=np.float64)).all():
        raise MMRagNativeError("filter_eval: set_values must be finite")
    for f in range(F):
        lo, hi = off[f], off[f + 1]
        if not 1 <= hi - lo <= MAX_FILTER_OPS:
            raise MMRagNativeError(f"filter_eval: program {f} holds {hi - lo} instructions, 1..{MAX_FILTER_OPS}")
        depth = 0
        for i in range(lo, hi):
            code, column, set_off, set_len, value = (ops[i][name].item() for name in
                                                     ("code", "column", "set_off", "set_len", "value"))
            if not 0 <= code <= 11:
                raise MMRagNativeError(f"filter_eval: instruction {i} has the unknown code {code}")
            if code in (2, 3):
                depth -= 1
                if depth < 1:
                    raise MMRagNativeError(f"filter_eval: program {f} pops an empty stack")
                continue
            depth += 1
            if code >= 4 and not 0 <= column < n_columns:
                raise MMRagNativeError(f"filter_eval: instruction {i} reads column {column} outside 0..{n_columns - 1}")
            if code >= 10 and not (0 <= set_len <= MAX_FILTER_SET and 0 <= set_off <= n_set - set_len):
                raise MMRagNativeError(f"filter_eval: instruction {i} reads a set outside set_values "
                                       f"(offset {set_off}, length {set_len}, at most {MAX_FILTER_SET})")
            if 4 <= code <= 9 and not np.isfinite(value):
                raise MMRagNativeError(f"filter_eval: instruction {i} compares with {value}")
        if depth != 1:
            raise MMRagNativeError(f"filter_eval: program {f} leaves {depth} values on the stack")
    return F


def filter_eval(ops: np.ndarray, prog_off, set_values, columns, n: int, alive_bits: Optional[torch.Tensor] = None,
                device=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F filter programs over n rows -> bitmaps [F, filter_words(n)] int32 on the device (include/mmrag.h
    mmrag_filter_eval, csrc/filtered.hip), ANDed with alive_bits when given; bits at and past n are zero.  `ops`
    (filters.OP_DTYPE), `prog_off` and `set_values` are HOST arrays (filters.pack_programs): checked here
    (check_filter_programs) and uploaded in one transfer.  `columns`: at most MAX_FILTER_COLUMNS device tensors of at
    least n values, float64 (numbers, NaN = missing) or int32 (string ordinals, -1 = missing).  `out`: a contiguous
    device int32 [F, filter_words(n)] to write instead of a new tensor.  One launch on the current stream, no host
    synchronisation."""
    columns = list(columns)
    n = int(n)
    if len(columns) > MAX_FILTER_COLUMNS:
        raise MMRagNativeError(f"filter_eval: {len(columns)} columns, at most {MAX_FILTER_COLUMNS}")
    _dev_check(alive_bits, *columns)
    dev = columns[0].device if columns else (alive_bits.device if alive_bits is not None else torch.device(device))
    for c in columns:
        if (c.dim() != 1 or c.dtype not in (torch.float64, torch.int32) or not c.is_contiguous() or c.numel() < n
                or c.device != dev):
            raise MMRagNativeError("filter_eval: a column must be a contiguous float64 or int32 tensor of at least n "
                                   "values on one device")
    if alive_bits is not None and (alive_bits.dim() != 1 or alive_bits.dtype != torch.int32
                                   or not alive_bits.is_contiguous() or alive_bits.numel() * 32 < n
                                   or alive_bits.device != dev):
        raise MMRagNativeError("filter_eval: alive must be a contiguous int32 bitmap of at least n bits on the columns' "
                               "device")
    ops = np.ascontiguousarray(ops)
    if ops.dtype.itemsize != 24:
        raise MMRagNativeError("filter_eval: ops must be an array of filters.OP_DTYPE (24-byte instructions)")
    off = np.ascontiguousarray(prog_off, dtype=np.int32).reshape(-1)
    sets = np.ascontiguousarray(set_values, dtype=np.float64).reshape(-1)
    F = check_filter_programs(ops, off, sets, len(columns))
    W = filter_words(n)
    if n < 0 or (W == 0 and n != 0):
        raise MMRagNativeError(f"filter_eval: n={n} outside 0..2^31-1")
    # one pinned copy: [ops | set_values (8-byte aligned: 24 n_ops is) | prog_off]; a spare double keeps the pointer real
    blob = np.concatenate([ops.view(np.uint8).reshape(-1), np.append(sets, 0.0).view(np.uint8), off.view(np.uint8)])
    packed = _pinned_to_device(torch.from_numpy(blob), dev)
    at_sets = ops.nbytes
    at_off = at_sets + (sets.size + 1) * 8
    if out is None:
        out = torch.empty((F, W), dtype=torch.int32, device=dev)
    elif (not out.is_cuda or out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (F, W)
          or out.device != dev):
        raise MMRagNativeError(f"filter_eval: out must be a contiguous int32 [{F}, {W}] tensor on the columns' device")
    if W == 0:
        return out
    ptrs = (c_void_p * MAX_FILTER_COLUMNS)(*[c.data_ptr() for c in columns])
    kinds = (c_int32 * MAX_FILTER_COLUMNS)(*[0 if c.dtype == torch.float64 else 1 for c in columns])
    with torch.cuda.device(dev):
        st = lib().mmrag_filter_eval(packed.data_ptr(), len(ops), packed.data_ptr() + at_off, F,
                                     packed.data_ptr() + at_sets, sets.size, ptrs, kinds, len(columns), n,
                                     alive_bits.data_ptr() if alive_bits is not None else None, out.data_ptr(),
                                     _stream_ptr(dev))
    _check(st, "mmrag_filter_eval")
    return out


def filtered_topk(q: torch.Tensor, rows: torch.Tensor, n: int, d: int, k: int, filter_of_query, vis_bits: torch.Tensor,
                  workspace: Optional[torch.Tensor] = None, row_offset: int = 0, cap: int = 0, dbg: int = 0,
                  count_items: bool = False):
    """Top-k of each query of q [B, ld] over the rows ITS bitmap holds among the first n of `rows` [cap, ld]
    (include/mmrag.h mmrag_filtered_topk): query b sees row r iff bit r of vis_bits[filter_of_query[b]] is set.
    `vis_bits`: a contiguous device int32 [F, filter_words(n)], from filter_eval or from anywhere else.
    `filter_of_query`: B HOST integers in 0..F-1, checked here (the device cannot report them) and uploaded.  Returns
    (scores [B, k] float32 descending, rows [B, k] int64 + row_offset), (-inf, -1) padded.  No host synchronisation
    unless n exceeds the candidate slots of a query.  `cap`, `dbg`, `count_items` (tests and tools): fewer slots;
    dbg & 1 = no bound passes; a third result, the device int64 count of (row tile, query tile) items the main pass
    issued."""
    _dev_check(q, rows, vis_bits)
    _check_q_rows("filtered_topk", q, rows, n, other="rows")
    _check_stored_rows("filtered_topk", rows)
    B, ld = q.shape
    n, k = int(n), int(k)
    if not 1 <= k <= MAX_K_DEEP:
        raise ValueError(f"filtered_topk: k={k} outside 1..{MAX_K_DEEP}")
    dev = q.device
    W = filter_words(n)
    if (vis_bits.dim() != 2 or vis_bits.dtype != torch.int32 or not vis_bits.is_contiguous() or vis_bits.shape[0] < 1
            or vis_bits.shape[1] != W or vis_bits.device != dev):
        raise MMRagNativeError(f"filtered_topk: vis_bits must be a contiguous int32 [F, {W}] tensor on the rows' device")
    F = vis_bits.shape[0]
    foq = torch.as_tensor(filter_of_query, dtype=torch.int32).reshape(-1).cpu()
    if foq.numel() != B:
        raise MMRagNativeError(f"filtered_topk: filter_of_query holds {foq.numel()} entries for {B} queries")
    if B and (int(foq.min()) < 0 or int(foq.max()) >= F):
        raise MMRagNativeError(f"filtered_topk: filter_of_query outside 0..{F - 1}")
    foq_dev = _pinned_to_device(foq, dev)
    need = filtered_topk_workspace_bytes(B, n, k)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    out_s, out_r = _topk_out(B, k, dev)
    items = torch.zeros(1, dtype=torch.int64, device=dev) if count_items else None
    with torch.cuda.device(dev):
        st = lib().mmrag_internal_filtered_topk_ex(
            q.data_ptr(), rows.data_ptr(), B, n, int(d), ld, _TORCH2DT[q.dtype], k, int(row_offset), foq_dev.data_ptr(),
            F, vis_bits.data_ptr() if vis_bits.numel() else None, out_s.data_ptr(), out_r.data_ptr(),
            workspace.data_ptr(), _nbytes(workspace), _stream_ptr(dev), int(cap), int(dbg),
            items.data_ptr() if items is not None else None)
    _check(st, "mmrag_filtered_topk")
    return (out_s, out_r, items) if count_items else (out_s, out_r)


def range_scan_workspace_bytes(B: int, n: int, limit: int, facet_slots: int = 0) -> int:
    return int(lib().mmrag_range_scan_workspace_bytes(int(B), int(n), int(limit), int(facet_slots)))


def range_scan(q: torch.Tensor, rows: torch.Tensor, n: int, d: int, threshold, limit: int, facet_cols=(),
               facet_sizes=(), filter_of_query=None, vis_bits: Optional[torch.Tensor] = None,
               workspace: Optional[torch.Tensor] = None, row_offset: int = 0, cap: int = 0, dbg: int = 0):
    """Everything at or above a score (include/mmrag.h mmrag_range_scan, where the definitions are): for each query of
    q [B, ld] over the first n of `rows` [cap, ld], the number of rows it sees whose score is >= its threshold, their
    spread over the codes of up to MAX_FACET_COLUMNS int32 device columns, and the `limit` best of them, in one scan.
    `threshold`: one finite float, B of them (a HOST sequence, checked here) or a device float32 [B] tensor (taken as it
    is).  `limit`: 0..MAX_K_DEEP; 0 = counts and facets only.  `facet_cols` / `facet_sizes`: device int32 columns of at
    least n codes and their G_c; a code outside 0..G_c-1 counts in the column's last slot.  `vis_bits`: a contiguous
    device int32 [F, filter_words(n)] with `filter_of_query`, B HOST integers (an index outside 0..F-1 sees nothing);
    None: every row below n is visible.  Returns (counts [B] int32, facets [B, sum(G_c + 1)] int32 or None without
    columns, scores [B, limit] float32 descending, rows [B, limit] int64 + row_offset, (-inf, -1) padded; both None for
    limit == 0).  No host synchronisation unless limit > 0 and n exceeds the candidate slots of a query.  `cap`, `dbg`
    (tests): fewer slots; dbg & 1 = no bound passes."""
    n, limit = int(n), int(limit)
    facet_cols, facet_sizes = list(facet_cols), [int(g) for g in facet_sizes]
    if not 0 <= limit <= MAX_K_DEEP:
        raise ValueError(f"range_scan: limit={limit} outside 0..{MAX_K_DEEP}")
    if len(facet_cols) > MAX_FACET_COLUMNS:
        raise MMRagNativeError(f"range_scan: {len(facet_cols)} facet columns, at most {MAX_FACET_COLUMNS}")
    if len(facet_sizes) != len(facet_cols) or any(g < 0 for g in facet_sizes):
        raise MMRagNativeError("range_scan: facet_sizes must hold one G >= 0 per facet column")
    _dev_check(q, rows, vis_bits, *facet_cols)
    _check_q_rows("range_scan", q, rows, n, other="rows")
    _check_stored_rows("range_scan", rows)
    B, ld = q.shape
    dev = q.device
    for c in facet_cols:
        if c.dim() != 1 or c.dtype != torch.int32 or not c.is_contiguous() or c.numel() < n or c.device != dev:
            raise MMRagNativeError("range_scan: a facet column must be a contiguous int32 tensor of at least n codes on "
                                   "the rows' device")
    if isinstance(threshold, torch.Tensor) and threshold.is_cuda:
        thr = threshold
        if thr.dtype != torch.float32 or thr.dim() != 1 or thr.numel() != B or not thr.is_contiguous() or thr.device != dev:
            raise MMRagNativeError(f"range_scan: a device threshold must be a contiguous float32 [{B}] tensor")
    else:
        host = torch.as_tensor(threshold, dtype=torch.float32).reshape(-1)
        if host.numel() == 1:
            host = host.expand(B)
        if host.numel() != B:
            raise MMRagNativeError(f"range_scan: threshold holds {host.numel()} entries for {B} queries")
        if not bool(torch.isfinite(host).all()):
            raise ValueError("range_scan: thresholds must be finite")
        thr = _pinned_to_device(host, dev)
    foq_dev, F = None, 0
    if vis_bits is not None:
        W = filter_words(n)
        if (vis_bits.dim() != 2 or vis_bits.dtype != torch.int32 or not vis_bits.is_contiguous()
                or vis_bits.shape[0] < 1 or vis_bits.shape[1] != W or vis_bits.device != dev):
            raise MMRagNativeError(f"range_scan: vis_bits must be a contiguous int32 [F, {W}] tensor on the rows' device")
        F = vis_bits.shape[0]
        if filter_of_query is None:
            raise MMRagNativeError("range_scan: vis_bits needs filter_of_query")
        foq = torch.as_tensor(filter_of_query, dtype=torch.int32).reshape(-1).cpu()
        if foq.numel() != B:
            raise MMRagNativeError(f"range_scan: filter_of_query holds {foq.numel()} entries for {B} queries")
        foq_dev = _pinned_to_device(foq, dev)
    slots = sum(g + 1 for g in facet_sizes)
    need = range_scan_workspace_bytes(B, n, limit, slots)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    facets = torch.empty((B, slots), dtype=torch.int32, device=dev) if facet_cols else None
    out_s, out_r = _topk_out(B, limit, dev) if limit else (None, None)
    ptrs = (c_void_p * MAX_FACET_COLUMNS)(*[c.data_ptr() for c in facet_cols])
    sizes = (c_int32 * MAX_FACET_COLUMNS)(*facet_sizes)
    with torch.cuda.device(dev):
        st = lib().mmrag_internal_range_scan_ex(
            q.data_ptr(), rows.data_ptr(), B, n, int(d), ld, _TORCH2DT[q.dtype], thr.data_ptr(), limit, int(row_offset),
            foq_dev.data_ptr() if foq_dev is not None else None, F,
            vis_bits.data_ptr() if vis_bits is not None and vis_bits.numel() else None, ptrs, sizes, len(facet_cols),
            counts.data_ptr(), facets.data_ptr() if facets is not None else None,
            out_s.data_ptr() if limit else None, out_r.data_ptr() if limit else None, workspace.data_ptr(),
            _nbytes(workspace), _stream_ptr(dev), int(cap), int(dbg))
    _check(st, "mmrag_range_scan")
    return counts, facets, out_s, out_r


def related_groups_workspace_bytes(M: int, S: int, n: int, n_groups: int, k: int) -> int:
    return int(lib().mmrag_related_groups_workspace_bytes(int(M), int(S), int(n), int(n_groups), int(k)))


def related_groups(sets: torch.Tensor, set_off, rows: torch.Tensor, n: int, d: int, k: int, group_col: torch.Tensor,
                   n_groups: int, threshold: float, exclude=None, alive_bits: Optional[torch.Tensor] = None,
                   table_bytes: Optional[int] = None, grid: int = 0):
    """Set-to-group similarity of S sets of vectors against the first n of `rows` [cap, ld] (include/mmrag.h
    mmrag_related_groups, where the definition is): `sets` [M, ld] in the rows' dtype and padded width holds the sets'
    vectors, set s owning rows set_off[s] : set_off[s + 1] (a HOST sequence of S + 1 ascending offsets from 0 to M);
    group_col [>= n] int32 is the rows' group ordinal (outside 0..n_groups-1 = no group); `exclude`: one ordinal per set
    that is no candidate of it (HOST sequence, -1 or None = none).  Returns device tensors
        (similarity [S, k] float32 desc, group [S, k] int32, covered [S, k] int32, best [M, k] float32,
         best_row [M, k] int64),
    (-inf, -1, 0, -inf, -1) padded.  No host synchronisation.  A call whose table of 8 * M * n_groups bytes would exceed
    `table_bytes` (default: settings.MMRAG_RELATED_TABLE_BYTES) runs as sub-calls of whole sets, which is exact; raises
    ValueError when one set alone exceeds it, for more than MAX_RELATED_SETS sets or MAX_RELATED_ROWS vectors, k outside
    1..MAX_K_DEEP, or offsets that do not fit.  `grid` (tests only): the scan's workgroups."""
    _dev_check(sets, rows, alive_bits, group_col)
    _check_q_rows("related_groups", sets, rows, n, other="rows")
    _check_stored_rows("related_groups", rows)
    M, ld = sets.shape
    n, k, n_groups = int(n), int(k), int(n_groups)
    _check_alive("related_groups", alive_bits, n, rows)
    dev = rows.device
    if (group_col.dim() != 1 or group_col.dtype != torch.int32 or not group_col.is_contiguous()
            or group_col.numel() < n or group_col.device != dev):
        raise MMRagNativeError("related_groups: group_col must be a contiguous int32 tensor of at least n ordinals on "
                               "the rows' device")
    off = [int(v) for v in set_off]
    S = len(off) - 1
    if S < 1 or off[0] != 0 or off[-1] != M or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError(f"related_groups: set_off must hold S + 1 >= 2 ascending offsets from 0 to M={M}")
    if S > MAX_RELATED_SETS or M > MAX_RELATED_ROWS:
        raise ValueError(f"related_groups: at most {MAX_RELATED_SETS} sets and {MAX_RELATED_ROWS} vectors per call "
                         f"(S={S}, M={M})")
    if not 1 <= k <= MAX_K_DEEP:
        raise ValueError(f"related_groups: k={k} outside 1..{MAX_K_DEEP}")
    excl = [-1] * S if exclude is None else [-1 if v is None else int(v) for v in exclude]
    if len(excl) != S:
        raise ValueError(f"related_groups: exclude holds {len(excl)} entries for {S} sets")
    if table_bytes is None:
        from .config import settings

        table_bytes = int(settings.MMRAG_RELATED_TABLE_BYTES)
    # sub-calls of whole sets [s0, s1) whose tables fit the budget
    cell = 8 * max(n_groups, 0)
    parts, s0 = [], 0
    for s in range(S):
        if (off[s + 1] - off[s]) * cell > table_bytes:
            raise ValueError(f"related_groups: set {s} alone needs a table of {(off[s + 1] - off[s]) * cell} bytes, "
                             f"above MMRAG_RELATED_TABLE_BYTES={table_bytes}")
        if (off[s + 1] - off[s0]) * cell > table_bytes:
            parts.append((s0, s))
            s0 = s
    parts.append((s0, S))
    # one pinned copy of every sub-call's offsets and exclusions
    host = []
    for a, b in parts:
        host += [v - off[a] for v in off[a: b + 1]] + excl[a:b]
    packed = _pinned_to_device(torch.tensor(host, dtype=torch.int32), dev)
    out_sim = torch.empty((S, k), dtype=torch.float32, device=dev)
    out_grp = torch.empty((S, k), dtype=torch.int32, device=dev)
    out_cov = torch.empty((S, k), dtype=torch.int32, device=dev)
    # one spare row: the pointers are real at M == 0 too
    out_best = torch.empty((M + 1, k), dtype=torch.float32, device=dev)
    out_row = torch.empty((M + 1, k), dtype=torch.int64, device=dev)
    need = max(related_groups_workspace_bytes(off[b] - off[a], b - a, n, n_groups, k) for a, b in parts)
    workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    sets_ptr = sets.data_ptr() if M else workspace.data_ptr()      # no vectors: never read
    at = 0
    with torch.cuda.device(dev):
        for a, b in parts:
            Sp, c0, Mp = b - a, off[a], off[b] - off[a]
            st = lib().mmrag_internal_related_groups_ex(
                sets_ptr + c0 * ld * sets.element_size(), Mp, packed[at:].data_ptr(), Sp, rows.data_ptr(), n, int(d),
                ld, _TORCH2DT[rows.dtype], alive_bits.data_ptr() if alive_bits is not None else None,
                group_col.data_ptr(), n_groups, packed[at + Sp + 1:].data_ptr(), float(threshold), k,
                out_sim[a:].data_ptr(), out_grp[a:].data_ptr(), out_cov[a:].data_ptr(), out_best[c0:].data_ptr(),
                out_row[c0:].data_ptr(), workspace.data_ptr(), _nbytes(workspace), _stream_ptr(dev), int(grid))
            _check(st, "mmrag_related_groups")
            at += 2 * Sp + 1
    return out_sim, out_grp, out_cov, out_best[:M], out_row[:M]


def boosted_topk_workspace_bytes(B: int, n: int, k: int) -> int:
    return int(lib().mmrag_boosted_topk_workspace_bytes(int(B), int(n), int(k)))


def _boost_operand(who: str, what: str, t, count: int, exact: bool, device) -> torch.Tensor:
    """`what` (prior / weight) of boosted_topk on `device`: a HOST array is checked (float32-representable finite
    values, `count` entries; at least `count` when not `exact`) and uploaded through pinned memory, a device float32
    tensor is the caller's own (VectorIndex checked it when the column was built).  Raises ValueError."""
    if isinstance(t, torch.Tensor) and t.is_cuda:
        if (t.dim() != 1 or t.dtype != torch.float32 or not t.is_contiguous() or t.device != device
                or (t.numel() != count if exact else t.numel() < count)):
            raise ValueError(f"{who}: {what} must be a contiguous float32 tensor of {count} entries on the rows' device")
        return t
    host = torch.as_tensor(t, dtype=torch.float64).reshape(-1).to(torch.float32)
    if host.numel() != count:
        raise ValueError(f"{who}: {what} holds {host.numel()} entries, expected {count}")
    if not bool(torch.isfinite(host).all()):
        raise ValueError(f"{who}: {what} must be finite")
    if host.numel() == 0:
        host = torch.zeros(1, dtype=torch.float32)    # keeps the pointer real
    return _pinned_to_device(host, device)


def boosted_topk(q: torch.Tensor, rows: torch.Tensor, n: int, d: int, k: int, prior, weight,
                 alive_bits: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                 row_offset: int = 0, cap: int = 0, dbg: int = 0,
                 want_boost: bool = True) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Top-k of each query of q [B, ld] over the first n of `rows` [cap, ld] by cosine plus a score prior
    (include/mmrag.h mmrag_boosted_topk): final[b][r] = fmaf(weight[b], prior[r], <q_b, x_r>), applied inside one exact
    scan.  `prior`: n float32 values, a host array (checked finite and uploaded) or a device tensor of at least n the
    caller vouches for; `weight`: a number or one per query, likewise.  Returns (scores [B, k] float32 = final
    descending, rows [B, k] int64 + row_offset, boosts [B, k] float32 = weight * prior of each hit or None), (-inf, -1,
    0) padded.  No host synchronisation unless n exceeds the candidate slots of a query.  Raises ValueError for a
    non-finite or wrong-length prior or weight and k outside 1..MAX_K_DEEP, before anything is launched.  `cap`, `dbg`
    (tests only): fewer slots; dbg & 1 = no bound passes."""
    _dev_check(q, rows, alive_bits)
    _check_q_rows("boosted_topk", q, rows, n, other="rows")
    _check_stored_rows("boosted_topk", rows)
    B, ld = q.shape
    n, k = int(n), int(k)
    if not 1 <= k <= MAX_K_DEEP:
        raise ValueError(f"boosted_topk: k={k} outside 1..{MAX_K_DEEP}")
    _check_alive("boosted_topk", alive_bits, n, rows)
    dev = q.device
    if not isinstance(weight, torch.Tensor) and not hasattr(weight, "__len__"):
        weight = [float(weight)] * B
    prior_dev = _boost_operand("boosted_topk", "prior", prior, n, False, dev)
    weight_dev = _boost_operand("boosted_topk", "weight", weight, B, True, dev)
    need = boosted_topk_workspace_bytes(B, n, k)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    out_s, out_r = _topk_out(B, k, dev)
    out_b = torch.empty((B, k), dtype=torch.float32, device=dev) if want_boost else None
    with torch.cuda.device(dev):
        st = lib().mmrag_internal_boosted_topk_ex(
            q.data_ptr(), rows.data_ptr(), B, n, int(d), ld, _TORCH2DT[q.dtype], k, int(row_offset),
            alive_bits.data_ptr() if alive_bits is not None else None, prior_dev.data_ptr(), weight_dev.data_ptr(),
            out_s.data_ptr(), out_r.data_ptr(), out_b.data_ptr() if out_b is not None else None,
            workspace.data_ptr(), _nbytes(workspace), _stream_ptr(dev), int(cap), int(dbg))
    _check(st, "mmrag_boosted_topk")
    return out_s, out_r, out_b


def recommend_topk_workspace_bytes(R: int, n: int, k: int) -> int:
    return int(lib().mmrag_recommend_topk_workspace_bytes(int(R), int(n), int(k)))


def pack_examples(positives, negatives, dim: int, dtype: torch.dtype, device,
                  rows: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The example block of recommend_topk from ragged lists: `positives[g]` / `negatives[g]` (negatives, or one of its
    entries, may be None) are request g's examples, each a vector of `dim` numbers -- or, when the stored `rows`
    [capacity, ld] are given, an int: that stored row, gathered on the device.  Returns (examples [16 R, ld] of `dtype`
    with zero pad columns, sign int8 [16 R]) on `device`: a request's positives first (+1), then its negatives (-1),
    the rest of its 16 slots zero with sign 0.  The one place the request rules live -- ValueError for no request, a
    request without a positive or with more than MAX_RECOMMEND_EXAMPLES examples, a vector of the wrong length and
    one whose norm is off by more than 1e-2 (as queries are checked)."""
    E = MAX_RECOMMEND_EXAMPLES
    positives = list(positives)
    R = len(positives)
    if R == 0:
        raise ValueError("pack_examples: no request")
    negatives = [None] * R if negatives is None else list(negatives)
    if len(negatives) != R:
        raise ValueError(f"pack_examples: {len(negatives)} negative lists for {R} requests")
    ld = int(rows.shape[1]) if rows is not None else padded_dim(dim, dtype)
    host = np.zeros((E * R, dim), dtype=np.float32)
    sign = np.zeros(E * R, dtype=np.int8)
    slots, gathered = [], []
    for g in range(R):
        pos = list(positives[g]) if positives[g] is not None else []
        neg = list(negatives[g]) if negatives[g] is not None else []
        if not pos:
            raise ValueError(f"pack_examples: request {g} has no positive example")
        if len(pos) + len(neg) > E:
            raise ValueError(f"pack_examples: request {g} has {len(pos) + len(neg)} examples, at most {E}")
        for j, e in enumerate(pos + neg):
            at = E * g + j
            sign[at] = 1 if j < len(pos) else -1
            if rows is not None and isinstance(e, (int, np.integer)) and not isinstance(e, bool):
                if not 0 <= int(e) < rows.shape[0]:
                    raise ValueError(f"pack_examples: request {g}: stored row {int(e)} out of range")
                slots.append(at)
                gathered.append(int(e))
                continue
            v = np.asarray(e.detach().cpu() if isinstance(e, torch.Tensor) else e, dtype=np.float32).reshape(-1)
            if v.size != dim:
                raise ValueError(f"pack_examples: request {g}: an example holds {v.size} numbers, expected {dim}")
            nrm = float(np.sqrt(np.dot(v.astype(np.float64), v.astype(np.float64))))
            if not abs(nrm - 1.0) <= 1e-2:       # false for NaN too
                raise ValueError(f"pack_examples: request {g}: example {j} has norm {nrm:.4f}; examples are unit "
                                 f"vectors, as queries are -- L2-normalise them first")
            host[at] = v
    packed = torch.zeros((E * R, ld), dtype=dtype)
    packed[:, :dim] = torch.from_numpy(host).to(dtype)
    dev = torch.device(device)
    if dev.type == "cpu":
        if gathered:
            packed[slots] = rows[gathered].to(dtype)
        return packed, torch.from_numpy(sign)
    examples = _pinned_to_device(packed, dev)
    if gathered:
        examples[_pinned_to_device(torch.tensor(slots, dtype=torch.int64), dev)] = \
            rows[_pinned_to_device(torch.tensor(gathered, dtype=torch.int64), dev)]
    return examples, _pinned_to_device(torch.from_numpy(sign), dev)


def check_recommend_request(who: str, sign, neg_weight, R: int):
    """HOST sign [16 R] and weights [R] (or one number) of recommend_topk, checked: (int8 [16 R], float32 [R]); None
    passes through (a device tensor the caller vouches for).  ValueError for a wrong length, a sign outside
    {-1, 0, 1}, a request without a positive and a non-finite or negative weight."""
    E = MAX_RECOMMEND_EXAMPLES
    s = w = None
    if sign is not None:
        s = np.asarray(sign.cpu() if isinstance(sign, torch.Tensor) else sign).reshape(-1)
        if s.size != E * R:
            raise ValueError(f"{who}: sign holds {s.size} entries, expected {E} per request = {E * R}")
        if not np.isin(s, (-1, 0, 1)).all():
            raise ValueError(f"{who}: a sign must be -1, 0 or 1")
        s = s.astype(np.int8)
        lacking = np.nonzero(~(s.reshape(R, E) > 0).any(axis=1))[0]
        if lacking.size:
            raise ValueError(f"{who}: request {int(lacking[0])} has no positive example")
    if neg_weight is not None:
        w = np.asarray(neg_weight.cpu() if isinstance(neg_weight, torch.Tensor) else neg_weight,
                       dtype=np.float64).reshape(-1)
        if np.ndim(neg_weight) == 0:                  # a number, or a 0-d array / tensor: the same for every request
            w = np.full(R, w[0])
        if w.size != R:
            raise ValueError(f"{who}: neg_weight holds {w.size} entries, expected {R}")
        if not (np.isfinite(w).all() and (w >= 0).all()):
            raise ValueError(f"{who}: neg_weight must be finite and >= 0")
        w = w.astype(np.float32)
    return s, w


def recommend_topk(examples: torch.Tensor, sign, neg_weight, rows: torch.Tensor, n: int, d: int, k: int,
                   alive_bits: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                   row_offset: int = 0, cap: int = 0, dbg: int = 0, want_explain: bool = True, checked: bool = False):
    """Top-k of each request over the first n of `rows` [cap, ld] by "more like these, less like those"
    (include/mmrag.h mmrag_recommend_topk): `examples` [16 R, ld] and `sign` [16 R] as pack_examples returns them,
    final = fmaf(-w, max(neg, 0), pos) inside one exact scan.  `sign` / `neg_weight` (a number, or one per request)
    are checked on the host and uploaded; device tensors (int8 / float32) are used as they are after a copy of them was
    checked, which waits for the stream -- unless `checked`: pack_examples and check_recommend_request made them
    (VectorIndex).  Returns (scores [R, k] float32 = final descending, rows [R, k] int64 + row_offset, pos, neg [R, k]
    float32, pos_arg, neg_arg [R, k] int32 = the slot that gave them, -1 for none), (-inf, -1, 0, 0, -1, -1) padded;
    the last four are None without `want_explain`.  Raises ValueError for a request without a positive, a sign outside
    {-1, 0, 1}, a non-finite or negative weight, a wrong length and k outside 1..MAX_K_DEEP, before anything is
    launched.  `cap`, `dbg` (tests only): fewer slots; dbg & 1 = no bound passes."""
    E = MAX_RECOMMEND_EXAMPLES
    _dev_check(examples, rows, alive_bits)
    _check_q_rows("recommend_topk", examples, rows, n, other="rows")
    _check_stored_rows("recommend_topk", rows)
    n, k = int(n), int(k)
    if examples.shape[0] == 0 or examples.shape[0] % E:
        raise ValueError(f"recommend_topk: examples hold {examples.shape[0]} rows, expected {E} per request")
    R, ld = examples.shape[0] // E, examples.shape[1]
    if not 1 <= k <= MAX_K_DEEP:
        raise ValueError(f"recommend_topk: k={k} outside 1..{MAX_K_DEEP}")
    _check_alive("recommend_topk", alive_bits, n, rows)
    dev = examples.device
    sign_dev = sign if isinstance(sign, torch.Tensor) and sign.is_cuda else None
    w_dev = neg_weight if isinstance(neg_weight, torch.Tensor) and neg_weight.is_cuda else None
    if sign_dev is not None and (sign_dev.dtype != torch.int8 or sign_dev.numel() != E * R
                                 or not sign_dev.is_contiguous() or sign_dev.device != dev):
        raise ValueError(f"recommend_topk: sign must be a contiguous int8 tensor of {E * R} entries on the rows' device")
    if w_dev is not None and (w_dev.dtype != torch.float32 or w_dev.numel() != R or not w_dev.is_contiguous()
                              or w_dev.device != dev):
        raise ValueError(f"recommend_topk: neg_weight must be a contiguous float32 tensor of {R} entries on the rows' "
                         f"device")
    s_host, w_host = check_recommend_request("recommend_topk", None if checked and sign_dev is not None else sign,
                                             None if checked and w_dev is not None else neg_weight, R)
    if sign_dev is None:
        sign_dev = _pinned_to_device(torch.from_numpy(s_host), dev)
    if w_dev is None:
        w_dev = _pinned_to_device(torch.from_numpy(w_host), dev)
    need = recommend_topk_workspace_bytes(R, n, k)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    out_s, out_r = _topk_out(R, k, dev)
    expl = [None] * 4
    if want_explain:
        expl = [torch.empty((R, k), dtype=t, device=dev)
                for t in (torch.float32, torch.float32, torch.int32, torch.int32)]
    with torch.cuda.device(dev):
        st = lib().mmrag_internal_recommend_topk_ex(
            examples.data_ptr(), sign_dev.data_ptr(), w_dev.data_ptr(), rows.data_ptr(), R, n, int(d), ld,
            _TORCH2DT[examples.dtype], k, int(row_offset), alive_bits.data_ptr() if alive_bits is not None else None,
            out_s.data_ptr(), out_r.data_ptr(), *[t.data_ptr() if t is not None else None for t in expl],
            workspace.data_ptr(), _nbytes(workspace), _stream_ptr(dev), int(cap), int(dbg))
    _check(st, "mmrag_recommend_topk")
    return (out_s, out_r, *expl)


_DT_NAME = {torch.float16: "float16", torch.uint8: "uint8"}     # what the MaxSim wrappers call their row tensors


def check_late_tables(q_rows: int, d_rows: int, q_start, q_len, d_start, d_len, pair_q, pair_d) -> Tuple[int, int, int]:
    """The sequence and pair tables of maxsim_scores as HOST integer sequences, checked the way the device cannot
    report (there a bad pair only gets a NaN): returns (n_q, n_d, P).  Raises MMRagNativeError for tables of unequal
    length, no pair or more than MAX_LATE_PAIRS, a pair index outside its table, a query of 0 or more than
    MAX_LATE_QUERY_TOKENS tokens, a passage of 0 or more than MAX_LATE_DOC_TOKENS, and a sequence that does not lie
    inside its buffer's rows."""
    qs, ql, ds, dl = ([int(v) for v in t] for t in (q_start, q_len, d_start, d_len))
    pq, pd = [int(v) for v in pair_q], [int(v) for v in pair_d]
    if len(qs) != len(ql) or len(ds) != len(dl) or not qs or not ds:
        raise MMRagNativeError("maxsim_scores: start and len tables must have one entry per sequence, at least one "
                               "sequence on each side")
    if len(pq) != len(pd) or not 1 <= len(pq) <= MAX_LATE_PAIRS:
        raise MMRagNativeError(f"maxsim_scores: pair_q and pair_d must hold the same 1..{MAX_LATE_PAIRS} pairs "
                               f"(got {len(pq)} and {len(pd)})")
    for side, starts, lens, rows, most in (("query", qs, ql, int(q_rows), MAX_LATE_QUERY_TOKENS),
                                           ("passage", ds, dl, int(d_rows), MAX_LATE_DOC_TOKENS)):
        for s, (a, n) in enumerate(zip(starts, lens)):
            if not 1 <= n <= most:
                raise MMRagNativeError(f"maxsim_scores: {side} {s} has {n} tokens, outside 1..{most}")
            if a < 0 or a + n > rows:
                raise MMRagNativeError(f"maxsim_scores: {side} {s} (rows {a}..{a + n}) is outside the {rows} rows given")
    for name, idx, n in (("pair_q", pq, len(qs)), ("pair_d", pd, len(ds))):
        bad = [v for v in idx if not 0 <= v < n]
        if bad:
            raise MMRagNativeError(f"maxsim_scores: {name} {bad[0]} outside 0..{n - 1}")
    return len(qs), len(ds), len(pq)


def maxsim_scores(q_tok: torch.Tensor, d_tok: torch.Tensor, dim: int, q_start, q_len, d_start, d_len, pair_q, pair_d,
                  want_best: bool = True, _f8: bool = False):
    """Late-interaction (MaxSim) scores of (query, passage) pairs over fp16 token rows (include/mmrag.h
    mmrag_maxsim_scores).  `q_tok` [q_rows, ld] and `d_tok` [d_rows, ld] are device tensors of unit rows (they may be the
    same tensor); sequence s of a side is rows start[s] .. start[s] + len[s].  The six tables are HOST integer tensors
    or sequences: they are checked here (check_late_tables) and copied to the device in one transfer.  Returns device
    tensors (sums [P] float32, best_sim [P, MAX_LATE_QUERY_TOKENS] float32, best_idx [P, MAX_LATE_QUERY_TOKENS] int32),
    the last two None unless `want_best`; slots i >= q_len of a pair are not written.  One launch on the current
    stream, no host synchronisation.  (`_f8`: maxsim_scores_f8's switch.)"""
    who, row_dtype = ("maxsim_scores_f8", torch.uint8) if _f8 else ("maxsim_scores", torch.float16)
    _dev_check(q_tok, d_tok)
    for name, t in (("q_tok", q_tok), ("d_tok", d_tok)):
        if t.dim() != 2 or not t.is_contiguous() or t.dtype != row_dtype:
            raise MMRagNativeError(f"{who}: {name} must be a contiguous 2-D {_DT_NAME[row_dtype]} tensor")
    if q_tok.device != d_tok.device:
        raise MMRagNativeError(f"{who}: q_tok and d_tok must be on one device")
    tables = [torch.as_tensor(t, dtype=torch.int32).reshape(-1).cpu()
              for t in (q_start, q_len, d_start, d_len, pair_q, pair_d)]
    n_q, n_d, P = check_late_tables(q_tok.shape[0], d_tok.shape[0], *(t.tolist() for t in tables))
    dev = q_tok.device
    packed = _pinned_to_device(torch.cat(tables), dev)
    at = [0, n_q, 2 * n_q, 2 * n_q + n_d, 2 * n_q + 2 * n_d, 2 * n_q + 2 * n_d + P]
    qs, ql, ds, dl, pq, pd = (packed[lo:] for lo in at)
    sums = torch.empty(P, dtype=torch.float32, device=dev)
    best_sim = torch.empty((P, MAX_LATE_QUERY_TOKENS), dtype=torch.float32, device=dev) if want_best else None
    best_idx = torch.empty((P, MAX_LATE_QUERY_TOKENS), dtype=torch.int32, device=dev) if want_best else None
    with torch.cuda.device(dev):
        fn = lib().mmrag_maxsim_scores_f8 if _f8 else lib().mmrag_maxsim_scores
        st = fn(q_tok.data_ptr(), q_tok.shape[0], q_tok.shape[1], d_tok.data_ptr(), d_tok.shape[0], d_tok.shape[1],
                int(dim), qs.data_ptr(), ql.data_ptr(), n_q, ds.data_ptr(), dl.data_ptr(), n_d, pq.data_ptr(),
                pd.data_ptr(), P, sums.data_ptr(), _ptr(best_sim), _ptr(best_idx), _stream_ptr(dev))
    _check(st, "mmrag_" + who)
    return sums, best_sim, best_idx


def maxsim_scores_f8(q_codes: torch.Tensor, d_codes: torch.Tensor, dim: int, q_start, q_len, d_start, d_len, pair_q,
                     pair_d, want_best: bool = True):
    """maxsim_scores over rows of E4M3 codes on BOTH sides (include/mmrag.h mmrag_maxsim_scores_f8): contiguous uint8
    tensors [rows, ld], ld = padded_dim(dim, torch.float8_e4m3fn) or more whole slabs, as f8_encode_rows writes them.
    A similarity is the decoded rows' float32 dot product times 2^-16; everything else is maxsim_scores'."""
    return maxsim_scores(q_codes, d_codes, dim, q_start, q_len, d_start, d_len, pair_q, pair_d, want_best, _f8=True)


def maxsim_windows(q_tok: torch.Tensor, d_tok: torch.Tensor, dim: int, q_start, q_len, d_start, d_len, pair_q, pair_d,
                   window_blocks: int, _f8: bool = False):
    """The best window of each (query, passage) pair by windowed MaxSim (include/mmrag.h mmrag_maxsim_windows).  The
    arguments are maxsim_scores' (the same host table checks, one transfer) plus `window_blocks`, the window width in
    blocks of LATE_WINDOW_TOKENS passage tokens, 1..MAX_LATE_WINDOWS.  Returns device tensors (sums [P] float32, the
    bits of maxsim_scores'; win [P, MAX_LATE_WINDOWS] float32, -inf past a pair's last window; best [P, 3] int32:
    start, first, last in blocks).  One launch on the current stream, no host synchronisation.  (`_f8`:
    maxsim_windows_f8's switch.)"""
    who, row_dtype = ("maxsim_windows_f8", torch.uint8) if _f8 else ("maxsim_windows", torch.float16)
    _dev_check(q_tok, d_tok)
    for name, t in (("q_tok", q_tok), ("d_tok", d_tok)):
        if t.dim() != 2 or not t.is_contiguous() or t.dtype != row_dtype:
            raise MMRagNativeError(f"{who}: {name} must be a contiguous 2-D {_DT_NAME[row_dtype]} tensor")
    if q_tok.device != d_tok.device:
        raise MMRagNativeError(f"{who}: q_tok and d_tok must be on one device")
    if not 1 <= int(window_blocks) <= MAX_LATE_WINDOWS:
        raise MMRagNativeError(f"{who}: window_blocks={window_blocks} outside 1..{MAX_LATE_WINDOWS}")
    tables = [torch.as_tensor(t, dtype=torch.int32).reshape(-1).cpu()
              for t in (q_start, q_len, d_start, d_len, pair_q, pair_d)]
    n_q, n_d, P = check_late_tables(q_tok.shape[0], d_tok.shape[0], *(t.tolist() for t in tables))
    dev = q_tok.device
    packed = _pinned_to_device(torch.cat(tables), dev)
    at = [0, n_q, 2 * n_q, 2 * n_q + n_d, 2 * n_q + 2 * n_d, 2 * n_q + 2 * n_d + P]
    qs, ql, ds, dl, pq, pd = (packed[lo:] for lo in at)
    sums = torch.empty(P, dtype=torch.float32, device=dev)
    win = torch.empty((P, MAX_LATE_WINDOWS), dtype=torch.float32, device=dev)
    best = torch.empty((P, 3), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        fn = lib().mmrag_maxsim_windows_f8 if _f8 else lib().mmrag_maxsim_windows
        st = fn(q_tok.data_ptr(), q_tok.shape[0], q_tok.shape[1], d_tok.data_ptr(), d_tok.shape[0], d_tok.shape[1],
                int(dim), qs.data_ptr(), ql.data_ptr(), n_q, ds.data_ptr(), dl.data_ptr(), n_d, pq.data_ptr(),
                pd.data_ptr(), P, int(window_blocks), sums.data_ptr(), win.data_ptr(), best.data_ptr(),
                _stream_ptr(dev))
    _check(st, "mmrag_" + who)
    return sums, win, best


def maxsim_windows_f8(q_codes: torch.Tensor, d_codes: torch.Tensor, dim: int, q_start, q_len, d_start, d_len, pair_q,
                      pair_d, window_blocks: int):
    """maxsim_windows over rows of E4M3 codes on BOTH sides (include/mmrag.h mmrag_maxsim_windows_f8), the operands of
    maxsim_scores_f8; sums has the bits of maxsim_scores_f8's."""
    return maxsim_windows(q_codes, d_codes, dim, q_start, q_len, d_start, d_len, pair_q, pair_d, window_blocks,
                          _f8=True)


def summary_select(rows: torch.Tensor, d: int, unit_start: torch.Tensor, unit_len: torch.Tensor, cost: torch.Tensor,
                   budget: torch.Tensor, k: int, edge_threshold: float, alpha: float, iterations: int, lam: float,
                   bias_rows: Optional[torch.Tensor] = None, unit_bias: Optional[torch.Tensor] = None,
                   want_rel: bool = True, out=None):
    """Extractive selection by sentence centrality (include/mmrag.h mmrag_summary_select): unit u is the sentences
    rows[unit_start[u] : unit_start[u] + unit_len[u]] (1..MAX_SUMMARY_SENTENCES of them) with costs cost[...] and the
    budget budget[u]; LexRank centrality over the unit's similarity graph, then at most k picks by budgeted MMR.
    `rows` [n_rows, ld] is a device tensor of a storage dtype (float32 / float16 / bfloat16), pad columns zero; the
    four tables are DEVICE int32 tensors (unit_start, unit_len, budget [n_units]; cost [n_rows]) and are not read by
    the host: a unit whose entry is out of range gets NaN in val[u, 0].  `bias_rows` [n_bias, ld] with `unit_bias`
    [n_units] (device int32, -1 = none for that unit) bias units toward a row, e.g. an encoded question.  Returns
    device tensors (pos [n_units, k] int32, -1 padded; val [n_units, k] float32, -inf padded; rel [n_rows] float32 or
    None unless `want_rel`, rows of no valid unit not written; used [n_units] int32).  `out`: the four to write into
    (a caller that replays a captured graph).  One launch on the current stream, no host synchronisation."""
    who = "summary_select"
    tables = (unit_start, unit_len, cost, budget)
    _dev_check(rows, bias_rows, unit_bias, *tables)
    _check_stored_rows(who, rows)
    for t in tables + ((unit_bias,) if unit_bias is not None else ()):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != rows.device:
            raise MMRagNativeError(f"{who}: the tables must be contiguous 1-D int32 tensors on the rows' device")
    n_rows, n_units = int(rows.shape[0]), int(unit_start.shape[0])
    if unit_len.shape[0] != n_units or budget.shape[0] != n_units or cost.shape[0] != n_rows:
        raise MMRagNativeError(f"{who}: unit_start, unit_len and budget need one entry per unit, cost one per row")
    if (bias_rows is None) != (unit_bias is None):
        raise MMRagNativeError(f"{who}: bias_rows and unit_bias go together")
    if bias_rows is not None:
        _check_q_rows(who, bias_rows, rows, other="rows")
        if unit_bias.shape[0] != n_units or bias_rows.device != rows.device:
            raise MMRagNativeError(f"{who}: unit_bias needs one entry per unit, bias_rows the rows' device")
    dev = rows.device
    if out is None:
        k_alloc = max(int(k), 1)
        out = (torch.empty((n_units, k_alloc), dtype=torch.int32, device=dev),
               torch.empty((n_units, k_alloc), dtype=torch.float32, device=dev),
               torch.empty(n_rows, dtype=torch.float32, device=dev) if want_rel else None,
               torch.empty(n_units, dtype=torch.int32, device=dev))
    pos, val, rel, used = out
    with torch.cuda.device(dev):
        st = lib().mmrag_summary_select(rows.data_ptr(), rows.shape[1], _TORCH2DT[rows.dtype], int(d), n_rows,
                                        unit_start.data_ptr(), unit_len.data_ptr(), n_units, cost.data_ptr(),
                                        budget.data_ptr(), _ptr(bias_rows),
                                        int(bias_rows.shape[0]) if bias_rows is not None else 0, _ptr(unit_bias),
                                        float(edge_threshold), float(alpha), int(iterations), float(lam), int(k),
                                        pos.data_ptr(), val.data_ptr(), _ptr(rel), used.data_ptr(), _stream_ptr(dev))
    _check(st, "mmrag_summary_select")
    return pos, val, rel, used


def chunk_boundaries(rows: torch.Tensor, d: int, doc_start: torch.Tensor, doc_len: torch.Tensor, cost: torch.Tensor,
                     max_cost: int, max_sentences: int, threshold: float = 0.0, auto_scale: float = 0.0,
                     penalty: float = 0.0, out=None):
    """Semantic chunking (include/mmrag.h mmrag_chunk_boundaries): document u is the sentences rows[doc_start[u] :
    doc_start[u] + doc_len[u]] (any number of them) with costs cost[...]; the partition into chunks of at most
    `max_sentences` (1..MAX_CHUNK_SENTENCES) sentences and at most `max_cost` (a single sentence is always a chunk)
    with the greatest sum of (S_ij - tau) over the pairs inside a chunk minus `penalty` per chunk.  tau is `threshold`,
    or with auto_scale > 0 auto_scale times the document's mean adjacent similarity.  `rows` [n_rows, ld] is a device
    tensor of a storage dtype (float32 / float16 / bfloat16), pad columns zero; the three tables are DEVICE int32
    tensors (doc_start, doc_len [n_docs]; cost [n_rows]) and are not read by the host: a document whose entry is out
    of range gets NaN in score[u].  Returns device tensors (prev [n_rows] int32: prev[doc_start + b - 1] = where the
    chunk that ends before sentence b begins; best [n_rows] float32; tau [n_docs] float32; score [n_docs] float32);
    rows of no valid document are not written.  `out`: the four to write into (a caller that replays a captured
    graph).  One launch on the current stream, no host synchronisation."""
    who = "chunk_boundaries"
    tables = (doc_start, doc_len, cost)
    _dev_check(rows, *tables)
    _check_stored_rows(who, rows)
    for t in tables:
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != rows.device:
            raise MMRagNativeError(f"{who}: the tables must be contiguous 1-D int32 tensors on the rows' device")
    n_rows, n_docs = int(rows.shape[0]), int(doc_start.shape[0])
    if doc_len.shape[0] != n_docs or cost.shape[0] != n_rows:
        raise MMRagNativeError(f"{who}: doc_start and doc_len need one entry per document, cost one per row")
    if not 1 <= int(max_cost) < 2 ** 31:
        raise MMRagNativeError(f"{who}: max_cost={max_cost} outside 1..2^31 - 1")
    dev = rows.device
    if out is None:
        out = (torch.empty(n_rows, dtype=torch.int32, device=dev), torch.empty(n_rows, dtype=torch.float32, device=dev),
               torch.empty(n_docs, dtype=torch.float32, device=dev), torch.empty(n_docs, dtype=torch.float32, device=dev))
    prev, best, tau, score = out
    _dev_check(*out)
    with torch.cuda.device(dev):
        st = lib().mmrag_chunk_boundaries(rows.data_ptr(), rows.shape[1], _TORCH2DT[rows.dtype], int(d), n_rows,
                                          doc_start.data_ptr(), doc_len.data_ptr(), n_docs, cost.data_ptr(),
                                          int(max_cost), int(max_sentences), float(threshold), float(auto_scale),
                                          float(penalty), prev.data_ptr(), best.data_ptr(), tau.data_ptr(),
                                          score.data_ptr(), _stream_ptr(dev))
    _check(st, "mmrag_chunk_boundaries")
    return prev, best, tau, score


def attribute(rows: torch.Tensor, d: int, claim_start: torch.Tensor, claim_len: torch.Tensor, ev_start: torch.Tensor,
              ev_len: torch.Tensor, ev_source: torch.Tensor, n_sources: int, m: int, max_claims: int,
              want_support: bool = True, out=None):
    """Answer citations (include/mmrag.h mmrag_attribute): unit u is the claims rows[claim_start[u] : + claim_len[u]]
    (1..MAX_CLAIMS) and the evidence rows[ev_start[u] : + ev_len[u]] (0..MAX_EVIDENCE), evidence row j belonging to
    source ev_source[ev_start[u] + j]; for every claim and source the best-supporting evidence row, then per claim the
    `m` best sources.  `rows` [n_rows, ld] is a device tensor of a storage dtype (float32 / float16 / bfloat16), pad
    columns zero; the five tables are DEVICE int32 tensors (the four unit tables [n_units]; ev_source [n_rows]) and are
    not read by the host: a unit whose entry is out of range gets NaN in score[u, 0, 0].  Returns device tensors (src,
    ev [n_units, max_claims, m] int32, -1 padded; score [n_units, max_claims, m] float32, -inf padded; support
    [n_units, max_claims, n_sources] float32 or None unless `want_support`, claims past a unit's not written).  `out`:
    the four to write into (a caller that replays a captured graph).  One launch on the current stream, no host
    synchronisation."""
    who = "attribute"
    tables = (claim_start, claim_len, ev_start, ev_len, ev_source)
    _dev_check(rows, *tables)
    _check_stored_rows(who, rows)
    for t in tables:
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != rows.device:
            raise MMRagNativeError(f"{who}: the tables must be contiguous 1-D int32 tensors on the rows' device")
    n_rows, n_units = int(rows.shape[0]), int(claim_start.shape[0])
    if any(t.shape[0] != n_units for t in tables[1:4]) or ev_source.shape[0] != n_rows:
        raise MMRagNativeError(f"{who}: the unit tables need one entry per unit, ev_source one per row")
    dev = rows.device
    if out is None:
        shape = (n_units, max(int(max_claims), 1), max(int(m), 1))
        out = (torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.int32, device=dev),
               torch.empty(shape, dtype=torch.float32, device=dev),
               torch.empty(shape[:2] + (max(int(n_sources), 1),), dtype=torch.float32, device=dev)
               if want_support else None)
    src, ev, score, support = out
    _dev_check(*out)
    with torch.cuda.device(dev):
        st = lib().mmrag_attribute(rows.data_ptr(), rows.shape[1], _TORCH2DT[rows.dtype], int(d), n_rows,
                                   claim_start.data_ptr(), claim_len.data_ptr(), ev_start.data_ptr(),
                                   ev_len.data_ptr(), n_units, ev_source.data_ptr(), int(n_sources), int(m),
                                   int(max_claims), src.data_ptr(), ev.data_ptr(), score.data_ptr(), _ptr(support),
                                   _stream_ptr(dev))
    _check(st, "mmrag_attribute")
    return src, ev, score, support


def f8_encode_rows(src: torch.Tensor, d: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The E4M3 code rows of `src` [m, >= d] (a device float16 or float32 tensor whose rows are contiguous; d defaults
    to its width): uint8 [m, padded_dim(d, torch.float8_e4m3fn)], pad columns code 0 (include/mmrag.h
    mmrag_f8_encode_rows).  One launch on the current stream."""
    _dev_check(src)
    if (src.dim() != 2 or src.dtype not in (torch.float16, torch.float32) or src.stride(1) != 1
            or (src.shape[0] > 1 and src.stride(0) < src.shape[1])):
        raise MMRagNativeError("f8_encode_rows: src must be a 2-D float16 or float32 tensor with contiguous rows")
    m, d = int(src.shape[0]), int(src.shape[1] if d is None else d)
    if not 0 < d <= src.shape[1]:
        raise MMRagNativeError(f"f8_encode_rows: d={d} outside 1..{src.shape[1]}")
    ld = padded_dim(d, torch.float8_e4m3fn)
    if out is None:
        out = torch.empty((m, ld), dtype=torch.uint8, device=src.device)
    elif (out.dim() != 2 or out.dtype != torch.uint8 or not out.is_contiguous() or out.shape[0] < m
          or out.shape[1] < ld or out.device != src.device):
        raise MMRagNativeError(f"f8_encode_rows: out must be a contiguous uint8 tensor of at least [{m}, {ld}] on "
                               f"src's device")
    src_ld = int(src.stride(0)) if m > 1 else int(src.shape[1])
    with torch.cuda.device(src.device):
        st = lib().mmrag_f8_encode_rows(src.data_ptr(), _TORCH2DT[src.dtype], m, d, src_ld, out.data_ptr(),
                                        out.shape[1], _stream_ptr(src.device))
    _check(st, "mmrag_f8_encode_rows")
    return out[:m]


def maxsim_topk_workspace_bytes(Q: int, n_items: int, k: int, dim: int = 0, max_tiles: int = 0,
                                dtype: torch.dtype = torch.float16) -> int:
    """the public bound (any dim, a tile per question), or with `dim` what a call at that dim with at most `max_tiles`
    question tiles (0: Q) needs; `dtype`: torch.float16 (mmrag_maxsim_topk) or torch.float8_e4m3fn (the FP8 scan)"""
    if dtype not in (torch.float16, torch.float8_e4m3fn):
        raise ValueError(f"maxsim_topk_workspace_bytes: dtype must be float16 or float8_e4m3fn (got {dtype})")
    L, f8 = lib(), dtype == torch.float8_e4m3fn
    if not dim:
        fn = L.mmrag_maxsim_topk_f8_workspace_bytes if f8 else L.mmrag_maxsim_topk_workspace_bytes
        return int(fn(int(Q), int(n_items), int(k)))
    fn = L.mmrag_internal_maxsim_topk_f8_workspace_bytes_ex if f8 else L.mmrag_internal_maxsim_topk_workspace_bytes_ex
    return int(fn(int(Q), int(n_items), int(k), int(dim), int(max_tiles)))


def late_question_tiles(q_start, q_len, q_rows: int) -> int:
    """the 128-row tiles the scan packs these questions into (whole questions, greedily, in order; a question the
    device would refuse is in none): the kernel's own rule on the host copies, at least 1"""
    tiles, used = 0, MAX_LATE_QUERY_TOKENS + 1
    for a, n in zip(q_start, q_len):
        if not 1 <= n <= MAX_LATE_QUERY_TOKENS or a < 0 or a + n > q_rows:
            continue
        if used + n > MAX_LATE_QUERY_TOKENS:
            tiles, used = tiles + 1, 0
        used += n
    return max(tiles, 1)


def maxsim_topk(q_tok: torch.Tensor, q_start, q_len, tok: torch.Tensor, n_rows: int, item_off: torch.Tensor,
                n_items: int, dim: int, k: int, alive_bits: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None, chunk_rows: int = 0, cap: int = 0, dbg: int = 0,
                check_tables: bool = True, _f8: bool = False):
    """Each question's exact MaxSim top-k over the items of a token plane (include/mmrag.h mmrag_maxsim_topk).
    `q_tok` [q_rows, ld] and `tok` [>= n_rows, ld] are contiguous device float16 tensors; question s is rows
    q_start[s] .. q_start[s] + q_len[s] (HOST integer sequences, checked here unless `check_tables` is false -- then a
    bad question only gets padding -- and uploaded in one transfer).  `item_off`: a device int32 tensor of at least
    n_items + 1 ascending offsets into the first n_rows rows of `tok`; `alive_bits`: an optional device int32 bitmap
    over items.  Returns (scores [Q, k] float32 descending, items [Q, k] int64), (-inf, -1) padded.  No host
    synchronisation unless n_items exceeds the candidate slots of a question.  `chunk_rows`, `cap`, `dbg` (tests and
    tools): the plane rows per chunk, fewer candidate slots, dbg & 1 = no bound passes.  (`_f8`: maxsim_topk_f8's
    switch.)"""
    who, row_dtype = ("maxsim_topk_f8", torch.uint8) if _f8 else ("maxsim_topk", torch.float16)
    _dev_check(q_tok, tok, item_off)
    for name, t in (("q_tok", q_tok), ("tok", tok)):
        if t.dim() != 2 or not t.is_contiguous() or t.dtype != row_dtype:
            raise MMRagNativeError(f"{who}: {name} must be a contiguous 2-D {_DT_NAME[row_dtype]} tensor")
    dev = q_tok.device
    n_rows, n_items, k = int(n_rows), int(n_items), int(k)
    if not 1 <= k <= MAX_K_DEEP:
        raise ValueError(f"{who}: k={k} outside 1..{MAX_K_DEEP}")
    if tok.device != dev or item_off.device != dev or (alive_bits is not None and alive_bits.device != dev):
        raise MMRagNativeError(f"{who}: q_tok, tok, item_off and alive_bits must be on one device")
    if not 0 <= n_rows <= tok.shape[0]:
        raise MMRagNativeError(f"{who}: n_rows={n_rows} outside the {tok.shape[0]} rows of tok")
    if (item_off.dim() != 1 or item_off.dtype != torch.int32 or not item_off.is_contiguous() or n_items < 0
            or item_off.numel() < n_items + 1):
        raise MMRagNativeError(f"{who}: item_off must be a contiguous int32 tensor of at least n_items + 1 = "
                               f"{n_items + 1} offsets")
    if alive_bits is not None and (alive_bits.dtype != torch.int32 or not alive_bits.is_contiguous()
                                   or alive_bits.numel() * 32 < n_items):
        raise MMRagNativeError(f"{who}: alive_bits must be a contiguous int32 bitmap over {n_items} items")
    tables = [torch.as_tensor(t, dtype=torch.int32).reshape(-1).cpu() for t in (q_start, q_len)]
    Q = tables[0].numel()
    if tables[1].numel() != Q or not 1 <= Q <= MAX_LATE_QUESTIONS:
        raise MMRagNativeError(f"{who}: q_start and q_len must hold the same 1..{MAX_LATE_QUESTIONS} questions "
                               f"(got {Q} and {tables[1].numel()})")
    if check_tables:
        for s, (a, n) in enumerate(zip(tables[0].tolist(), tables[1].tolist())):
            if not 1 <= n <= MAX_LATE_QUERY_TOKENS:
                raise MMRagNativeError(f"{who}: question {s} has {n} tokens, outside 1..{MAX_LATE_QUERY_TOKENS}")
            if a < 0 or a + n > q_tok.shape[0]:
                raise MMRagNativeError(f"{who}: question {s} (rows {a}..{a + n}) is outside the "
                                       f"{q_tok.shape[0]} rows given")
    packed = _pinned_to_device(torch.cat(tables), dev)
    # the host tables say how many question tiles there are: the grid and the packed tiles are sized by that, not by Q
    tiles = late_question_tiles(tables[0].tolist(), tables[1].tolist(), q_tok.shape[0])
    need = maxsim_topk_workspace_bytes(Q, n_items, k, int(dim), tiles, torch.float8_e4m3fn if _f8 else torch.float16)
    if need == 0:
        raise MMRagNativeError(f"{who}: dim must be a multiple of 64, at most 1024 (dim={dim})")
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    out_s, out_r = _topk_out(Q, k, dev)
    with torch.cuda.device(dev):
        fn = lib().mmrag_internal_maxsim_topk_f8_ex if _f8 else lib().mmrag_internal_maxsim_topk_ex
        st = fn(
            q_tok.data_ptr(), q_tok.shape[0], q_tok.shape[1], packed.data_ptr(), packed[Q:].data_ptr(), Q,
            tok.data_ptr(), n_rows, tok.shape[1], item_off.data_ptr(), n_items, _ptr(alive_bits), int(dim), k,
            out_s.data_ptr(), out_r.data_ptr(), workspace.data_ptr(), _nbytes(workspace), _stream_ptr(dev),
            int(chunk_rows), int(cap), int(dbg), tiles)
    _check(st, "mmrag_" + who)
    return out_s, out_r


def maxsim_topk_f8(q_codes: torch.Tensor, q_start, q_len, codes: torch.Tensor, n_rows: int, item_off: torch.Tensor,
                   n_items: int, dim: int, k: int, alive_bits: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None, chunk_rows: int = 0, cap: int = 0, dbg: int = 0,
                   check_tables: bool = True):
    """maxsim_topk over a plane of E4M3 code rows and code rows of the questions (include/mmrag.h mmrag_maxsim_topk_f8):
    contiguous uint8 tensors [rows, ld], ld = padded_dim(dim, torch.float8_e4m3fn) or more whole slabs.  Scores are
    the quantised rows' own (decoded dot products times 2^-16); everything else is maxsim_topk's."""
    return maxsim_topk(q_codes, q_start, q_len, codes, n_rows, item_off, n_items, dim, k, alive_bits, workspace,
                       chunk_rows, cap, dbg, check_tables, _f8=True)


def join_tile(T: int, at: int, slot_order: bool = False) -> Tuple[int, int]:
    """(ti, tj) of tile-pair id `at` of a T x T triangle: row-major, or (slot_order) in the order the join kernel runs"""
    ti, tj = c_int64(0), c_int64(0)
    fn = lib().mmrag_internal_join_slot_tile if slot_order else lib().mmrag_internal_join_tile
    _check(fn(int(T), int(at), ctypes.byref(ti), ctypes.byref(tj)), "mmrag_internal_join_tile")
    return ti.value, tj.value


def device_info() -> dict:
    """CU count, maximum shader clock and HBM size of the current device (mmrag_device_info)"""
    cus, mhz, mem = c_int(0), c_int(0), c_int64(0)
    _check(lib().mmrag_device_info(ctypes.byref(cus), ctypes.byref(mhz), ctypes.byref(mem)), "mmrag_device_info")
    return {"compute_units": cus.value, "max_clock_mhz": mhz.value, "hbm_bytes": mem.value}


def measure_peaks(device: torch.device, seconds: float = 0.4) -> dict:
    """Measured stream-copy bandwidth and fp16 MFMA rate of this device (the library's own micro-kernels,
    each held for `seconds` so the chip reaches the clock it sustains): the second set of roofline peaks."""
    L = lib()
    out = {}
    with torch.cuda.device(device):
        stream = _stream_ptr(device)
        nbytes = 1 << 30
        src = torch.empty(nbytes, dtype=torch.uint8, device=device)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=device)
        src.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(fn, min_s):
            import time
            fn(); torch.cuda.synchronize(device)
            t_end = time.time() + min_s / 2
            while time.time() < t_end:   # reach the sustained clock first
                for _ in range(4): fn()
                torch.cuda.synchronize(device)
            n = 0
            e0.record()
            t_end = time.time() + min_s / 2
            while time.time() < t_end:
                for _ in range(4): fn()
                n += 4
                torch.cuda.synchronize(device)
            e1.record(); torch.cuda.synchronize(device)
            return e0.elapsed_time(e1) * 1e-3 / n

        t = timed(lambda: _check(L.mmrag_bench_stream_copy(dst.data_ptr(), src.data_ptr(), nbytes, stream), "copy"), seconds)
        out["stream_copy_GBps"] = round(2 * nbytes / t / 1e9, 1)      # bytes read + bytes written
        sink = torch.empty(256 * 8 * 256, dtype=torch.float32, device=device)
        t = timed(lambda: _check(L.mmrag_bench_stream_read(src.data_ptr(), nbytes, sink.data_ptr(), stream), "read"), seconds)
        out["stream_read_GBps"] = round(nbytes / t / 1e9, 1)           # a read-only stream: what a corpus scan is
        t = timed(lambda: _check(L.mmrag_bench_stream_write(dst.data_ptr(), nbytes, stream), "write"), seconds)
        out["stream_write_GBps"] = round(nbytes / t / 1e9, 1)
        del src, dst, sink
        seed = (torch.randn(256 * 8, device=device) * 0.5).to(torch.float16)
        res = torch.empty(256 * 1024, dtype=torch.float32, device=device)
        flops = c_int64(0)
        iters = 20000
        t = timed(lambda: _check(L.mmrag_bench_mfma_f16(seed.data_ptr(), res.data_ptr(), iters, ctypes.byref(flops), stream),
                                 "mfma"), seconds)
        out["mfma_f16_TFLOPs"] = round(flops.value / t / 1e12, 1)
        iters = 5000
        t = timed(lambda: _check(L.mmrag_bench_mfma_f16_16x16x32(seed.data_ptr(), res.data_ptr(), iters,
                                                                 ctypes.byref(flops), stream), "mfma16"), seconds)
        out["mfma_f16_16x16x32_TFLOPs"] = round(flops.value / t / 1e12, 1)
    return out


def cosine_topk_workspace_bytes(B: int, n: int, k: int) -> int:
    return int(lib().mmrag_cosine_topk_workspace_bytes(B, n, k))


def merge_topk(scores: torch.Tensor, rows: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device merge of [G, B, k_in] shard results into [B, k]."""
    _dev_check(scores, rows)
    G, B, k_in = scores.shape
    scores = scores.contiguous()
    rows = rows.contiguous()
    out_s, out_r = _topk_out(B, k, scores.device)
    with torch.cuda.device(scores.device):
        st = lib().mmrag_merge_topk(scores.data_ptr(), rows.data_ptr(), G, B, k_in, k, out_s.data_ptr(),
                                    out_r.data_ptr(), _stream_ptr(scores.device))
    _check(st, "mmrag_merge_topk")
    return out_s, out_r


def merge_topk_host(scores: torch.Tensor, rows: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host (C++) merge of [G, B, k_in] shard results held in CPU tensors into [B, k]."""
    if scores.is_cuda or rows.is_cuda:
        raise MMRagNativeError("merge_topk_host takes CPU tensors")
    G, B, k_in = scores.shape
    scores = scores.contiguous().to(torch.float32)
    rows = rows.contiguous().to(torch.int64)
    out_s = torch.empty((B, k), dtype=torch.float32)
    out_r = torch.empty((B, k), dtype=torch.int64)
    st = lib().mmrag_merge_topk_host(scores.data_ptr(), rows.data_ptr(), G, B, k_in, k, out_s.data_ptr(),
                                     out_r.data_ptr())
    _check(st, "mmrag_merge_topk_host")
    return out_s, out_r


def packed_block_bytes(B: int, k: int) -> int:
    return (B * k * 12 + 7) // 8 * 8


def merge_topk_host_packed(blocks: torch.Tensor, G: int, B: int, k_in: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host merge of G packed rank blocks [rows B*k_in i64 | scores B*k_in f32 | pad to 8 B] (CPU uint8)."""
    if blocks.is_cuda or blocks.dtype != torch.uint8 or blocks.numel() != G * packed_block_bytes(B, k_in):
        raise MMRagNativeError("merge_topk_host_packed takes a CPU uint8 tensor of G * packed_block_bytes(B, k_in) bytes")
    out_s = torch.empty((B, k), dtype=torch.float32)
    out_r = torch.empty((B, k), dtype=torch.int64)
    st = lib().mmrag_merge_topk_host_packed(blocks.data_ptr(), G, B, k_in, k, out_s.data_ptr(), out_r.data_ptr())
    _check(st, "mmrag_merge_topk_host_packed")
    return out_s, out_r


def append_rows(corpus: torch.Tensor, n_used: int, new_rows: torch.Tensor, d: int) -> None:
    """corpus[n_used : n_used+m, :d] = cast(new_rows) with zero pad columns."""
    _dev_check(corpus, new_rows)
    new_rows = new_rows.to(torch.float32).contiguous()
    m = new_rows.shape[0]
    with torch.cuda.device(corpus.device):
        st = lib().mmrag_append_rows(corpus.data_ptr(), corpus.shape[0], corpus.shape[1], _TORCH2DT[corpus.dtype],
                                     n_used, new_rows.data_ptr(), m, d, _stream_ptr(corpus.device))
    _check(st, "mmrag_append_rows")


def gather_rows(dst: torch.Tensor, src: torch.Tensor, keep_rows: torch.Tensor) -> None:
    _dev_check(dst, src, keep_rows)
    keep_rows = keep_rows.to(torch.int64).contiguous()
    with torch.cuda.device(src.device):
        st = lib().mmrag_gather_rows(dst.data_ptr(), src.data_ptr(), src.shape[1], _TORCH2DT[src.dtype],
                                     keep_rows.data_ptr(), keep_rows.numel(), _stream_ptr(src.device))
    _check(st, "mmrag_gather_rows")


def fetch_rows_f32(corpus: torch.Tensor, rows: torch.Tensor, d: int) -> torch.Tensor:
    _dev_check(corpus, rows)
    rows = rows.to(torch.int64).contiguous()
    out = torch.empty((rows.numel(), d), dtype=torch.float32, device=corpus.device)
    with torch.cuda.device(corpus.device):
        st = lib().mmrag_fetch_rows_f32(corpus.data_ptr(), corpus.shape[1], _TORCH2DT[corpus.dtype], rows.data_ptr(),
                                        rows.numel(), d, out.data_ptr(), _stream_ptr(corpus.device))
    _check(st, "mmrag_fetch_rows_f32")
    return out


def cosine_topk_lists(q: torch.Tensor, corpus: torch.Tensor, n: int, d: int, k: int, workspace: torch.Tensor,
                      alive_bits: Optional[torch.Tensor] = None, dbg: int = 0) -> None:
    """Phase 1 of cosine_topk: the fused GEMM + selection kernel; candidates stay in `workspace`."""
    _dev_check(q, corpus, workspace, alive_bits)
    if q.dtype != corpus.dtype or q.shape[1] != corpus.shape[1] or not q.is_contiguous() or not corpus.is_contiguous():
        raise MMRagNativeError("cosine_topk_lists: q and corpus must be contiguous and share dtype and padded width")
    if n > corpus.shape[0]:
        raise MMRagNativeError(f"cosine_topk_lists: n={n} exceeds corpus capacity {corpus.shape[0]}")
    B, ld = q.shape
    with torch.cuda.device(q.device):
        st = lib().mmrag_internal_cosine_topk_lists_ex(
            q.data_ptr(), corpus.data_ptr(), B, n, d, ld, _TORCH2DT[q.dtype], k,
            alive_bits.data_ptr() if alive_bits is not None else None, workspace.data_ptr(),
            _nbytes(workspace), _stream_ptr(q.device), int(dbg))
    _check(st, "mmrag_cosine_topk_lists")


def cosine_topk_select(B: int, n: int, k: int, row_offset: int, workspace: torch.Tensor,
                       out_scores: Optional[torch.Tensor] = None,
                       out_rows: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Phase 2 of cosine_topk: merge the candidate lists in `workspace` into [B, k]."""
    _dev_check(workspace)
    dev = workspace.device
    if out_scores is None:
        out_scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    if out_rows is None:
        out_rows = torch.empty((B, k), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = lib().mmrag_cosine_topk_select(B, n, k, row_offset, workspace.data_ptr(), out_scores.data_ptr(),
                                            out_rows.data_ptr(), _stream_ptr(dev))
    _check(st, "mmrag_cosine_topk_select")
    return out_scores, out_rows


# ----------------------------------------------------------------------------------------------
# encoder building blocks (fp16 tensors on the device)
# ----------------------------------------------------------------------------------------------
ACT_NONE, ACT_GELU, ACT_QUICK_GELU = 0, 1, 2
ARCH_BERT, ARCH_PRELN = 0, 1
POOL_MEAN, POOL_FIRST, POOL_SELECT = 0, 1, 2


class EncoderDesc(ctypes.Structure):
    """mirror of `mmrag_encoder_desc` (include/mmrag.h)"""
    _fields_ = [("arch", c_int32), ("n_layers", c_int32), ("hidden", c_int32), ("n_heads", c_int32),
                ("intermediate", c_int32), ("vocab", c_int32), ("max_pos", c_int32), ("pool", c_int32),
                ("act", c_int32), ("causal", c_int32), ("normalize", c_int32), ("out_dim", c_int32),
                ("ln_eps", c_float), ("image", c_int32), ("patch", c_int32)]


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def linear_f16(x: torch.Tensor, wt: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
               resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M, N] = act(x[M, K] @ wt[N, K].T + bias) (+ resid)"""
    _dev_check(x, wt, bias, resid, out)
    M, K = x.shape
    Nf = wt.shape[0]
    if x.dtype != torch.float16 or wt.dtype != torch.float16 or wt.shape[1] != K:
        raise MMRagNativeError("linear_f16: x [M,K] and wt [N,K] must be fp16 with matching K")
    if out is None:
        out = torch.empty((M, Nf), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        st = lib().mmrag_linear_f16(x.data_ptr(), M, K, wt.data_ptr(), Nf, _ptr(bias), act, _ptr(resid),
                                    out.data_ptr(), _stream_ptr(x.device))
    _check(st, "mmrag_linear_f16")
    return out


def layernorm_f16(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    _dev_check(x, gamma, beta)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = lib().mmrag_layernorm_f16(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), x.shape[0],
                                       x.shape[1], eps, _stream_ptr(x.device))
    _check(st, "mmrag_layernorm_f16")
    return out


def embed_ln_f16(ids, pos_ids, tok, pos, type0, gamma, beta, eps: float) -> torch.Tensor:
    _dev_check(ids, pos_ids, tok, pos, type0, gamma, beta)
    T, H = ids.numel(), tok.shape[1]
    out = torch.empty((T, H), dtype=torch.float16, device=tok.device)
    with torch.cuda.device(tok.device):
        st = lib().mmrag_embed_ln_f16(ids.data_ptr(), pos_ids.data_ptr(), tok.data_ptr(), pos.data_ptr(), _ptr(type0),
                                      _ptr(gamma), _ptr(beta), out.data_ptr(), T, H, tok.shape[0], pos.shape[0], eps,
                                      _stream_ptr(tok.device))
    _check(st, "mmrag_embed_ln_f16")
    return out


def attention_f16(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, n_heads: int,
                  causal: bool = False) -> torch.Tensor:
    _dev_check(qkv, cu_seqlens)
    T, H3 = qkv.shape
    H = H3 // 3
    ctx = torch.empty((T, H), dtype=torch.float16, device=qkv.device)
    with torch.cuda.device(qkv.device):
        st = lib().mmrag_attention_f16(qkv.data_ptr(), cu_seqlens.data_ptr(), ctx.data_ptr(), cu_seqlens.numel() - 1,
                                       max_len, H, n_heads, int(causal), _stream_ptr(qkv.device))
    _check(st, "mmrag_attention_f16")
    return ctx


def pool_normalize_f16(x: torch.Tensor, cu_seqlens: torch.Tensor, pool: int, normalize: bool = True,
                       sel: Optional[torch.Tensor] = None) -> torch.Tensor:
    _dev_check(x, cu_seqlens, sel)
    B, H = cu_seqlens.numel() - 1, x.shape[1]
    out = torch.empty((B, H), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib().mmrag_pool_normalize_f16(x.data_ptr(), cu_seqlens.data_ptr(), _ptr(sel), out.data_ptr(), B, H, pool,
                                            int(normalize), _stream_ptr(x.device))
    _check(st, "mmrag_pool_normalize_f16")
    return out


def linear_f16_norms(x: torch.Tensor, wt: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                     resid: Optional[torch.Tensor] = None, ln_gamma: Optional[torch.Tensor] = None,
                     ln_beta: Optional[torch.Tensor] = None, ln_eps: float = 1e-12,
                     ln_stats_out: Optional[torch.Tensor] = None, res_stats: Optional[torch.Tensor] = None,
                     res_gamma: Optional[torch.Tensor] = None, res_beta: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(tests) one GEMM of the single-query forward (M <= 64): out = act(LN(x) @ wt.T + bias) (+ LN'(resid)), where LN
    is applied when ln_gamma is given (its per-row (mean, rstd) go to ln_stats_out, float32 [M, 2]) and LN' when
    res_stats (float32 [M, 2]) is given"""
    _dev_check(x, wt, bias, resid, ln_gamma, ln_beta, ln_stats_out, res_stats, res_gamma, res_beta)
    M, K = x.shape
    Nf = wt.shape[0]
    out = torch.empty((M, Nf), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        st = lib().mmrag_internal_linear_f16_norms(x.data_ptr(), M, K, wt.data_ptr(), Nf, _ptr(bias), act, _ptr(resid),
                                                   out.data_ptr(), _ptr(ln_gamma), _ptr(ln_beta), ln_eps,
                                                   _ptr(ln_stats_out), _ptr(res_stats), _ptr(res_gamma), _ptr(res_beta),
                                                   _stream_ptr(x.device))
    _check(st, "mmrag_internal_linear_f16_norms")
    return out


def attention_f32(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, n_heads: int) -> torch.Tensor:
    """(tests) the fp32 forward's attention on its own: qkv float32 [T, 3H] -> ctx float32 [T, H]"""
    _dev_check(qkv, cu_seqlens)
    T, H3 = qkv.shape
    ctx = torch.empty((T, H3 // 3), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        st = lib().mmrag_internal_attention_f32(qkv.data_ptr(), cu_seqlens.data_ptr(), ctx.data_ptr(),
                                                cu_seqlens.numel() - 1, max_len, H3 // 3, n_heads,
                                                _stream_ptr(qkv.device))
    _check(st, "mmrag_internal_attention_f32")
    return ctx


def layernorm_f32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """(tests) the fp32 forward's LayerNorm on its own"""
    _dev_check(x, gamma, beta)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = lib().mmrag_internal_layernorm_f32(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                x.shape[0], x.shape[1], eps, _stream_ptr(x.device))
    _check(st, "mmrag_internal_layernorm_f32")
    return out


def pool_norm_f32(x: torch.Tensor, cu_seqlens: torch.Tensor, pool: int, normalize: bool = True,
                  sel: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(tests) the fp32 forward's pooling + L2 normalisation on its own"""
    _dev_check(x, cu_seqlens, sel)
    B, H = cu_seqlens.numel() - 1, x.shape[1]
    out = torch.empty((B, H), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib().mmrag_internal_pool_norm_f32(x.data_ptr(), cu_seqlens.data_ptr(), _ptr(sel), out.data_ptr(), B, H,
                                                pool, int(normalize), _stream_ptr(x.device))
    _check(st, "mmrag_internal_pool_norm_f32")
    return out


def encoder_workspace_bytes(desc: EncoderDesc, T: int, B: int, f32: bool = False) -> int:
    if f32:
        return int(lib().mmrag_encoder_f32_workspace_bytes(ctypes.byref(desc), T, B))
    return int(lib().mmrag_encoder_workspace_bytes(ctypes.byref(desc), T, B))


def linear_f32(x: torch.Tensor, wt: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
               resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = act(x . wt^T + bias) (+ resid), float32 on the exact float32 matrix instruction (the fp32 encoder's GEMM)"""
    _dev_check(x, wt, bias, resid)
    M, K = x.shape
    N = wt.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib().mmrag_linear_f32(x.data_ptr(), M, K, wt.data_ptr(), N, _ptr(bias), act, _ptr(resid), out.data_ptr(),
                                    _stream_ptr(x.device))
    _check(st, "mmrag_linear_f32")
    return out


def encoder_forward(desc: EncoderDesc, weight_ptrs, ids: torch.Tensor, pos_ids: torch.Tensor,
                    cu_seqlens: torch.Tensor, max_len: int, sel: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    f32: bool = False) -> torch.Tensor:
    """One encoder pass over packed token ids -> [B, out_dim] float32.  `weight_ptrs` is a ctypes
    array of c_void_p in the order include/mmrag.h documents (see encoder.DeviceEncoder).  `f32`: the float32 mode
    (mmrag_encoder_forward_f32; every weight float32)."""
    _dev_check(ids, pos_ids, cu_seqlens, sel, workspace, out)
    T, B = ids.numel(), cu_seqlens.numel() - 1
    need = encoder_workspace_bytes(desc, T, B, f32)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=ids.device)
    if out is None:
        out = torch.empty((B, desc.out_dim), dtype=torch.float32, device=ids.device)
    fn = lib().mmrag_encoder_forward_f32 if f32 else lib().mmrag_encoder_forward
    with torch.cuda.device(ids.device):
        st = fn(ctypes.byref(desc), weight_ptrs, ids.data_ptr(), pos_ids.data_ptr(),
                                         cu_seqlens.data_ptr(), _ptr(sel), T, B, max_len, out.data_ptr(),
                                         workspace.data_ptr(), _nbytes(workspace),
                                         _stream_ptr(ids.device))
    _check(st, "mmrag_encoder_forward")
    return out


def encoder_tokens_workspace_bytes(desc: EncoderDesc, T: int, B: int, out_dim: int) -> int:
    return int(lib().mmrag_encoder_tokens_workspace_bytes(ctypes.byref(desc), T, B, int(out_dim)))


def encoder_forward_tokens(desc: EncoderDesc, weight_ptrs, ids: torch.Tensor, pos_ids: torch.Tensor,
                           cu_seqlens: torch.Tensor, max_len: int, proj: Optional[torch.Tensor] = None,
                           workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One encoder pass over packed token ids -> token rows [T, ld] float16 (include/mmrag.h
    mmrag_encoder_forward_tokens): row t is the L2-normalised last hidden state of packed token t, through `proj`
    [out_dim, hidden] fp16 (bias-free) when given.  out_dim is a multiple of 64, so ld = padded_dim(out_dim, float16)
    is out_dim itself: the rows have no pad columns."""
    _dev_check(ids, pos_ids, cu_seqlens, proj, workspace, out)
    T, B = ids.numel(), cu_seqlens.numel() - 1
    out_dim = desc.hidden
    if proj is not None:
        if proj.dim() != 2 or proj.dtype != torch.float16 or not proj.is_contiguous() or proj.shape[1] != desc.hidden:
            raise MMRagNativeError("encoder_forward_tokens: proj must be a contiguous [out_dim, hidden] float16 tensor")
        out_dim = int(proj.shape[0])
    need = encoder_tokens_workspace_bytes(desc, T, B, out_dim)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=ids.device)
    if out is None:
        out = torch.empty((max(T, 1), max(out_dim, 1)), dtype=torch.float16, device=ids.device)
    with torch.cuda.device(ids.device):
        st = lib().mmrag_encoder_forward_tokens(ctypes.byref(desc), weight_ptrs, ids.data_ptr(), pos_ids.data_ptr(),
                                                cu_seqlens.data_ptr(), T, B, max_len, _ptr(proj), out_dim,
                                                out.data_ptr(), workspace.data_ptr(), _nbytes(workspace),
                                                _stream_ptr(ids.device))
    _check(st, "mmrag_encoder_forward_tokens")
    return out


# ---- learned sparse retrieval (include/mmrag.h: mmrag_sparse_expand_forward, _pool, _select, mmrag_impact_topk) ----
MAX_SPARSE_CHUNK_TOKENS, MAX_SPARSE_CHUNKS, MAX_SPARSE_VOCAB = 512, 65536, 65536
MAX_SPARSE_TERMS, MAX_SPARSE_QUERY_TERMS = 256, 64


def sparse_limits() -> dict:
    """csrc/sparse_score.hip's and csrc/sparse_expand.hip's path sizes (mmrag_internal_sparse_limits; tests restate them
    and compare)"""
    v = [ctypes.c_int(0) for _ in range(5)]
    _check(lib().mmrag_internal_sparse_limits(*[ctypes.byref(x) for x in v]), "mmrag_internal_sparse_limits")
    return dict(zip(("impact_rows", "pool_batch", "pool_vrun", "select_terms", "tile_rows"), (int(x.value) for x in v)))


def sparse_expand_forward_workspace_bytes(desc: EncoderDesc, T: int, B: int) -> int:
    return int(lib().mmrag_sparse_expand_forward_workspace_bytes(ctypes.byref(desc), T, B))


def sparse_expand_forward(desc: EncoderDesc, weight_ptrs, ids: torch.Tensor, pos_ids: torch.Tensor,
                          cu_seqlens: torch.Tensor, max_len: int, head_w: torch.Tensor, head_b: torch.Tensor,
                          head_ln_g: torch.Tensor, head_ln_b: torch.Tensor, workspace: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One encoder pass, then a masked-LM head's transform (dense + erf GELU + LayerNorm) -> token rows [T, hidden]
    float16, NOT normalised: the plane sparse_pool reads."""
    _dev_check(ids, pos_ids, cu_seqlens, head_w, head_b, head_ln_g, head_ln_b, workspace, out)
    T, B, H = ids.numel(), cu_seqlens.numel() - 1, desc.hidden
    if head_w.dtype != torch.float16 or tuple(head_w.shape) != (H, H) or not head_w.is_contiguous():
        raise MMRagNativeError("sparse_expand_forward: head_w must be a contiguous [hidden, hidden] float16 tensor")
    for t in (head_b, head_ln_g, head_ln_b):
        if t.dtype != torch.float32 or t.numel() != H or not t.is_contiguous():
            raise MMRagNativeError("sparse_expand_forward: head bias / LayerNorm vectors must be [hidden] float32")
    need = sparse_expand_forward_workspace_bytes(desc, T, B)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=ids.device)
    if out is None:
        out = torch.empty((max(T, 1), H), dtype=torch.float16, device=ids.device)
    with torch.cuda.device(ids.device):
        st = lib().mmrag_sparse_expand_forward(ctypes.byref(desc), weight_ptrs, ids.data_ptr(), pos_ids.data_ptr(),
                                               cu_seqlens.data_ptr(), T, B, max_len, head_w.data_ptr(),
                                               head_b.data_ptr(), head_ln_g.data_ptr(), head_ln_b.data_ptr(),
                                               out.data_ptr(), workspace.data_ptr(), _nbytes(workspace),
                                               _stream_ptr(ids.device))
    _check(st, "mmrag_sparse_expand_forward")
    return out


def sparse_pool(tok: torch.Tensor, cu: torch.Tensor, E: torch.Tensor, dim: int, n_rows: Optional[int] = None,
                V: Optional[int] = None, vrun: int = 0) -> torch.Tensor:
    """pooled [n_chunks, V] float32 = per chunk (rows cu[c] .. cu[c + 1] of `tok`) the maximum over its rows of the
    dot products with the decoder rows `E` [V, ld] (mmrag_sparse_pool).  `tok`, `E`: contiguous 2-D float16, widths of
    whole 128-byte slabs; `cu` int32 on the device.  `vrun` > 0: the vocabulary tiles a workgroup takes
    (mmrag_internal_sparse_pool_ex; the output does not depend on it)."""
    _dev_check(tok, cu, E)
    for name, t in (("tok", tok), ("E", E)):
        if t.dim() != 2 or t.dtype != torch.float16 or not t.is_contiguous():
            raise MMRagNativeError(f"sparse_pool: {name} must be a contiguous 2-D float16 tensor")
    if cu.dtype != torch.int32 or cu.dim() != 1 or not cu.is_contiguous() or cu.numel() < 2:
        raise MMRagNativeError("sparse_pool: cu must be a contiguous int32 vector of n_chunks + 1 offsets")
    T = tok.shape[0] if n_rows is None else int(n_rows)
    V = E.shape[0] if V is None else int(V)
    if T > tok.shape[0] or V > E.shape[0]:
        raise MMRagNativeError("sparse_pool: n_rows / V exceed the tensors")
    n_chunks = cu.numel() - 1
    pooled = torch.empty((max(n_chunks, 1), max(V, 1)), dtype=torch.float32, device=tok.device)
    with torch.cuda.device(tok.device):
        args = (tok.data_ptr(), T, tok.shape[1], cu.data_ptr(), n_chunks, E.data_ptr(), V, E.shape[1], int(dim),
                pooled.data_ptr())
        if vrun:
            st = lib().mmrag_internal_sparse_pool_ex(*args, _stream_ptr(tok.device), int(vrun))
        else:
            st = lib().mmrag_sparse_pool(*args, None, 0, _stream_ptr(tok.device))
    _check(st, "mmrag_sparse_pool")
    return pooled


def sparse_select(pooled: torch.Tensor, bias: torch.Tensor, scale: float, m: int,
                  skip_bits: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(count [n_chunks], terms [n_chunks, m], impacts [n_chunks, m]) int32 on the device: per chunk the m terms of
    highest 8-bit impact min(255, rint(log1p(relu(pooled + bias)) * scale)) >= 1, ties to the lower term id, written
    in ascending term id; (-1, 0) behind them (mmrag_sparse_select)."""
    _dev_check(pooled, bias, skip_bits)
    if pooled.dim() != 2 or pooled.dtype != torch.float32 or not pooled.is_contiguous():
        raise MMRagNativeError("sparse_select: pooled must be a contiguous [n_chunks, V] float32 tensor")
    n_chunks, V = pooled.shape
    if bias.dtype != torch.float32 or bias.numel() != V or not bias.is_contiguous():
        raise MMRagNativeError("sparse_select: bias must be a contiguous [V] float32 tensor")
    if skip_bits is not None and (skip_bits.dtype != torch.int32 or skip_bits.numel() < (V + 31) // 32
                                  or not skip_bits.is_contiguous()):
        raise MMRagNativeError("sparse_select: skip_bits must be ceil(V / 32) int32 words")
    dev = pooled.device
    cnt = torch.empty(max(n_chunks, 1), dtype=torch.int32, device=dev)
    terms = torch.empty((max(n_chunks, 1), max(int(m), 1)), dtype=torch.int32, device=dev)
    imps = torch.empty_like(terms)
    with torch.cuda.device(dev):
        st = lib().mmrag_sparse_select(pooled.data_ptr(), bias.data_ptr(), _ptr(skip_bits), n_chunks, V, float(scale),
                                       int(m), cnt.data_ptr(), terms.data_ptr(), imps.data_ptr(), _stream_ptr(dev))
    _check(st, "mmrag_sparse_select")
    return cnt, terms, imps


def impact_topk_workspace_bytes(B: int, n: int, k: int) -> int:
    return int(lib().mmrag_impact_topk_workspace_bytes(B, n, k))


def impact_topk(term_off: torch.Tensor, post_row: torch.Tensor, post_imp: torch.Tensor, n_terms: int, n: int,
                q_off: torch.Tensor, q_terms: torch.Tensor, q_imp: torch.Tensor, k: int,
                alive_bits: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                cap: int = 0, dbg: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores [B, k] float32 desc, rows [B, k] int64; (-inf, -1) padding) on the device: the exact top-k by integer
    impact score over the inverted CSR (mmrag_impact_topk).  `cap` / `dbg`: the test hook's candidate capacity and
    switches (mmrag_internal_impact_topk_ex)."""
    _dev_check(term_off, post_row, post_imp, q_off, q_terms, q_imp, alive_bits, workspace)
    B = q_off.numel() - 1
    dev = q_off.device
    need = impact_topk_workspace_bytes(B, n, k)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    out_s, out_r = _topk_out(max(B, 1), max(k, 1), dev)
    args = (term_off.data_ptr(), post_row.data_ptr(), post_imp.data_ptr(), int(n_terms), int(n), q_off.data_ptr(),
            q_terms.data_ptr(), q_imp.data_ptr(), B, int(k), _ptr(alive_bits), out_s.data_ptr(), out_r.data_ptr(),
            workspace.data_ptr(), _nbytes(workspace), _stream_ptr(dev))
    with torch.cuda.device(dev):
        if cap or dbg:
            st = lib().mmrag_internal_impact_topk_ex(*args, int(cap), int(dbg))
        else:
            st = lib().mmrag_impact_topk(*args)
    _check(st, "mmrag_impact_topk")
    return out_s, out_r


MAX_TERM_GROUPS = 4096   # mmrag_group_terms (MMRAG_MAX_TERM_GROUPS)


def terms_limits() -> dict:
    """csrc/terms.hip's path sizes (mmrag_internal_terms_limits; tests put their cases on them): groups per launch,
    term ids per workgroup, the longest postings list one wave takes alone, the workgroup's stride over a longer one"""
    v = [ctypes.c_int(0) for _ in range(4)]
    _check(lib().mmrag_internal_terms_limits(*[ctypes.byref(x) for x in v]), "mmrag_internal_terms_limits")
    return dict(zip(("groups", "block_terms", "wave_limit", "block_stride"), (int(x.value) for x in v)))


def group_terms_workspace_bytes(n_groups: int, n_terms: int, top: int) -> int:
    return int(lib().mmrag_group_terms_workspace_bytes(n_groups, n_terms, top))


def group_terms(term_off: torch.Tensor, post_row: torch.Tensor, df: torch.Tensor, n_terms: int, n: int,
                group: torch.Tensor, group_size: torch.Tensor, n_live: int, top: int, min_count: int = 2,
                term_bits: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """(scores [G, top] float32 desc, terms [G, top] int64, counts [G, top] int32; (-inf, -1, 0) padding) on the device:
    each group's significant terms by the JLH score over the inverted CSR (mmrag_group_terms).  `group` int32 [>= n]
    labels the rows (-1: none), `group_size` int32 [G] counts them, `term_bits` int32 words mask the terms."""
    _dev_check(term_off, post_row, df, group, group_size, term_bits, workspace)
    G = int(group_size.numel())
    if group.dtype != torch.int32 or group_size.dtype != torch.int32 or group.numel() < n:
        raise MMRagNativeError(f"group_terms: group must be int32 [>= {n}] and group_size int32")
    if term_bits is not None and (term_bits.dtype != torch.int32 or term_bits.numel() * 32 < n_terms):
        raise MMRagNativeError(f"group_terms: term_bits must hold {n_terms} bits as int32 words")
    dev = group.device
    need = group_terms_workspace_bytes(G, n_terms, top)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    out_s, out_t = _topk_out(max(G, 1), max(top, 1), dev)
    out_c = torch.empty((max(G, 1), max(top, 1)), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(lib().mmrag_group_terms(term_off.data_ptr(), post_row.data_ptr(), df.data_ptr(), int(n_terms), int(n),
                                       group.data_ptr(), group_size.data_ptr(), G, int(n_live), _ptr(term_bits),
                                       int(min_count), int(top), out_s.data_ptr(), out_t.data_ptr(), out_c.data_ptr(),
                                       workspace.data_ptr(), _nbytes(workspace), _stream_ptr(dev)), "mmrag_group_terms")
    return out_s, out_t, out_c


def cross_encoder_workspace_bytes(desc: EncoderDesc, T: int, B: int, f32: bool = False) -> int:
    fn = lib().mmrag_cross_encoder_f32_workspace_bytes if f32 else lib().mmrag_cross_encoder_workspace_bytes
    return int(fn(ctypes.byref(desc), T, B))


def cross_encoder_forward(desc: EncoderDesc, weight_ptrs, n_labels: int, ids: torch.Tensor, type_ids: torch.Tensor,
                          pos_ids: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int,
                          workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                          f32: bool = False) -> torch.Tensor:
    """One cross-encoder pass over packed (query, passage) sequences -> logits [B, n_labels] float32.  `weight_ptrs`
    in the order include/mmrag.h documents for mmrag_cross_encoder_forward (see reranker.DeviceCrossEncoder)."""
    _dev_check(ids, type_ids, pos_ids, cu_seqlens, workspace, out)
    T, B = ids.numel(), cu_seqlens.numel() - 1
    need = cross_encoder_workspace_bytes(desc, T, B, f32)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=ids.device)
    if out is None:
        out = torch.empty((B, n_labels), dtype=torch.float32, device=ids.device)
    fn = lib().mmrag_cross_encoder_forward_f32 if f32 else lib().mmrag_cross_encoder_forward
    with torch.cuda.device(ids.device):
        st = fn(ctypes.byref(desc), weight_ptrs, n_labels, ids.data_ptr(), type_ids.data_ptr(), pos_ids.data_ptr(),
                cu_seqlens.data_ptr(), T, B, max_len, out.data_ptr(), workspace.data_ptr(),
                _nbytes(workspace), _stream_ptr(ids.device))
    _check(st, "mmrag_cross_encoder_forward")
    return out


# ---- extractive reader (include/mmrag.h: mmrag_span_select, mmrag_reader_forward) ----
def _reader_outs(B: int, T: int, n_best: int, logits: bool, dev):
    n = max(int(n_best), 1)
    return (torch.empty((B, n, 2), dtype=torch.int32, device=dev), torch.empty((B, n), dtype=torch.float32, device=dev),
            torch.empty(B, dtype=torch.float32, device=dev), torch.empty((B, 2), dtype=torch.float32, device=dev),
            torch.empty((T, 2), dtype=torch.float32, device=dev) if logits else None)


def _reader_tables(cu_seqlens, ctx_start, ctx_len):
    B = cu_seqlens.numel() - 1
    for t in (cu_seqlens, ctx_start, ctx_len):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise MMRagNativeError("reader: cu_seqlens / ctx_start / ctx_len must be contiguous int32 vectors")
    if B < 1 or ctx_start.numel() != B or ctx_len.numel() != B:
        raise MMRagNativeError("reader: ctx_start / ctx_len need one entry per sequence")
    return B


def span_select(hidden: torch.Tensor, qa_w: torch.Tensor, qa_b: torch.Tensor, cu_seqlens: torch.Tensor,
                ctx_start: torch.Tensor, ctx_len: torch.Tensor, max_answer_tokens: int, n_best: int,
                logits: bool = False, hidden_dim: Optional[int] = None):
    """(spans [B, n_best, 2] int32, scores [B, n_best], null [B], lse [B, 2], logits [T, 2] or None) on the device:
    the reader's span head on final hidden states `hidden` [T, ld] float16 (mmrag_span_select).  `hidden_dim`: the
    columns that are the hidden state (default: all of them)."""
    _dev_check(hidden, qa_w, qa_b, cu_seqlens, ctx_start, ctx_len)
    if hidden.dim() != 2 or hidden.dtype != torch.float16 or not hidden.is_contiguous():
        raise MMRagNativeError("span_select: hidden must be a contiguous [T, ld] float16 tensor")
    T, ld = hidden.shape
    H = ld if hidden_dim is None else int(hidden_dim)
    if qa_w.dtype != torch.float32 or tuple(qa_w.shape) != (2, H) or not qa_w.is_contiguous() \
            or qa_b.dtype != torch.float32 or qa_b.numel() != 2 or not qa_b.is_contiguous():
        raise MMRagNativeError("span_select: qa_w must be [2, hidden] and qa_b [2], contiguous float32")
    B = _reader_tables(cu_seqlens, ctx_start, ctx_len)
    span, score, null, lse, lg = _reader_outs(B, T, n_best, logits, hidden.device)
    with torch.cuda.device(hidden.device):
        st = lib().mmrag_span_select(hidden.data_ptr(), ld, H, qa_w.data_ptr(), qa_b.data_ptr(), cu_seqlens.data_ptr(),
                                     ctx_start.data_ptr(), ctx_len.data_ptr(), T, B, int(max_answer_tokens),
                                     int(n_best), span.data_ptr(), score.data_ptr(), null.data_ptr(), lse.data_ptr(),
                                     _ptr(lg), _stream_ptr(hidden.device))
    _check(st, "mmrag_span_select")
    return span, score, null, lse, lg


def reader_workspace_bytes(desc: EncoderDesc, T: int, B: int) -> int:
    return int(lib().mmrag_reader_workspace_bytes(ctypes.byref(desc), T, B))


def reader_forward(desc: EncoderDesc, weight_ptrs, ids: torch.Tensor, type_ids: torch.Tensor, pos_ids: torch.Tensor,
                   cu_seqlens: torch.Tensor, ctx_start: torch.Tensor, ctx_len: torch.Tensor, max_len: int,
                   max_answer_tokens: int, n_best: int, logits: bool = False,
                   workspace: Optional[torch.Tensor] = None):
    """One reader pass over packed (question, passage) sequences -> span_select's outputs.  `weight_ptrs` in the order
    include/mmrag.h documents for mmrag_reader_forward (see reader.DeviceReader)."""
    _dev_check(ids, type_ids, pos_ids, cu_seqlens, ctx_start, ctx_len, workspace)
    T = ids.numel()
    B = _reader_tables(cu_seqlens, ctx_start, ctx_len)
    need = reader_workspace_bytes(desc, T, B)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=ids.device)
    span, score, null, lse, lg = _reader_outs(B, T, n_best, logits, ids.device)
    with torch.cuda.device(ids.device):
        st = lib().mmrag_reader_forward(ctypes.byref(desc), weight_ptrs, ids.data_ptr(), type_ids.data_ptr(),
                                        pos_ids.data_ptr(), cu_seqlens.data_ptr(), ctx_start.data_ptr(),
                                        ctx_len.data_ptr(), T, B, int(max_len), int(max_answer_tokens), int(n_best),
                                        span.data_ptr(), score.data_ptr(), null.data_ptr(), lse.data_ptr(), _ptr(lg),
                                        workspace.data_ptr(), _nbytes(workspace), _stream_ptr(ids.device))
    _check(st, "mmrag_reader_forward")
    return span, score, null, lse, lg


def embed_types_ln(ids, type_ids, pos_ids, tok, pos, type_tab, gamma, beta, eps: float) -> torch.Tensor:
    """(tests) the cross-encoder's embedding kernel on its own: LN(tok[ids] + pos[pos_ids] + type_tab[type_ids]); fp16
    tables -> fp16 rows, fp32 tables -> fp32 rows"""
    _dev_check(ids, type_ids, pos_ids, tok, pos, type_tab, gamma, beta)
    T, H = ids.numel(), tok.shape[1]
    f32 = tok.dtype == torch.float32
    out = torch.empty((T, H), dtype=tok.dtype, device=tok.device)
    fn = lib().mmrag_internal_embed_types_ln_f32 if f32 else lib().mmrag_internal_embed_types_ln_f16
    with torch.cuda.device(tok.device):
        st = fn(ids.data_ptr(), type_ids.data_ptr(), pos_ids.data_ptr(), tok.data_ptr(), pos.data_ptr(),
                type_tab.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), T, H, tok.shape[0], pos.shape[0],
                type_tab.shape[0], eps, _stream_ptr(tok.device))
    _check(st, "mmrag_internal_embed_types_ln")
    return out


def cls_head_f32(cls: torch.Tensor, wp, bp, wc, bc) -> torch.Tensor:
    """(tests) the classification head on its own: W_c tanh(W_p cls + b_p) + b_c, all float32"""
    _dev_check(cls, wp, bp, wc, bc)
    B, H = cls.shape
    NL = wc.shape[0]
    ws = torch.empty(int(lib().mmrag_internal_cls_head_workspace_bytes(B, H, NL)) + 256, dtype=torch.uint8,
                     device=cls.device)
    off = (-ws.data_ptr()) % 256
    out = torch.empty((B, NL), dtype=torch.float32, device=cls.device)
    with torch.cuda.device(cls.device):
        st = lib().mmrag_internal_cls_head_f32(cls.data_ptr(), wp.data_ptr(), bp.data_ptr(), wc.data_ptr(), bc.data_ptr(),
                                               out.data_ptr(), B, H, NL, ws.data_ptr() + off, ws.numel() - off,
                                               _stream_ptr(cls.device))
    _check(st, "mmrag_internal_cls_head_f32")
    return out


PIXELS_F16_CHW, PIXELS_U8_HWC = 0, 1


def vit_forward(desc: EncoderDesc, weight_ptrs, pixels: torch.Tensor, pixel_kind: int, cu_seqlens: torch.Tensor,
                workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CLIP-style vision tower: images -> [B, out_dim] float32 L2-normalised."""
    _dev_check(pixels, cu_seqlens, workspace, out)
    B = pixels.shape[0]
    S = (desc.image // desc.patch) ** 2 + 1
    need = encoder_workspace_bytes(desc, B * S, B)
    if workspace is None or _nbytes(workspace) < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=pixels.device)
    if out is None:
        out = torch.empty((B, desc.out_dim), dtype=torch.float32, device=pixels.device)
    with torch.cuda.device(pixels.device):
        st = lib().mmrag_vit_forward(ctypes.byref(desc), weight_ptrs, pixels.data_ptr(), pixel_kind,
                                     cu_seqlens.data_ptr(), B, out.data_ptr(), workspace.data_ptr(),
                                     _nbytes(workspace), _stream_ptr(pixels.device))
    _check(st, "mmrag_vit_forward")
    return out


def patchify(pixels: torch.Tensor, image: int, patch: int) -> torch.Tensor:
    """(tests) the vision tower's patchify kernel on its own: uint8 [B, image, image, 3] (CLIP normalisation fused) or
    fp16 [B, 3, image, image] -> fp16 [B, (image/patch)^2, 3 * patch * patch], patch vector order (c, ph, pw)"""
    _dev_check(pixels)
    kind = PIXELS_U8_HWC if pixels.dtype == torch.uint8 else PIXELS_F16_CHW
    want = (image, image, 3) if kind == PIXELS_U8_HWC else (3, image, image)
    if pixels.dtype not in (torch.uint8, torch.float16) or tuple(pixels.shape[1:]) != want or not pixels.is_contiguous():
        raise MMRagNativeError(f"patchify: bad pixel tensor {tuple(pixels.shape)} {pixels.dtype}")
    if patch <= 0 or image % patch != 0:
        raise MMRagNativeError(f"patchify: bad image/patch {image}/{patch}")
    B, G = pixels.shape[0], image // patch
    out = torch.empty((B, G * G, 3 * patch * patch), dtype=torch.float16, device=pixels.device)
    with torch.cuda.device(pixels.device):
        st = lib().mmrag_internal_patchify(pixels.data_ptr(), kind, out.data_ptr(), B, image, patch,
                                           _stream_ptr(pixels.device))
    _check(st, "mmrag_internal_patchify")
    return out


def vit_assemble_ln(emb: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                    eps: float) -> torch.Tensor:
    """(tests) the vision tower's embedding kernel on its own: emb fp16 [B, S - 1, H], cls fp16 [H], pos fp16 [S, H]
    -> LN(concat(cls, emb[b]) + pos) as fp16 [B * S, H]"""
    _dev_check(emb, cls, pos, gamma, beta)
    B, S, H = emb.shape[0], pos.shape[0], pos.shape[1]
    if tuple(emb.shape) != (B, S - 1, H) or cls.numel() != H or gamma.numel() != H or beta.numel() != H:
        raise MMRagNativeError("vit_assemble_ln: emb [B, S-1, H], cls [H], pos [S, H], gamma / beta [H]")
    if any(t.dtype != torch.float16 or not t.is_contiguous() for t in (emb, cls, pos)):
        raise MMRagNativeError("vit_assemble_ln: emb, cls, pos must be contiguous fp16")
    out = torch.empty((B * S, H), dtype=torch.float16, device=emb.device)
    with torch.cuda.device(emb.device):
        st = lib().mmrag_internal_vit_assemble_ln(emb.data_ptr(), cls.data_ptr(), pos.data_ptr(), gamma.data_ptr(),
                                                  beta.data_ptr(), out.data_ptr(), B, S, H, eps,
                                                  _stream_ptr(emb.device))
    _check(st, "mmrag_internal_vit_assemble_ln")
    return out


def normalize_rows(x: torch.Tensor) -> torch.Tensor:
    """(tests) the pre-LN head's last kernel on its own: fp16 [B, D] -> x / max(||x||, 1e-12) as float32"""
    _dev_check(x)
    if x.dtype != torch.float16 or x.dim() != 2 or not x.is_contiguous():
        raise MMRagNativeError("normalize_rows: x must be contiguous fp16 [B, D]")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib().mmrag_internal_normalize_rows(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                                 _stream_ptr(x.device))
    _check(st, "mmrag_internal_normalize_rows")
    return out


def pool_f16(x: torch.Tensor, cu_seqlens: torch.Tensor, pool: int, sel: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(tests) the pre-LN head's pooling on its own: the fp16-out pooling kernel without normalisation -> fp16 [B, H]"""
    _dev_check(x, cu_seqlens, sel)
    if x.dtype != torch.float16 or x.dim() != 2 or not x.is_contiguous():
        raise MMRagNativeError("pool_f16: x must be contiguous fp16 [T, H]")
    B, H = cu_seqlens.numel() - 1, x.shape[1]
    out = torch.empty((B, H), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        st = lib().mmrag_internal_pool_f16(x.data_ptr(), cu_seqlens.data_ptr(), _ptr(sel), out.data_ptr(), B, H, pool,
                                           _stream_ptr(x.device))
    _check(st, "mmrag_internal_pool_f16")
    return out


def resample_coeffs(in_size: int, out_size: int, first: int, count: int):
    """HOST: Pillow's fixed-point bicubic taps of output indices [first, first+count).  Returns numpy
    (bounds [count,2] int32, taps [count,ksize] int32).  No GPU needed."""
    import numpy as np

    ks = lib().mmrag_resample_ksize(in_size, out_size)
    bounds = np.zeros((count, 2), np.int32)
    taps = np.zeros((count, max(ks, 1)), np.int32)
    _check(lib().mmrag_resample_coeffs(in_size, out_size, first, count, bounds.ctypes.data, taps.ctypes.data),
           "mmrag_resample_coeffs")
    return bounds, taps


def resize_crop_u8(src: torch.Tensor, bx: torch.Tensor, kx: torch.Tensor, by: torch.Tensor, ky: torch.Tensor,
                   y_lo: int, y_hi: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src [H,W,3] uint8 (device) -> [len(by), len(bx), 3] uint8: horizontal taps (bx,kx) per output column,
    then vertical taps (by,ky) per output row; bit-exact with Pillow's 8-bit bicubic resize."""
    _dev_check(src, bx, kx, by, ky, out)
    if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3 or src.stride(2) != 1 or src.stride(1) != 3:
        raise MMRagNativeError("resize_crop_u8: src must be [H, W, 3] uint8 with packed pixels")
    H, W = int(src.shape[0]), int(src.shape[1])
    out_h, out_w = int(by.shape[0]), int(bx.shape[0])
    if out is None:
        out = torch.empty((out_h, out_w, 3), dtype=torch.uint8, device=src.device)
    tmp = torch.empty(((y_hi - y_lo) * out_w * 3,), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        st = lib().mmrag_resize_crop_u8(src.data_ptr(), H, W, src.stride(0), bx.data_ptr(), kx.data_ptr(),
                                        int(kx.shape[1]), by.data_ptr(), ky.data_ptr(), int(ky.shape[1]), out_h, out_w,
                                        y_lo, y_hi, tmp.data_ptr(), out.data_ptr(), _stream_ptr(src.device))
    _check(st, "mmrag_resize_crop_u8")
    return out


def copy_to_host_async(dst_host: torch.Tensor, src_dev: torch.Tensor, stream: int) -> None:
    """Stream-ordered device -> pinned host copy on a raw hipStream_t (no torch stream context)."""
    nbytes = src_dev.numel() * src_dev.element_size()
    if dst_host.is_cuda or not src_dev.is_cuda or dst_host.numel() * dst_host.element_size() < nbytes:
        raise MMRagNativeError("copy_to_host_async: need a host destination at least as large as the device source")
    _check(lib().mmrag_copy_to_host_async(dst_host.data_ptr(), src_dev.data_ptr(), nbytes, stream),
           "mmrag_copy_to_host_async")


class SearchPlan:
    """Pre-validated, pointer-cached form of cosine_topk_lists / cosine_topk_select for hot loops
    (a serving loop or bench.py issues the same shapes thousands of times; argument checking and
    torch context managers would otherwise dominate the host time per batch at small shard sizes).
    The tensors are kept alive by the plan; `stream` arguments are raw hipStream_t values."""

    def __init__(self, q: torch.Tensor, corpus: torch.Tensor, n: int, d: int, k: int, workspace: torch.Tensor,
                 alive_bits: Optional[torch.Tensor] = None):
        _dev_check(q, corpus, workspace, alive_bits)
        if q.dtype != corpus.dtype or q.shape[1] != corpus.shape[1] or not q.is_contiguous() or not corpus.is_contiguous():
            raise MMRagNativeError("SearchPlan: q and corpus must be contiguous and share dtype and padded width")
        if n > corpus.shape[0]:
            raise MMRagNativeError(f"SearchPlan: n={n} exceeds corpus capacity {corpus.shape[0]}")
        need = lib().mmrag_cosine_topk_workspace_bytes(q.shape[0], n, k)
        if _nbytes(workspace) < need:
            raise MMRagNativeError("SearchPlan: workspace too small")
        self._keep = (q, corpus, workspace, alive_bits)
        self.B, self.n, self.k = q.shape[0], n, k
        self._scan_args = (q.data_ptr(), corpus.data_ptr(), q.shape[0], n, d, q.shape[1], _TORCH2DT[q.dtype], k,
                           alive_bits.data_ptr() if alive_bits is not None else None, workspace.data_ptr(),
                           _nbytes(workspace))
        self._ws = workspace.data_ptr()
        self._scan = lib().mmrag_cosine_topk_lists
        self._select = lib().mmrag_cosine_topk_select

    def scan(self, stream: int) -> None:
        st = self._scan(*self._scan_args, stream)
        if st:
            _check(st, "mmrag_cosine_topk_lists")

    def select(self, row_offset: int, out_scores_ptr: int, out_rows_ptr: int, stream: int) -> None:
        st = self._select(self.B, self.n, self.k, row_offset, self._ws, out_scores_ptr, out_rows_ptr, stream)
        if st:
            _check(st, "mmrag_cosine_topk_select")
