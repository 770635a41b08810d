#!/usr/bin/env python3
"""One-process A/B of the cross-encoder against the plain encoder forward at the cross-encoder/ms-marco-MiniLM-L-6-v2
shape (random weights): B (query, passage) pairs of about 256 tokens, mmrag_cross_encoder_forward vs
mmrag_encoder_forward on the same packed tokens and cu_seqlens, interleaved, device time by HIP events.

    python tools/rerank_once.py [--batches 20,100] [--reps 50] [--precision fp16]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/rerank_once.py --profile     (a run of its own)

--profile only runs 20 cross-encoder forwards per batch size (for the kernel statistics: the share of
cls_head_f32_kernel and embed_types_ln_kernel in the forward).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_rag_amd import _native  # noqa: E402
from multimodal_rag_amd.reranker import MS_MARCO_MINILM_L6, DeviceCrossEncoder  # noqa: E402


def packed(B, g, q_len=32, p_len=221):
    ids = np.concatenate([[101] + g.integers(1000, 30522, q_len).tolist() + [102]
                          + g.integers(1000, 30522, p_len).tolist() + [102] for _ in range(B)]).astype(np.int32)
    L = q_len + p_len + 3
    types = np.tile(np.r_[np.zeros(q_len + 2), np.ones(p_len + 1)].astype(np.int32), B)
    pos = np.tile(np.arange(L, dtype=np.int32), B)
    cu = (np.arange(B + 1) * L).astype(np.int32)
    d = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    return d(ids), d(types), d(pos), d(cu), L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="20,100")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    enc = DeviceCrossEncoder.random_init(MS_MARCO_MINILM_L6, n_labels=1, seed=0, precision=a.precision)
    f32 = a.precision == "fp32"
    g = np.random.default_rng(0)
    report = {"shape": "ms-marco-MiniLM-L-6 (6 x 384, 12 heads, I 1536)", "precision": a.precision}
    for B in [int(x) for x in a.batches.split(",")]:
        ids, types, pos, cu, L = packed(B, g)
        T = ids.numel()
        ws = torch.empty(max(_native.cross_encoder_workspace_bytes(enc.desc, T, B, f32),
                             _native.encoder_workspace_bytes(enc.desc, T, B, f32)), dtype=torch.uint8, device="cuda")
        logits = torch.empty((B, 1), dtype=torch.float32, device="cuda")
        emb = torch.empty((B, enc.cfg.hidden), dtype=torch.float32, device="cuda")
        cross = lambda: _native.cross_encoder_forward(enc.desc, enc._ptrs, 1, ids, types, pos, cu, L, ws, logits, f32)  # noqa: E731
        # the plain forward reads w[2] as the type-0 row: the full table starts with it
        plain = lambda: _native.encoder_forward(enc.desc, enc._ptrs, ids, pos, cu, L, workspace=ws, out=emb, f32=f32)  # noqa: E731
        if a.profile:
            for _ in range(20):
                cross()
            torch.cuda.synchronize()
            continue
        for _ in range(5):
            cross(), plain()
        torch.cuda.synchronize()
        times = {"cross": [], "plain": []}
        for _ in range(a.reps):
            for name, fn in (("cross", cross), ("plain", plain)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        c, p = float(np.median(times["cross"])), float(np.median(times["plain"]))
        report[f"B={B}"] = {"tokens": T, "cross_us": round(c, 1), "plain_us": round(p, 1),
                            "cross_over_plain": round(c / p, 4)}
    print(json.dumps(report))


if __name__ == "__main__":
    main()
