#!/usr/bin/env python3
"""Late-interaction re-ranking beside the cross-encoder, one process, MiniLM shape, random weights: n candidates of 256
tokens and a 32-word question, `EmbeddingManager.late_rerank` (one bi-encoder forward over the question and the
candidates + one MaxSim launch) against `DeviceCrossEncoder.predict` on the same texts (one forward over n pairs), wall
clock, interleaved.  Both tokenise with the native WordPiece tokenizer over a synthetic vocabulary.

    python tools/late_bench.py [--candidates 20,100] [--reps 30]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/late_bench.py --profile     (a run of its own)

--profile only runs 20 late_rerank calls per candidate count (for the kernel statistics: maxsim_kernel and
token_norm_kernel beside the forward's kernels).  Ranking quality is not measured: there are no trained weights here.
"""
import argparse
import asyncio
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_rag_amd.embedder import EmbeddingManager  # noqa: E402
from multimodal_rag_amd.encoder import PRESETS, DeviceEncoder  # noqa: E402
from multimodal_rag_amd.reranker import MS_MARCO_MINILM_L6, DeviceCrossEncoder  # noqa: E402
from multimodal_rag_amd.tokenizer import NativeWordPieceTokenizer  # noqa: E402

WORDS = 5000


def text(g, n_words):
    return " ".join(f"w{i}" for i in g.integers(0, WORDS, n_words))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="20,100")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    vocab = {t: i for i, t in enumerate(["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + [f"w{i}" for i in range(WORDS)])}
    tok = NativeWordPieceTokenizer(vocab)
    enc = DeviceEncoder.random_init(PRESETS["all-MiniLM-L6-v2"], seed=0)
    engine = types.SimpleNamespace(encoder=enc, tokenizer=tok, device="cuda:0", device_name="cuda", dim=enc.dim,
                                   max_seq_length=enc.cfg.max_seq_length)
    m = EmbeddingManager(engine=engine, enable_cache=False)
    m.is_initialized = True          # no collection is needed: late_rerank reads the hits' documents only
    cross = DeviceCrossEncoder.random_init(MS_MARCO_MINILM_L6, n_labels=1, seed=0, precision="fp16", tokenizer=tok)
    loop = asyncio.new_event_loop()
    g = np.random.default_rng(0)
    question = text(g, 32)
    report = {"shape": "all-MiniLM-L6-v2 / ms-marco-MiniLM-L-6 (6 x 384, 12 heads, I 1536), random weights",
              "question_tokens": 32, "candidate_tokens": 256}
    for n in [int(x) for x in a.candidates.split(",")]:
        docs = [text(g, 254) for _ in range(n)]      # + [CLS] and [SEP]: 256 tokens each
        hits = {"ids": [f"id{i}" for i in range(n)], "distances": [0.0] * n, "metadatas": [{}] * n, "documents": docs}
        late = lambda: loop.run_until_complete(m.late_rerank(question, hits, top_k=5))  # noqa: E731
        ce = lambda: cross.predict([(question, d) for d in docs], batch_size=n)  # noqa: E731
        if a.profile:
            for _ in range(20):
                late()
            torch.cuda.synchronize()
            continue
        for _ in range(3):
            late(), ce()
        torch.cuda.synchronize()
        times = {"late": [], "cross": []}
        for _ in range(a.reps):
            for name, fn in (("late", late), ("cross", ce)):
                t0 = time.perf_counter()
                fn()                 # both end in a copy of the scores to the host
                times[name].append((time.perf_counter() - t0) * 1e3)
        lt, ct = float(np.median(times["late"])), float(np.median(times["cross"]))
        report[f"n={n}"] = {"late_rerank_ms": round(lt, 3), "cross_predict_ms": round(ct, 3),
                            "late_over_cross": round(lt / ct, 3)}
    print(json.dumps(report))


if __name__ == "__main__":
    main()
