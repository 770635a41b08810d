#!/usr/bin/env python3
"""The token store, one process, MiniLM shape, random weights.

(a) `EmbeddingManager.late_rerank` of n candidates of 256 tokens against a 32-word question, with the candidates'
    token rows in the store (one forward over the question + one MaxSim launch) and without it (one forward over the
    question and the candidates + one MaxSim launch, the path before the store), wall clock, interleaved.
(b) `VectorIndex.late_search` over stored chunks of about 200 tokens at 384-d: wall clock and device time (events
    around the call: plan, pack, bound passes, scan and select together) for Q = 1 and 16 questions of 32 tokens, the
    plane's bytes over the device time against the measured read peak, the survivors per question the main pass left
    in the counters, and `kmeans_assign` (the same tile body, arg-max epilogue) of the same plane against 128 centroids.
    The plane is filled with random unit rows on the device: the scan's cost does not depend on the values.

    python tools/late_store_bench.py [--candidates 20,100] [--chunks 10000,100000] [--reps 30] [--dtype float16]

--dtype float8_e4m3fn keeps both stores as E4M3 code rows: the rerank and the scan then run the FP8
kernels, the questions are quantised per call (counted in the times), and kmeans_assign, which reads fp16 rows only,
is left out.  `--candidates ""` skips (a).
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/late_store_bench.py --profile      (a run of its own)

--profile runs 10 late_rerank calls per candidate count and 10 late_search calls per case, for the kernel statistics
(maxsim_scan_kernel, maxsim_kernel, deep_select_kernel beside the forward's kernels).  Ranking quality is not measured:
there are no trained weights here.
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
from multimodal_rag_amd import _native  # noqa: E402
from multimodal_rag_amd.embedder import EmbeddingManager  # noqa: E402
from multimodal_rag_amd.encoder import PRESETS, DeviceEncoder  # noqa: E402
from multimodal_rag_amd.index import VectorIndex  # noqa: E402
from multimodal_rag_amd.tokenizer import NativeWordPieceTokenizer  # noqa: E402

WORDS = 5000


def text(g, n_words):
    return " ".join(f"w{i}" for i in g.integers(0, WORDS, n_words))


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def device_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def unit_plane(rows, dim, seed):
    """[rows, dim] fp16 random unit rows, made on the device in slices"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((rows, dim), dtype=torch.float16, device="cuda")
    for lo in range(0, rows, 1 << 20):
        x = torch.randn((min(1 << 20, rows - lo), dim), generator=g, device="cuda")
        out[lo: lo + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).half()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="20,100")
    ap.add_argument("--chunks", default="10000,100000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dtype", default="float16", choices=("float16", "float8_e4m3fn"))
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    reps = 10 if a.profile else a.reps
    vocab = {t: i for i, t in enumerate(["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + [f"w{i}" for i in range(WORDS)])}
    tok = NativeWordPieceTokenizer(vocab)
    enc = DeviceEncoder.random_init(PRESETS["all-MiniLM-L6-v2"], seed=0)
    engine = types.SimpleNamespace(encoder=enc, tokenizer=tok, device="cuda:0", device_name="cuda", dim=enc.dim,
                                   max_seq_length=enc.cfg.max_seq_length)
    m = EmbeddingManager(engine=engine, enable_cache=False)
    m.is_initialized = True
    loop = asyncio.new_event_loop()
    g = np.random.default_rng(0)
    question = text(g, 32)
    report = {"shape": "all-MiniLM-L6-v2 (6 x 384, 12 heads, I 1536), random weights", "question_tokens": 32,
              "reps": reps, "store_dtype": a.dtype, "rerank": {}, "scan": {}}

    # ---- (a) late_rerank with and without the store
    for n in [int(x) for x in a.candidates.split(",") if x]:
        docs = [text(g, 254) for _ in range(n)]      # + [CLS] and [SEP]: 256 tokens each
        ids = [f"id{i}" for i in range(n)]
        m.collection = VectorIndex(dim=enc.dim, dtype=torch.float16)
        m.collection.add(unit_plane(n, enc.dim, n).float().cpu().numpy(), documents=docs, ids=ids)
        m.collection.enable_token_store(enc.dim, m._get_late().max_doc_tokens, dtype=a.dtype)
        m._store_tokens(ids, docs)
        hits = {"ids": ids, "distances": [0.0] * n, "metadatas": [{}] * n, "documents": docs}
        unknown = {**hits, "ids": ["x" + i for i in ids]}            # ids the store does not know: the path before it
        with_store = lambda: loop.run_until_complete(m.late_rerank(question, hits, top_k=5))  # noqa: E731
        without = lambda: loop.run_until_complete(m.late_rerank(question, unknown, top_k=5))  # noqa: E731
        assert with_store()["rerank_scores"] == without()["rerank_scores"]
        report["rerank"][n] = {"store_ms": median_ms(with_store, reps), "no_store_ms": median_ms(without, reps),
                               "store_bytes": m.collection.token_stats()["bytes"]}

    # ---- (b) late_search over a plane of random unit rows
    peaks = None if a.profile else _native.measure_peaks(torch.device("cuda:0"))
    if peaks is not None:
        report["peaks"] = peaks
    dim = enc.dim
    for n in [int(x) for x in a.chunks.split(",") if x]:
        lens = g.integers(150, 251, n)                       # about 200 tokens a chunk
        idx = VectorIndex(dim=dim, dtype=torch.float16, capacity=n)
        step = 1 << 16
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            idx.add(unit_plane(hi - lo, dim, lo + 1).float().cpu().numpy(), ids=[f"c{i}" for i in range(lo, hi)])
        st = idx.enable_token_store(dim, 512, dtype=a.dtype)
        for lo in range(0, n, 4096):
            hi = min(n, lo + 4096)
            st.set_tokens(range(lo, hi), unit_plane(int(lens[lo:hi].sum()), dim, 7 + lo), lens[lo:hi])
        T = st.n_rows
        plane_bytes = T * st.bytes_per_row
        case = {"tokens": T, "plane_bytes": plane_bytes, "bytes_per_token": st.bytes_per_row}
        if not st.f8:
            cent = unit_plane(128, dim, 3)
            km = device_ms(lambda: _native.kmeans_assign(st.plane, T, dim, cent), reps)
            case["kmeans_assign_128_ms"] = km
            case["kmeans_assign_tflops"] = 2.0 * T * 128 * dim / km / 1e9
        for Q in (1, 16):
            q_tok = unit_plane(32 * Q, dim, 11 + Q)
            qs, ql = np.arange(Q, dtype=np.int32) * 32, np.full(Q, 32, np.int32)
            run = lambda: idx.late_search(q_tok, qs, ql, 10)  # noqa: E731
            wall, dev = median_ms(run, reps), device_ms(run, reps)
            run()
            torch.cuda.synchronize()
            survivors = idx._late_ws[: 4 * Q].view(torch.int32).cpu().numpy()
            tiles = (32 * Q + 127) // 128
            case[f"Q{Q}"] = {"wall_ms": wall, "device_ms": dev, "plane_gb_per_s": plane_bytes / dev / 1e6,
                             "tflops_of_128_row_tiles": 2.0 * T * 128 * tiles * dim / dev / 1e9,
                             "survivors_per_question": [int(survivors.min()), int(np.median(survivors)),
                                                        int(survivors.max())]}
        report["scan"][n] = case
        del idx, st
        torch.cuda.empty_cache()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
