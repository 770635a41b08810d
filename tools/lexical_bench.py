"""Measure the BM25 lexical leg (csrc/lexical.hip) on a synthetic Zipf corpus built directly as term-id arrays
(vocabulary 200k, s = 1.1, ~150 tokens per row), plus the analyzer's throughput and hybrid vs dense-only latency.

    python tools/lexical_bench.py [--rows 100000,1000000] [--quick]

Device times come from HIP events around steady-state repetitions (median of 20 after 5 warm-up calls); kernel times
come from a separate `rocprofv3 --kernel-trace --stats -- python tools/lexical_bench.py --quick` run.  Prints one JSON
object per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd.lexical import Lexicon, LexicalIndex, LEX_DOCUMENTS  # noqa: E402

V = 200_000


def zipf_corpus(n, seed=0, tokens=150):
    g = np.random.default_rng(seed)
    lens = g.integers(tokens // 2, tokens * 3 // 2, n)
    tok = (g.zipf(1.1, int(lens.sum())) - 1) % V
    key = np.repeat(np.arange(n, dtype=np.int64), lens) * V + tok
    uk, cnt = np.unique(key, return_counts=True)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(uk // V, minlength=n), out=off[1:])
    return off, (uk % V).astype(np.int32), cnt.astype(np.int32), lens.astype(np.int32)


def timed(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def cpu_bm25(off, ids, tfs, dl, order_t, p_rows, p_tf, q, k, k1=1.2, b=0.75):
    n = dl.size
    avgdl = dl.sum() / n
    acc = np.zeros(n)
    for t in q:
        lo, hi = np.searchsorted(order_t, [t, t + 1])
        r, tf = p_rows[lo:hi], p_tf[lo:hi].astype(np.float64)
        idf = np.log1p((n - (hi - lo) + 0.5) / (hi - lo + 0.5))
        acc[r] += idf * tf * (k1 + 1) / (tf + k1 * (1 - b + b * dl[r] / avgdl))
    cand = np.nonzero(acc > 0)[0]
    return cand[np.lexsort((cand, -acc[cand]))[:k]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--quick", action="store_true", help="one size, few shapes (for the rocprofv3 run)")
    args = ap.parse_args()
    dev = "cuda:0"
    sizes = [100_000] if args.quick else [int(x) for x in args.rows.split(",")]
    g = np.random.default_rng(1)
    for n in sizes:
        off, ids, tfs, dl = zipf_corpus(n)
        lex = LexicalIndex(dev)
        lex.append_postings(off, ids, tfs, dl)
        lex._max_term = V - 1
        P = int(ids.size)

        def rebuild():
            lex._csr_n = -1
            lex._ensure_csr()

        print(json.dumps({"what": "csr_rebuild", "rows": n, "postings": P, "us": round(timed(rebuild, 5, 2), 1)}),
              flush=True)
        term_off = lex._ensure_csr()[0].cpu().numpy()
        df = np.diff(term_off)
        order = np.argsort(ids, kind="stable")
        p_rows = np.repeat(np.arange(n), np.diff(off))[order]
        p_t, p_tf = ids[order], tfs[order]
        for B in ([1, 256] if args.quick else [1, 32, 256]):
            qs = [list(dict.fromkeys(((g.zipf(1.1, 5) - 1) % V).tolist())) for _ in range(B)]
            q_off = np.zeros(B + 1, np.int32)
            np.cumsum([len(q) for q in qs], out=q_off[1:])
            q_terms = np.asarray([t for q in qs for t in q], np.int32)
            bytes_q = float(np.mean([8 * df[q].sum() for q in qs]))
            for k in (5, 50):
                us = timed(lambda: lex.topk_ids(q_off, q_terms, k))
                rec = {"what": "bm25_topk", "rows": n, "B": B, "k": k, "us": round(us, 1),
                       "us_per_query": round(us / B, 2), "postings_bytes_per_query": int(bytes_q),
                       "GBps_postings": round(bytes_q * B / us / 1e3, 1)}
                if B == 1:
                    t0 = time.perf_counter()
                    for q in qs:
                        cpu_bm25(off, ids, tfs, dl, p_t, p_rows, p_tf, q, k)
                    rec["cpu_float64_us"] = round((time.perf_counter() - t0) * 1e6 / B, 1)
                print(json.dumps(rec), flush=True)
        del lex
        torch.cuda.empty_cache()
    # analyzer throughput on synthetic Vietnamese-like text (host only)
    syll = ["học", "máy", "dữ", "liệu", "ngôn", "ngữ", "khái", "niệm", "cơ", "bản", "về", "trí", "tuệ", "nhân", "tạo",
            "GPU", "kernel", "C++", "printf()", "Python"]
    docs = [" ".join(g.choice(syll, 150)) + "." for _ in range(20_000)]
    lx = Lexicon()
    t0 = time.perf_counter()
    lx.analyze_batch(docs, LEX_DOCUMENTS)
    dt = time.perf_counter() - t0
    print(json.dumps({"what": "analyzer", "docs": len(docs), "tokens_per_doc": 150, "threads": lx.n_threads,
                      "docs_per_s": int(len(docs) / dt)}), flush=True)
    if args.quick:
        return
    # hybrid vs dense-only at B = 1 on 1M x 768 fp16
    from multimodal_rag_amd.index import VectorIndex

    n, d = 1_000_000, 768
    idx = VectorIndex(d, dtype=torch.float16, device=dev, capacity=n)
    rows = torch.randn((n, idx.ld), device=dev, dtype=torch.float32)
    rows[:, d:] = 0
    rows = (rows / rows.norm(dim=1, keepdim=True)).half()
    words = [f"w{i}" for i in range(50_000)]
    docs = [" ".join(words[j] for j in ((g.zipf(1.1, 12) - 1) % len(words))) for _ in range(n)]
    idx.add_rows_device(rows, docs, None, [f"id{i}" for i in range(n)])
    idx.enable_lexical()
    q = np.asarray(torch.randn(1, d).numpy(), np.float32)
    q /= np.linalg.norm(q)
    text = "w1 w7 w100 w2500 w40000"
    idx.lexical_query([text], n_results=5)
    dense = timed(lambda: idx.search(q, 50), 20, 5)
    lexical = timed(lambda: idx._lexical_search([text], 50, None), 20, 5)
    t0 = time.perf_counter()
    for _ in range(20):
        idx.hybrid_query(q, [text], n_results=5)
    hybrid_wall = (time.perf_counter() - t0) / 20 * 1e6
    t0 = time.perf_counter()
    for _ in range(20):
        idx.query(q, n_results=5)
    dense_wall = (time.perf_counter() - t0) / 20 * 1e6
    print(json.dumps({"what": "hybrid_vs_dense", "rows": n, "dim": d, "dense_leg_us": round(dense, 1),
                      "lexical_leg_us": round(lexical, 1), "hybrid_query_wall_us": round(hybrid_wall, 1),
                      "dense_query_wall_us": round(dense_wall, 1)}), flush=True)


if __name__ == "__main__":
    main()
