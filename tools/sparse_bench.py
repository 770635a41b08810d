"""Measure the learned sparse leg (csrc/sparse_expand.hip, csrc/sparse_score.hip).

    python tools/sparse_bench.py [--quick] [--skip-scoring] [--rows 100000,1000000]

Expansion: `mmrag_sparse_pool` (vocabulary projection + per-chunk max, nothing of size T x V written) beside the
project's own `mmrag_linear_f16` producing the [T, V] logits for the same operands (the unfused alternative, without
its max pass), for 256 chunks x 256 tokens and for 256 eight-token queries; H = 768, V = 30 522 (padded to 30 524
columns for the GEMM, which wants a multiple of 4).  The fraction of the measured 16x16x32 MFMA rate is taken against
`mmrag_bench_mfma_f16_16x16x32` in the same process.
Scoring: `mmrag_impact_topk` beside `mmrag_bm25_topk` on the same postings (128 terms per row, 32-term queries), and
the share of queries that took the overflow re-run (survivor counts above the candidate slots).

Device times come from HIP events around steady-state repetitions (median of 11 after 3 warm-up calls), one process.
Prints one JSON object per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402
from multimodal_rag_amd.lexical import LexicalIndex  # noqa: E402
from multimodal_rag_amd.sparse import ImpactIndex  # noqa: E402


def timed(fn, reps=11, warm=3):
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


def expansion(dev, n_chunks, chunk_tokens, H, V, mfma_tflops):
    T = n_chunks * chunk_tokens
    g = torch.Generator(device=dev).manual_seed(0)
    tok = torch.randn((T, H), generator=g, device=dev).half()
    Vp = (V + 3) // 4 * 4
    E = torch.zeros((Vp, H), dtype=torch.float16, device=dev)
    E[:V] = (torch.randn((V, H), generator=g, device=dev) * 0.05).half()
    cu = torch.arange(0, T + 1, chunk_tokens, dtype=torch.int32, device=dev)
    flops = 2.0 * T * V * H
    fused = timed(lambda: _native.sparse_pool(tok, cu, E, H, V=V))
    rec = {"what": "expansion", "chunks": n_chunks, "chunk_tokens": chunk_tokens, "T": T, "H": H, "V": V,
           "sparse_pool_us": round(fused, 1), "sparse_pool_tflops": round(flops / fused / 1e6, 1),
           "sparse_pool_bytes_written": n_chunks * V * 4, "logits_bytes_written": T * Vp * 2}
    if mfma_tflops:
        rec["sparse_pool_fraction_of_measured_mfma"] = round(flops / fused / 1e6 / mfma_tflops, 3)
    if T * Vp * 2 <= 8 << 30:
        out = torch.empty((T, Vp), dtype=torch.float16, device=dev)
        gemm = timed(lambda: _native.linear_f16(tok, E, out=out))
        rec["linear_f16_logits_us"] = round(gemm, 1)
        rec["fused_over_gemm"] = round(fused / gemm, 3)
        del out
    print(json.dumps(rec), flush=True)
    # the run of vocabulary tiles per workgroup (the product's choice: about four workgroups per CU, at most 16)
    runs = {v: round(timed(lambda: _native.sparse_pool(tok, cu, E, H, V=V, vrun=v)), 1) for v in (1, 2, 4, 8, 16, 32)}
    print(json.dumps({"what": "expansion_vrun_sweep", "T": T, "us_by_vrun": runs}), flush=True)


def scoring(dev, n, V=30522, doc_terms=128, q_terms=32, B=32):
    g = np.random.default_rng(2)
    # terms by a Zipf law over the vocabulary (expansion terms are common), distinct within a row
    key = np.repeat(np.arange(n, dtype=np.int64), doc_terms + 16) * V + (g.zipf(1.1, n * (doc_terms + 16)) - 1) % V
    uk = np.unique(key)
    rows, terms = uk // V, (uk % V).astype(np.int32)
    rank = np.arange(uk.size) - np.searchsorted(rows, rows)
    keep = rank < doc_terms
    rows, terms = rows[keep], terms[keep]
    imps = g.integers(1, 256, terms.size).astype(np.int32)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=off[1:])
    imp = ImpactIndex(dev, V)
    imp.append(off, terms, imps)
    lex = LexicalIndex(dev)
    lex.append_postings(off, terms, imps, np.diff(off).astype(np.int32))
    lex._max_term = V - 1
    qs = [np.unique((g.zipf(1.1, q_terms * 2) - 1) % V)[:q_terms] for _ in range(B)]
    q_off = np.zeros(B + 1, np.int64)
    np.cumsum([q.size for q in qs], out=q_off[1:])
    qt = np.concatenate(qs).astype(np.int32)
    qi = g.integers(1, 256, qt.size).astype(np.int32)
    for k in (5, 50):
        us_imp = timed(lambda: imp.topk(q_off, qt, qi, k))
        us_bm = timed(lambda: lex.topk_ids(q_off.astype(np.int32), qt, k))
        cnt = imp._search_ws[: 4 * B].view(torch.int32).cpu().numpy()      # the main pass's survivor counts
        cap = _native.candidate_capacity(k)
        print(json.dumps({"what": "scoring", "rows": n, "postings": int(terms.size), "B": B, "k": k,
                          "impact_topk_us": round(us_imp, 1), "bm25_topk_us": round(us_bm, 1),
                          "survivors_median": int(np.median(cnt)), "survivors_max": int(cnt.max()),
                          "rerun_share": round(float((cnt > cap).mean()), 3)}), flush=True)
    del imp, lex
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--quick", action="store_true", help="smaller shapes")
    ap.add_argument("--skip-scoring", action="store_true", help="the expansion measurements alone")
    args = ap.parse_args()
    dev = "cuda:0"
    mfma = None
    try:
        mfma = _native.measure_peaks(torch.device(dev), 0.2).get("mfma_f16_16x16x32_TFLOPs")
    except Exception as e:      # the peak is a denominator only
        print(json.dumps({"what": "mfma_peak", "error": str(e)}), flush=True)
    print(json.dumps({"what": "mfma_peak", "mfma_f16_16x16x32_TFLOPs": mfma}), flush=True)
    H, V = 768, 30522
    if args.quick:
        expansion(dev, 64, 256, H, V, mfma)
    else:
        expansion(dev, 256, 256, H, V, mfma)
    expansion(dev, 256, 8, H, V, mfma)
    for n in ([] if args.skip_scoring else [100_000] if args.quick else [int(x) for x in args.rows.split(",")]):
        scoring(dev, n)


if __name__ == "__main__":
    main()
