"""Measure multi-query fusion (csrc/fuse.hip): the fuse launch alone, the same lists fused on the host (`.cpu()` plus a
Python dict: lexical.rrf_fuse generalised to V lists), a whole `VectorIndex.fused_query`, the search it contains, and
V sequential `query` calls -- what a caller does without the feature (this change touches neither `query` nor a search
kernel, so that figure is the parent commit's too).

    python tools/fuse_bench.py [--rows 1000000]

Random unit rows, 1M x 768 fp16; G = 1 and G = 64 questions x V = 4 phrasings (a question's phrasings are noisy copies
of one vector, so their lists overlap) x C = 50, n = 5.  Device times come from HIP events around the call, wall times
from a host clock around a call that ends with its results on the host; each is the median of 20 calls after the same
call has been held for 0.5 s so the chip sits at the clock it sustains.  One process; prints
one JSON object per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402
from tools.mmr_bench import random_index, timed  # noqa: E402

V, C, N_RESULTS, RRF_K = 4, 50, 5, 60


def wall(fn, reps=20, hold=0.5):
    """median host time (us) of fn(), which ends with its results on the host"""
    fn()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < hold:
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e6)
    return round(float(np.median(ts)), 1)


def host_fuse(scores, rows, G, n):
    """the lists on the host, fused by reciprocal rank in a dict per question (float64, as lexical.rrf_fuse)"""
    s, r = scores.cpu().tolist(), rows.cpu().tolist()
    out = []
    for g in range(G):
        acc = {}
        for l in range(g * V, (g + 1) * V):
            for rank, row in enumerate(r[l], 1):
                if row < 0:
                    break
                acc[row] = acc.get(row, 0.0) + 1.0 / (RRF_K + rank)
        out.append(sorted(acc.items(), key=lambda kv: (-kv[1], kv[0]))[:n])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    args = ap.parse_args()
    dev = "cuda:0"
    n, d = args.rows, 768
    idx = random_index(n, d, torch.float16, dev)
    for G in (1, 64):
        base = torch.randn((G, 1, d), device=dev)
        q = (base + 0.6 * torch.randn((G, V, d), device=dev)).reshape(G * V, d)
        q = (q / q.norm(dim=1, keepdim=True)).contiguous()
        off = list(range(0, G * V + 1, V))
        off_dev = torch.tensor(off, dtype=torch.int32, device=dev)
        s, r = idx.search(q, C)
        s, r = s.contiguous(), r.contiguous()
        info = _native.fuse_select(s, r, off_dev, N_RESULTS, rrf_k=RRF_K)[5].cpu()
        singles = [q[i:i + 1].contiguous() for i in range(G * V)]
        rec = {"what": "fuse", "rows": n, "dim": d, "G": G, "V": V, "C": C, "n": N_RESULTS,
               "distinct_min": int(info[:, 0].min()), "distinct_max": int(info[:, 0].max()),
               "fuse_launch_us": timed(lambda: _native.fuse_select(s, r, off_dev, N_RESULTS, rrf_k=RRF_K)),
               "host_fuse_wall_us": wall(lambda: host_fuse(s, r, G, N_RESULTS)),
               "fuse_to_host_wall_us": wall(lambda: [t.cpu() for t in _native.fuse_select(s, r, off_dev, N_RESULTS,
                                                                                        rrf_k=RRF_K)]),
               "search_C_us": timed(lambda: idx.search(q, C)),
               "fused_search_us": timed(lambda: idx.fused_search(q, off, N_RESULTS)),
               "fused_query_us": timed(lambda: idx.fused_query(q, off, n_results=N_RESULTS)),
               "fused_query_wall_us": wall(lambda: idx.fused_query(q, off, n_results=N_RESULTS)),
               "sequential_query_wall_us": wall(lambda: [idx.query(one, n_results=N_RESULTS) for one in singles]),
               "sequential_query_C_wall_us": wall(lambda: [idx.query(one, n_results=C) for one in singles])}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
