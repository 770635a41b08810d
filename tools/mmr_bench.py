"""Measure MMR diversified retrieval (csrc/mmr.hip): the select kernel alone in both forms, `VectorIndex.mmr_search`
as a whole, and beside them the dense searches the caller pays anyway (`search(fetch_k)`) and a plain query costs
(`search(n_results)`; this change touches no search kernel, so that figure is the parent commit's too).

    python tools/mmr_bench.py [--quick]

Random unit rows: 1M x 768 fp16 and 100k x 384 fp32; B in {1, 32, 256}; (n_results, fetch_k) in {(5, 50), (10, 64),
(20, 200), (20, 1024)}.  Device times come from HIP events, median of 20 calls, after the same call has been held for
0.5 s so the chip sits at the clock it sustains.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/mmr_bench.py --quick` run (one shape: 1M x 768, B = 256, 5 / 50).
Prints one JSON object per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402
from multimodal_rag_amd.index import VectorIndex  # noqa: E402


def timed(fn, reps=20, hold=0.5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < hold:
        for _ in range(8):
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
    return round(float(np.median(ts)), 1)


def random_index(n, d, dtype, dev):
    idx = VectorIndex(d, dtype=dtype, device=dev, capacity=n)
    step = 100_000
    for lo in range(0, n, step):
        m = min(step, n - lo)
        rows = torch.randn((m, idx.ld), device=dev, dtype=torch.float32)
        rows[:, d:] = 0
        rows = (rows / rows.norm(dim=1, keepdim=True)).to(dtype)
        idx.add_rows_device(rows, None, None, [f"id{i}" for i in range(lo, lo + m)])
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one shape, no hold (for the rocprofv3 run)")
    args = ap.parse_args()
    dev = "cuda:0"
    corpora = [(1_000_000, 768, torch.float16)] if args.quick else [(1_000_000, 768, torch.float16),
                                                                    (100_000, 384, torch.float32)]
    batches = [256] if args.quick else [1, 32, 256]
    shapes = [(5, 50)] if args.quick else [(5, 50), (10, 64), (20, 200), (20, 1024)]
    hold = 0.0 if args.quick else 0.5
    for n, d, dtype in corpora:
        idx = random_index(n, d, dtype, dev)
        for B in batches:
            q = torch.randn((B, d), device=dev)
            q = q / q.norm(dim=1, keepdim=True)
            for k, fetch_k in shapes:
                s, r = idx.search(q, fetch_k)
                s, r = s.contiguous(), r.contiguous()
                rec = {"what": "mmr", "rows": n, "dim": d, "dtype": str(dtype).split(".")[-1], "B": B,
                       "n_results": k, "fetch_k": fetch_k,
                       "staged_fits": fetch_k * ((d * idx.matrix.element_size() + 15) // 16) * 16 <= 128 * 1024}
                rec["select_us"] = timed(lambda: _native.mmr_select(idx.matrix, d, s, r, k, 0.5), hold=hold)
                rec["select_streamed_us"] = timed(
                    lambda: _native.mmr_select(idx.matrix, d, s, r, k, 0.5, dbg=_native.MMR_DBG_STREAM), hold=hold)
                rec["mmr_search_us"] = timed(lambda: idx.mmr_search(q, k, fetch_k=fetch_k, lambda_mult=0.5), hold=hold)
                rec["search_fetch_k_us"] = timed(lambda: idx.search(q, fetch_k), hold=hold)
                rec["search_n_results_us"] = timed(lambda: idx.search(q, k), hold=hold)
                print(json.dumps(rec), flush=True)
        del idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
