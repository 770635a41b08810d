"""Measure the related-groups scan (csrc/related.hip, _native.related_groups) against the k-means assign step
(csrc/kmeans.hip, _native.kmeans_assign) with k = M centroids on the same rows: the same 128 x 128 pair-tile GEMM with
an arg-max epilogue, so the ratio isolates the segmented-max epilogue and its atomics.

    python tools/related_bench.py [--shapes 1000000x768xfloat16,100000x384xfloat32] [--ms 1,128,1024] [--doc-rows 50]

Workload: unit Gaussian rows, one set of M unit Gaussian vectors, k = 10 winners.  Documents: `--doc-rows` contiguous
rows each (rows in ingest order, the expected case), and the same ordinals shuffled over the rows (every run of a lane
has length 1: the worst case for the atomics).  Each call is timed with device events around it in steady state: after
a warm-up of all three, ROUNDS rounds of ITERS calls each, the three alternating round by round; the median round's
time per call is reported with the fastest and slowest.  A related_groups call includes its table's zero fill, the
finish, select and gather launches, and the wrapper's upload of the offsets.  Prints one JSON object per case."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402

ROUNDS = 5
ITERS = 5
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}


def make_rows(n, d, dtype, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.zeros((n, _native.padded_dim(d, dtype)), dtype=dtype, device=dev)
    for lo in range(0, n, 100_000):
        x = torch.randn((min(100_000, n - lo), d), device=dev, generator=g)
        out[lo: lo + len(x), :d] = (x / x.norm(dim=1, keepdim=True)).to(dtype)
    return out


def event_us(fn, iters):
    """device microseconds per call of `iters` back-to-back calls"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def spread(times):
    t = sorted(times)
    return {"median_us": round(t[len(t) // 2], 1), "min_us": round(t[0], 1), "max_us": round(t[-1], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000x768xfloat16,100000x384xfloat32")
    ap.add_argument("--ms", default="1,128,1024")
    ap.add_argument("--doc-rows", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("related_bench: no GPU; nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        n, d, name = shape.split("x")
        n, d, dtype = int(n), int(d), DTYPES[name]
        rows = make_rows(n, d, dtype, dev)
        contiguous = (torch.arange(n, device=dev) // args.doc_rows).to(torch.int32)
        n_groups = int(contiguous[-1]) + 1
        shuffled = contiguous[torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(2))]
        shuffled = shuffled.contiguous()
        for M in (int(m) for m in args.ms.split(",")):
            sets = make_rows(M, d, dtype, dev, seed=1)
            calls = {
                "contiguous": lambda: _native.related_groups(sets, [0, M], rows, n, d, args.k, contiguous, n_groups, 0.5),
                "shuffled": lambda: _native.related_groups(sets, [0, M], rows, n, d, args.k, shuffled, n_groups, 0.5),
                "kmeans_assign": lambda: _native.kmeans_assign(rows, n, d, sets),
            }
            for fn in calls.values():                                              # warm-up of all
                event_us(fn, 2)
            times = {name_: [] for name_ in calls}
            for _ in range(ROUNDS):                                                # in turn: one device state
                for name_, fn in calls.items():
                    times[name_].append(event_us(fn, ITERS))
            out = {name_: spread(t) for name_, t in times.items()}
            base = out["kmeans_assign"]["median_us"]
            print(json.dumps({
                "what": "related_groups vs kmeans_assign (k = M)", "rows": n, "dim": d, "dtype": name, "M": M,
                "doc_rows": args.doc_rows, "n_groups": n_groups, "table_bytes": 8 * M * n_groups, **out,
                "contiguous_over_assign": round(out["contiguous"]["median_us"] / base, 3),
                "shuffled_over_assign": round(out["shuffled"]["median_us"] / base, 3)}), flush=True)
        del rows, contiguous, shuffled


if __name__ == "__main__":
    main()
