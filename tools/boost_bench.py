"""Measure the boosted scan (csrc/boosted.hip, _native.boosted_topk) against the project's exact any-k scan, the deep
search (csrc/search_deep.hip, _native.cosine_topk_deep), at the same (B, n, d, k).

    python tools/boost_bench.py [--shapes 1000000x768xfloat16,100000x384xfloat32] [--batches 1,256] [--ks 5,50]

Workload: unit Gaussian rows; a prior rising linearly with the row number from 0 to 1 (a recency prior) and weight 0.2 for
every query; prior and weight already on the device, so a call is the launches of the C entry point alone.  Each call is
timed with device events around it in steady state: after a warm-up of both, ROUNDS rounds of ITERS calls each, the two
scans alternating round by round; the median round's time per call is reported with the fastest and slowest.  Both
entry points synchronise the stream once per call at these sizes (n exceeds the candidate slots), which the events
include.  The counters the boosted main pass leaves in its workspace give the survivors per query (mean, maximum) and
whether any query overflowed its slots.  The top-k of a weight-0 boosted call is compared with the deep search's (same
rows per query, scores within 2e-4).  Prints one JSON object per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402

ROUNDS = 5
ITERS = 10
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
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--ks", default="5,50")
    ap.add_argument("--weight", type=float, default=0.2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("boost_bench: no GPU; nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        n, d, name = shape.split("x")
        n, d, dtype = int(n), int(d), DTYPES[name]
        rows = make_rows(n, d, dtype, dev)
        prior = torch.linspace(0.0, 1.0, n, dtype=torch.float32, device=dev)
        for B in (int(b) for b in args.batches.split(",")):
            q = make_rows(B, d, dtype, dev, seed=1)
            weight = torch.full((B,), args.weight, dtype=torch.float32, device=dev)
            zero = torch.zeros(B, dtype=torch.float32, device=dev)
            for k in (int(v) for v in args.ks.split(",")):
                ws_b = torch.empty(_native.boosted_topk_workspace_bytes(B, n, k), dtype=torch.uint8, device=dev)
                ws_d = torch.empty(_native.cosine_topk_deep_workspace_bytes(B, n, k), dtype=torch.uint8, device=dev)
                boosted = lambda w=weight: _native.boosted_topk(q, rows, n, d, k, prior, w, workspace=ws_b)   # noqa: E731
                deep = lambda: _native.cosine_topk_deep(q, rows, n, d, k, workspace=ws_d)                     # noqa: E731
                for fn in (boosted, deep):                                             # warm-up of both
                    event_us(fn, 3)
                times = {"boosted": [], "deep": []}
                for _ in range(ROUNDS):                                                # in turn: one device state
                    times["boosted"].append(event_us(boosted, ITERS))
                    times["deep"].append(event_us(deep, ITERS))
                boosted()
                torch.cuda.synchronize()
                counts = ws_b[: 4 * B].view(torch.int32).cpu().numpy().astype(np.int64)   # the main pass's counters
                s0, r0, _ = boosted(zero)
                s1, r1 = deep()
                s0, r0, s1, r1 = (t.cpu().numpy() for t in (s0, r0, s1, r1))
                b_us, d_us = spread(times["boosted"]), spread(times["deep"])
                print(json.dumps({
                    "what": "boosted_topk vs cosine_topk_deep", "rows": n, "dim": d, "dtype": name, "batch": B, "k": k,
                    "weight": args.weight, "prior": "linear 0..1 in the row number", "boosted": b_us, "deep": d_us,
                    "boosted_over_deep": round(b_us["median_us"] / d_us["median_us"], 3),
                    "candidate_slots": _native.candidate_capacity(k),
                    "survivors_mean": round(float(counts.mean()), 1), "survivors_max": int(counts.max()),
                    "queries_overflowed": int((counts > _native.candidate_capacity(k)).sum()),
                    "weight0_same_rows_as_deep": int((np.sort(r0, 1) == np.sort(r1, 1)).all(1).sum()),
                    "weight0_max_score_difference": float(np.abs(s0 - s1).max())}), flush=True)
                del ws_b, ws_d
        del rows, prior


if __name__ == "__main__":
    main()
