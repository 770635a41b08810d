"""Measure the range scan (csrc/range.hip, _native.range_scan) against the filtered top-k of the same batch and k
(csrc/filtered.hip, _native.filtered_topk): the same masked scan with another epilogue.

    python tools/range_bench.py [--rows 1000000] [--batches 1,64,256] [--limit 10] [--doc-rows 500]

Workload: `rows` x 768 float16 unit Gaussian rows, a batch of B unit Gaussian queries, one all-ones bitmap for every
query (both kernels read it: the comparison is of the epilogues).  A cosine of such rows is about N(0, 1 / 768), so the
thresholds z / sqrt(768) for z = 4.265, 3.09 and 0.524 pass about 1e-5, 1e-3 and 0.3 of the rows; the measured share is
printed.  Facet columns: none, `type` (3 values, row i has i % 3: neighbours differ, every passing row is an atomic of its
own), and `type` + `doc` (rows / doc-rows values in contiguous runs).  Per (B, pass rate, columns), in this process on the
same rows, each timed as the wall clock of a call that ends in a device synchronise:
  range       range_scan with `limit` hits
  range_0     range_scan with limit 0 (counts and facets only: no candidates, no select)
  filtered    filtered_topk with k = `limit` (once per B: it has no threshold and no columns)
After a warm-up of each, ROUNDS rounds run them in turn; the median, fastest and slowest round are printed, and
"range_over_filtered", the ratio of the medians.  One JSON object per line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402

ROUNDS = 5
RATES = (("1e-5", 4.265), ("1e-3", 3.09), ("0.3", 0.524))


def make_rows(n, d, dtype, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.zeros((n, _native.padded_dim(d, dtype)), dtype=dtype, device=dev)
    for lo in range(0, n, 100_000):
        x = torch.randn((min(100_000, n - lo), d), device=dev, generator=g)
        out[lo: lo + len(x), :d] = (x / x.norm(dim=1, keepdim=True)).to(dtype)
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(times):
    t = sorted(times)
    return {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--doc-rows", type=int, default=500)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("range_bench: no GPU; nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    n, d, dtype, limit = args.rows, 768, torch.float16, args.limit
    rows = make_rows(n, d, dtype, dev)
    at = torch.arange(n, device=dev)
    col_type = (at % 3).to(torch.int32)
    col_doc = (at // args.doc_rows).to(torch.int32)
    n_docs = (n + args.doc_rows - 1) // args.doc_rows
    columns = {0: ([], []), 1: ([col_type], [3]), 2: ([col_type, col_doc], [3, n_docs])}
    vis = torch.full((1, _native.filter_words(n)), -1, dtype=torch.int32, device=dev)
    for B in (int(b) for b in args.batches.split(",")):
        q = make_rows(B, d, dtype, dev, seed=1)
        foq = [0] * B
        ws_f = torch.empty(_native.filtered_topk_workspace_bytes(B, n, limit), dtype=torch.uint8, device=dev)
        filtered = lambda: _native.filtered_topk(q, rows, n, d, limit, foq, vis, workspace=ws_f)      # noqa: E731
        for name, z in RATES:
            thr = torch.full((B,), z / d ** 0.5, dtype=torch.float32, device=dev)
            for n_cols, (cols, sizes) in columns.items():
                slots = sum(g + 1 for g in sizes)
                ws = torch.empty(_native.range_scan_workspace_bytes(B, n, limit, slots), dtype=torch.uint8, device=dev)
                full = lambda: _native.range_scan(q, rows, n, d, thr, limit, cols, sizes, filter_of_query=foq,   # noqa: E731
                                                  vis_bits=vis, workspace=ws)
                zero = lambda: _native.range_scan(q, rows, n, d, thr, 0, cols, sizes, filter_of_query=foq,       # noqa: E731
                                                  vis_bits=vis, workspace=ws)
                for fn in (full, zero, filtered):
                    wall_ms(fn)
                times = {"range": [], "range_0": [], "filtered": []}
                for _ in range(ROUNDS):                                       # in turn: one device state
                    ms, out = wall_ms(full)
                    times["range"].append(ms)
                    times["range_0"].append(wall_ms(zero)[0])
                    times["filtered"].append(wall_ms(filtered)[0])
                med = {key: spread(t)["median_ms"] for key, t in times.items()}
                print(json.dumps({"what": "range_scan", "rows": n, "dim": d, "dtype": "float16", "batch": B,
                                  "limit": limit, "pass_rate": name, "facet_columns": n_cols, "facet_slots": slots,
                                  "measured_pass_rate": float(out[0].double().mean().item() / n),
                                  **{key: spread(t) for key, t in times.items()},
                                  "range_over_filtered": round(med["range"] / med["filtered"], 3),
                                  "range_0_over_filtered": round(med["range_0"] / med["filtered"], 3)}), flush=True)


if __name__ == "__main__":
    main()
