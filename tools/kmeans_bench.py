"""Measure topic clustering (csrc/kmeans.hip): the nearest-centroid kernel against torch, and one whole
VectorIndex.cluster().

    python tools/kmeans_bench.py [--rows 1000000] [--no-cluster]

Shapes: one mmrag_kmeans_assign at 1M x 768 float16 with k = 256 and k = 1024; one cluster() at 1M x 384 float16 with
k = 256.  Rows are unit Gaussian; the centroids are k of the rows.  Baseline, in this process on the same tensors: torch.matmul
of row chunks (65536 rows) against the centroids, then max / argmax.  Device times come from HIP events around `REPS`
back-to-back calls after a warm-up of the same; the median, the fastest and the slowest of `ROUNDS` such windows are
printed, kernel and baseline windows alternating.  Beside each time stand the two floors of the shape: the rows read once
from HBM (n . ld . bytes / 8 TB/s) and the matrix work (2 n k d / the v_mfma_f32_16x16x32_f16 rate that
mmrag_bench_mfma_f16_16x16x32 measures on this device).  The two assignments are compared: rows that differ must differ by
a score tie (both scores within 2e-4).  Prints one JSON object per measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402

HBM_BYTES_PER_S = 8e12
CHUNK, REPS, ROUNDS = 65536, 5, 5


def make_rows(n, d, dtype, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.zeros((n, _native.padded_dim(d, dtype)), dtype=dtype, device=dev)
    for lo in range(0, n, 100_000):
        x = torch.randn((min(100_000, n - lo), d), device=dev, generator=g)
        out[lo: lo + len(x), :d] = (x / x.norm(dim=1, keepdim=True)).to(dtype)
    return out


def window_ms(fn):
    """device time of REPS back-to-back calls, per call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS, out


def torch_assign(rows, n, cent):
    best = torch.empty(n, dtype=torch.float32, device=rows.device)
    arg = torch.empty(n, dtype=torch.int64, device=rows.device)
    for lo in range(0, n, CHUNK):
        s = torch.matmul(rows[lo: lo + CHUNK], cent.T)
        v, a = s.max(dim=1)
        best[lo: lo + CHUNK], arg[lo: lo + CHUNK] = v.float(), a
    return arg, best


def spread(times):
    t = sorted(times)
    return {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--no-cluster", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kmeans_bench: no GPU; nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    peak = _native.measure_peaks(dev)["mfma_f16_16x16x32_TFLOPs"]
    n, d, dtype = args.rows, 768, torch.float16
    rows = make_rows(n, d, dtype, dev)
    for k in (256, 1024):
        cent = rows[torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(k))[:k]].contiguous()
        kernel = lambda: _native.kmeans_assign(rows, n, d, cent)     # noqa: E731
        base = lambda: torch_assign(rows, n, cent)                  # noqa: E731
        window_ms(kernel), window_ms(base)                          # warm-up of both
        tk, tb = [], []
        for _ in range(ROUNDS):                                     # alternating windows: one device state for both
            ms, (a, s) = window_ms(kernel)
            tk.append(ms)
            ms, (ta, ts) = window_ms(base)
            tb.append(ms)
        differ = (a.long() != ta).nonzero().squeeze(1)
        tie = bool(((s[differ] - ts[differ]).abs() <= 2e-4).all()) if differ.numel() else True
        flops = 2.0 * n * k * d
        rec = {"what": "kmeans_assign", "rows": n, "dim": d, "dtype": "float16", "k": k,
               "kernel": spread(tk), "torch_chunks": spread(tb),
               "speedup_median": round(spread(tb)["median_ms"] / spread(tk)["median_ms"], 2),
               "hbm_floor_ms": round(n * rows.shape[1] * rows.element_size() / HBM_BYTES_PER_S * 1e3, 3),
               "mfma_floor_ms": round(flops / (peak * 1e12) * 1e3, 3), "mfma_f16_16x16x32_TFLOPs": peak,
               "kernel_TFLOPs": round(flops / spread(tk)["median_ms"] / 1e9, 1),
               "rows_that_differ": int(differ.numel()), "all_differences_are_ties": tie}
        print(json.dumps(rec), flush=True)
    del rows
    torch.cuda.empty_cache()
    if args.no_cluster:
        return
    from multimodal_rag_amd.index import VectorIndex

    d = 384
    idx = VectorIndex(dim=d, dtype=dtype, device="cuda:0", capacity=n)
    idx.add_rows_device(make_rows(n, d, dtype, dev, seed=1), None, None, [str(i) for i in range(n)])
    idx.cluster(n_clusters=256, max_iter=2)                         # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        rep = idx.cluster(n_clusters=256, max_iter=10)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"what": "VectorIndex.cluster (wall clock, report included)", "rows": n, "dim": d,
                      "dtype": "float16", "k": 256, "max_iter": 10, "iterations": rep["iterations"],
                      "converged": rep["converged"], **spread(times),
                      "objective_first_last": [round(rep["objective"][0], 4), round(rep["objective"][-1], 4)]}),
          flush=True)


if __name__ == "__main__":
    main()
