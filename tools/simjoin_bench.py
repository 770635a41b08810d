"""Measure the near-duplicate self-join (csrc/simjoin.hip, mmrag_sim_join) against the join done the only way the
library allowed before it: torch blocks of X[a:a+8192] @ X[b:b+8192].T, `>= t`, nonzero, over the upper triangle.

    python tools/simjoin_bench.py [--shapes 100k,250k,1m] [--no-baseline]

Shapes: 100k x 384 float32, 250k x 768 float16, 1M x 768 float16; unit Gaussian rows with about 0.1 % planted
near-copies (cosine 0.99), joined at 0.95.  Both joins run in this process on the same device and data.  Device times
come from HIP events: the kernel is the median of three calls after one warm-up call, the baseline one pass after a
warm-up of its first blocks.  The pair counts of the two must agree.  The kernel's FLOP/s (n (n - 1) / 2 pairs x 2 d, the
padded tile work not counted) are given as a fraction of the v_mfma_f32_16x16x32_f16 rate that
mmrag_bench_mfma_f16_16x16x32 measures on this device (float32 rows run on the float32 matrix instruction, 1/16 of that
rate by design).  Prints one JSON object per shape."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402

SHAPES = {"100k": (100_000, 384, torch.float32), "250k": (250_000, 768, torch.float16),
          "1m": (1_000_000, 768, torch.float16)}
T, COS, BLOCK = 0.95, 0.99, 8192


def make_rows(n, d, dtype, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    ld = _native.padded_dim(d, dtype)
    out = torch.zeros((n, ld), dtype=dtype, device=dev)
    step = 100_000
    for lo in range(0, n, step):
        x = torch.randn((min(step, n - lo), d), device=dev, generator=g)
        out[lo: lo + len(x), :d] = (x / x.norm(dim=1, keepdim=True)).to(dtype)
    m = max(1, n // 1000)
    pick = torch.randperm(n, device=dev, generator=g)[: 2 * m]
    src, dst = pick[:m], pick[m:]
    base = out[src, :d].float()
    u = torch.randn((m, d), device=dev, generator=g)
    u -= (u * base).sum(1, keepdim=True) * base
    u /= u.norm(dim=1, keepdim=True)
    out[dst, :d] = (COS * base + (1 - COS * COS) ** 0.5 * u).to(dtype)
    return out, m


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def kernel_join(rows, n, d, cap=1 << 20):
    L, dev = _native.lib(), rows.device
    pairs = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    scores = torch.empty(cap, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def call():
        st = L.mmrag_sim_join(rows.data_ptr(), n, rows.shape[1], _native._TORCH2DT[rows.dtype], d, None, T,
                              pairs.data_ptr(), scores.data_ptr(), cap, count.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
        _native._check(st, "mmrag_sim_join")

    event_ms(call)
    times = sorted(event_ms(call)[0] for _ in range(3))
    return times[1], int(count.item())


def torch_join(rows, n, d, max_blocks=None):
    x = rows[:, :d]
    total, done = 0, 0
    for a in range(0, n, BLOCK):
        for b in range(a, n, BLOCK):
            hit = (x[a: a + BLOCK] @ x[b: b + BLOCK].T) >= T
            if a == b:
                hit = torch.triu(hit, 1)
            total += torch.nonzero(hit).shape[0]
            done += 1
            if max_blocks is not None and done >= max_blocks:
                return total
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100k,250k,1m")
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    peak = _native.measure_peaks(dev)["mfma_f16_16x16x32_TFLOPs"]
    for key in args.shapes.split(","):
        n, d, dtype = SHAPES[key]
        rows, planted = make_rows(n, d, dtype, dev)
        ms, count = kernel_join(rows, n, d)
        flops = n * (n - 1) / 2 * 2 * d
        rec = {"what": "simjoin", "rows": n, "dim": d, "dtype": str(dtype).replace("torch.", ""), "threshold": T,
               "planted": planted, "pairs_kernel": count, "kernel_ms": round(ms, 3),
               "kernel_TFLOPs": round(flops / ms / 1e9, 1), "mfma_f16_16x16x32_TFLOPs": peak,
               "fraction_of_mfma_rate": round(flops / ms / 1e9 / peak, 4)}
        if not args.no_baseline:
            torch_join(rows, n, d, max_blocks=4)
            torch.cuda.synchronize()
            base_ms, base_count = event_ms(lambda: torch_join(rows, n, d))
            rec.update(torch_blocks_ms=round(base_ms, 3), pairs_torch=base_count, counts_agree=base_count == count,
                       speedup=round(base_ms / ms, 2))
        print(json.dumps(rec), flush=True)
        del rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
