"""FP8 collections against the fp16 search on one device, one process.

    python tools/f8_bench.py [--rows 1000000] [--dim 768]

Per (B, k): the fp16 index's search(k); the FP8 list scan alone (mmrag_cosine_topk on the codes, depth k); the FP8
candidate search at the default over-fetch; mmrag_rescore_topk alone; the whole re-scored search(k).  The workload is
held 0.5 s first, then timed with device events, median of 20.  Prints one JSON line per row of the table."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_rag_amd import _native  # noqa: E402
from multimodal_rag_amd.config import settings  # noqa: E402
from multimodal_rag_amd.index import VectorIndex  # noqa: E402


def timed(fn, hold=0.5, reps=20):
    t0 = time.time()
    while time.time() - t0 < hold:
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    a = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    f16 = VectorIndex(a.dim, dtype=torch.float16, device=dev, capacity=a.rows)
    f8 = VectorIndex(a.dim, dtype=torch.float8_e4m3fn, device=dev, capacity=a.rows)
    step = 100000
    for lo in range(0, a.rows, step):
        m = min(step, a.rows - lo)
        x = torch.nn.functional.normalize(torch.randn(m, a.dim, device=dev, generator=g), dim=1)
        ids = [str(i) for i in range(lo, lo + m)]
        f16.add(x, ids=ids)
        f8.add(x, ids=ids)
    print(json.dumps({"rows": a.rows, "dim": a.dim, "fp16_bytes": f16.bytes_per_row() * a.rows,
                      "fp8_scan_bytes": f8.ld * a.rows, "fp8_plane_bytes": f8.plane_ld * f8.plane.element_size() * a.rows}), flush=True)
    for B in (1, 32, 256):
        q = torch.nn.functional.normalize(torch.randn(B, a.dim, device=dev, generator=g), dim=1)
        q8 = f8._pack_queries(q, check_norm=False)
        qp = f8._pack_plane_queries(q)
        for k in (5, 20):
            C = min(max(_native.MAX_K, int(settings.MMRAG_F8_OVERSAMPLE) * k), _native.MAX_K_DEEP)
            _, cand = f8._scan(q8, C, None)
            cand = cand.contiguous()
            row = {"B": B, "k": k, "C": C,
                   "fp16_search_us": timed(lambda: f16.search(q, k)),
                   "fp8_list_scan_us": timed(lambda: f8._scan(q8, k, None)),
                   "fp8_candidates_us": timed(lambda: f8._scan(q8, C, None)),
                   "rescore_us": timed(lambda: _native.rescore_topk(qp, f8.plane, a.dim, cand, k)),
                   "fp8_search_us": timed(lambda: f8.search(q, k))}
            print(json.dumps({k_: (round(v, 1) if isinstance(v, float) else v) for k_, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
