"""Measure the recommend scan (csrc/recommend.hip, _native.recommend_topk) against the boosted scan
(csrc/boosted.hip, _native.boosted_topk) at the same number of example / query COLUMNS: R requests of 16 slots are
16 R columns of the 128 x 128 tile body, so R = 64 does the MFMA and HBM work of a boosted batch of B = 1024 and appends
a sixteenth of the candidates.

    python tools/recommend_bench.py [--shape 1000000x768xfloat16] [--requests 64] [--k 5]

Workload: unit Gaussian rows and examples; requests of 16 examples (8 positive, 8 negative) and of 3 (2 positive, 1
negative; the other 13 slots unused but still computed: padding a request to 16 columns is deliberate), weight 1;
the boosted batch with a prior rising linearly from 0 to 1 and weight 0.2.  All operands already on the device, so a
call is the launches of the C entry point alone.  Each call is timed with device events in steady state: after a warm-up
of all three, ROUNDS rounds of ITERS calls each, the three taking turns round by round; the median round's time per call
is reported with the fastest and slowest, and the collection's bytes once over that time as GB/s.  Prints one JSON
object."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402
from tools.boost_bench import DTYPES, event_us, make_rows, spread  # noqa: E402

ROUNDS = 5
ITERS = 20
E = _native.MAX_RECOMMEND_EXAMPLES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1000000x768xfloat16")
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--k", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("recommend_bench: no GPU; nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    n, d, name = args.shape.split("x")
    n, d, dtype, R, k = int(n), int(d), DTYPES[name], args.requests, args.k
    rows = make_rows(n, d, dtype, dev)
    examples = make_rows(E * R, d, dtype, dev, seed=1)
    w = torch.ones(R, dtype=torch.float32, device=dev)
    signs = {}
    for label, (p, m) in (("16_examples", (8, 8)), ("3_examples", (2, 1))):
        s = np.zeros((R, E), np.int8)
        s[:, :p] = 1
        s[:, p: p + m] = -1
        signs[label] = torch.from_numpy(s.reshape(-1)).to(dev)
    B = E * R
    prior = torch.linspace(0.0, 1.0, n, dtype=torch.float32, device=dev)
    weight = torch.full((B,), 0.2, dtype=torch.float32, device=dev)
    ws_r = torch.empty(_native.recommend_topk_workspace_bytes(R, n, k), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(_native.boosted_topk_workspace_bytes(B, n, k), dtype=torch.uint8, device=dev)
    runs = {label: (lambda s=s: _native.recommend_topk(examples, s, w, rows, n, d, k, workspace=ws_r))
            for label, s in signs.items()}
    runs["boosted"] = lambda: _native.boosted_topk(examples, rows, n, d, k, prior, weight, workspace=ws_b)
    for fn in runs.values():
        event_us(fn, 2)
    times = {label: [] for label in runs}
    for _ in range(ROUNDS):                                                # in turn: one device state
        for label, fn in runs.items():
            times[label].append(event_us(fn, ITERS))
    out = {"what": "recommend_topk vs boosted_topk at the same columns", "rows": n, "dim": d, "dtype": name, "k": k,
           "requests": R, "boosted_batch": B, "rounds": ROUNDS, "calls_per_round": ITERS,
           "candidate_slots": _native.candidate_capacity(k)}
    nbytes = n * rows.shape[1] * rows.element_size()
    for label in runs:
        t = spread(times[label])
        t["collection_gb_per_s"] = round(nbytes / t["median_us"] / 1e3, 1)
        out[label] = t
    for label in signs:
        runs[label]()
        torch.cuda.synchronize()
        counts = ws_r[: 4 * R].view(torch.int32).cpu().numpy().astype(np.int64)   # the main pass's counters
        out[label]["survivors_mean"] = round(float(counts.mean()), 1)
        out[label]["requests_overflowed"] = int((counts > _native.candidate_capacity(k)).sum())
        out[label + "_over_boosted"] = round(out[label]["median_us"] / out["boosted"]["median_us"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
