"""Measure grouping hits by document (csrc/group.hip): the grouping kernel alone, `VectorIndex.grouped_search` as a
whole at a fixed depth, and beside them the dense search of the same depth that the grouped call contains
(`search(C)`; this change touches no search kernel, so that figure is the parent commit's too).

    python tools/group_bench.py [--quick]

Random unit rows, 1M x 768 fp16, 50 000 documents of 20 rows each (rows dealt round-robin); B = 256; (C, G, S) in
{(64, 5, 1), (256, 5, 3), (4096, 256, 16)}.  Device times come from HIP events, median of 20 calls, after the same call
has been held for 0.5 s so the chip sits at the clock it sustains.  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats -- python tools/group_bench.py --quick` run (five grouped_query calls per
shape, no hold).  Prints one JSON object per measurement."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402
from multimodal_rag_amd.index import VectorIndex  # noqa: E402
from tools.mmr_bench import timed  # noqa: E402

SHAPES = [(64, 5, 1), (256, 5, 3), (4096, 256, 16)]


def document_index(n, d, dtype, dev, n_docs):
    idx = VectorIndex(d, dtype=dtype, device=dev, capacity=n)
    step = 100_000
    for lo in range(0, n, step):
        m = min(step, n - lo)
        rows = torch.randn((m, idx.ld), device=dev, dtype=torch.float32)
        rows[:, d:] = 0
        rows = (rows / rows.norm(dim=1, keepdim=True)).to(dtype)
        idx.add_rows_device(rows, None, [{"doc_id": f"doc{i % n_docs}"} for i in range(lo, lo + m)],
                            [f"id{i}" for i in range(lo, lo + m)])
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="five grouped_query calls per shape, no hold (rocprofv3 run)")
    args = ap.parse_args()
    dev = "cuda:0"
    n, d, B = 1_000_000, 768, 256
    idx = document_index(n, d, torch.float16, dev, 50_000)
    col = idx.enable_grouping("doc_id")["col"]
    q = torch.randn((B, d), device=dev)
    q = q / q.norm(dim=1, keepdim=True)
    for C, G, S in SHAPES:
        if args.quick:
            for _ in range(5):
                idx.grouped_query(q, n_groups=G, group_size=S, fetch_k=C, include=())
            torch.cuda.synchronize()
            continue
        s, r = idx.search(q, C)
        s, r = s.contiguous(), r.contiguous()
        info = _native.group_select(s, r, col, n, G, S)[4].cpu()
        rec = {"what": "group", "rows": n, "dim": d, "B": B, "C": C, "G": G, "S": S,
               "groups_found_min": int(info[:, 0].min()), "valid_min": int(info[:, 1].min()),
               "select_us": timed(lambda: _native.group_select(s, r, col, n, G, S)),
               "grouped_search_us": timed(lambda: idx.grouped_search(q, G, S, fetch_k=C)),
               "search_C_us": timed(lambda: idx.search(q, C)),
               "search_5_us": timed(lambda: idx.search(q, 5))}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
