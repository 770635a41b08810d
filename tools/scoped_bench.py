"""Measure document-scoped retrieval (csrc/scoped.hip, VectorIndex.scoped_search) against the two ways the same batch was
served without it.

    python tools/scoped_bench.py [--rows 1000000] [--doc-rows 500] [--batch 256] [--k 5]

Workload: a float16 collection of `rows` x 768 unit Gaussian rows in documents of `doc-rows` contiguous rows; `batch`
queries, each with its own single-document scope (distinct documents drawn with a fixed seed).  Three ways, in this
process on the same collection, each timed as the wall clock of a call that ends in a device synchronise (the host work
-- scope tables, bitmaps -- is part of what a caller waits for):
  1. scoped          one scoped_search of the batch
  2. where_per_query the same queries as `batch` search(where={"doc_id": x}) calls (a host bitmap and a full scan each)
  3. unfiltered      one search of the batch over every row (what the batch costs with no restriction at all)
After a warm-up of each, ROUNDS rounds run the three in turn; the median, fastest and slowest round are printed.  The
answers of 1 and 2 are compared (same rows per query, scores within 2e-4), and the share of 128-row tiles the scoped scan
skips is counted on the host from the group column.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402

ROUNDS = 5
TILE = 128


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


def skipped_tiles(col, ordinals_per_query):
    """(share of row tiles no query tile wants, share of (row tile, query tile) items skipped)"""
    n = col.size
    tiles = (n + TILE - 1) // TILE
    tile_of_row = np.arange(n) // TILE
    wanted_any = np.zeros(tiles, bool)
    items = skipped = 0
    for lo in range(0, len(ordinals_per_query), TILE):
        union = np.unique(np.concatenate([np.asarray(o) for o in ordinals_per_query[lo: lo + TILE]]))
        wanted = np.zeros(tiles, bool)
        wanted[np.unique(tile_of_row[np.isin(col, union)])] = True
        wanted_any |= wanted
        items += tiles
        skipped += int((~wanted).sum())
    return float((~wanted_any).mean()), skipped / items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--doc-rows", type=int, default=500)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scoped_bench: no GPU; nothing is measured on a CPU")
    from multimodal_rag_amd.index import VectorIndex

    dev = torch.device("cuda:0")
    n, d, dtype, B, k = args.rows, 768, torch.float16, args.batch, args.k
    n_docs = (n + args.doc_rows - 1) // args.doc_rows
    if B > n_docs:
        sys.exit(f"scoped_bench: {B} distinct documents asked of {n_docs}")
    idx = VectorIndex(dim=d, dtype=dtype, device="cuda:0", capacity=n)
    names = [f"doc{i // args.doc_rows}" for i in range(n)]
    idx.add_rows_device(make_rows(n, d, dtype, dev), None, [{"doc_id": s} for s in names], [str(i) for i in range(n)])
    del names
    g = np.random.default_rng(0)
    picked = g.choice(n_docs, B, replace=False)
    scopes = [f"doc{i}" for i in picked]
    q = make_rows(B, d, torch.float32, dev, seed=1)[:, :d].contiguous()
    st = idx.enable_grouping("doc_id")

    scoped = lambda: idx.scoped_search(q, k, scopes)                                        # noqa: E731
    per_query = lambda: [idx.search(q[b: b + 1], k, where={"doc_id": scopes[b]}) for b in range(B)]   # noqa: E731
    unfiltered = lambda: idx.search(q, k)                                                   # noqa: E731
    for fn in (scoped, per_query, unfiltered):                                              # warm-up of all three
        wall_ms(fn)
    times = {"scoped": [], "where_per_query": [], "unfiltered": []}
    for _ in range(ROUNDS):                                                                 # in turn: one device state
        ms, (s1, r1) = wall_ms(scoped)
        times["scoped"].append(ms)
        ms, parts = wall_ms(per_query)
        times["where_per_query"].append(ms)
        ms, _ = wall_ms(unfiltered)
        times["unfiltered"].append(ms)
    s2 = torch.cat([p[0] for p in parts]).cpu().numpy()
    r2 = torch.cat([p[1] for p in parts]).cpu().numpy()
    s1, r1 = s1.cpu().numpy(), r1.cpu().numpy()
    same_rows = int((np.sort(r1, 1) == np.sort(r2, 1)).all(1).sum())
    col = st["col"][:n].cpu().numpy()
    tiles_free, items_free = skipped_tiles(col, [[st["ordinal"][s]] for s in scopes])
    rec = {"what": "scoped_search", "rows": n, "dim": d, "dtype": "float16", "documents": n_docs,
           "rows_per_document": args.doc_rows, "batch": B, "k": k, "distinct_scopes": len(set(scopes)),
           "share_of_rows_in_scope": round(B * args.doc_rows / n, 4),
           **{name: spread(t) for name, t in times.items()},
           "scoped_over_where_per_query": round(spread(times["scoped"])["median_ms"]
                                                / spread(times["where_per_query"])["median_ms"], 4),
           "scoped_over_unfiltered": round(spread(times["scoped"])["median_ms"]
                                           / spread(times["unfiltered"])["median_ms"], 3),
           "row_tiles_skipped": round(tiles_free, 4), "tile_items_skipped": round(items_free, 4),
           "queries_with_the_same_rows": same_rows, "max_score_difference": float(np.abs(s1 - s2).max())}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
