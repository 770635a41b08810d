"""Measure filtered retrieval (csrc/filtered.hip, VectorIndex.filtered_search) against the two ways the same batch was
served without it.

    python tools/filtered_bench.py [--rows 1000000] [--doc-rows 500] [--batch 256] [--k 5] [--mix doc,page,type]

Workload: a float16 collection of `rows` x 768 unit Gaussian rows in documents of `doc-rows` contiguous rows, metadata
doc_id, type (one of 3) and page (1 .. doc-rows); `batch` queries.  Filter mixes:
  doc    `batch` distinct doc_id equalities (the shape of tools/scoped_bench.py: most row tiles are skipped)
  page   `batch` distinct page windows of a tenth of a document's pages each, about 10 % of the rows, scattered over the
         whole collection: no tile is skipped
  type   one {"type": "table"} for all: a third of the rows
Three ways per mix, in this process on the same collection, each timed as the wall clock of a call that ends in a device
synchronise (the host work -- compiling, tables, bitmaps -- is part of what a caller waits for):
  1. filtered         one filtered_search of the batch
  2. where_per_query  the same queries as single search(where=...) calls with MMRAG_DEVICE_FILTERS off: the host bitmap
                      and a full scan each.  A page window is a Python scan of every row per call and a type filter a
                      bitmap of a third of them, so only the first `--singles` (default 8) calls of those mixes are timed;
                      "where_per_query_batch_ms" is that median scaled to the batch and says so with "timed_calls"
  3. unfiltered       one search of the batch over every row
After a warm-up of each, ROUNDS rounds run the three in turn; the median, fastest and slowest round are printed.  The
answers of 1 and 2 are compared on the timed queries (same rows, scores within 2e-4); "eval_ms" is the wall clock of the
filter programs' evaluation alone, "items_issued" the (row tile, query tile) items of the main pass out of "items".
Prints one JSON object per mix."""
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
TYPES = ("text", "table", "image")


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
    ap.add_argument("--doc-rows", type=int, default=500)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--mix", default="doc,page,type")
    ap.add_argument("--singles", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("filtered_bench: no GPU; nothing is measured on a CPU")
    from multimodal_rag_amd.index import VectorIndex

    dev = torch.device("cuda:0")
    n, d, dtype, B, k, per_doc = args.rows, 768, torch.float16, args.batch, args.k, args.doc_rows
    n_docs = (n + per_doc - 1) // per_doc
    if B > n_docs or B > per_doc:
        sys.exit(f"filtered_bench: {B} distinct documents / page windows asked of {n_docs} / {per_doc}")
    idx = VectorIndex(dim=d, dtype=dtype, device="cuda:0", capacity=n)
    idx.device_filters = False
    metas = [{"doc_id": f"doc{i // per_doc}", "type": TYPES[i % 3], "page": i % per_doc + 1} for i in range(n)]
    idx.add_rows_device(make_rows(n, d, dtype, dev), None, metas, [str(i) for i in range(n)])
    del metas
    g = np.random.default_rng(0)
    window = max(1, per_doc // 10)
    starts = g.choice(per_doc - window + 1, B, replace=False) + 1
    mixes = {"doc": [{"doc_id": f"doc{i}"} for i in g.choice(n_docs, B, replace=False)],
             "page": [{"page": {"$gte": int(lo), "$lt": int(lo) + window}} for lo in starts],
             "type": [{"type": "table"}] * B}
    q = make_rows(B, d, torch.float32, dev, seed=1)[:, :d].contiguous()
    tiles = (n + TILE - 1) // TILE
    for name in args.mix.split(","):
        wheres = mixes[name]
        timed = B if name == "doc" else min(args.singles, B)
        filtered = lambda: idx.filtered_search(q, k, wheres)                                  # noqa: E731
        per_query = lambda: [idx.search(q[b: b + 1], k, where=wheres[b]) for b in range(timed)]   # noqa: E731
        unfiltered = lambda: idx.search(q, k)                                                 # noqa: E731
        for fn in (filtered, per_query, unfiltered):                                          # warm-up of all three
            wall_ms(fn)
        times = {"filtered": [], "where_per_query": [], "unfiltered": []}
        for _ in range(ROUNDS):                                                               # in turn: one device state
            ms, (s1, r1) = wall_ms(filtered)
            times["filtered"].append(ms)
            ms, parts = wall_ms(per_query)
            times["where_per_query"].append(ms)
            ms, _ = wall_ms(unfiltered)
            times["unfiltered"].append(ms)
        s2 = torch.cat([p[0] for p in parts]).cpu().numpy()
        r2 = torch.cat([p[1] for p in parts]).cpu().numpy()
        s1, r1 = s1.cpu().numpy()[:timed], r1.cpu().numpy()[:timed]
        # the pieces: the programs' evaluation alone, and the items the main pass issues
        with idx._lock:
            programs = list(dict.fromkeys(idx._compiled(w)[0] for w in wheres))
            vis = torch.empty((len(programs), _native.filter_words(n)), dtype=torch.int32, device=dev)
            evals = [wall_ms(lambda: idx._eval_programs(programs, vis, None))[0] for _ in range(ROUNDS + 1)][1:]
            of_query = [programs.index(idx._compiled(w)[0]) for w in wheres]
            qp = idx._pack_queries(q)
            items = _native.filtered_topk(qp, idx.matrix, n, d, k, of_query, vis, count_items=True)[2]
        med = {key: spread(t)["median_ms"] for key, t in times.items()}
        rec = {"what": "filtered_search", "mix": name, "rows": n, "dim": d, "dtype": "float16", "batch": B, "k": k,
               "distinct_filters": len(programs), "share_of_rows_visible": round(float(_bit_count(vis[0]) / n), 4),
               **{key: spread(t) for key, t in times.items()},
               "timed_calls": timed, "where_per_query_batch_ms": round(med["where_per_query"] * B / timed, 3),
               "filtered_over_where_per_query": round(med["filtered"] / (med["where_per_query"] * B / timed), 5),
               "filtered_over_unfiltered": round(med["filtered"] / med["unfiltered"], 3),
               "eval_ms": spread(evals), "items_issued": int(items.item()), "items": tiles * ((B + TILE - 1) // TILE),
               "queries_with_the_same_rows": int((np.sort(r1, 1) == np.sort(r2, 1)).all(1).sum()),
               "max_score_difference": float(np.abs(s1 - s2).max())}
        print(json.dumps(rec), flush=True)


def _bit_count(words: torch.Tensor) -> int:
    w = words.cpu().numpy().view(np.uint32)
    return int(np.unpackbits(w.view(np.uint8)).sum())


if __name__ == "__main__":
    main()
