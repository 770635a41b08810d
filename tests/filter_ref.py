"""Plain Python / numpy reference of filtered retrieval (csrc/filtered.hip, VectorIndex.filtered_search) and the generated
metadata and filters its tests share.  Query b sees row r iff r is alive and index.match_where(metadata[r], wheres[b])
is true, with the row's add time injected as "$added_at" into a copy of its metadata; its answer is the exact top-k of the
search oracle over the sub-matrix of the rows it sees, mapped back to global rows and padded with (-inf, -1) -- the
construction of tests/scoped_ref.py.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from multimodal_rag_amd.index import match_where
from oracle import search_oracle as O

T0 = 1_700_000_000.0      # the add time of row 0 of metadata(); row i: T0 + 60 i, every 13th unknown


def visible(metas: Sequence[Dict[str, Any]], where, alive: Optional[np.ndarray] = None,
            times: Optional[np.ndarray] = None) -> np.ndarray:
    """bool[n]: match_where per row ("$added_at" = the row's time where it is known), AND alive"""
    out = np.zeros(len(metas), dtype=bool)
    for i, meta in enumerate(metas):
        if times is not None and not np.isnan(times[i]):
            meta = {**meta, "$added_at": float(times[i])}
        out[i] = match_where(meta, where)
    if alive is not None:
        out &= np.asarray(alive, dtype=bool)[: out.size]
    return out


def topk_of_visible(q: np.ndarray, rows: np.ndarray, k: int, vis_of_query: Sequence[np.ndarray],
                    row_offset: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """q [B, d], rows [n, d] (the stored values, up-cast exactly); vis_of_query[b] = bool[n].  Returns (scores [B, k]
    float32 descending, ties to the lower row; rows [B, k] int64 + row_offset), (-inf, -1) padded."""
    B = q.shape[0]
    out_s = np.full((B, k), O.NEG_INF, dtype=np.float32)
    out_r = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        vis = np.nonzero(vis_of_query[b])[0]
        if vis.size == 0:
            continue
        ss, rr = O.cosine_topk(q[b: b + 1], rows[vis], k)
        live = rr[0] >= 0
        out_s[b, : live.sum()] = ss[0][live]
        out_r[b, : live.sum()] = vis[rr[0][live]] + row_offset
    return out_s, out_r


TYPES = ["text", "table", "image"]


def metadata(n: int, seed: int) -> Tuple[List[Dict[str, Any]], np.ndarray]:
    """n rows of metadata and their add times.  Keys: doc_id (str), type (3 strings), page (int 1..50, missing in about
    10 %), score (float of both signs, missing in about 15 %, None in a few), flag (bool), mixed (str in some rows, int
    in others), big (2**60) and nan (float NaN)"""
    g = np.random.default_rng(seed)
    metas = []
    for i in range(n):
        m: Dict[str, Any] = {"doc_id": f"doc{i // 7}", "type": TYPES[int(g.integers(0, 3))], "flag": bool(g.integers(0, 2)),
                             "mixed": f"m{i % 3}" if i % 2 else i % 5, "big": 2 ** 60, "nan": float("nan")}
        if g.random() > 0.1:
            m["page"] = int(g.integers(1, 51))
        u = g.random()
        if u > 0.15:
            m["score"] = float(np.round(g.normal(0.0, 2.0), 2))
        elif u < 0.03:
            m["score"] = None
        metas.append(m)
    times = T0 + 60.0 * np.arange(n)
    times[::13] = np.nan
    return metas, times


def _leaf(g, n_docs: int) -> Dict[str, Any]:
    kind = int(g.integers(0, 8))
    if kind <= 2:       # a number key
        key = ["page", "score", "flag"][kind]
        consts = {"page": [1, 7, 25, 25.0, 50, 51, 0, -3, 12.5, True], "score": [0, 0.0, -1.25, 1.5, 2, -2, 100, False],
                  "flag": [True, False, 1, 0, 0.5, 2]}[key]
        ops = ["$eq", "$ne", "$gt", "$gte", "$lt", "$lte", "$in", "$nin", None]
    elif kind <= 4:     # a string key
        key = ["doc_id", "type"][kind - 3]
        consts = [f"doc{int(g.integers(0, n_docs))}" for _ in range(6)] + ["nowhere"] if key == "doc_id" else TYPES + ["audio"]
        ops = ["$eq", "$ne", "$in", "$nin", None]
    elif kind == 5:     # a key no row has: numbers and strings alike
        key, consts = "ghost", [1, "x", 2.5, True]
        ops = ["$eq", "$ne", "$gt", "$gte", "$lt", "$lte", "$in", "$nin", None]
    elif kind == 6:     # the add time
        key = "$added_at"
        consts = [T0 - 1, T0, T0 + 60.0 * 100, T0 + 60.0 * 250 + 30, T0 + 1e9]
        ops = ["$eq", "$ne", "$gt", "$gte", "$lt", "$lte", "$in", "$nin"]
    else:               # a range on one key: several operators under it
        lo = int(g.integers(1, 40))
        return {"page": {"$gte": lo, "$lt": lo + int(g.integers(1, 20))}}
    op = ops[int(g.integers(0, len(ops)))]
    pick = lambda: consts[int(g.integers(0, len(consts)))]       # noqa: E731
    if op is None:
        return {key: pick()}
    if op in ("$in", "$nin"):
        return {key: {op: [pick() for _ in range(int(g.integers(1, 6)))]}}
    return {key: {op: pick()}}


def _tree(g, depth: int, n_docs: int) -> Dict[str, Any]:
    if depth <= 1 or g.random() < 0.25:
        return _leaf(g, n_docs)
    how = int(g.integers(0, 3))
    subs = [_tree(g, depth - 1, n_docs) for _ in range(int(g.integers(2, 4)) if depth <= 2 else 2)]
    if how == 2:        # several keys in one dict (AND): keys may collide, the later one wins as in any dict
        merged: Dict[str, Any] = {}
        for s in subs:
            merged.update(s)
        return merged
    return {"$and" if how == 0 else "$or": subs}


def covered_filters(n_rows: int, seed: int) -> List[Optional[Dict[str, Any]]]:
    """A seeded family of more than 300 filters the compiler must cover: every operator on every kind of key with
    present and absent constants, missing keys, $in of 1 and of 64, $and / $or / several keys / several operators
    nested up to depth 4, and the largest program there is (16 leaves, 31 instructions: a postfix program of binary
    combinators always holds an odd number)"""
    g = np.random.default_rng(seed)
    n_docs = max(1, n_rows // 7)
    out: List[Optional[Dict[str, Any]]] = [None, {}, {"$and": []}, {"$or": []}]
    for key, consts in (("page", [7, 25.0, 51, True]), ("score", [0, -1.25, 2]), ("flag", [True, 0, 0.5]),
                        ("ghost", [1, "x"]), ("$added_at", [T0, T0 + 6000.0])):
        for c in consts:
            for op in ("$eq", "$ne", "$gt", "$gte", "$lt", "$lte"):
                out.append({key: {op: c}})
            out += [{key: {"$in": [c]}}, {key: {"$nin": [c]}}]
            if key != "$added_at":
                out.append({key: c})
    for key, consts in (("doc_id", ["doc0", "doc3", "nowhere"]), ("type", ["table", "audio"])):
        for c in consts:
            out += [{key: c}, {key: {"$eq": c}}, {key: {"$ne": c}}, {key: {"$in": [c]}}, {key: {"$nin": [c]}},
                    {key: {"$in": [c, "other", "doc1"]}}, {key: {"$nin": ["other", c]}}]
    out += [{"page": {"$in": list(range(1, 65))}}, {"page": {"$nin": list(range(-10, 54))}},
            {"doc_id": {"$in": [f"doc{i}" for i in range(64)]}}, {"doc_id": {"$nin": [f"doc{2 * i}" for i in range(64)]}},
            {"type": {"$in": ["a%d" % i for i in range(64)]}}, {"ghost": {"$in": list(range(64))}}]
    out.append({"$and": [{"page": {"$ne": p}} for p in range(1, 17)]})                 # 31 instructions
    out.append({"$or": [{"$and": [{"page": {"$gte": 10 * i}}, {"page": {"$lt": 10 * i + 3}}]} for i in range(8)]})  # 31
    out.append({"$or": [{"$and": [{"type": "table", "flag": True}, {"$or": [{"page": {"$lt": 5}}, {"score": {"$gt": 1}}]}]},
                        {"doc_id": "doc2"}]})                                           # depth 4
    while len(out) < 340:
        out.append(_tree(g, int(g.integers(1, 5)), n_docs))
    return out


def uncovered_filters() -> List[Tuple[str, Dict[str, Any]]]:
    """(what it is, filter) for the forms the compiler must refuse, each with a reason"""
    return [
        ("a key of strings and ints", {"mixed": "m1"}),
        ("a key of strings and ints, in a tree", {"$and": [{"type": "table"}, {"mixed": {"$ne": 3}}]}),
        ("ints beyond 2**53", {"big": {"$eq": 2 ** 60}}),
        ("float NaN values", {"nan": {"$gt": 0}}),
        ("an ordering operator on strings", {"type": {"$gt": "a"}}),
        ("a string constant on a number key", {"page": "x"}),
        ("a string constant on a number key, in a list", {"page": {"$in": [1, "x"]}}),
        ("a number constant on a string key", {"type": {"$ne": 3}}),
        ("a None constant", {"page": None}),
        ("a None constant under an operator", {"score": {"$ne": None}}),
        ("an int constant beyond 2**53", {"page": {"$lt": 2 ** 60}}),
        ("a NaN constant", {"score": {"$gt": float("nan")}}),
        ("$in of 65", {"page": {"$in": list(range(65))}}),
        ("$in of none", {"page": {"$in": []}}),
        ("equality with a list", {"page": [1, 2]}),
        ("33 instructions", {"$and": [{"page": {"$ne": p}} for p in range(1, 18)]}),
    ]
