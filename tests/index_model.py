"""A NumPy model of one collection (VectorIndex) across its whole lifecycle.  TEST INFRASTRUCTURE ONLY.

`IndexModel` keeps, per stored row in insertion order, everything the index keeps beside its matrix -- id, float64
vector, document, metadata, add time, token rows, sparse vector, named prior values, a live flag -- and mirrors the
index's bookkeeping: an existing id is ignored by `add`, a duplicate id inside a batch keeps its first entry, a deleted
id that is added again becomes a NEW row at the end, a delete is a tombstone until `compact` (also reached lazily from
`delete`, by the index's own rule), compaction is stable, `reset` drops everything derived.  Group ordinals are numbered
as `enable_grouping` numbers them (first appearance over the rows in use when the key is enabled, dead rows included,
then over the appended rows; kept by a compaction, dropped by a reset), because two modes break ties by ordinal.

Every mode is answered by that mode's existing reference (tests/*_ref.py, oracle/search_oracle.py) over the model's
rows with the model's live flags.  Row numbers of the model equal the index's as long as the index is right; the tests
compare IDS (`ids_of`), so "ties go to the lower row" reads "ties go to the earlier insert" across compactions.

Exact data.  `exact_rows` draws unit rows of dim 64 of three kinds -- 4 non-zeros of +-1/2, 16 of +-1/4, 64 of +-1/8.
Every entry is a power of two: exact in fp16, bf16 and fp32, exact as the E4M3 code of x * 256 (128, 64, 32), and the
bf16 split of the fp32 path has a zero low half.  Every dot product is a multiple of 2^-6 of magnitude at most 1, so a
float32 sum of them is exact in any order, and every comparison in tests/test_index_lifecycle_gpu.py except BM25's and
reciprocal-rank fusion's can be bit for bit.  Priors are multiples of 1/8 (times lie whole half-lives before NOW),
weights and lambda are powers of two, set sizes are powers of two."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from multimodal_rag_amd.index import match_where
from oracle import search_oracle as O
from tests import (bm25_ref, boost_ref, cluster_ref, dedup_ref, filter_ref, fuse_ref, group_ref, late_f8_ref,
                   late_store_ref, mmr_ref, range_ref, recommend_ref, related_ref, scoped_ref, sparse_ref)

DIM = 64
TOKEN_DIM = 64
N_TERMS = 512                      # the sparse vocabulary
NOW = 1_700_000_000.0              # the `now` of the BoostSpec; add times lie 0..3 hours before it
HOUR = 3600.0
WORDS = ["học", "máy", "dữ", "liệu", "gpu", "kernel", "bảng", "ảnh", "văn", "bản", "mô", "hình", "vector", "index",
         "tìm", "kiếm", "tài", "lược", "đồ", "thị", "sparse", "dense", "token", "row"]
TAGS = ["a", "b", "c", "d"]


# ------------------------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------------------------
def exact_rows(g: np.random.Generator, m: int, d: int = DIM) -> np.ndarray:
    """m unit rows (float64) of the three exact kinds, mixed"""
    out = np.zeros((m, d), np.float64)
    for i, kind in enumerate(g.integers(0, 3, m).tolist()):
        nz, mag = ((4, 0.5), (16, 0.25), (64, 0.125))[kind]
        cols = g.choice(d, nz, replace=False)
        out[i, cols] = mag * g.choice(np.array([-1.0, 1.0]), nz)
    return out


def row_fields(c: int) -> Dict[str, Any]:
    """metadata and add time of the c-th row ever generated: six rows per doc_id; `sec` (the second group key) is
    missing on every 7th row; `n` numeric, `tag` a string; the time a whole number of hours before NOW, unknown (NaN)
    on every 11th row"""
    meta: Dict[str, Any] = {"doc_id": f"d{c // 6}", "n": c % 10, "tag": TAGS[(c // 3) % 4]}
    if c % 7:
        meta["sec"] = f"s{c % 5}"
    return {"meta": meta, "time": float("nan") if c % 11 == 0 else NOW - HOUR * (c % 4)}


class Generator:
    """Seeded source of rows, queries, token rows and sparse vectors.  Every 5th row repeats the vector, token rows and
    sparse vector of the row generated 9 before it, so exact duplicates lie on both sides of every batch and delete
    boundary of the lifecycle script."""

    def __init__(self, seed: int):
        self.g = np.random.default_rng(seed)
        self.c = 0
        self.history: List[Dict[str, Any]] = []

    def text(self) -> str:
        return " ".join(self.g.choice(WORDS, int(self.g.integers(2, 10))).tolist())

    def tokens(self) -> np.ndarray:
        """1..40 token rows; every 6th item has none"""
        L = int(self.g.integers(1, 41))
        rows = exact_rows(self.g, L, TOKEN_DIM)
        return rows[:0] if self.c % 6 == 5 else rows

    def sparse(self):
        """0..6 of 48 active terms (ascending, distinct) spread over the vocabulary, impacts 1..255"""
        m = int(self.g.integers(0, 7))
        terms = np.sort(self.g.choice(48, m, replace=False) * 10 + 3).astype(np.int32)
        return terms, self.g.integers(1, 256, m).astype(np.int32)

    def sparse_queries(self, B: int):
        """(off, terms, impacts) of B sparse queries of 1..8 active terms"""
        off, terms, imps = [0], [], []
        for _ in range(B):
            m = int(self.g.integers(1, 9))
            terms.append(np.sort(self.g.choice(48, m, replace=False) * 10 + 3))
            imps.append(self.g.integers(1, 256, m))
            off.append(off[-1] + m)
        return np.asarray(off, np.int64), np.concatenate(terms).astype(np.int32), np.concatenate(imps).astype(np.int32)

    def rows(self, m: int, ids: Optional[Sequence[str]] = None) -> List[Dict[str, Any]]:
        """m new rows as dicts (id, vec, doc, meta, time, tok, sp_terms, sp_imps); `ids` overrides the fresh ids"""
        out = []
        vecs = exact_rows(self.g, m)
        for i in range(m):
            c = self.c
            row = {"id": f"r{c}" if ids is None else ids[i], "vec": vecs[i], "doc": self.text(), **row_fields(c)}
            row["tok"] = self.tokens()
            row["sp_terms"], row["sp_imps"] = self.sparse()
            if c % 5 == 0 and len(self.history) >= 9:
                twin = self.history[-9]
                row.update(vec=twin["vec"].copy(), tok=twin["tok"].copy(), sp_terms=twin["sp_terms"].copy(),
                           sp_imps=twin["sp_imps"].copy())
            self.history.append(row)
            self.c += 1
            out.append(row)
        return out

    def queries(self, B: int, stored: Sequence[np.ndarray] = ()) -> np.ndarray:
        """B float32 query rows: the first is a stored vector when one is given (a score of exactly 1 and its ties)"""
        q = exact_rows(self.g, B)
        for i, v in enumerate(list(stored)[:1]):
            q[i] = v
        return q.astype(np.float32)


def batch_arrays(rows: Sequence[Dict[str, Any]]):
    """what VectorIndex.add takes for these rows: (vectors f32, documents, metadatas, ids, times, sparse triple)"""
    vecs = np.stack([r["vec"] for r in rows]).astype(np.float32) if rows else np.zeros((0, DIM), np.float32)
    off = np.concatenate([[0], np.cumsum([r["sp_terms"].size for r in rows])]).astype(np.int64)
    terms = np.concatenate([r["sp_terms"] for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    imps = np.concatenate([r["sp_imps"] for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    return (vecs, [r["doc"] for r in rows], [dict(r["meta"]) for r in rows], [r["id"] for r in rows],
            np.array([r["time"] for r in rows], np.float64), (off, terms, imps))


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
class IndexModel:
    COMPACT_DEAD_FRACTION = 0.25

    def __init__(self, compact_min_dead: int = 4096):
        self.compact_min_dead = int(compact_min_dead)
        self.rows: List[Dict[str, Any]] = []          # the rows in use, dead ones included until a compaction
        self.groups: Dict[str, List[Any]] = {}        # enabled key -> values by ordinal
        self.prior_names: List[str] = []

    # ---------------------------------------------------------------- bookkeeping
    @property
    def n(self) -> int:
        return len(self.rows)

    def count(self) -> int:
        return sum(r["live"] for r in self.rows)

    def alive(self) -> np.ndarray:
        return np.array([r["live"] for r in self.rows], bool)

    def live_ids(self) -> List[str]:
        return [r["id"] for r in self.rows if r["live"]]

    def row_of(self, id_: str) -> int:
        for i, r in enumerate(self.rows):
            if r["live"] and r["id"] == id_:
                return i
        return -1

    def ids_of(self, rows) -> List[Optional[str]]:
        return [self.rows[int(r)]["id"] if int(r) >= 0 else None for r in np.asarray(rows).reshape(-1)]

    def add(self, batch: Sequence[Dict[str, Any]]) -> List[int]:
        """append the rows of `batch` the index would keep; returns their positions in the batch"""
        have = {r["id"] for r in self.rows if r["live"]}
        kept = []
        for i, row in enumerate(batch):
            if row["id"] in have:
                continue
            have.add(row["id"])
            kept.append(i)
            new = dict(row, live=True, meta=dict(row["meta"]), priors={name: np.float32(0.0) for name in self.prior_names})
            self.rows.append(new)
            for key, values in self.groups.items():
                self._ordinal(values, new["meta"].get(key), grow=True)
        return kept

    def delete(self, ids: Optional[Sequence[str]] = None, where: Optional[Dict[str, Any]] = None) -> List[str]:
        if ids is not None:
            want = set(ids)
            hit = [r for r in self.rows if r["live"] and r["id"] in want and match_where(r["meta"], where)]
        else:
            hit = [r for r in self.rows if r["live"] and match_where(r["meta"], where)]
        for r in hit:
            r["live"] = False
        dead = self.n - self.count()
        if hit and dead >= self.compact_min_dead and dead > self.COMPACT_DEAD_FRACTION * self.n:
            self.compact()
        return sorted(r["id"] for r in hit)

    def compact(self):
        self.rows = [r for r in self.rows if r["live"]]

    def reset(self):
        self.rows, self.groups, self.prior_names = [], {}, []

    # ---------------------------------------------------------------- derived state, as the index keeps it
    @staticmethod
    def _ordinal(values: List[Any], v, grow: bool) -> int:
        if v is None:
            return -1
        if v in values:
            return values.index(v)
        if not grow:
            return -1
        values.append(v)
        return len(values) - 1

    def enable_grouping(self, key: str):
        if key not in self.groups:
            values: List[Any] = []
            for r in self.rows:
                self._ordinal(values, r["meta"].get(key), grow=True)
            self.groups[key] = values
        return self.groups[key]

    def group_column(self, key: str) -> np.ndarray:
        values = self.enable_grouping(key)
        return np.array([self._ordinal(values, r["meta"].get(key), grow=False) for r in self.rows], np.int32)

    def group_counts(self, key: str) -> List[int]:
        """rows stored per ordinal over the LIVE rows: what the index's counts equal after a compaction"""
        col = self.group_column(key)[self.alive()]
        return np.bincount(col[col >= 0], minlength=len(self.groups[key])).tolist()

    def set_prior(self, name: str, values: Sequence[float]):
        """one value per live row in row order; rows added later get 0.0"""
        live = [r for r in self.rows if r["live"]]
        assert len(values) == len(live)
        if name not in self.prior_names:
            self.prior_names.append(name)
        for r in self.rows:
            r["priors"][name] = np.float32(0.0)
        for r, v in zip(live, values):
            r["priors"][name] = np.float32(v)

    def prior_column(self, prior) -> np.ndarray:
        """float32 [n]: a named column, or a (recency, half_life_s, values, now) spec computed from times and metadata"""
        if isinstance(prior, str):
            return np.array([r["priors"][prior] for r in self.rows], np.float32)
        recency, half_life, tables, now = prior
        out = np.zeros(self.n, np.float64)
        for i, r in enumerate(self.rows):
            if not np.isnan(r["time"]):
                out[i] += recency * 2.0 ** (-max(0.0, now - r["time"]) / half_life)
            for key, table in tables.items():
                out[i] += table.get(r["meta"].get(key), 0.0)
        return out.astype(np.float32)

    def matrix(self) -> np.ndarray:
        return np.stack([r["vec"] for r in self.rows]).astype(np.float32) if self.rows else np.zeros((0, DIM), np.float32)

    def metas(self) -> List[Dict[str, Any]]:
        return [r["meta"] for r in self.rows]

    def times(self) -> np.ndarray:
        return np.array([r["time"] for r in self.rows], np.float64)

    def row_times(self) -> np.ndarray:
        return self.times()[self.alive()] if self.rows else np.zeros(0)

    def visible(self, where) -> np.ndarray:
        """bool [n]: live rows that match `where` ("$added_at" = the row's add time)"""
        if not self.rows:
            return np.zeros(0, bool)
        return filter_ref.visible(self.metas(), where, self.alive(), self.times())

    def token_plane(self):
        """(token rows [T, dim] float64 in row order, item_off int64 [n + 1])"""
        toks = [r["tok"] for r in self.rows]
        off = np.concatenate([[0], np.cumsum([t.shape[0] for t in toks])]).astype(np.int64)
        plane = np.concatenate(toks + [np.zeros((0, TOKEN_DIM))]) if toks else np.zeros((0, TOKEN_DIM))
        return plane, off

    def sparse_log(self):
        return batch_arrays(self.rows)[5]

    # ---------------------------------------------------------------- the modes
    def get(self, ids=None, where=None) -> Dict[str, Any]:
        if ids is not None:
            rows = [self.row_of(i) for i in ids]
            rows = [r for r in rows if r >= 0 and match_where(self.rows[r]["meta"], where)]
        else:
            rows = [i for i, r in enumerate(self.rows) if r["live"] and match_where(r["meta"], where)]
        return {"ids": [self.rows[r]["id"] for r in rows], "documents": [self.rows[r]["doc"] for r in rows],
                "metadatas": [self.rows[r]["meta"] for r in rows],
                "embeddings": [self.rows[r]["vec"].tolist() for r in rows]}

    def search(self, q, k: int, where=None):
        """(scores [B, k] float32, rows [B, k]): regime_ref.expected's oracle over the visible rows"""
        q = np.asarray(q, np.float32)
        if not self.rows:
            return np.full((len(q), k), -np.inf, np.float32), np.full((len(q), k), -1, np.int64)
        return O.cosine_topk(q, self.matrix(), k, alive=self.visible(where))

    def mmr(self, q, k: int, fetch_k: int, lam: float, where=None):
        s, r = self.search(q, fetch_k, where)
        X = self.matrix()
        outs = [mmr_ref.select_padded(s[b], r[b], X, k, lam) for b in range(len(s))]
        return tuple(np.stack(col) for col in zip(*outs))

    def grouped(self, q, G: int, S: int, key: str, fetch_k=None, where=None, base: int = 64):
        """per query (depth, the five blocks of group_ref.select_padded)"""
        col = self.group_column(key)
        s, r = self.search(q, max(self.count(), 1), where)
        out = []
        for b in range(len(s)):
            live = r[b] >= 0
            out.append(group_ref.ladder(s[b][live], r[b][live], col, self.n, G, S, base=base, fetch_k=fetch_k))
        return out

    def scoped(self, q, k: int, scopes: Sequence[Sequence[Any]], key: str, where=None):
        values = self.enable_grouping(key)
        sets = [sorted({values.index(v) for v in scope if v in values}) for scope in scopes]
        if not self.rows:
            return np.full((len(q), k), -np.inf, np.float32), np.full((len(q), k), -1, np.int64)
        return scoped_ref.scoped_topk(np.asarray(q, np.float32), self.matrix(), k, self.group_column(key),
                                      list(range(len(sets))), sets, alive=self.visible(where))

    def filtered(self, q, k: int, wheres: Sequence[Any]):
        q = np.asarray(q, np.float32)
        if not self.rows:
            return np.full((len(q), k), -np.inf, np.float32), np.full((len(q), k), -1, np.int64)
        return filter_ref.topk_of_visible(q, self.matrix(), k, [self.visible(w) for w in wheres])

    def range(self, q, thr, limit: int, wheres: Sequence[Any], facets: Sequence[str]):
        q = np.asarray(q, np.float32)
        codes = [self.group_column(key) for key in facets]
        sizes = [len(self.groups[key]) for key in facets]
        vis = np.stack([self.visible(w) for w in wheres]) if self.rows else np.zeros((len(q), 0), bool)
        return range_ref.range_ref(q, self.matrix(), thr, limit, vis, codes, sizes)

    def related(self, sets: Sequence[Any], k: int, key: str, threshold: float, where=None):
        """sets: arrays of vectors, or {"value": v} = the live rows of that document (which it then excludes)"""
        values = self.enable_grouping(key)
        col = self.group_column(key)
        X = self.matrix().astype(np.float64)
        parts, off, excl = [], [0], []
        for entry in sets:
            if isinstance(entry, dict):
                rows = [i for i, r in enumerate(self.rows) if r["live"] and r["meta"].get(key) == entry["value"]]
                parts.append(X[rows])
                excl.append(values.index(entry["value"]))
            else:
                parts.append(np.asarray(entry, np.float64))
                excl.append(-1)
            off.append(off[-1] + len(parts[-1]))
        out, _ = related_ref.related_groups(np.concatenate(parts), off, X, col, len(values), k, threshold,
                                            exclude=excl, alive=self.visible(where))
        return out

    def power_of_two_documents(self, key: str = "doc_id") -> List[Any]:
        """values of `key` whose live rows number 1, 2, 4 or 8 (a mean over them is exact), in ordinal order"""
        counts = self.group_counts(key)
        return [v for v, c in zip(self.groups[key], counts) if c in (1, 2, 4, 8)]

    def boosted(self, q, k: int, prior, weight, where=None):
        q = np.asarray(q, np.float32)
        return boost_ref.boosted_topk(q, self.matrix(), k, self.prior_column(prior), weight, alive=self.visible(where)
                                      if self.rows else None)

    def recommend(self, positive, negative, k: int, weight, where=None):
        """entries: vectors, or ids of live rows"""
        vec = lambda e: self.rows[self.row_of(e)]["vec"] if isinstance(e, str) else np.asarray(e)   # noqa: E731
        pos = [[vec(e) for e in p] for p in positive]
        neg = [[vec(e) for e in n_] for n_ in negative]
        ex, sign = recommend_ref.pack(pos, neg, DIM)
        return recommend_ref.recommend_topk(ex, sign, weight, self.matrix(), k,
                                            alive=self.visible(where) if self.rows else None)

    def fused(self, q, list_off, n: int, depth: int, weights=None, method="rrf", rrf_k: int = 60, where=None):
        s, r = self.search(q, depth, where)
        return fuse_ref.fuse_select(s, r, list_off, n, None if weights is None else np.asarray(weights, np.float32),
                                    method, rrf_k)

    def late(self, q_tok, q_start, q_len, k: int, where=None, f8: bool = False):
        plane, off = self.token_plane()
        alive = self.visible(where) if self.rows else None
        if f8:
            s, r = late_f8_ref.topk(late_f8_ref.encode_rows(q_tok), q_start, q_len, late_f8_ref.encode_rows(plane), off,
                                    k, alive)
        else:
            s, r = late_store_ref.topk(q_tok, q_start, q_len, plane, off, k, alive)
        return s.astype(np.float32), r

    def lexical(self, text: str):
        """(float64 scores [n], matched [n]) of BM25 over the live rows' documents"""
        ref = bm25_ref.RefIndex.from_texts([r["doc"] for r in self.rows])
        return ref.scores(ref.query_ids(text), self.alive())

    def lexical_rows(self, text: str, k: int, where=None) -> np.ndarray:
        acc, matched = self.lexical(text)
        return bm25_ref.topk(acc, matched, self.visible(where), k)

    def sparse(self, queries, k: int, where=None):
        """queries = (off, terms, impacts); (scores [B, k] float32, rows [B, k])"""
        off, terms, imps = self.sparse_log()
        q_off, q_terms, q_imps = queries
        allowed = self.visible(where) if self.rows else None
        out = []
        for b in range(len(q_off) - 1):
            lo, hi = int(q_off[b]), int(q_off[b + 1])
            out.append(sparse_ref.topk(sparse_ref.scores(off, terms, imps, N_TERMS, q_terms[lo:hi], q_imps[lo:hi]), k,
                                       allowed))
        return np.stack([s for s, _ in out]), np.stack([r for _, r in out])

    def near_duplicates(self, t: float, where=None):
        """({(row_a, row_b): cosine} in row order, the components as row lists in keeper order)"""
        found = dedup_ref.pairs(self.matrix().astype(np.float64), self.visible(where), t) if self.n > 1 else {}
        return found, dedup_ref.components(sorted(found))

    def assign(self, seed_ids: Sequence[str], where=None):
        """cluster_ref.assign of every row against the rows of `seed_ids` as centroids: (label, score) per row"""
        X = self.matrix().astype(np.float64)
        cent = np.stack([X[self.row_of(i)] for i in seed_ids])
        arg, best, _ = cluster_ref.assign(X, cent, self.visible(where))
        return arg, best
