"""Device-resident vector collection: what `chromadb`'s collection is to the reference.

Replaces the engine calls made by app/utils/embedder.py:
    collection.add(embeddings, documents, metadatas, ids)          :518
    collection.query(query_embeddings, n_results, where, include)  :596-601, :900-905
    collection.get(where|ids, include)                             :632-635, :887-891
    collection.delete(ids)                                         :639-642
    collection.count()                                             :700
The vectors live in one [capacity, ld] matrix in HBM (fp16 by default, rows padded to the
kernel's 128-byte slabs); ids / documents / metadata stay in host tables indexed by row, as
SURVEY.md section 8b "Ownership" lays out.  Search is exact (fused MFMA GEMM + top-k in
libmmrag.so), distance = 1 - cos (the committed collection's hnsw:space=cosine).

No arithmetic over the stored rows happens in this file: torch provides device buffers and copies, and in cluster() the
sort of the labels and the [k, d] centroid update between the two kernels of csrc/kmeans.hip.
"""
from __future__ import annotations

import gc
import logging
import operator
import threading
import time
from collections import OrderedDict
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .boost import BoostSpec, check_prior_values
from .filters import ColumnRegistry, names_added_at, pack_programs, try_compile
from .hostutil import load_hostrows
from .tracing import stage

_HOSTROWS = load_hostrows()

logger = logging.getLogger(__name__)


# --------------------------------------------------------------------------------------------
# `where` filters (the subset of Chroma's grammar that is expressible on flat metadata)
# --------------------------------------------------------------------------------------------
_CMP: Dict[str, Callable[[Any, Any], bool]] = {
    "$eq": lambda a, b: a == b,
    "$ne": lambda a, b: a != b,
    "$gt": lambda a, b: a is not None and a > b,
    "$gte": lambda a, b: a is not None and a >= b,
    "$lt": lambda a, b: a is not None and a < b,
    "$lte": lambda a, b: a is not None and a <= b,
    "$in": lambda a, b: a in b,
    "$nin": lambda a, b: a not in b,
}


def match_where(meta: Dict[str, Any], where: Optional[Dict[str, Any]]) -> bool:
    if not where:
        return True
    for key, cond in where.items():
        if key == "$and":
            if not all(match_where(meta, w) for w in cond):
                return False
        elif key == "$or":
            if not any(match_where(meta, w) for w in cond):
                return False
        elif isinstance(cond, dict):
            for op, val in cond.items():
                if op not in _CMP:
                    raise ValueError(f"unsupported where operator {op!r}")
                if not _CMP[op](meta.get(key), val):
                    return False
        else:
            if meta.get(key) != cond:
                return False
    return True


class MetaIndex:
    """Inverted index over the rows' metadata: (key, value) -> ascending row list.  Answers the `where`
    forms the service actually sends -- equality, `$eq`, `$in`, `$and`, `$or` over hashable scalars -- in time
    proportional to the matches instead of one Python predicate call per stored row (a filtered query or a
    `delete_document` on a 1M-row shard was a second of host time); anything else returns None and the caller
    falls back to the full scan.  Rows are only ever appended; after a compaction the owner rebuilds it."""

    def __init__(self):
        self.n = 0
        self._kv: Dict[Any, Dict[Any, List[int]]] = {}

    def append(self, metadatas: Sequence[Dict[str, Any]]):
        for meta in metadatas:
            for k, v in meta.items():
                try:
                    self._kv.setdefault(k, {}).setdefault(v, []).append(self.n)
                except TypeError:        # unhashable value: only the full scan can match it
                    self._kv.setdefault(k, {}).setdefault(_UNHASHABLE, []).append(self.n)
            self.n += 1

    def _eq(self, key, val) -> Optional[np.ndarray]:
        by_val = self._kv.get(key)
        if by_val is None:
            return np.zeros(0, np.int64) if val is not None else None   # meta.get(key) is None for every row
        if _UNHASHABLE in by_val or val is None:
            return None
        try:
            return np.asarray(by_val.get(val, ()), dtype=np.int64)
        except TypeError:
            return None

    def rows(self, where: Optional[Dict[str, Any]]) -> Optional[np.ndarray]:
        """Ascending rows matching `where`, or None when the form is not covered."""
        if not where:
            return np.arange(self.n, dtype=np.int64)
        acc: Optional[np.ndarray] = None
        for key, cond in where.items():
            if key == "$and":
                parts = [self.rows(w) for w in cond]
                if any(p is None for p in parts):
                    return None
                cur = np.arange(self.n, dtype=np.int64)
                for p in parts:
                    cur = np.intersect1d(cur, p, assume_unique=True)
            elif key == "$or":
                parts = [self.rows(w) for w in cond]
                if any(p is None for p in parts):
                    return None
                cur = np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.int64)
            elif isinstance(cond, dict):
                cur = np.arange(self.n, dtype=np.int64)
                for op, val in cond.items():
                    if op == "$eq":
                        part = self._eq(key, val)
                    elif op == "$in" and isinstance(val, (list, tuple, set)):
                        sub = [self._eq(key, v) for v in val]
                        part = None if any(x is None for x in sub) else (
                            np.unique(np.concatenate(sub)) if sub else np.zeros(0, np.int64))
                    else:
                        return None
                    if part is None:
                        return None
                    cur = np.intersect1d(cur, part, assume_unique=True)
            else:
                cur = self._eq(key, cond)
                if cur is None:
                    return None
            acc = cur if acc is None else np.intersect1d(acc, cur, assume_unique=True)
        return acc


_UNHASHABLE = object()


def _cat_pairs(parts, dim: int):
    """(scores, rows) pairs of partial searches joined along `dim`; a single pair is returned as it is"""
    if len(parts) == 1:
        return parts[0]
    return torch.cat([p[0] for p in parts], dim), torch.cat([p[1] for p in parts], dim)


class DuplicateReportTruncated(ValueError):
    """drop_duplicates refused: the near-duplicate report holds fewer pairs than exist, so its groups are wrong"""


class VectorIndex:
    """One shard of the corpus matrix on one GPU plus its host-side row tables.

    Rows are appended in insertion order and never move while they are alive, so "lower row" always means
    "earlier insert" (the tie rule).  A delete is a TOMBSTONE: the row's bit is cleared in a device-resident alive
    bitmap that the search kernels consume (masked rows start at -inf, csrc/search*.hip), its id leaves the id map,
    and nothing else is touched -- `delete_document` on a 1M-row shard is O(victims) on the host and one small
    scatter on the device.  The matrix is compacted (stably) only when more than COMPACT_DEAD_FRACTION of the rows
    are dead, or on `compact()` / save.

    Vectors must be unit-norm (cosine = inner product of unit vectors; `distance = 1 - cos`).  The encoders of this
    package normalise; `add` / `query` reject rows whose norm is off by more than 1e-2 instead of silently ranking
    by raw inner product (Chroma's cosine space would have normalised them).

    FP8 collections (`dtype=torch.float8_e4m3fn`, include/mmrag.h MMRAG_F8E4M3): the matrix holds one-byte E4M3 codes
    (a float8_e4m3fn tensor; torch only allocates, copies and zeroes it, through its uint8 view) and is the SCAN plane (csrc/search_f8.hip).  FP8 alone does not rank well enough, so with
    a `rescore_dtype` (default float16; config MMRAG_F8_RESCORE) the index keeps a full-precision plane of the same
    rows next to it -- appended, tombstoned and compacted together -- and a search over-fetches
    C = min(max(20, MMRAG_F8_OVERSAMPLE * k), 4096) candidates from the scan plane and re-scores them exactly on that
    plane (csrc/rescore.hip), so scores and `distances` read like an fp16 collection's.  That mode costs 1.5x the
    memory of an fp16 collection: it buys scan time, not capacity.  `rescore_dtype=None` is the capacity mode (0.5x):
    searches return the quantised collection's own scores, and mmr / hybrid queries are refused."""

    COMPACT_DEAD_FRACTION = 0.25
    COMPACT_MIN_DEAD = 4096

    def __init__(self, dim: int, dtype: torch.dtype = torch.float16, device: str = "cuda:0",
                 capacity: int = 4096, name: str = "multimodal_rag",
                 metadata: Optional[Dict[str, Any]] = None, rescore_dtype: Any = "default"):
        if dtype not in (torch.float16, torch.float32, torch.bfloat16, torch.float8_e4m3fn):
            raise ValueError(f"unsupported storage dtype {dtype}")
        from .config import settings

        self.is_f8 = dtype == torch.float8_e4m3fn
        if not self.is_f8:
            if rescore_dtype not in ("default", None):
                raise ValueError("rescore_dtype applies to float8_e4m3fn collections only")
            rescore_dtype = None
        elif isinstance(rescore_dtype, str) and rescore_dtype == "default":
            rescore_dtype = settings.f8_rescore_dtype()
        if rescore_dtype not in (None, torch.float16, torch.float32, torch.bfloat16):
            raise ValueError(f"unsupported rescore dtype {rescore_dtype}")
        self.rescore_dtype: Optional[torch.dtype] = rescore_dtype
        _native.lib()  # fail loudly if the HIP library is absent
        self.name = name
        self.metadata = dict(metadata or {})
        self.dim = int(dim)
        self.dtype = dtype
        self.device = torch.device(device)
        self.ld = _native.padded_dim(self.dim, dtype)
        cap = max(int(capacity), 256)
        self._matrix = self._new_rows(cap, zero=True)
        self.plane_ld = _native.padded_dim(self.dim, rescore_dtype) if rescore_dtype is not None else 0
        self._plane: Optional[torch.Tensor] = None     # FP8 collections: full-precision rows for the exact re-scoring
        if rescore_dtype is not None:
            self._plane = torch.zeros((cap, self.plane_ld), dtype=rescore_dtype, device=self.device)
        self._alive_dev = torch.zeros(self._n_words(cap), dtype=torch.int32, device=self.device)
        self._alive_host = np.zeros(self._n_words(cap), dtype=np.uint32)
        self._n = 0            # rows in use (alive + dead)
        self._n_dead = 0
        self._ids: List[Optional[str]] = []
        self._documents: List[Optional[str]] = []
        self._metadatas: List[Dict[str, Any]] = []
        self._meta_index = MetaIndex()
        self._row_of: Dict[str, int] = {}
        self._lock = threading.RLock()
        self._search_ws: Optional[torch.Tensor] = None    # candidate-list workspace of the search kernels, reused
        self._deep_ws: Optional[torch.Tensor] = None      # workspace of the deep search (n_results > 20), reused
        self._scoped_ws: Optional[torch.Tensor] = None    # workspace of the scoped search, reused
        self._lex = None   # lexical.LexicalIndex once enable_lexical() ran (lazily: first lexical / hybrid query)
        self._sparse = None          # sparse.ImpactIndex once enable_sparse() ran (opt-in: learned sparse vectors)
        self._pending_sparse = None  # the vectors of the rows add() is appending, consumed by _appended()
        self._groups: Dict[str, Dict[str, Any]] = {}   # metadata key -> group column state once enable_grouping(key) ran
        self._boosted_ws: Optional[torch.Tensor] = None   # workspace of the boosted search, reused
        self._recommend_ws: Optional[torch.Tensor] = None   # workspace of the recommend search, reused
        self._added_at = np.full(cap, np.nan, dtype=np.float64)   # when each row in use was added (NaN = unknown)
        self._priors: Dict[str, Any] = {}     # set_prior names -> a device float32 [capacity] column, or a BoostSpec
        # spec columns by (canonical JSON of the spec, floored now) -> {"spec", "now", "col"}; at most MAX_SPEC_COLUMNS
        self._spec_cols: "OrderedDict[Tuple[str, float], Dict[str, Any]]" = OrderedDict()
        self.f32_exact = bool(settings.MMRAG_F32_EXACT_SEARCH)   # float32 collections only (see config.py)
        # typed metadata columns of the device filters (filters.py): built per key on first use, derived, not persisted
        self._filter_cols = ColumnRegistry(lambda: (self._metadatas, self._n, self._added_at))
        self._filtered_ws: Optional[torch.Tensor] = None   # workspace of the filtered search, reused
        self._range_ws: Optional[torch.Tensor] = None      # workspace of the range search, reused
        self.device_filters = bool(settings.MMRAG_DEVICE_FILTERS)   # _where_bits builds its bitmap on the device
        self._tokens = None    # late_store.TokenStore once enable_token_store() ran: token rows of the items, item = row
        self._late_ws: Optional[torch.Tensor] = None      # workspace of the late search, reused

    def _new_rows(self, rows: int, zero: bool) -> torch.Tensor:
        """[rows, ld] in the storage dtype; FP8 codes are allocated as bytes and viewed as float8_e4m3fn"""
        make = torch.zeros if zero else torch.empty
        if self.is_f8:
            return make((rows, self.ld), dtype=torch.uint8, device=self.device).view(torch.float8_e4m3fn)
        return make((rows, self.ld), dtype=self.dtype, device=self.device)

    def _raw(self, t: torch.Tensor) -> torch.Tensor:
        """the tensor torch's own copy / fill kernels see: the byte view of FP8 codes, anything else as it is"""
        return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t

    @staticmethod
    def _n_words(rows: int) -> int:
        return (rows + 31) // 32 + 8   # the kernels read whole words of the last tile

    # ------------------------------------------------------------------ storage ----------
    @property
    def matrix(self) -> torch.Tensor:
        return self._matrix

    @property
    def plane(self) -> Optional[torch.Tensor]:
        """FP8 collections: the full-precision re-scoring plane (None in capacity mode and for every other dtype)"""
        return self._plane

    @property
    def _full(self) -> torch.Tensor:
        """the most precise copy of the rows: what get(embeddings), MMR and the hybrid distances read"""
        return self._plane if self._plane is not None else self._matrix

    def bytes_per_row(self) -> int:
        b = self.ld * self._matrix.element_size()
        return b + (self.plane_ld * self._plane.element_size() if self._plane is not None else 0)

    def _need_plane(self, what: str):
        if self.is_f8 and self._plane is None:
            raise ValueError(f"{what} needs full-precision rows: this float8_e4m3fn collection was created with "
                             f"rescore_dtype=None (MMRAG_F8_RESCORE=none)")

    def count(self) -> int:
        return self._n - self._n_dead

    @property
    def rows_in_use(self) -> int:
        """rows of the matrix that hold a vector, dead ones included (what the kernels scan)"""
        return self._n

    def _reserve(self, rows: int):
        cap = self._matrix.shape[0]
        if rows <= cap:
            return
        new_cap = max(rows, cap * 2)
        self._matrix = self._regrown(self._matrix, new_cap, 0)
        if self._plane is not None:
            self._plane = self._regrown(self._plane, new_cap, 0)
        words = torch.zeros(self._n_words(new_cap), dtype=torch.int32, device=self.device)
        words[: self._alive_dev.numel()].copy_(self._alive_dev)
        self._alive_dev = words
        host = np.zeros(self._n_words(new_cap), dtype=np.uint32)
        host[: self._alive_host.size] = self._alive_host
        self._alive_host = host
        for st in self._groups.values():
            st["col"] = self._regrown(st["col"], new_cap, -1)
        times = np.full(new_cap, np.nan, dtype=np.float64)
        times[: self._n] = self._added_at[: self._n]
        self._added_at = times
        self._map_prior_columns(lambda col: self._regrown(col, new_cap, 0))

    def _regrown(self, t: torch.Tensor, cap: int, fill: int) -> torch.Tensor:
        """a per-row device tensor (matrix, plane, group column) at capacity `cap`: rows in use copied, tail filled"""
        raw = self._raw(t)
        new = torch.empty((cap,) + raw.shape[1:], dtype=raw.dtype, device=raw.device)
        new[: self._n].copy_(raw[: self._n])
        new[self._n:].fill_(fill)
        return new if raw is t else new.view(t.dtype)

    def _compacted(self, t: torch.Tensor, cap: int, keep_dev: torch.Tensor, fill: int) -> torch.Tensor:
        """a per-row device tensor at capacity `cap` holding the rows `keep_dev` of `t` in order, the tail filled; rows
        of vectors move with the gather kernel, a column (a scalar per row, below its 16-byte granule) by index copy"""
        raw = self._raw(t)
        new = torch.full((cap,) + raw.shape[1:], fill, dtype=raw.dtype, device=raw.device)
        new = new if raw is t else new.view(t.dtype)
        if keep_dev.numel() and t.dim() == 2:
            _native.gather_rows(new, t, keep_dev)
        elif keep_dev.numel():
            new[: keep_dev.numel()] = t[keep_dev]
        return new

    def _set_alive(self, lo: int, hi: int):
        """mark rows [lo, hi) alive (appends): touch only the words they fall in"""
        idx = np.arange(lo, hi, dtype=np.int64)
        np.bitwise_or.at(self._alive_host, idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
        w0, w1 = lo >> 5, ((hi - 1) >> 5) + 1
        self._alive_dev[w0:w1].copy_(torch.from_numpy(self._alive_host[w0:w1].view(np.int32)), non_blocking=False)

    def _clear_alive(self, rows: np.ndarray):
        np.bitwise_and.at(self._alive_host, rows >> 5, ~(np.uint32(1) << (rows & 31).astype(np.uint32)))
        touched = np.unique(rows >> 5)
        self._alive_dev[torch.from_numpy(touched).to(self.device)] = torch.from_numpy(
            self._alive_host[touched].view(np.int32)).to(self.device)

    @staticmethod
    def _bad_norm(what: str, i: int, nrm: float):
        return ValueError(f"{what}: row {i} has norm {nrm:.4f}; this collection is cosine (inner product of unit "
                          f"vectors) -- L2-normalise the vectors first")

    def _to_device_f32(self, x, what: str = "vectors", check_norm: bool = True) -> torch.Tensor:
        """[m, dim] float32 on the device; unit norm is checked where the data already is (host arrays on the host:
        a device-side check would put a synchronisation into every single-query call)"""
        if isinstance(x, torch.Tensor):
            t = x
            if t.dim() == 1:
                t = t.unsqueeze(0)
            if t.dim() == 2 and t.shape[0] and t.is_cuda and check_norm:
                nrm = torch.linalg.vector_norm(t.float(), dim=1)
                bad = (nrm - 1.0).abs() > 1e-2
                if bool(bad.any()):
                    i = int(torch.nonzero(bad)[0])
                    raise self._bad_norm(what, i, float(nrm[i]))
            elif t.dim() == 2 and t.shape[0] and not t.is_cuda:
                x = t.numpy()
        if not isinstance(x, torch.Tensor):
            a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
            if a.ndim == 1:
                a = a[None, :]
            if a.ndim == 2 and a.shape[0]:
                nrm = np.sqrt(np.einsum("ij,ij->i", a, a))
                bad = np.abs(nrm - 1.0) > 1e-2
                if bad.any():
                    i = int(np.argmax(bad))
                    raise self._bad_norm(what, i, float(nrm[i]))
            t = torch.from_numpy(a)
        if t.dim() != 2 or t.shape[1] != self.dim:
            raise ValueError(f"embedding dimension {tuple(t.shape)} does not match collection dimensionality {self.dim}")
        return t.to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()

    def _pack_queries(self, q, check_norm: bool = True) -> torch.Tensor:
        """float32 [B, d] -> storage dtype [B, ld] with zero pad columns (device-side cast kernel).  A float32 device
        tensor that _to_device_f32 already returned passes through it unchanged (give check_norm=False)."""
        qf = self._to_device_f32(q, "query", check_norm)
        if self.dtype == torch.float32 and self.ld == self.dim:
            return qf          # already the stored form: no cast pass (one launch less on the single-query path)
        packed = self._new_rows(qf.shape[0], zero=False)
        _native.append_rows(packed, 0, qf, self.dim)
        return packed

    def _pack_plane_queries(self, qf: torch.Tensor) -> torch.Tensor:
        """float32 [B, d] on the device -> the re-scoring plane's dtype and padded width"""
        packed = torch.empty((qf.shape[0], self.plane_ld), dtype=self.rescore_dtype, device=self.device)
        _native.append_rows(packed, 0, qf, self.dim)
        return packed

    # ------------------------------------------------------------------ collection API ----
    def add(self, embeddings, documents: Optional[Sequence[Optional[str]]] = None,
            metadatas: Optional[Sequence[Dict[str, Any]]] = None, ids: Optional[Sequence[str]] = None,
            dedup_threshold: Optional[float] = None, timestamps=None, sparse=None):
        """Append rows (collection.add).  `sparse`: the rows' learned sparse vectors (off, terms, impacts) as
        `DeviceSparseEncoder.expand_ids` returns them (needs enable_sparse(); without it the rows get empty vectors).  `timestamps`: when each row was added, a UNIX time or one per row (NaN =
        unknown; default: now) -- what a recency prior reads (set_prior), stored beside the rows and never in their
        metadata.  `dedup_threshold` (None: off, returns None): a cosine t in (0, 1]; a row whose
        best stored row scores >= t, or that pairs (>= t) with an earlier row of this batch that is itself kept, is
        skipped and never reaches the matrix, the row tables or the lexical / group columns.  Returns then
        {"added": [ids], "skipped": [(id, duplicate_of, cosine)]}."""
        if ids is None:
            raise ValueError("ids are required")
        if dedup_threshold is not None:
            dedup_threshold = self._join_threshold(dedup_threshold, "dedup_threshold")
            self._need_plane("add(dedup_threshold=...)")
        emb = self._to_device_f32(embeddings, "add")
        m = emb.shape[0]
        if len(ids) != m:
            raise ValueError(f"{len(ids)} ids for {m} embeddings")
        documents = list(documents) if documents is not None else [None] * m
        metadatas = [dict(x) if x else {} for x in metadatas] if metadatas is not None else [{} for _ in range(m)]
        if len(documents) != m or len(metadatas) != m:
            raise ValueError("documents / metadatas length mismatch")
        times = self._row_times(timestamps, m)
        if sparse is not None:
            from .sparse import check_sparse_rows

            if self._sparse is None:
                raise ValueError("add(sparse=...) needs enable_sparse(vocab_size) first")
            sparse = check_sparse_rows(*sparse, self._sparse.n_terms, m, _native.MAX_SPARSE_TERMS, "add(sparse=...)")
        with self._lock:
            fresh = [i for i, s in enumerate(ids) if s not in self._row_of]
            seen = set()
            keep = []
            for i in fresh:
                if ids[i] not in seen:
                    seen.add(ids[i])
                    keep.append(i)
            skipped: List[Tuple[str, str, float]] = []
            if len(keep) != m:
                logger.warning("Add of existing embedding ID ignored for %d of %d items", m - len(keep), m)
                if not keep:
                    return None if dedup_threshold is None else {"added": [], "skipped": []}
                emb = emb[torch.tensor(keep, device=self.device)].contiguous()
            if dedup_threshold is not None:
                kept, skipped = self._dedup_batch(emb, [ids[i] for i in keep], dedup_threshold)
                if len(kept) != len(keep):
                    if not kept:
                        return {"added": [], "skipped": skipped}
                    emb = emb[torch.tensor(kept, device=self.device)].contiguous()
                    keep = [keep[j] for j in kept]
            self._reserve(self._n + len(keep))
            _native.append_rows(self._matrix, self._n, emb, self.dim)
            if self._plane is not None:
                _native.append_rows(self._plane, self._n, emb, self.dim)
            for j, i in enumerate(keep):
                self._row_of[ids[i]] = self._n + j
                self._ids.append(ids[i])
                self._documents.append(documents[i])
                self._metadatas.append(metadatas[i])
            if sparse is not None:      # the vectors of the kept rows, in their order
                off, terms, imps = sparse
                lens = np.diff(off)[keep]
                src = np.repeat(off[keep], lens) + (np.arange(int(lens.sum()), dtype=np.int64)
                                                    - np.repeat(np.cumsum(lens) - lens, lens))
                self._pending_sparse = (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), terms[src], imps[src])
            self._appended(len(keep), times[keep])
            return None if dedup_threshold is None else {"added": [ids[i] for i in keep], "skipped": skipped}

    # ------------------------------------------------------------------ near-duplicates ----
    DEDUP_BATCH_PAIRS_PER_ROW = 4     # pair capacity of an ingest batch's first join; an overflow is joined once more
    DEDUP_BATCH_MIN_PAIRS = 1024

    @staticmethod
    def _join_threshold(t, what: str) -> float:
        t = float(t)
        if not 0.0 < t <= 1.0:      # false for NaN too
            raise ValueError(f"{what} must be a cosine in (0, 1] (got {t!r})")
        return t

    def _dedup_batch(self, emb: torch.Tensor, ids: Sequence[str], t: float):
        """which rows of the new batch `emb` [m, dim] (float32, device) to keep at threshold t (caller holds the lock):
        (positions kept, [(id, duplicate_of, cosine)] of the rest).  Greedy in input order, first wins: a row is
        skipped for a stored duplicate (the top-1 search: exact, tombstones honoured, FP8 re-scored), else for the
        lowest earlier row of the batch that pairs with it AND is kept (the join of the batch as it would be stored).
        A row whose only partners were skipped is kept -- unlike near_duplicates' components (a~b~c without a~c keeps
        a and c here)."""
        m = emb.shape[0]
        best_s = best_r = None
        if self.count() > 0:
            s_dev, r_dev = self._launch_search(emb, 1, None, check_norm=False)
            best_s, best_r = s_dev[:, 0].cpu().numpy(), r_dev[:, 0].cpu().numpy()
        packed = self._pack_plane_queries(emb) if self._plane is not None else self._pack_queries(emb, check_norm=False)
        cap = max(self.DEDUP_BATCH_PAIRS_PER_ROW * m, self.DEDUP_BATCH_MIN_PAIRS)
        pairs, scores, total = _native.sim_join(packed, m, self.dim, t, capacity=cap)
        if total > cap:
            if total > _native.MAX_JOIN_PAIRS:
                raise ValueError(f"add(dedup_threshold={t}): {total} duplicate pairs inside one batch exceed "
                                 f"{_native.MAX_JOIN_PAIRS}; add it in smaller batches")
            pairs, scores, total = _native.sim_join(packed, m, self.dim, t, capacity=total)   # the count is exact
        pairs_h, scores_h = pairs.cpu().numpy(), scores.cpu().numpy()
        partners: Dict[int, List[Tuple[int, float]]] = {}
        for (i, j), s in zip(pairs_h.tolist(), scores_h.tolist()):     # sorted by (i, j): ascending i per j
            partners.setdefault(j, []).append((i, s))
        alive = [False] * m
        kept: List[int] = []
        skipped: List[Tuple[str, str, float]] = []
        for j in range(m):
            if best_s is not None and best_r[j] >= 0 and best_s[j] >= t:
                skipped.append((ids[j], self._ids[int(best_r[j])], float(best_s[j])))
                continue
            first = next(((i, s) for i, s in partners.get(j, ()) if alive[i]), None)
            if first is not None:
                skipped.append((ids[j], ids[first[0]], float(first[1])))
                continue
            alive[j] = True
            kept.append(j)
        return kept, skipped

    def near_duplicates(self, threshold: Optional[float] = None, where: Optional[Dict[str, Any]] = None,
                        max_pairs: int = 1 << 20) -> Dict[str, Any]:
        """Every pair of live rows (matching `where`) whose cosine is >= threshold (default
        MMRAG_DEDUP_REPORT_THRESHOLD): the exact self-join of csrc/simjoin.hip over the full-precision rows (an FP8
        collection's re-scoring plane).  Returns {"threshold", "total_pairs" (exact), "truncated" (more than max_pairs),
        "pairs": [(id_a, id_b, cosine)] in (row_a, row_b) order with row_a < row_b, "groups": the connected components
        of the pair graph, each in row order (its first id, the earliest stored, is the keeper), in keeper order}."""
        from .config import settings

        t = self._join_threshold(settings.MMRAG_DEDUP_REPORT_THRESHOLD if threshold is None else threshold, "threshold")
        with self._lock:
            self._need_plane("near_duplicates")
            bits = self._where_bits(where)
            pairs, scores, total = _native.sim_join(self._full, self._n, self.dim, t, alive=bits, capacity=int(max_pairs))
            pairs_h, scores_h = pairs.cpu().numpy().tolist(), scores.cpu().numpy().tolist()
            parent: Dict[int, int] = {}

            def find(x: int) -> int:
                root = x
                while parent.setdefault(root, root) != root:
                    root = parent[root]
                while parent[x] != root:
                    parent[x], x = root, parent[x]
                return root

            for a, b in pairs_h:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)      # the root of a component is its lowest row: the keeper
            members: Dict[int, List[int]] = {}
            for row in sorted(parent):
                members.setdefault(find(row), []).append(row)
            ids = self._ids
            return {"threshold": t, "total_pairs": total, "truncated": total > len(pairs_h),
                    "pairs": [(ids[a], ids[b], s) for (a, b), s in zip(pairs_h, scores_h)],
                    "groups": [[ids[r] for r in members[root]] for root in sorted(members)]}

    def drop_duplicates(self, threshold: Optional[float] = None, where: Optional[Dict[str, Any]] = None,
                        max_pairs: int = 1 << 20) -> List[str]:
        """Delete every non-keeper of near_duplicates(...) (through delete(ids=...): tombstones, lazy compaction, the
        lexical and group columns follow) and return the deleted ids.  A truncated report has wrong components: then
        DuplicateReportTruncated (a ValueError), nothing deleted."""
        with self._lock:
            report = self.near_duplicates(threshold, where, max_pairs)
            if report["truncated"]:
                raise DuplicateReportTruncated(f"drop_duplicates: {report['total_pairs']} pairs at threshold {report['threshold']} "
                                 f"exceed max_pairs={max_pairs}; nothing was deleted (raise max_pairs or the threshold)")
            victims = [s for group in report["groups"] for s in group[1:]]
            return self.delete(ids=victims) if victims else []

    # ------------------------------------------------------------------ topic clustering ----
    def _cluster_k(self, n_clusters: Optional[int], init, live: int) -> int:
        """the number of clusters of cluster(...): explicit, from `init`, or MMRAG_TOPICS (0 = automatic), see there"""
        from .config import auto_topics, settings

        if init is not None:
            if n_clusters is not None and int(n_clusters) != len(init):
                raise ValueError(f"cluster: n_clusters={n_clusters} but init names {len(init)} rows")
            n_clusters = len(init)
        if n_clusters is None:
            k = settings.topics() or auto_topics(live)
            return min(k, live)
        k = int(n_clusters)
        if not 1 <= k <= _native.MAX_CLUSTERS:
            raise ValueError(f"cluster: n_clusters must be in 1..{_native.MAX_CLUSTERS} (got {n_clusters!r})")
        if live and k > live:
            raise ValueError(f"cluster: n_clusters={k} exceeds the {live} live rows that match")
        return k

    def cluster(self, n_clusters: Optional[int] = None, where: Optional[Dict[str, Any]] = None, max_iter: int = 25,
                tol: float = 1e-3, seed: int = 0, init: Optional[Sequence[str]] = None, representatives: int = 3,
                return_labels: bool = False, terms: int = 0) -> Dict[str, Any]:
        """Topics of the collection: spherical k-means over the live rows (matching `where`), on the full-precision rows
        (an FP8 collection's re-scoring plane).  The two hot steps are csrc/kmeans.hip (nearest centroid of every row;
        deterministic per-cluster sums); the rest is torch on [k, d] and a device sort.  It changes no search result.

        k: `n_clusters`, else len(init), else MMRAG_TOPICS, whose 0 means min(256, max(2, round(sqrt(live / 2)))); a
        default k is capped at the live rows, an explicit one above them (or outside 1..4096) is a ValueError.
        Seeds: the rows of the stored ids `init` (k distinct live matching ids), else k distinct live rows drawn
        reproducibly from (`seed`, the live rows, k).
        One iteration: round the float32 master centroids to the storage dtype; assign; count the rows that changed
        cluster; stop (converged) when at most tol * live rows changed and no cluster is empty; else each centroid
        becomes sum / |sum| of its members and every empty (or zero-sum) cluster, in index order, takes the alive row
        with the lowest score (distinct rows, ties to the lower row).  One host synchronisation per iteration.  After
        `max_iter` iterations without convergence one more assign follows, so labels, scores and centroids agree.

        Returns {"n_clusters", "iterations" (assign + update rounds), "converged", "objective": the mean score of the
        live rows after every assign, "clusters": [{"cluster", "size", "cohesion" (mean cosine to the centroid),
        "representatives": [(id, cosine)] best first, ties to the lower row, "documents": the five most frequent doc_id
        values [(value, count)]}] by size descending then cluster index, "centroids": float32 [k, d] on the device}
        and, with return_labels, "labels": {id: cluster}.  No matching row: a report without clusters.
        `terms` > 0: every cluster also carries "terms", its `terms` significant terms (significant_terms' dicts, under
        its defaults and MMRAG_KEYWORD_MIN_LENGTH) with the final assign's device labels as the grouping; 0 (default):
        no such key and no lexical work."""
        if int(max_iter) < 1 or not float(tol) >= 0.0 or int(representatives) < 0:
            raise ValueError("cluster: need max_iter >= 1, tol >= 0 and representatives >= 0")
        if not 0 <= int(terms) <= _native.MAX_K_DEEP:
            raise ValueError(f"cluster: terms must be in 0..{_native.MAX_K_DEEP} (got {terms!r})")
        with self._lock:
            self._need_plane("cluster")
            live_rows = self._rows_where(where)
            m = int(live_rows.size)
            k = self._cluster_k(n_clusters, init, m)
            if m == 0:
                out = {"n_clusters": 0, "iterations": 0, "converged": True, "objective": [], "clusters": [],
                       "centroids": torch.zeros((0, self.dim), dtype=torch.float32, device=self.device)}
                if return_labels:
                    out["labels"] = {}
                return out
            if init is not None:
                seeds = [self._row_of.get(i, -1) for i in init]
                ok = set(live_rows.tolist())
                if len(set(seeds)) != k or any(r not in ok for r in seeds):
                    raise ValueError("cluster: init must name distinct stored ids of live rows that match `where`")
                seeds = np.asarray(seeds, dtype=np.int64)
            else:
                seeds = np.random.default_rng(int(seed)).choice(live_rows, k, replace=False)
            rows, n, d, dev = self._full, self._n, self.dim, self.device
            bits = self._where_bits(where)
            cent = rows[torch.from_numpy(seeds).to(dev), :d].float()           # float32 master centroids [k, d]
            packed = torch.zeros((k, rows.shape[1]), dtype=rows.dtype, device=dev)

            def assign():
                packed[:, :d] = cent.to(rows.dtype)
                return _native.kmeans_assign(rows, n, d, packed, alive=bits)

            def live_mean(score):
                return float(torch.where(labels >= 0, score, torch.zeros_like(score)).double().sum().item()) / m

            prev = torch.full((n,), -1, dtype=torch.int32, device=dev)
            objective: List[float] = []
            iterations, converged = 0, False
            for _ in range(int(max_iter)):
                labels, score = assign()
                iterations += 1
                # members by cluster, ascending rows inside one; dead rows (label -1) sort first and are skipped by seg_off
                order = torch.sort(labels, stable=True).indices.to(torch.int32)
                seg_off = torch.cumsum(torch.bincount(labels.long() + 1, minlength=k + 1), 0)
                sums = _native.cluster_sums(rows, d, order, seg_off, k)
                norms = torch.linalg.vector_norm(sums, dim=1)
                bad = (seg_off[1:] == seg_off[:-1]) | (norms == 0)
                changed, n_bad = torch.stack([(labels != prev).sum(), bad.sum()]).tolist()    # the iteration's one sync
                objective.append(live_mean(score))
                prev = labels
                if changed <= tol * m and n_bad == 0:
                    converged = True
                    break
                cent = sums / torch.where(norms > 0, norms, torch.ones_like(norms)).unsqueeze(1)
                if n_bad:
                    # score ascending, ties to the lower row (stable); dead rows hold -inf: push them behind
                    low = torch.sort(torch.where(labels >= 0, score, torch.full_like(score, float("inf"))),
                                     stable=True).indices[:n_bad]
                    cent[bad.nonzero().squeeze(1)] = rows[low, :d].float()
            if not converged:
                labels, score = assign()
                objective.append(live_mean(score))

            # ---- the report (not a hot path): members by (cluster, cosine descending, row ascending)
            live_dev = (labels >= 0).nonzero().squeeze(1)
            by_score = live_dev[torch.sort(score[live_dev], descending=True, stable=True).indices]
            by_cluster = by_score[torch.sort(labels[by_score], stable=True).indices]
            members = by_cluster.cpu().numpy()
            labels_h, score_h = labels.cpu().numpy(), score.cpu().numpy().astype(np.float64)
            sizes = np.bincount(labels_h[members], minlength=k)
            starts = np.concatenate([[0], np.cumsum(sizes)])
            ids, metas = self._ids, self._metadatas
            clusters = []
            for c in range(k):
                mine = members[starts[c]: starts[c + 1]]
                docs: Dict[Any, int] = {}
                for r in np.sort(mine).tolist():
                    v = metas[r].get("doc_id")
                    if v is not None:
                        docs[v] = docs.get(v, 0) + 1
                clusters.append({
                    "cluster": c, "size": int(sizes[c]),
                    "cohesion": float(score_h[mine].mean()) if mine.size else 0.0,
                    "representatives": [(ids[r], float(score_h[r])) for r in mine[: int(representatives)].tolist()],
                    "documents": sorted(docs.items(), key=lambda kv: -kv[1])[:5]})    # stable: ties by first appearance
            if int(terms) > 0:
                from .config import settings

                lists = self._group_term_lists(labels, torch.from_numpy(sizes.astype(np.int32)).to(dev), int(terms), 2,
                                               settings.keyword_min_length(), ())
                for c, found in zip(clusters, lists):
                    c["terms"] = found
            clusters.sort(key=lambda c: (-c["size"], c["cluster"]))
            out = {"n_clusters": k, "iterations": iterations, "converged": converged, "objective": objective,
                   "clusters": clusters, "centroids": cent}
            if return_labels:
                out["labels"] = {ids[r]: int(labels_h[r]) for r in np.sort(members).tolist()}
            return out

    def add_rows_device(self, rows_packed: torch.Tensor, documents, metadatas, ids,
                        plane_rows: Optional[torch.Tensor] = None, timestamps=None):
        """Append rows that are already in storage layout [m, ld] (bulk loads, benchmarks).  FP8 collections take the
        E4M3 codes (uint8 or float8_e4m3fn) and, when they keep a re-scoring plane, the same rows in the plane's layout
        [m, plane_ld] as `plane_rows`.  `timestamps` as add()'s."""
        m = rows_packed.shape[0]
        if self.is_f8 and rows_packed.dtype not in (torch.uint8, torch.float8_e4m3fn):
            raise ValueError("a float8_e4m3fn collection takes E4M3 codes (uint8 or float8_e4m3fn)")
        if (self._plane is None) != (plane_rows is None) or (plane_rows is not None and plane_rows.shape[0] != m):
            raise ValueError("plane_rows must be given exactly when the collection keeps a re-scoring plane, one per row")
        times = self._row_times(timestamps, m)
        with self._lock:
            self._reserve(self._n + m)
            self._raw(self._matrix)[self._n: self._n + m].copy_(self._raw(rows_packed))
            if plane_rows is not None:
                self._plane[self._n: self._n + m].copy_(plane_rows)
            for i in range(m):
                self._row_of[ids[i]] = self._n + i
            self._ids.extend(ids)
            self._documents.extend(documents if documents is not None else [None] * m)
            self._metadatas.extend(metadatas if metadatas is not None else [{} for _ in range(m)])
            self._appended(m, times)

    @staticmethod
    def _row_times(timestamps, m: int) -> np.ndarray:
        """`timestamps` of add() as float64 [m]: None = now, a number = that time for every row"""
        if timestamps is None:
            return np.full(m, time.time(), dtype=np.float64)
        t = np.asarray(timestamps, dtype=np.float64)
        if np.isinf(t).any():
            raise ValueError("timestamps must be UNIX times or NaN")
        if t.ndim == 0:
            return np.full(m, float(t), dtype=np.float64)
        if t.shape != (m,):
            raise ValueError(f"{t.size} timestamps for {m} rows")
        return t.copy()

    def _appended(self, m: int, times: np.ndarray):
        """m rows, added at `times`, were appended to the matrix and the row tables (caller holds the lock): what is
        derived follows"""
        lo, hi = self._n, self._n + m
        self._added_at[lo:hi] = times
        # a cached spec column stays current, at ITS now; one of a floored hour that has passed is dropped instead: no
        # search asks for it again, and the cost of an add stays that of the columns in use
        for key, st in list(self._spec_cols.items()):
            if st["spec"].now is None and st["spec"].resolved_now() != st["now"]:
                del self._spec_cols[key]
                continue
            new = st["spec"].column(times, self._metadatas[lo:hi], st["now"])
            st["col"][lo:hi].copy_(_native._pinned_to_device(torch.from_numpy(new), self.device))
        self._meta_index.append(self._metadatas[lo:hi])
        self._filter_cols.appended(self._metadatas[lo:hi], lo)
        self._set_alive(lo, hi)
        if self._lex is not None:
            self._lex.append(self._documents[lo:hi])
        if self._sparse is not None:
            pending, self._pending_sparse = self._pending_sparse, None
            if pending is not None:
                self._sparse.append(*pending)
            else:
                self._sparse.append_empty(m)
        if self._groups:
            self._groups_appended(lo, hi)
        self._n = hi
        self._grown(m)

    def _grown(self, m: int):
        """row tables grew by m (caller holds the lock): see config.MMRAG_GC_FREEZE_ROWS"""
        self._unfrozen_rows = getattr(self, "_unfrozen_rows", 0) + m
        from .config import settings

        every = settings.MMRAG_GC_FREEZE_ROWS
        if every > 0 and self._unfrozen_rows >= every:
            gc.freeze()
            self._unfrozen_rows = 0

    def _is_dead(self, rows: np.ndarray) -> np.ndarray:
        return ((self._alive_host[rows >> 5] >> (rows & 31).astype(np.uint32)) & 1) == 0

    def _rows_where(self, where: Optional[Dict[str, Any]]) -> np.ndarray:
        """Ascending LIVE rows whose metadata matches `where` (inverted index when the form allows, else a scan)."""
        fast = self._meta_index.rows(where)
        if fast is None:
            fast = np.fromiter((i for i in range(self._n) if match_where(self._metadatas[i], where)), dtype=np.int64)
        if self._n_dead and fast.size:
            fast = fast[~self._is_dead(fast)]
        return fast

    def _where_bits(self, where: Optional[Dict[str, Any]]) -> Optional[torch.Tensor]:
        """device alive bitmap for one search: tombstones AND `where` (ANDed on the device), or None = every row"""
        if not where:
            return self._alive_dev if self._n_dead else None
        if self.device_filters:
            words = self._where_bits_device(where)
            if words is not None:
                return words
        flags = np.zeros(self._alive_host.size * 32, dtype=bool)
        flags[self._rows_where(where)] = True
        words = torch.from_numpy(np.packbits(flags, bitorder="little").view(np.int32)).to(self.device)
        return torch.bitwise_and(words, self._alive_dev) if self._n_dead else words

    def _launch_search(self, query_embeddings, n_results: int, where, check_norm: bool = True):
        """enqueue the search (caller holds the lock); returns device tensors, no host sync"""
        if n_results < 1:
            raise ValueError("n_results must be >= 1")
        if self._plane is not None:
            return self._launch_search_rescored(query_embeddings, n_results, where, check_norm)
        q = self._pack_queries(query_embeddings, check_norm)
        bits = self._where_bits(where)
        return self._scan(q, n_results, bits)

    def _launch_search_rescored(self, query_embeddings, n_results: int, where, check_norm: bool):
        """FP8 collection with a re-scoring plane (caller holds the lock): over-fetch from the scan plane, then the
        exact scores of those candidates on the full-precision plane and the best n_results of them, same stream"""
        from .config import settings

        qf = self._to_device_f32(query_embeddings, "query", check_norm)     # converted and norm-checked once
        q8 = self._pack_queries(qf, check_norm=False)
        qp = self._pack_plane_queries(qf)
        bits = self._where_bits(where)
        if n_results <= _native.MAX_K_DEEP:
            C = min(max(_native.MAX_K, int(settings.MMRAG_F8_OVERSAMPLE) * n_results), _native.MAX_K_DEEP)
            C = max(C, n_results)
            _, cand = self._scan(q8, C, bits)
            return _native.rescore_topk(qp, self._plane, self.dim, cand.contiguous(), n_results, packed_out=True)
        # deeper than one candidate list: the single-query masked-pass loop, over-fetch 1, each pass re-scored (passes
        # stay in the scan plane's order, each pass ordered by its exact scores)
        scores, rows = self._scan(q8, n_results, bits)
        return _cat_pairs([_native.rescore_topk(qp, self._plane, self.dim, rows[:, i:i + _native.MAX_K].contiguous(),
                                                min(_native.MAX_K, rows.shape[1] - i))
                           for i in range(0, rows.shape[1], _native.MAX_K)], 1)

    def _scan(self, q: torch.Tensor, n_results: int, bits):
        """the search kernels on the stored matrix for packed queries q (caller holds the lock)"""
        if n_results <= _native.MAX_K and self.f32_exact and self.dtype == torch.float32 and q.shape[0] > 64:
            # exact float32 scores whatever the batch size (MMRAG_F32_EXACT_SEARCH): 64 queries per scan keep the exact
            # float32 matrix instruction; bigger batches would take the bf16-split path of csrc/search.hip
            return self._in_slices(q, 64, lambda qi: _native.cosine_topk(qi, self._matrix, self._n, self.dim, n_results,
                                                                         alive_bits=bits))
        if n_results <= _native.MAX_K:
            need = _native.cosine_topk_workspace_bytes(q.shape[0], self._n, n_results)
            return _native.cosine_topk(q, self._matrix, self._n, self.dim, n_results, alive_bits=bits,
                                       workspace=self._workspace("_search_ws", need), packed_out=True)
        if n_results <= _native.MAX_K_DEEP:
            # deeper than the kernel's lists (get_similar_documents asks for n_results + 1): the threshold-filter scan
            # and per-query select of csrc/search_deep.hip, any batch, one call (it synchronises the stream once)
            step = 64 if self.f32_exact and self.dtype == torch.float32 else q.shape[0]   # as above: exact float32

            def deep(qi: torch.Tensor):
                need = _native.cosine_topk_deep_workspace_bytes(qi.shape[0], self._n, n_results)
                return _native.cosine_topk_deep(qi, self._matrix, self._n, self.dim, n_results, alive_bits=bits,
                                                workspace=self._workspace("_deep_ws", need))

            return self._in_slices(q, step, deep)
        if q.shape[0] != 1:
            raise ValueError(f"n_results > {_native.MAX_K_DEEP} is supported for single queries only")
        # deeper than the deep search (MAX_K_DEEP): further passes with the rows already returned masked out -- still
        # exact, still ordered
        if bits is None:
            bits = self._alive_dev
        bits = bits.clone()
        out_s, out_r, left = [], [], n_results
        while left > 0:
            k = min(left, _native.MAX_K)
            s, r = _native.cosine_topk(q, self._matrix, self._n, self.dim, k, alive_bits=bits)
            out_s.append(s)
            out_r.append(r)
            got = r[0]
            got = got[got >= 0]
            if got.numel() < k:
                break
            host = got.cpu().numpy()
            w = bits.cpu().numpy().view(np.uint32).copy()
            np.bitwise_and.at(w, host >> 5, ~(np.uint32(1) << (host & 31).astype(np.uint32)))
            bits = torch.from_numpy(w.view(np.int32)).to(self.device)
            left -= k
        return torch.cat(out_s, 1), torch.cat(out_r, 1)

    def _workspace(self, name: str, need: int) -> Optional[torch.Tensor]:
        """the reusable workspace `name` (_search_ws, _deep_ws) with at least `need` bytes if the caller is on the
        default stream, else None.  One per index: searches are enqueued under the lock on the caller's current stream,
        and every caller thread of the service uses the default stream, so consecutive scans are ordered on the device"""
        if torch.cuda.current_stream(self.device) != torch.cuda.default_stream(self.device):
            return None
        ws = getattr(self, name)
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            setattr(self, name, ws)
        return ws

    @staticmethod
    def _in_slices(q: torch.Tensor, step: int, run):
        """run(q[i:i + step]) -> (scores, rows), `step` queries at a time, joined in query order"""
        return _cat_pairs([run(q[i:i + step]) for i in range(0, q.shape[0], step)], 0)

    def search(self, query_embeddings, n_results: int, where: Optional[Dict[str, Any]] = None):
        """Raw device search: (scores [B, k] float32 desc, rows [B, k] int64, -1 = none).

        Any batch size for n_results up to MAX_K_DEEP = 4096: up to MAX_K = 20 in the kernel's register lists (one
        scan), above that the deep search (bound, filter scan, select; one stream synchronisation).  Deeper than 4096:
        single queries only, in passes of 20 with the rows already returned masked out."""
        with self._lock:
            return self._launch_search(query_embeddings, n_results, where)

    def _tables(self):
        """the row tables as they are now (caller holds the lock).  They are append-only between compactions (a delete
        only clears alive bits and the id map) and a compaction swaps in NEW lists, so a result is built from this
        snapshot after the lock is dropped: a hit deleted after the launch is returned whole, as if the delete came later"""
        return self._ids, self._documents, self._metadatas

    @staticmethod
    def _rows_of(tables, rows: Sequence[int], include: Sequence[str]):
        """(ids, documents or None, metadatas or None) of these rows of a _tables() snapshot; the metadatas are copies"""
        ids_t, docs_t, metas_t = tables
        return ([ids_t[r] for r in rows],
                [docs_t[r] for r in rows] if "documents" in include else None,
                [dict(metas_t[r]) for r in rows] if "metadatas" in include else None)

    @classmethod
    def _append_hits(cls, out: Dict[str, Any], tables, rows: Sequence[int], include: Sequence[str]):
        """one query's hits appended to the lists of lists of a Chroma-shaped result (a None list stays None)"""
        for key, col in zip(("ids", "documents", "metadatas"), cls._rows_of(tables, rows, include)):
            if col is not None:
                out[key].append(col)

    accepts_device_queries = True   # query() takes a device tensor as it is (EmbeddingManager's no-round-trip path)

    def query(self, query_embeddings, n_results: int = 10, where: Optional[Dict[str, Any]] = None,
              include: Sequence[str] = ("metadatas", "documents", "distances"), check_norm: bool = True) -> Dict[str, Any]:
        """Chroma-shaped result: lists of lists, ascending distance = 1 - cos, at most count() hits.
        `check_norm=False` (not in Chroma): the caller vouches for unit-norm rows -- the engine's own embeddings on the
        device, where the check would cost a host synchronisation per call.

        The lock is held only while the kernels are enqueued: concurrent callers (asyncio.to_thread workers,
        embedder.py:595) overlap their host waits and result building, which reads the snapshot of _tables()."""
        with self._lock, stage("search"):
            scores, rows = self._launch_search(query_embeddings, n_results, where, check_norm)
            tables = self._tables()
            emb_src = self._full if "embeddings" in include else None
        with stage("collect"):
            return self._collect(scores, rows, include, *tables, emb_src)

    def _collect(self, scores, rows, include, ids_t, docs_t, metas_t, emb_src) -> Dict[str, Any]:
        # one device -> host copy each, then plain Python lists: per-element numpy scalars cost 10x a list item
        with stage("collect.wait"):               # (the device's share of the call: encoder + search finish here)
            if rows.is_cuda and rows._base is not None and scores._base is not None and rows._base.data_ptr() == scores._base.data_ptr():
                # packed [rows | scores] (cosine_topk(packed_out=True)): ONE copy into pinned memory and a wait for
                # ITS event -- a blocking copy to pageable memory (`.cpu()`) holds the stream inside the runtime
                # until it is through, and other callers' launches queue up behind it
                host = torch.empty(rows._base.shape, dtype=rows._base.dtype).pin_memory()
                host.copy_(rows._base, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()
                nb = rows.numel()
                rows_h = host[: nb * 8].view(torch.int64).view(rows.shape)
                scores_h = host[nb * 8:].view(torch.float32).view(scores.shape)
            else:
                rows_h, scores_h = rows.cpu(), scores.cpu()
        dist_l = (1.0 - scores_h).tolist() if "distances" in include else None        # float32 arithmetic, as before
        want_m, want_d, want_e = "metadatas" in include, "documents" in include, "embeddings" in include
        out: Dict[str, Any] = {"ids": [], "distances": [] if dist_l is not None else None,
                               "metadatas": [] if want_m else None, "documents": [] if want_d else None,
                               "embeddings": [] if want_e else None}
        # every table is read with ONE itemgetter call over all hits of the batch (a C loop), then cut per query:
        # B x k Python-level index operations and dict() calls were most of the host time of a 256-query batch
        no_miss = bool(rows_h.numel()) and int(rows_h.min()) >= 0
        if no_miss and _HOSTROWS is not None and not want_e:
            # every query has all its k hits: one pass in C over the row numbers (csrc/hostrows.c) -- the same objects
            # in the same order as the comprehensions below, without the interpreter in the loop
            ids_ll, docs_ll, metas_ll = _HOSTROWS.gather(rows_h.contiguous().numpy(), rows_h.shape[1], ids_t,
                                                         docs_t if want_d else None, metas_t if want_m else None)
            out["ids"], out["documents"], out["metadatas"] = ids_ll, docs_ll, metas_ll
            if dist_l is not None:
                out["distances"] = dist_l
            return out
        if not no_miss:                                                          # short lists: query by query
            for b, row in enumerate(rows_h.tolist()):
                hit = [r for r in row if r >= 0]                                 # misses (-1) only trail
                self._append_hits(out, (ids_t, docs_t, metas_t), hit, include)
                if dist_l is not None:
                    out["distances"].append(dist_l[b][: len(hit)])
                if want_e:
                    out["embeddings"].append(self._fetch(hit, emb_src))
            return out
        flat = rows_h.reshape(-1).tolist()                                       # every query has all its k hits
        if len(flat) == 1:
            pick = lambda table: (table[flat[0]],)                               # noqa: E731  (itemgetter(x) alone returns the item)
        else:
            getter = operator.itemgetter(*flat)
            pick = lambda table: getter(table)                                   # noqa: E731
        ids_f = pick(ids_t)
        metas_f = list(map(dict, pick(metas_t))) if want_m else None
        docs_f = pick(docs_t) if want_d else None
        # cut the flat columns with one comprehension each
        k_, nf = rows_h.shape[1], len(flat)
        out["ids"] = [list(ids_f[lo:lo + k_]) for lo in range(0, nf, k_)]
        if dist_l is not None:
            out["distances"] = dist_l
        if want_m:
            out["metadatas"] = [metas_f[lo:lo + k_] for lo in range(0, nf, k_)]
        if want_d:
            out["documents"] = [list(docs_f[lo:lo + k_]) for lo in range(0, nf, k_)]
        if want_e:
            out["embeddings"] = [self._fetch(flat[lo:lo + k_], emb_src) for lo in range(0, nf, k_)]
        return out

    def ids_of_rows(self, rows: Sequence[int]) -> List[str]:
        """ids of the given local rows (row numbers are stable until the next compaction)."""
        with self._lock:
            return [self._ids[int(r)] for r in rows]

    def _fetch(self, rows: List[int], matrix: Optional[torch.Tensor] = None) -> List[List[float]]:
        if not rows:
            return []
        m = self._full if matrix is None else matrix
        t = _native.fetch_rows_f32(m, torch.tensor(rows, dtype=torch.int64, device=self.device), self.dim)
        return t.cpu().numpy().tolist()

    def get(self, ids: Optional[Sequence[str]] = None, where: Optional[Dict[str, Any]] = None,
            include: Sequence[str] = ("metadatas", "documents")) -> Dict[str, Any]:
        with self._lock:
            if ids is not None:
                rows = [self._row_of[i] for i in ids if i in self._row_of]
                rows = [r for r in rows if match_where(self._metadatas[r], where)]
            else:
                rows = self._rows_where(where).tolist()
            ids_l, docs_l, metas_l = self._rows_of(self._tables(), rows, include)
            return {"ids": ids_l, "metadatas": metas_l, "documents": docs_l,
                    "embeddings": self._fetch(rows) if "embeddings" in include else None}

    def delete(self, ids: Optional[Sequence[str]] = None, where: Optional[Dict[str, Any]] = None) -> List[str]:
        """Tombstone the matching rows (collection.delete, embedder.py:639-642): clear their alive bits on the
        device, drop them from the id map.  O(victims); the matrix is compacted only past COMPACT_DEAD_FRACTION."""
        with self._lock:
            if ids is not None:
                rows = [self._row_of[i] for i in ids if i in self._row_of]
                if where:
                    rows = [r for r in rows if match_where(self._metadatas[r], where)]
                rows = np.asarray(sorted(set(rows)), dtype=np.int64)
            else:
                rows = self._rows_where(where)
            if rows.size == 0:
                return []
            gone = [self._ids[int(r)] for r in rows]
            for s in gone:
                del self._row_of[s]
            # The row tables (_ids, _documents, _metadatas) are NOT touched: a query() that enqueued its search before
            # this delete builds its result from them after dropping the lock, and must still find the hit's id and
            # text there.  The alive bitmap and _row_of are what say "dead"; compact() drops the entries for good.
            self._clear_alive(rows)
            self._n_dead += int(rows.size)
            if self._lex is not None:
                self._lex.delete_rows(rows)
            if self._n_dead >= self.COMPACT_MIN_DEAD and self._n_dead > self.COMPACT_DEAD_FRACTION * self._n:
                self.compact()
            return sorted(gone)

    def compact(self):
        """Drop the dead rows (stable: survivors keep their order).  New tables and a new matrix are swapped in, so
        result-building threads that still hold the old ones are unaffected."""
        with self._lock:
            if self._n_dead == 0:
                return
            keep = np.nonzero(~self._is_dead(np.arange(self._n, dtype=np.int64)))[0]
            cap = max(256, int(keep.size), self._matrix.shape[0] // 2 if keep.size < self._matrix.shape[0] // 4 else self._matrix.shape[0])
            keep_dev = torch.from_numpy(keep).to(self.device)
            self._matrix = self._compacted(self._matrix, cap, keep_dev, 0)
            if self._plane is not None:
                self._plane = self._compacted(self._plane, cap, keep_dev, 0)
            self._ids = [self._ids[r] for r in keep]
            self._documents = [self._documents[r] for r in keep]
            self._metadatas = [self._metadatas[r] for r in keep]
            self._row_of = {s: i for i, s in enumerate(self._ids)}
            self._n = int(keep.size)
            self._n_dead = 0
            self._meta_index = MetaIndex()
            self._meta_index.append(self._metadatas)
            self._alive_host = np.zeros(self._n_words(cap), dtype=np.uint32)
            self._alive_dev = torch.zeros(self._n_words(cap), dtype=torch.int32, device=self.device)
            if self._n:
                self._set_alive(0, self._n)
            if self._lex is not None:
                self._lex.compact(keep)
            if self._sparse is not None:
                self._sparse.compact(keep)
            for st in self._groups.values():      # the same kept rows, in order; ordinals keep their values
                st["col"] = self._compacted(st["col"], cap, keep_dev, -1)
                live = st["col"][: self._n]
                st["counts"] = torch.bincount(live[live >= 0], minlength=len(st["values"])).tolist()
            times = np.full(cap, np.nan, dtype=np.float64)
            times[: self._n] = self._added_at[keep]
            self._added_at = times
            self._filter_cols.compacted(keep)
            self._map_prior_columns(lambda col: self._compacted(col, cap, keep_dev, 0))
            if self._tokens is not None:
                self._tokens.compact(keep)     # the same kept rows, in order: item stays row

    def reset(self):
        with self._lock:
            self._n = 0
            self._n_dead = 0
            self._ids, self._documents, self._metadatas, self._row_of = [], [], [], {}
            self._meta_index = MetaIndex()
            self._alive_host[:] = 0
            self._alive_dev.zero_()
            if self._lex is not None:
                self._lex.reset()
            if self._sparse is not None:
                self._sparse.reset()
            self._groups = {}
            self._added_at[:] = np.nan
            self._filter_cols.reset()
            self._priors = {}
            self._spec_cols.clear()
            if self._tokens is not None:
                self._tokens.reset()

    # ------------------------------------------------------------------ diversified (MMR) ----
    def _launch_mmr(self, query_embeddings, n_results: int, fetch_k, lambda_mult, where, check_norm: bool = True):
        """enqueue the dense search for the candidates and the MMR selection over them, on one stream (caller holds
        the lock): device (scores, rows, positions, mmr values) [B, n_results] in pick order, no host sync of its own"""
        from .config import settings

        self._need_plane("mmr_query")
        if n_results < 1:
            raise ValueError("n_results must be >= 1")
        if n_results > _native.MAX_MMR_CANDIDATES:
            raise ValueError(f"n_results must be <= {_native.MAX_MMR_CANDIDATES} for MMR selection")
        C = max(n_results, settings.MMRAG_MMR_CANDIDATES) if fetch_k is None else int(fetch_k)
        C = max(min(C, _native.MAX_MMR_CANDIDATES), n_results)
        lam = float(settings.MMRAG_MMR_LAMBDA if lambda_mult is None else lambda_mult)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"lambda_mult must be in [0, 1] (got {lambda_mult!r})")
        scores, rows = self._launch_search(query_embeddings, C, where, check_norm)
        return _native.mmr_select(self._full, self.dim, scores.contiguous(), rows.contiguous(), n_results, lam)

    def mmr_search(self, query_embeddings, n_results: int, fetch_k: Optional[int] = None,
                   lambda_mult: Optional[float] = None, where: Optional[Dict[str, Any]] = None):
        """Raw diversified search: maximal-marginal-relevance selection (csrc/mmr.hip, include/mmrag.h
        mmrag_mmr_select) of n_results of the fetch_k best dense hits.  Returns device tensors [B, n_results] in PICK
        order: (scores float32 = the dense scores, rows int64, positions int32 in the dense order, mmr values float32),
        unused slots (-inf, -1, -1, -inf).  fetch_k defaults to max(n_results, MMRAG_MMR_CANDIDATES), is clipped to
        MAX_MMR_CANDIDATES = 1024 and raised to n_results; lambda_mult defaults to MMRAG_MMR_LAMBDA (1 = the dense
        order, 0 = pure diversity after the first pick).  The candidates are search()'s, so deleted and filtered rows
        never appear."""
        with self._lock:
            return self._launch_mmr(query_embeddings, n_results, fetch_k, lambda_mult, where)

    def mmr_query(self, query_embeddings, n_results: int = 10, fetch_k: Optional[int] = None,
                  lambda_mult: Optional[float] = None, where: Optional[Dict[str, Any]] = None,
                  include: Sequence[str] = ("metadatas", "documents", "distances"),
                  check_norm: bool = True) -> Dict[str, Any]:
        """query() with maximal-marginal-relevance selection (see mmr_search): the Chroma-shaped dict of query() plus
        `mmr_scores`, the value lambda * cos - (1 - lambda) * (largest cos to an earlier pick) each hit was picked
        with (the first hit: its cos).  Results are in PICK order, so `distances` (1 - cos) are NOT ascending."""
        with self._lock, stage("search"):
            scores, rows, _, mmr = self._launch_mmr(query_embeddings, n_results, fetch_k, lambda_mult, where,
                                                    check_norm)
            tables = self._tables()
            emb_src = self._full if "embeddings" in include else None
        with stage("collect"):
            out = self._collect(scores, rows, include, *tables, emb_src)
            out["mmr_scores"] = [vals[: len(ids)] for vals, ids in zip(mmr.cpu().tolist(), out["ids"])]
            return out

    # ------------------------------------------------------------------ grouped by a metadata key ----
    def _group_ordinals(self, st: Dict[str, Any], metadatas: Sequence[Dict[str, Any]]) -> torch.Tensor:
        """group ordinals (host int32) of rows with these metadatas, in row order: distinct values of meta.get(key) are
        numbered by first appearance; a missing key, None or an unhashable value gives -1 (caller holds the lock)"""
        key, ordinal, values, counts = st["key"], st["ordinal"], st["values"], st["counts"]
        out = np.full(len(metadatas), -1, dtype=np.int32)
        for i, meta in enumerate(metadatas):
            v = meta.get(key)
            if v is None:
                continue
            try:
                o = ordinal.get(v)
                if o is None:
                    o = ordinal[v] = len(values)
                    values.append(v)
                    counts.append(0)
            except TypeError:        # unhashable: the row has no key
                continue
            out[i] = o
            counts[o] += 1
        return torch.from_numpy(out)

    def enable_grouping(self, key: str = "doc_id") -> Dict[str, Any]:
        """Build the group column of metadata key `key`: a device int32 [capacity] with each row's group ordinal
        (distinct values of meta.get(key) numbered by first appearance in row order; -1 where the key is missing, None
        or unhashable), the host table ordinal -> value and, beside it, the rows stored per ordinal (dead rows still
        counted until compact: an upper bound, what scoped_search sizes its candidate slots by).  From then on add,
        add_rows_device, capacity growth and compact keep them current; reset drops them; delete needs nothing (dead
        rows are never candidates).  Until then they do no grouping work.  Runs by itself on the first grouped_search /
        grouped_query / scoped_search for that key.  The column is derived from the metadata and is not persisted: a
        loaded collection rebuilds it on first use."""
        with self._lock:
            st = self._groups.get(key)
            if st is None:
                st = {"key": key, "ordinal": {}, "values": [], "counts": []}
                col = torch.full((self._matrix.shape[0],), -1, dtype=torch.int32, device=self.device)
                if self._n:
                    col[: self._n].copy_(self._group_ordinals(st, self._metadatas[: self._n]))
                st["col"] = col
                self._groups[key] = st
            return st

    def _groups_appended(self, lo: int, hi: int):
        """rows [lo, hi) were appended to the row tables (caller holds the lock)"""
        for st in self._groups.values():
            st["col"][lo:hi].copy_(self._group_ordinals(st, self._metadatas[lo:hi]))

    def _launch_grouped(self, query_embeddings, n_groups: int, group_size: int, group_by: str, fetch_k, where,
                        check_norm: bool = True):
        """enqueue the search(es) and the grouping of their hits (caller holds the lock): the five device tensors of
        _native.group_select for the whole batch, and each query's candidate depth"""
        from .config import settings

        G, S = int(n_groups), int(group_size)
        if not 1 <= G <= _native.MAX_GROUPS:
            raise ValueError(f"n_groups must be in 1..{_native.MAX_GROUPS}")
        if not 1 <= S <= _native.MAX_GROUP_SIZE:
            raise ValueError(f"group_size must be in 1..{_native.MAX_GROUP_SIZE}")
        top = _native.MAX_GROUP_CANDIDATES
        if fetch_k is None:
            C = min(max(int(settings.MMRAG_GROUP_CANDIDATES), 4 * G * S), top)
        else:
            C = min(max(int(fetch_k), G), top)
        st = self.enable_grouping(group_by)
        qf = self._to_device_f32(query_embeddings, "query", check_norm)     # converted and norm-checked once

        def one_pass(q: torch.Tensor, depth: int):
            scores, rows = self._launch_search(q, depth, where, check_norm=False)
            return _native.group_select(scores.contiguous(), rows.contiguous(), st["col"], self._n, G, S)

        out = one_pass(qf, C)
        depths = [C] * qf.shape[0]
        if fetch_k is None:
            todo, cur = torch.arange(qf.shape[0]), out
            while C < top:
                info = cur[4].cpu()                                          # the rung's host synchronisation
                todo = todo[(info[:, 0] < G) & (info[:, 1] >= C)]            # neither G groups nor an exhausted list
                if not todo.numel():
                    break
                C = min(4 * C, top)
                at = todo.to(self.device)
                cur = one_pass(qf[at].contiguous(), C)
                for whole, part in zip(out, cur):
                    whole[at] = part
                for b in todo.tolist():
                    depths[b] = C
        return out, depths

    def grouped_search(self, query_embeddings, n_groups: int, group_size: int = 1, group_by: str = "doc_id",
                       fetch_k: Optional[int] = None, where: Optional[Dict[str, Any]] = None):
        """Raw grouped search: the first n_groups groups of each query's dense hits with up to group_size members each,
        grouped by the metadata key `group_by` (csrc/group.hip, include/mmrag.h mmrag_group_select, where the
        definition is).  Returns device tensors (scores [B, G, S] float32 = the search's own scores, rows [B, G, S]
        int64, positions [B, G, S] int32 in the candidate list, group ordinals [B, G] int32 (-1 = a row without the
        key, a group of its own), info [B, 2] int32 = (groups found, valid candidates)) and the list of each query's
        candidate depth; unused slots hold (-inf, -1, -1) and -2.  n_groups <= 256, group_size <= 16.

        Candidate depth.  An explicit fetch_k is one pass at that depth, clipped to [n_groups, 4096], with no host
        synchronisation.  fetch_k=None walks a ladder: the first pass takes
        C0 = min(max(MMRAG_GROUP_CANDIDATES, 4 * n_groups * group_size), 4096) hits; a query is complete when it found
        n_groups groups or its list was exhausted (fewer than C valid candidates); the queries that are not are searched
        again, as a sub-batch, at min(4 * C, 4096), until all are complete or C = 4096.  A query's answer is the pass at
        which it first became complete, so it is the same alone or inside any batch.  Reading the info block costs ONE
        HOST SYNCHRONISATION PER RUNG below 4096.

        The candidates are search()'s: tombstones and `where` are honoured, a float8_e4m3fn collection is re-scored on
        its plane (in capacity mode the scores are the quantised collection's own, as in query())."""
        with self._lock:
            out, depths = self._launch_grouped(query_embeddings, n_groups, group_size, group_by, fetch_k, where)
        return (*out, depths)

    def grouped_query(self, query_embeddings, n_groups: int = 5, group_size: int = 1, group_by: str = "doc_id",
                      fetch_k: Optional[int] = None, where: Optional[Dict[str, Any]] = None,
                      include: Sequence[str] = ("metadatas", "documents", "distances"),
                      check_norm: bool = True) -> Dict[str, Any]:
        """query() grouped by a metadata key (see grouped_search): the n_groups best documents and the group_size best
        hits of each.  Returns
            {"groups": [[{"key": value or None, "ids": [...], "distances": [...], "metadatas": [...],
                          "documents": [...]}, ...] per query, in group-rank order],
             "exhaustive": [bool per query], "fetch_k": [int per query]}
        A group is ranked by its best hit; its hits are in ascending distance.  `key` is None for a row without the
        key, which is a group of its own.  `fetch_k` is the candidate depth the answer was taken at; `exhaustive` is
        False where that depth gave neither n_groups groups nor the end of the list (on the ladder: only at 4096), so
        further groups may exist below it.  Lists an `include` leaves out are None."""
        G = int(n_groups)
        with self._lock, stage("search"):
            out, depths = self._launch_grouped(query_embeddings, n_groups, group_size, group_by, fetch_k, where,
                                               check_norm)
            tables = self._tables()
            values = self._groups[group_by]["values"]
        with stage("collect"):
            scores_h, rows_h, _, group_h, info_h = (t.cpu() for t in out)
            dist_l = (1.0 - scores_h).tolist() if "distances" in include else None     # float32 arithmetic, as query()
            rows_l, group_l, info_l = rows_h.tolist(), group_h.tolist(), info_h.tolist()
            res: Dict[str, Any] = {"groups": [], "exhaustive": [], "fetch_k": depths}
            for b, (found, valid) in enumerate(info_l):
                groups = []
                for gi in range(found):
                    rows = [r for r in rows_l[b][gi] if r >= 0]                        # unused slots only trail
                    o = group_l[b][gi]
                    ids_l, docs_l, metas_l = self._rows_of(tables, rows, include)
                    groups.append({"key": values[o] if o >= 0 else None, "ids": ids_l,
                                   "distances": dist_l[b][gi][: len(rows)] if dist_l is not None else None,
                                   "metadatas": metas_l, "documents": docs_l})
                res["groups"].append(groups)
                res["exhaustive"].append(found >= G or valid < depths[b])
            return res

    # ------------------------------------------------------------------ per-query document scopes ----
    def _scope_tables(self, st: Dict[str, Any], scopes, B: int):
        """`scopes` (one entry per query: a metadata value or a list / tuple / set of values) as the host tables of
        _native.scoped_topk (caller holds the lock): (scope of each query, the S distinct scopes as ascending ordinal
        tuples, each scope's row-count bound, each query's values as given).  An unknown value matches nothing; equal
        ordinal sets are one scope."""
        scopes = list(scopes)
        if len(scopes) != B:
            raise ValueError(f"scopes holds {len(scopes)} entries for {B} queries")
        ordinal, counts = st["ordinal"], st["counts"]
        index: Dict[Tuple[int, ...], int] = {}
        of_query, given = [], []
        for entry in scopes:
            vals = list(entry) if isinstance(entry, (list, tuple, set, frozenset)) else [entry]
            ords = set()
            for v in vals:
                try:
                    o = ordinal.get(v)
                except TypeError:        # unhashable: no row has it as its key
                    o = None
                if o is not None:
                    ords.add(o)
            of_query.append(index.setdefault(tuple(sorted(ords)), len(index)))
            given.append(vals)
        sets = list(index)
        return of_query, sets, [sum(counts[o] for o in t) for t in sets], given

    def _launch_scoped(self, query_embeddings, n_results: int, scopes, key: str, where, check_norm: bool = True):
        """enqueue the scoped search (caller holds the lock): device (scores, rows) [B, n_results], no host sync on
        the kernel's path"""
        self._need_plane("scoped_query")
        k = int(n_results)
        if not 1 <= k <= _native.MAX_K_DEEP:
            raise ValueError(f"n_results must be in 1..{_native.MAX_K_DEEP} for a scoped search")
        st = self.enable_grouping(key)
        qf = self._to_device_f32(query_embeddings, "query", check_norm)     # converted and norm-checked once
        B = qf.shape[0]
        of_query, sets, bound, given = self._scope_tables(st, scopes, B)
        cap = _native.candidate_capacity(k)
        slow = [len(t) > _native.MAX_SCOPE_GROUPS or bound[s] > cap for s, t in enumerate(sets)]
        fast_q = [b for b in range(B) if not slow[of_query[b]]]
        out_s = out_r = None
        if fast_q:
            rows = self._full
            q = self._pack_plane_queries(qf) if self._plane is not None else self._pack_queries(qf, check_norm=False)
            if len(fast_q) < B:
                q = q[torch.tensor(fast_q, device=self.device)].contiguous()
            used = sorted({of_query[b] for b in fast_q})
            renum = {s: i for i, s in enumerate(used)}
            off = [0]
            for s in used:
                off.append(off[-1] + len(sets[s]))
            need = _native.scoped_topk_workspace_bytes(len(fast_q), self._n, k, len(st["values"]))
            out_s, out_r = _native.scoped_topk(
                q, rows, self._n, self.dim, k, st["col"], len(st["values"]), [renum[of_query[b]] for b in fast_q], off,
                [o for s in used for o in sets[s]], max([bound[s] for s in used] + [1]),
                alive_bits=self._where_bits(where), workspace=self._workspace("_scoped_ws", need))
            if len(fast_q) == B:
                return out_s, out_r
        # a scope of more groups than the kernel's lists hold, or of more rows than a query has candidate slots: the
        # filtered search, one per distinct scope, joined in query order
        scores = torch.empty((B, k), dtype=torch.float32, device=self.device)
        rows_o = torch.empty((B, k), dtype=torch.int64, device=self.device)
        if fast_q:
            at = torch.tensor(fast_q, device=self.device)
            scores[at], rows_o[at] = out_s, out_r
        for s in sorted({of_query[b] for b in range(B) if slow[of_query[b]]}):
            mine = [b for b in range(B) if of_query[b] == s]
            at = torch.tensor(mine, device=self.device)
            only = {key: {"$in": given[mine[0]]}}
            ss, rr = self._launch_search(qf[at].contiguous(), k, {"$and": [where, only]} if where else only,
                                         check_norm=False)
            scores[at], rows_o[at] = ss, rr
        return scores, rows_o

    def scoped_search(self, query_embeddings, n_results: int, scopes, key: str = "doc_id",
                      where: Optional[Dict[str, Any]] = None):
        """Raw device search with a scope PER QUERY (csrc/scoped.hip, include/mmrag.h mmrag_scoped_topk): query b is
        answered from the rows whose metadata `key` is one of the values of scopes[b] (a value or a list of values; an
        unknown value matches nothing, an empty list gives no hits) -- what search(where={key: {"$in": scopes[b]}})
        returns for each query, in ONE encode-free batch: one launch sequence, no host bitmap per scope, and the row
        tiles no query of the batch can see are not read.  Returns (scores [B, k] float32 desc, rows [B, k] int64,
        -1 = none), n_results up to MAX_K_DEEP.

        `where` narrows the whole batch further; tombstones are honoured.  A float8_e4m3fn collection is searched on its
        re-scoring plane (exact scores; capacity mode raises ValueError).  A scope of more than MAX_SCOPE_GROUPS values,
        or whose documents hold more rows than a query has candidate slots (32 * n_results, at least 16384; dead rows
        count until compact()), takes the filtered search instead, in the same result."""
        with self._lock:
            return self._launch_scoped(query_embeddings, n_results, scopes, key, where)

    def scoped_query(self, query_embeddings, n_results: int = 10, scopes=(), key: str = "doc_id",
                     where: Optional[Dict[str, Any]] = None,
                     include: Sequence[str] = ("metadatas", "documents", "distances"),
                     check_norm: bool = True) -> Dict[str, Any]:
        """query() with a scope per query (see scoped_search): the Chroma-shaped dict of query(), query b's hits taken
        from the rows whose `key` is in scopes[b] only."""
        with self._lock, stage("search"):
            scores, rows = self._launch_scoped(query_embeddings, n_results, scopes, key, where, check_norm)
            tables = self._tables()
            emb_src = self._full if "embeddings" in include else None
        with stage("collect"):
            return self._collect(scores, rows, include, *tables, emb_src)

    # ------------------------------------------------------------------ per-query metadata filters ----
    def _compiled(self, where):
        """(program or None, reason) of one filter (caller holds the lock).  A filter that names "$added_at" exists on
        the device path only: where that path does not cover it, ValueError."""
        prog, why = try_compile(where, self._filter_cols)
        if prog is None and names_added_at(where):
            raise ValueError(f'a filter on "$added_at" must run on the device, and this one cannot: {why}')
        return prog, why

    def _eval_programs(self, programs, out: torch.Tensor, alive: Optional[torch.Tensor]):
        """out[f, :W] = the bitmap of programs[f] over the rows in use (caller holds the lock): one mmrag_filter_eval
        launch per run of programs that read at most MAX_FILTER_COLUMNS columns between them"""
        cap = self._matrix.shape[0]
        lo = 0
        while lo < len(programs):
            keys: List[str] = []
            hi = lo
            while hi < len(programs):
                more = [k for k in programs[hi].keys if k not in keys]
                if hi > lo and len(keys) + len(more) > _native.MAX_FILTER_COLUMNS:
                    break
                keys += more
                hi += 1
            ops, off, sets, keys = pack_programs(programs[lo:hi])
            cols = [self._filter_cols.device(k, cap, self.device) for k in keys]
            _native.filter_eval(ops, off, sets, cols, self._n, alive_bits=alive, device=self.device, out=out[lo:hi])
            lo = hi

    def _where_bits_device(self, where) -> Optional[torch.Tensor]:
        """_where_bits on the device (MMRAG_DEVICE_FILTERS): the same words the host builds, or None when the compiler
        does not cover `where` (an unknown operator included: the host path raises it where match_where does)"""
        try:
            prog, _ = self._compiled(where)
        except ValueError:
            if names_added_at(where):
                raise
            return None
        if prog is None:
            return None
        words = torch.zeros(self._alive_host.size, dtype=torch.int32, device=self.device)
        if self._n:
            self._eval_programs([prog], words[: _native.filter_words(self._n)].unsqueeze(0),
                                self._alive_dev if self._n_dead else None)
        return words

    def filter_plan(self, where: Optional[Dict[str, Any]]) -> Dict[str, Any]:
        """How `where` would run: {"device": bool, "reason": why not, "columns": the metadata keys whose columns the
        program reads}.  Builds those columns if this is their first use.  An unknown operator raises ValueError."""
        with self._lock:
            return self._filter_cols.plan(where)

    def _launch_filtered(self, query_embeddings, n_results: int, wheres, check_norm: bool = True):
        """enqueue the filtered search (caller holds the lock): device (scores, rows) [B, n_results]"""
        from .config import settings

        self._need_plane("filtered_query")
        k = int(n_results)
        if not 1 <= k <= _native.MAX_K_DEEP:
            raise ValueError(f"n_results must be in 1..{_native.MAX_K_DEEP} for a filtered search")
        qf = self._to_device_f32(query_embeddings, "query", check_norm)     # converted and norm-checked once
        B = qf.shape[0]
        wheres = [wheres] * B if wheres is None or isinstance(wheres, dict) else list(wheres)
        if len(wheres) != B:
            raise ValueError(f"wheres holds {len(wheres)} entries for {B} queries")
        # equal filters are one program and one bitmap; what does not compile is grouped by the filter as written
        seen: Dict[int, Any] = {}
        programs: Dict[Any, int] = {}
        of_query: List[int] = [-1] * B
        slow: Dict[str, Tuple[Any, List[int]]] = {}
        for b, w in enumerate(wheres):
            if id(w) not in seen:
                seen[id(w)] = self._compiled(w)[0]
            prog = seen[id(w)]
            if prog is None:
                slow.setdefault(repr(w), (w, []))[1].append(b)
            else:
                of_query[b] = programs.setdefault(prog, len(programs))
        scores = torch.empty((B, k), dtype=torch.float32, device=self.device)
        rows_o = torch.empty((B, k), dtype=torch.int64, device=self.device)
        if programs:
            # equal filters next to each other: a query tile's union bitmap then holds few filters
            order = sorted((b for b in range(B) if of_query[b] >= 0), key=lambda b: of_query[b])
            rows = self._full
            q = self._pack_plane_queries(qf) if self._plane is not None else self._pack_queries(qf, check_norm=False)
            plist = list(programs)
            W = _native.filter_words(self._n)
            per_launch = max(1, int(settings.MMRAG_FILTER_BITMAP_BYTES) // max(4 * W, 1))
            alive = self._alive_dev if self._n_dead else None
            at = 0
            for f0 in range(0, len(plist), per_launch):
                f1 = min(f0 + per_launch, len(plist))
                mine = []
                while at < len(order) and of_query[order[at]] < f1:
                    mine.append(order[at])
                    at += 1
                vis = torch.empty((f1 - f0, W), dtype=torch.int32, device=self.device)
                if self._n:
                    self._eval_programs(plist[f0:f1], vis, alive)
                whole = len(mine) == B and mine == list(range(B))
                pick = None if whole else torch.tensor(mine, device=self.device)
                need = _native.filtered_topk_workspace_bytes(len(mine), self._n, k)
                ss, rr = _native.filtered_topk(q if whole else q[pick].contiguous(), rows, self._n, self.dim, k,
                                               [of_query[b] - f0 for b in mine], vis,
                                               workspace=self._workspace("_filtered_ws", need))
                if whole:
                    return ss, rr
                scores[pick], rows_o[pick] = ss, rr
        # not covered by the compiler: the filtered search of today, one per distinct filter, joined in query order
        for w, mine in slow.values():
            pick = torch.tensor(mine, device=self.device)
            scores[pick], rows_o[pick] = self._launch_search(qf[pick].contiguous(), k, w, check_norm=False)
        return scores, rows_o

    def filtered_search(self, query_embeddings, n_results: int, wheres):
        """Raw device search with a metadata filter PER QUERY (csrc/filtered.hip, include/mmrag.h mmrag_filter_eval and
        mmrag_filtered_topk): query b is answered from the live rows whose metadata matches wheres[b] -- match_where's
        semantics, what search(where=wheres[b]) returns for each query -- in ONE batch: the distinct filters are compiled
        to small programs (filters.py), one kernel evaluates them over typed metadata columns into row bitmaps, and one
        masked scan answers every query from its own bitmap, skipping the row tiles no query of a tile can see.
        `wheres`: one filter per query (None = every live row), or one dict for all.  Returns (scores [B, k] float32
        desc, rows [B, k] int64, -1 = none), n_results up to MAX_K_DEEP.

        The reserved key "$added_at" filters on the time a row was added (UNIX seconds; see row_times()); it exists on
        the device path only (ValueError where the filter cannot run there).  A filter the compiler does not cover (see
        filter_plan) takes search(where=...) inside the same call, one search per distinct filter; the result is in
        query order either way.  A float8_e4m3fn collection is searched on its re-scoring plane (exact scores; capacity
        mode raises ValueError).  At most MMRAG_FILTER_BITMAP_BYTES of bitmaps are evaluated per launch."""
        with self._lock:
            return self._launch_filtered(query_embeddings, n_results, wheres)

    def filtered_query(self, query_embeddings, n_results: int = 10, wheres=None,
                       include: Sequence[str] = ("metadatas", "documents", "distances"),
                       check_norm: bool = True) -> Dict[str, Any]:
        """query() with a filter per query (see filtered_search): the Chroma-shaped dict of query()"""
        with self._lock, stage("search"):
            scores, rows = self._launch_filtered(query_embeddings, n_results, wheres, check_norm)
            tables = self._tables()
            emb_src = self._full if "embeddings" in include else None
        with stage("collect"):
            return self._collect(scores, rows, include, *tables, emb_src)

    # ------------------------------------------------------------------ range retrieval (count, facets, hits) ----
    def _launch_range(self, query_embeddings, threshold, limit: int, wheres, facets, check_norm: bool = True):
        """enqueue the range scan(s) (caller holds the lock): (counts [B] int64, one [B, G + 1] int64 table per facet
        key, scores [B, limit], rows [B, limit], the keys' host tables ordinal -> value), all tensors on the device"""
        from .config import settings

        self._need_plane("range_query")
        limit = int(limit)
        if not 0 <= limit <= _native.MAX_K_DEEP:
            raise ValueError(f"limit must be in 0..{_native.MAX_K_DEEP} for a range search")
        facets = [facets] if isinstance(facets, str) else list(facets)
        if len(facets) > _native.MAX_FACET_COLUMNS or len(set(facets)) != len(facets):
            raise ValueError(f"facets: at most {_native.MAX_FACET_COLUMNS} distinct metadata keys (got {facets!r})")
        qf = self._to_device_f32(query_embeddings, "query", check_norm)     # converted and norm-checked once
        B = qf.shape[0]
        thr = np.asarray(threshold, dtype=np.float32).reshape(-1)
        if thr.size == 1:
            thr = np.repeat(thr, B)
        if thr.size != B:
            raise ValueError(f"threshold holds {thr.size} entries for {B} queries")
        if not np.isfinite(thr).all():
            raise ValueError("threshold must be finite")
        wheres = [wheres] * B if wheres is None or isinstance(wheres, dict) else list(wheres)
        if len(wheres) != B:
            raise ValueError(f"wheres holds {len(wheres)} entries for {B} queries")
        states = [self.enable_grouping(key) for key in facets]
        sizes = [len(st["values"]) for st in states]
        cols = [st["col"] for st in states]
        values = [list(st["values"]) for st in states]
        slots = sum(g + 1 for g in sizes)
        budget = int(settings.MMRAG_RANGE_TABLE_BYTES)
        if 4 * slots > budget:
            raise ValueError(f"range search: one query's facet tables take {4 * slots} bytes ({slots} slots), above "
                             f"MMRAG_RANGE_TABLE_BYTES={budget}")
        # equal filters are one bitmap: ("all",) = every live row, ("prog", program), ("slow", the filter as written)
        seen: Dict[int, Any] = {}
        index: Dict[Any, int] = {}
        filters: List[Tuple[Any, Any]] = []
        of_query: List[int] = []
        for w in wheres:
            if not w:
                kind: Any = ("all",)
            else:
                if id(w) not in seen:
                    seen[id(w)] = self._compiled(w)[0]
                kind = ("prog", seen[id(w)]) if seen[id(w)] is not None else ("slow", repr(w))
            if kind not in index:
                index[kind] = len(filters)
                filters.append((kind, w))
            of_query.append(index[kind])
        masked = bool(self._n_dead) or any(kind[0] != "all" for kind, _ in filters)
        W = _native.filter_words(self._n)
        alive = self._alive_dev if self._n_dead else None

        def bitmaps(fl: List[int]) -> Tuple[torch.Tensor, Dict[int, int]]:
            """the [F, W] table of filters fl, compiled programs first (one evaluation), and each filter's row in it"""
            fl = sorted(fl, key=lambda f: filters[f][0][0] != "prog")
            vis = torch.zeros((len(fl), W), dtype=torch.int32, device=self.device)
            n_prog = sum(filters[f][0][0] == "prog" for f in fl)
            if n_prog and self._n:
                self._eval_programs([filters[f][0][1] for f in fl[:n_prog]], vis[:n_prog], alive)
            for at in range(n_prog, len(fl)):
                kind, w = filters[fl[at]]
                # a filter the compiler does not cover: the bitmap every other search builds for it, into the table
                words = self._where_bits(w) if kind[0] == "slow" else alive
                if words is None:
                    vis[at].fill_(-1)          # every row; bits at and past n are ignored by the scan
                else:
                    m = min(W, words.numel())
                    vis[at, :m].copy_(words[:m])
            return vis, {f: at for at, f in enumerate(fl)}

        # chunks of queries, equal filters next to each other: at most the table budget of facet slots and at most
        # MMRAG_FILTER_BITMAP_BYTES of bitmaps each
        order = sorted(range(B), key=lambda b: of_query[b])
        max_q = max(1, budget // (4 * slots)) if slots else B
        max_f = max(1, int(settings.MMRAG_FILTER_BITMAP_BYTES) // max(4 * W, 1)) if masked else len(filters)
        chunks: List[List[int]] = []
        cur: List[int] = []
        cur_f: set = set()
        for b in order:
            if cur and (len(cur) >= max_q or (of_query[b] not in cur_f and len(cur_f) >= max_f)):
                chunks.append(cur)
                cur, cur_f = [], set()
            cur.append(b)
            cur_f.add(of_query[b])
        if cur:
            chunks.append(cur)

        rows = self._full
        q = self._pack_plane_queries(qf) if self._plane is not None else self._pack_queries(qf, check_norm=False)
        thr_dev = torch.from_numpy(thr).to(self.device)
        counts = torch.zeros(B, dtype=torch.int64, device=self.device)
        tables = torch.zeros((B, slots), dtype=torch.int64, device=self.device)
        scores = torch.full((B, limit), float("-inf"), dtype=torch.float32, device=self.device)
        rows_o = torch.full((B, limit), -1, dtype=torch.int64, device=self.device)
        for mine in chunks:
            whole = mine == list(range(B))
            pick = None if whole else torch.tensor(mine, device=self.device)
            vis, foq = None, None
            if masked:
                vis, at = bitmaps(sorted({of_query[b] for b in mine}))
                foq = [at[of_query[b]] for b in mine]
            need = _native.range_scan_workspace_bytes(len(mine), self._n, limit, slots)
            cc, ff, ss, rr = _native.range_scan(
                q if whole else q[pick].contiguous(), rows, self._n, self.dim,
                thr_dev if whole else thr_dev[pick].contiguous(), limit, cols, sizes, filter_of_query=foq, vis_bits=vis,
                workspace=self._workspace("_range_ws", need))
            if whole:
                counts = cc.to(torch.int64)
                if ff is not None:
                    tables = ff.to(torch.int64)
                if limit:
                    scores, rows_o = ss, rr
                break
            counts[pick] = cc.to(torch.int64)
            if ff is not None:
                tables[pick] = ff.to(torch.int64)
            if limit:
                scores[pick], rows_o[pick] = ss, rr
        per_key, lo = [], 0
        for g in sizes:
            per_key.append(tables[:, lo:lo + g + 1])
            lo += g + 1
        return counts, per_key, scores, rows_o, values

    def range_search(self, query_embeddings, threshold, limit: int = 100, wheres=None, facets=()):
        """Raw device range search (csrc/range.hip, include/mmrag.h mmrag_range_scan, where the definitions are): not the
        best k but EVERYTHING at or above a score.  For query b: how many of the live rows that match wheres[b] score
        >= threshold[b], how those rows spread over the values of each metadata key in `facets`, and the `limit` best
        of them -- counted inside one exact scan, the [B, n] scores never written.  `threshold`: one float or one per
        query (a cosine for unit rows).  `limit`: 0..MAX_K_DEEP; 0 = counts and facets only, with no host
        synchronisation.  `wheres`: as filtered_search's; a filter the compiler does not cover gets no slow path, its
        bitmap is built as every other search builds it and copied into the table, so one scan serves every filter.
        `facets`: at most MAX_FACET_COLUMNS metadata keys, each through enable_grouping(key)'s column and value table
        (built on first use, kept current by add and compact).

        Returns (counts [B] int64, one [B, G + 1] int64 table per key: slot g = ordinal g, slot G = rows without the key,
        scores [B, limit] float32 desc, rows [B, limit] int64 with -1 = none, one host table ordinal -> value per key);
        tensors on the device.  A float8_e4m3fn collection scans its re-scoring plane (capacity mode raises ValueError).
        A batch whose facet tables (4 bytes per query and slot) exceed MMRAG_RANGE_TABLE_BYTES runs as scans of fewer
        queries, which is exact; one query that exceeds it alone raises ValueError."""
        with self._lock:
            return self._launch_range(query_embeddings, threshold, limit, wheres, facets)

    @staticmethod
    def _facet_lists(table, values) -> List[List[Dict[str, Any]]]:
        """a host [B, G + 1] count table as, per query, [{"value", "count"}] of its non-zero slots: count descending,
        then first appearance; the last slot (rows without the key) has the value None"""
        out = []
        for row in np.asarray(table):
            nz = np.nonzero(row)[0]
            nz = nz[np.argsort(-row[nz], kind="stable")]
            out.append([{"value": values[g] if g < len(values) else None, "count": int(row[g])} for g in nz.tolist()])
        return out

    def range_query(self, query_embeddings, threshold, limit: int = 100, wheres=None, facets=(),
                    include: Sequence[str] = ("metadatas", "documents", "distances"),
                    check_norm: bool = True) -> Dict[str, Any]:
        """query() for a range search (see range_search): the Chroma-shaped dict of query() for the `limit` best rows
        at or above the cosine `threshold` in [-1, 1], plus per query "total" (how many rows pass), "truncated" (total >
        limit) and "facets": {key: [{"value": v, "count": c}, ...]} over ALL passing rows, non-zero slots only, count
        descending then first appearance, rows without the key as "value": None."""
        t = np.asarray(threshold, dtype=np.float64).reshape(-1)
        if not t.size or not bool(((t >= -1.0) & (t <= 1.0)).all()):      # false for NaN too
            raise ValueError(f"threshold must be a cosine in [-1, 1] (got {threshold!r})")
        facets = [facets] if isinstance(facets, str) else list(facets)
        with self._lock, stage("search"):
            counts, per_key, scores, rows, values = self._launch_range(query_embeddings, threshold, limit, wheres,
                                                                       facets, check_norm)
            tables = self._tables()
            emb_src = self._full if "embeddings" in include else None
        with stage("collect"):
            out = self._collect(scores, rows, include, *tables, emb_src)
            totals = counts.cpu().tolist()
            out["total"] = totals
            out["truncated"] = [c > int(limit) for c in totals]
            lists = [self._facet_lists(tab.cpu().numpy(), vals) for tab, vals in zip(per_key, values)]
            out["facets"] = [{key: lists[i][b] for i, key in enumerate(facets)} for b in range(len(totals))]
            return out

    # ------------------------------------------------------------------ related documents (set-to-document) ----
    def _launch_related(self, sets, n_results: int, key: str, threshold, exclude, where, check_norm: bool = True):
        """enqueue the related-groups scan (caller holds the lock): (the five device tensors of
        _native.related_groups, the sets' offsets, each column's item: the stored row of a {"value": v} set or the
        index inside a set of vectors, the threshold used)"""
        from .config import settings

        self._need_plane("related_query")
        k = int(n_results)
        if not 1 <= k <= _native.MAX_K_DEEP:
            raise ValueError(f"n_results must be in 1..{_native.MAX_K_DEEP} for a related search")
        t = self._join_threshold(settings.MMRAG_DEDUP_REPORT_THRESHOLD if threshold is None else threshold,
                                 "threshold")
        sets = list(sets)
        if not 1 <= len(sets) <= _native.MAX_RELATED_SETS:
            raise ValueError(f"sets must hold 1..{_native.MAX_RELATED_SETS} entries")
        if exclude is not None and len(list(exclude)) != len(sets):
            raise ValueError(f"exclude holds {len(list(exclude))} entries for {len(sets)} sets")
        st = self.enable_grouping(key)
        ordinal = st["ordinal"]

        def ordinal_of(v):
            try:
                return ordinal.get(v)
            except TypeError:        # unhashable: no row has it as its key
                return None

        parts, off, items, excl = [], [0], [], []
        for i, entry in enumerate(sets):
            if isinstance(entry, dict):
                if set(entry) != {"value"}:
                    raise ValueError(f'sets[{i}]: a dict entry is {{"value": v}}')
                o = ordinal_of(entry["value"])
                rows = self._rows_where({key: entry["value"]}) if o is not None else np.zeros(0, dtype=np.int64)
                if not rows.size:
                    raise ValueError(f"sets[{i}]: no stored row has {key}={entry['value']!r}")
                parts.append(rows)
                items += rows.tolist()
                own = o
            else:
                qf = self._to_device_f32(entry, f"sets[{i}]", check_norm)
                parts.append(qf)
                items += list(range(qf.shape[0]))
                own = None
            if exclude is not None:
                v = list(exclude)[i]
                own = ordinal_of(v) if v is not None else None
            excl.append(-1 if own is None else own)
            off.append(len(items))
        M = off[-1]
        if M > _native.MAX_RELATED_ROWS:
            raise ValueError(f"the sets hold {M} vectors, at most {_native.MAX_RELATED_ROWS} per call")
        full = self._full
        packed = torch.empty((max(M, 1), full.shape[1]), dtype=full.dtype, device=self.device)
        for c0, part in zip(off, parts):
            if isinstance(part, np.ndarray):     # stored rows, gathered on the device in row order
                _native.gather_rows(packed[c0: c0 + part.size], full, torch.from_numpy(part).to(self.device))
            elif part.shape[0]:
                _native.append_rows(packed, c0, part, self.dim)
        out = _native.related_groups(packed[:M], off, full, self._n, self.dim, k, st["col"], len(st["values"]), t,
                                     exclude=excl, alive_bits=self._where_bits(where))
        return out, off, items, t

    def related_search(self, sets, n_results: int, key: str = "doc_id", threshold: Optional[float] = None,
                       exclude=None, where: Optional[Dict[str, Any]] = None):
        """Raw device set-to-document similarity (csrc/related.hip, include/mmrag.h mmrag_related_groups, where the
        definition is): for each entry of `sets` -- a [m, dim] array of unit vectors, or {"value": v} = the live stored
        rows whose metadata `key` is v, gathered on the device in row order -- the n_results stored documents (distinct
        values of `key`) of highest
            similarity = mean over the set's vectors a of  max over the document's live rows r of cos(a, x_r),
        formed inside ONE exact scan of the collection, with covered = the number of the set's vectors whose best
        match in the document is >= threshold (default MMRAG_DEDUP_REPORT_THRESHOLD, "the same passage").  Returns
        device tensors (similarity [S, k] float32 desc, group ordinals [S, k] int32, covered [S, k] int32,
        best [M, k] float32, best_row [M, k] int64: each vector's best match in each winner of its set),
        (-inf, -1, 0, -inf, -1) padded; ordinal o is enable_grouping(key)["values"][o].  No host synchronisation on the
        kernels' path.

        `exclude`: one key value (or None) per set that is no candidate of it; by default a {"value": v} set excludes v
        itself and a set of vectors nothing.  An unknown v raises ValueError.  `where` narrows the candidate rows;
        tombstones are honoured; rows without the key belong to no document.  A float8_e4m3fn collection is compared on
        its re-scoring plane (capacity mode raises ValueError).  At most MAX_RELATED_SETS sets and MAX_RELATED_ROWS
        vectors per call.  One direction only: how much of the SET a document holds, not how much of the document the
        set holds."""
        with self._lock:
            return self._launch_related(sets, n_results, key, threshold, exclude, where)[0]

    def related_query(self, sets, n_results: int = 5, key: str = "doc_id", threshold: Optional[float] = None,
                      exclude=None, where: Optional[Dict[str, Any]] = None,
                      include: Sequence[str] = ("metadatas", "documents"), check_norm: bool = True) -> List[List[Dict]]:
        """related_search as host lists: per set, its related documents in rank order, each
            {"key": value, "similarity", "coverage": covered / m, "matched": covered, "rows_in_group": live rows,
             "pairs": [{"item": the id of the set's stored row, or the vector's index, "match_id", "score"}, ...]}
        with one pair per vector of the set, in set order; "documents" / "metadatas" in `include` add the matched
        row's "match_document" / "match_metadata" to each pair."""
        sets = list(sets)
        with self._lock, stage("search"):
            out, off, items, _ = self._launch_related(sets, n_results, key, threshold, exclude, where, check_norm)
            tables = self._tables()
            values = self._groups[key]["values"]
            by_value = [isinstance(e, dict) for e in sets]
            sim, grp, cov, best, best_row = (t.cpu() for t in out)       # the call's host synchronisation
            live = {o: int(self._rows_where({key: values[o]}).size) for o in set(grp.flatten().tolist()) if o >= 0}
        with stage("collect"):
            ids_t, docs_t, metas_t = tables
            sim_l, grp_l, cov_l, best_l, row_l = sim.tolist(), grp.tolist(), cov.tolist(), best.tolist(), best_row.tolist()
            res = []
            for s, stored in enumerate(by_value):
                lo, hi = off[s], off[s + 1]
                found = []
                for j, o in enumerate(grp_l[s]):
                    if o < 0:
                        break
                    pairs = []
                    for a in range(lo, hi):
                        r = row_l[a][j]
                        pair = {"item": ids_t[items[a]] if stored else items[a], "match_id": ids_t[r],
                                "score": best_l[a][j]}
                        if "documents" in include:
                            pair["match_document"] = docs_t[r]
                        if "metadatas" in include:
                            pair["match_metadata"] = dict(metas_t[r])
                        pairs.append(pair)
                    found.append({"key": values[o], "similarity": sim_l[s][j], "coverage": cov_l[s][j] / (hi - lo),
                                  "matched": cov_l[s][j], "rows_in_group": live[o], "pairs": pairs})
                res.append(found)
            return res

    # ------------------------------------------------------------------ score priors (boosted retrieval) ----
    MAX_SPEC_COLUMNS = 4

    def _map_prior_columns(self, f: Callable[[torch.Tensor], torch.Tensor]):
        """every prior column through f (capacity growth, compaction; caller holds the lock)"""
        for name, p in self._priors.items():
            if isinstance(p, torch.Tensor):
                self._priors[name] = f(p)
        for st in self._spec_cols.values():
            st["col"] = f(st["col"])

    def row_times(self) -> np.ndarray:
        """when each LIVE row was added (float64 UNIX times, NaN = unknown), in row order"""
        with self._lock:
            t = self._added_at[: self._n]
            return t[~self._is_dead(np.arange(self._n, dtype=np.int64))].copy() if self._n_dead else t.copy()

    def set_prior(self, name: str = "default", values=None, spec: Optional[BoostSpec] = None):
        """Name a score prior for boosted_search: either `values`, the caller's own finite numbers (pins, click counts),
        one per live row in row order -- rows added later get 0.0 until it is set again -- or a BoostSpec, whose column
        is built from the rows' add times and metadata when a search first needs it and kept current from then on.
        Columns are float32 on the device, follow add / growth / compact like the group columns, are dropped by reset()
        and are not persisted."""
        if (values is None) == (spec is None):
            raise ValueError("set_prior takes exactly one of values and spec")
        if spec is not None and not isinstance(spec, BoostSpec):
            raise ValueError("spec must be a BoostSpec")
        with self._lock:
            if spec is not None:
                self._priors[name] = spec
                return
            vals = check_prior_values(values, self.count())
            col = np.zeros(self._matrix.shape[0], dtype=np.float32)
            if self._n_dead:
                col[np.nonzero(~self._is_dead(np.arange(self._n, dtype=np.int64)))[0]] = vals
            else:
                col[: self._n] = vals
            self._priors[name] = torch.from_numpy(col).to(self.device)

    def _spec_column(self, spec: BoostSpec) -> torch.Tensor:
        """the device column of a spec at its (floored) now, from the cache or built as one numpy expression and one
        upload (caller holds the lock)"""
        key = spec.cache_key()
        st = self._spec_cols.get(key)
        if st is None:
            col = np.zeros(self._matrix.shape[0], dtype=np.float32)
            col[: self._n] = spec.column(self._added_at[: self._n], self._metadatas, key[1])
            st = {"spec": spec, "now": key[1], "col": torch.from_numpy(col).to(self.device)}
            self._spec_cols[key] = st
            while len(self._spec_cols) > self.MAX_SPEC_COLUMNS:
                self._spec_cols.popitem(last=False)
        return st["col"]

    def _prior_column(self, prior) -> torch.Tensor:
        if isinstance(prior, BoostSpec):
            return self._spec_column(prior)
        p = self._priors.get(prior) if isinstance(prior, str) else None
        if p is None:
            raise ValueError(f"unknown prior {prior!r}: name one with set_prior, or pass a BoostSpec")
        return self._spec_column(p) if isinstance(p, BoostSpec) else p

    def _launch_boosted(self, query_embeddings, n_results: int, prior, weight, where, check_norm: bool = True):
        """enqueue the boosted search (caller holds the lock): device (scores, rows, boosts, packed queries), no host
        sync unless the collection is larger than a query's candidate slots"""
        self._need_plane("boosted_query")
        k = int(n_results)
        if not 1 <= k <= _native.MAX_K_DEEP:
            raise ValueError(f"n_results must be in 1..{_native.MAX_K_DEEP} for a boosted search")
        col = self._prior_column(prior)
        qf = self._to_device_f32(query_embeddings, "query", check_norm)     # converted and norm-checked once
        q = self._pack_plane_queries(qf) if self._plane is not None else self._pack_queries(qf, check_norm=False)
        B = q.shape[0]
        w = np.asarray(weight, dtype=np.float64).reshape(-1)
        if w.size == 1:
            w = np.full(B, float(w[0]))
        if w.size != B:
            raise ValueError(f"weight holds {w.size} entries for {B} queries")
        need = _native.boosted_topk_workspace_bytes(B, self._n, k)
        scores, rows, boosts = _native.boosted_topk(
            q, self._full, self._n, self.dim, k, col, w, alive_bits=self._where_bits(where),
            workspace=self._workspace("_boosted_ws", need))
        return scores, rows, boosts, q

    def boosted_search(self, query_embeddings, n_results: int, prior="default", weight=1.0,
                       where: Optional[Dict[str, Any]] = None):
        """Raw device search ranked by cos(q_b, x_r) + weight_b * prior[r] (csrc/boosted.hip, include/mmrag.h
        mmrag_boosted_topk): the prior is applied INSIDE one exact scan, so a row with a large prior and a middling cosine
        is found although it is in no cosine top-k -- re-sorting a finished list cannot do that.  `prior`: a name given
        to set_prior, or a BoostSpec; `weight`: a number, or one per query.  Returns (scores [B, k] float32 = the final
        scores descending, rows [B, k] int64, -1 = none, boosts [B, k] float32 = weight * prior of each hit), n_results
        up to MAX_K_DEEP.  `where` narrows the batch and tombstones are honoured; a float8_e4m3fn collection is searched
        on its re-scoring plane (capacity mode raises ValueError)."""
        with self._lock:
            return self._launch_boosted(query_embeddings, n_results, prior, weight, where)[:3]

    def boosted_query(self, query_embeddings, n_results: int = 10, prior="default", weight=1.0,
                      where: Optional[Dict[str, Any]] = None,
                      include: Sequence[str] = ("metadatas", "documents", "distances"),
                      check_norm: bool = True) -> Dict[str, Any]:
        """query() ranked by boosted_search: the Chroma-shaped dict of query() plus `scores` (the final scores, descending)
        and `boosts` (weight * prior of each hit).  `distances` stay 1 - cosine -- the hits' own cosines, computed from
        the stored rows -- and are therefore NOT ascending."""
        from .lexical import rows_dot

        with self._lock, stage("search"):
            scores, rows, boosts, q = self._launch_boosted(query_embeddings, n_results, prior, weight, where, check_norm)
            B, k = rows.shape
            flat = rows.reshape(-1)
            qi = torch.arange(B, device=self.device, dtype=torch.int32).repeat_interleave(k)
            cos = rows_dot(q, self._full, self.dim, qi, flat.clamp(min=0)).view(B, k)    # padding: row 0, cut below
            tables = self._tables()
            emb_src = self._full if "embeddings" in include else None
        with stage("collect"):
            want = tuple(include) if "distances" in include else tuple(include) + ("distances",)
            out = self._collect(cos, rows, want, *tables, emb_src)
            lens = [len(ids) for ids in out["ids"]]
            if "distances" not in include:
                out["distances"] = None
            out["scores"] = [row[:m] for row, m in zip(scores.cpu().tolist(), lens)]
            out["boosts"] = [row[:m] for row, m in zip(boosts.cpu().tolist(), lens)]
            return out

    # ------------------------------------------------------------------ recommend (positive / negative examples) ----
    @staticmethod
    def _example_lists(positive, negative):
        """`positive` / `negative` of recommend_search: one list of entries per request, as lists.  ValueError for
        anything else: an id or a vector where a request's list belongs is not guessed at"""
        def per_request(x, what):
            if x is None or isinstance(x, (str, np.ndarray, torch.Tensor)) or not hasattr(x, "__iter__"):
                raise ValueError(f"recommend: `{what}` takes one list of ids and vectors per request")
            return list(x)

        pos = [per_request(x, "positive") for x in per_request(positive, "positive")]
        if negative is None:
            return pos, [[] for _ in pos]
        return pos, [[] if x is None else per_request(x, "negative") for x in per_request(negative, "negative")]

    def _launch_recommend(self, positive, negative, n_results: int, negative_weight, where, extra_depth: bool):
        """enqueue the recommend search (caller holds the lock): (the six device tensors of recommend_topk, the
        requests' positive and negative entries with ids replaced by their int rows, the weights float32 [R]).
        `extra_depth`: search n_results + the largest number of stored rows one request names, capped by MAX_K_DEEP"""
        from .config import settings

        self._need_plane("recommend_query")
        k = int(n_results)
        if not 1 <= k <= _native.MAX_K_DEEP:
            raise ValueError(f"n_results must be in 1..{_native.MAX_K_DEEP} for a recommend search")
        pos, neg = self._example_lists(positive, negative)
        if not pos:
            raise ValueError("recommend: no request")
        if len(neg) != len(pos):
            raise ValueError(f"recommend: {len(neg)} negative lists for {len(pos)} requests")

        def resolve(entries):
            out = []
            for e in entries or []:
                if isinstance(e, str):
                    r = self._row_of.get(e)      # live rows only: a delete drops the id from the map
                    if r is None:
                        raise ValueError(f"recommend: no stored item has the id {e!r}")
                    out.append(int(r))
                elif isinstance(e, (int, np.integer)) or np.ndim(e) != 1:
                    # (a row number would reach pack_examples' gather without the tombstone check above)
                    raise ValueError("recommend: an example is a vector or the id of a stored item")
                else:
                    out.append(e)
            return out

        pos_r, neg_r = [resolve(x) for x in pos], [resolve(x) for x in neg]
        examples, sign = _native.pack_examples(pos_r, neg_r, self.dim, self._full.dtype, self.device, rows=self._full)
        R = len(pos_r)
        w = settings.MMRAG_RECOMMEND_NEGATIVE_WEIGHT if negative_weight is None else negative_weight
        _, w = _native.check_recommend_request("recommend", None, w, R)
        if extra_depth:
            named = max(sum(isinstance(e, int) for e in p_ + n_) for p_, n_ in zip(pos_r, neg_r))
            k = min(k + named, _native.MAX_K_DEEP)
        need = _native.recommend_topk_workspace_bytes(R, self._n, k)
        out = _native.recommend_topk(examples, sign, w, self._full, self._n, self.dim, k, checked=True,
                                     alive_bits=self._where_bits(where),
                                     workspace=self._workspace("_recommend_ws", need))
        return out, pos_r, neg_r, w

    def recommend_search(self, positive, negative=None, n_results: int = 10, negative_weight=None,
                         where: Optional[Dict[str, Any]] = None):
        """Raw device search by examples, "more like these, less like those" (csrc/recommend.hip, include/mmrag.h
        mmrag_recommend_topk): `positive` / `negative` hold one list per request,
        each entry a unit vector or the id of a stored row, at most 16 per request and at least one positive.  A row x
        scores final = pos - w * max(neg, 0), pos / neg the largest cosine to a positive / negative example, formed
        INSIDE one exact scan: with negatives the winners are often far down the positive ranking, which no re-sort of
        a finished list finds.  Stored rows are gathered on the device.  Returns (scores [R, k] float32 = final
        descending, rows [R, k] int64, -1 = none, pos, neg [R, k] float32, pos_slot, neg_slot [R, k] int32: the
        request's example that gave them, positives counted first, -1 = none).  The examples themselves are NOT
        excluded here (recommend_query does that).  `negative_weight`: w, a number or one per request, default
        MMRAG_RECOMMEND_NEGATIVE_WEIGHT.  `where` narrows the batch and tombstones are honoured; a float8_e4m3fn
        collection is searched on its re-scoring plane (capacity mode raises ValueError); an unknown or deleted id
        raises ValueError."""
        with self._lock:
            return self._launch_recommend(positive, negative, n_results, negative_weight, where, False)[0]

    def recommend_query(self, positive, negative=None, n_results: int = 10, negative_weight=None,
                        where: Optional[Dict[str, Any]] = None,
                        include: Sequence[str] = ("metadatas", "documents", "distances"),
                        exclude_examples: bool = True) -> Dict[str, Any]:
        """query() ranked by recommend_search: the Chroma-shaped dict of query() plus `scores` (the finals, descending),
        `penalties` (w * max(neg, 0)), `matched` (per hit, the positive example that scored best: the stored id, or
        "vector:<i>" for entry i of the request's positives) and `repelled_by` (the same for the negatives, None when
        none fired).  `distances` are 1 - pos and therefore NOT ascending.  With `exclude_examples` the stored rows a
        request names are not returned: the search goes n_results + their number deep (at most MAX_K_DEEP) and they are
        dropped on the host, as get_similar_documents drops its source."""
        with self._lock, stage("search"):
            out_dev, pos_r, neg_r, w = self._launch_recommend(positive, negative, n_results, negative_weight, where,
                                                              exclude_examples)
            tables = self._tables()
            emb_src = self._full if "embeddings" in include else None
        with stage("collect"):
            scores, rows, p_dot, n_dot, p_arg, n_arg = [t.cpu().tolist() for t in out_dev]
            keys = ("ids", "distances", "metadatas", "documents", "embeddings")
            out: Dict[str, Any] = {key: [] if key == "ids" or key in include else None for key in keys}
            out.update(scores=[], penalties=[], matched=[], repelled_by=[])

            def name(entries, slot):
                e = entries[slot]
                return tables[0][e] if isinstance(e, int) else f"vector:{slot}"

            for g, (p_ent, n_ent) in enumerate(zip(pos_r, neg_r)):
                named = {e for e in p_ent + n_ent if isinstance(e, int)} if exclude_examples else set()
                keep = [j for j, r in enumerate(rows[g]) if r >= 0 and r not in named][: int(n_results)]
                hit = [rows[g][j] for j in keep]
                self._append_hits(out, tables, hit, include)
                if out["distances"] is not None:
                    out["distances"].append([1.0 - p_dot[g][j] for j in keep])
                if out["embeddings"] is not None:
                    out["embeddings"].append(self._fetch(hit, emb_src))
                out["scores"].append([scores[g][j] for j in keep])
                out["penalties"].append([float(w[g]) * max(n_dot[g][j], 0.0) for j in keep])
                out["matched"].append([name(p_ent, p_arg[g][j]) for j in keep])
                out["repelled_by"].append([name(n_ent, n_arg[g][j] - len(p_ent))
                                           if n_arg[g][j] >= 0 and n_dot[g][j] > 0 else None for j in keep])
            return out

    # ------------------------------------------------------------------ multi-query fusion ----
    def _launch_fused(self, query_embeddings, list_off, n_results: int, fetch_k, weights, method, where,
                      check_norm: bool = True):
        """enqueue ONE search over all the variants' rows and the fusion of their lists, on one stream (caller holds
        the lock): the six device tensors of _native.fuse_select, no host sync of its own"""
        from .config import settings

        n = int(n_results)
        if not 1 <= n <= _native.MAX_FUSE_RESULTS:
            raise ValueError(f"n_results must be in 1..{_native.MAX_FUSE_RESULTS} for multi-query fusion")
        C = max(n, int(settings.MMRAG_FUSE_CANDIDATES)) if fetch_k is None else int(fetch_k)
        if C < 1:
            raise ValueError("fetch_k must be >= 1")
        C = min(C, _native.MAX_FUSE_CANDIDATES)
        method = str(settings.MMRAG_FUSE_METHOD if method is None else method).lower()
        if method not in _native.FUSE_METHODS:
            raise ValueError(f"fusion method must be one of {sorted(_native.FUSE_METHODS)} (got {method!r})")
        # everything the fuse launch needs is on its way to the device BEFORE the scan is enqueued (offsets and weights
        # through pinned memory), so nothing between the scan and the fuse launch can make the host wait for the stream
        qf = self._to_device_f32(query_embeddings, "query", check_norm)     # converted and norm-checked once
        L = int(qf.shape[0])
        try:
            off_dev = _native.fuse_offsets(list_off, L, self.device)        # the one check of list_off
        except _native.MMRagNativeError as e:
            raise ValueError(str(e)) from None
        w = None
        if weights is not None:
            w = np.asarray(weights, dtype=np.float32).reshape(-1)
            if w.size != L or not np.isfinite(w).all():
                raise ValueError(f"weights must be {L} finite numbers, one per query variant")
            w = _native._pinned_to_device(torch.from_numpy(w), self.device)
        scores, rows = self._launch_search(qf, C, where, check_norm=False)
        return _native.fuse_select(scores.contiguous(), rows.contiguous(), off_dev, n, weights=w, method=method,
                                   rrf_k=int(settings.MMRAG_FUSE_RRF_K))

    def fused_search(self, query_embeddings, list_off, n_results: int, fetch_k: Optional[int] = None,
                     weights=None, method: Optional[str] = None, where: Optional[Dict[str, Any]] = None):
        """Raw multi-query search: the L rows of query_embeddings are phrasings ("variants") of G questions, question g
        owning rows list_off[g] .. list_off[g + 1] - 1 (ascending from 0 to L, at most 16 each, none allowed).  ONE
        search() call answers all L rows at depth fetch_k, then one launch (csrc/fuse.hip, include/mmrag.h
        mmrag_fuse_select, where the definition is) fuses each question's lists on the same stream.  Returns device
        tensors (fused scores [G, n] float32 descending, rows [G, n] int64, best [G, n] float32 = a row's largest cosine
        over the variants, best variant [G, n] int32 local to the question, count [G, n] int32 variants that returned
        the row, info [G, 2] int32 = (distinct rows, valid entries)), unused slots (-inf, -1, -inf, -1, 0).

        fetch_k defaults to max(n_results, MMRAG_FUSE_CANDIDATES) and is capped at 256; depths above 20 take the deep
        search as in search().  method: "rrf" (sum of weight / (MMRAG_FUSE_RRF_K + rank), the default
        MMRAG_FUSE_METHOD) or "max" (largest weight * cosine); weights: one per row, default 1.0.  The lists are
        search()'s: tombstones and `where` are honoured, a float8_e4m3fn collection is re-scored on its plane (in
        capacity mode the scores are the quantised collection's own)."""
        with self._lock:
            return self._launch_fused(query_embeddings, list_off, n_results, fetch_k, weights, method, where)

    def fused_query(self, query_embeddings, list_off, n_results: int = 10, fetch_k: Optional[int] = None,
                    weights=None, method: Optional[str] = None, where: Optional[Dict[str, Any]] = None,
                    include: Sequence[str] = ("metadatas", "documents", "distances"),
                    check_norm: bool = True) -> Dict[str, Any]:
        """query() over several phrasings of each question (see fused_search): one Chroma-shaped dict with one entry
        per QUESTION, in fused order, plus `fused_scores`, `matched_queries` (how many variants returned the hit) and
        `best_query` (the variant, local to the question, that scored it best).  `distances` are 1 - the best cosine
        over the variants, so they are NOT ascending."""
        with self._lock, stage("search"):
            fused, rows, best, best_list, count, _ = self._launch_fused(query_embeddings, list_off, n_results, fetch_k,
                                                                        weights, method, where, check_norm)
            tables = self._tables()
            emb_src = self._full if "embeddings" in include else None
        with stage("collect"):
            out = self._collect(best, rows, include, *tables, emb_src)
            for key, t in (("fused_scores", fused), ("matched_queries", count), ("best_query", best_list)):
                out[key] = [vals[: len(ids)] for vals, ids in zip(t.cpu().tolist(), out["ids"])]
            return out

    # ------------------------------------------------------------------ token store / late retrieval ----
    def enable_token_store(self, dim: int, max_doc_tokens: int, max_bytes: Optional[int] = None,
                           dtype: Optional[str] = None):
        """Attach the token store (late_store.TokenStore): a device fp16 plane [tokens, dim] of the stored chunks' token
        rows, item i being row i, with the `max_doc_tokens` its rows were trimmed to.  Rows keep no tokens until
        set_tokens names them.  delete needs nothing (the alive bitmap is over rows, i.e. items); compact and reset keep
        the store in step.  `max_bytes` (default MMRAG_LATE_STORE_MAX_BYTES; 0 = no cap): past it new rows keep no
        tokens.  `dtype` (default MMRAG_LATE_STORE_DTYPE): "float16", or "float8_e4m3fn" for a plane of E4M3 codes,
        one byte per element, scored by the FP8 MaxSim kernels.  Idempotent for the same (dim, max_doc_tokens, dtype)."""
        from .config import settings
        from .late_store import TokenStore

        with self._lock:
            if self._tokens is not None:
                if (self._tokens.dim, self._tokens.max_doc_tokens) != (int(dim), int(max_doc_tokens)):
                    raise ValueError(f"this collection's token store holds dim {self._tokens.dim}, max_doc_tokens "
                                     f"{self._tokens.max_doc_tokens}; reset it before changing them")
                if dtype is not None and dtype != self._tokens.dtype:
                    raise ValueError(f"this collection's token store holds {self._tokens.dtype} rows; reset it before "
                                     f"changing the dtype to {dtype}")
                return self._tokens
            cap = settings.MMRAG_LATE_STORE_MAX_BYTES if max_bytes is None else int(max_bytes)
            self._tokens = TokenStore(dim, max_doc_tokens, device=self.device, max_bytes=cap,
                                      dtype=settings.late_store_dtype() if dtype is None else dtype)
            return self._tokens

    @property
    def token_store(self):
        """the late_store.TokenStore, or None before enable_token_store()"""
        return self._tokens

    def _need_tokens(self, what: str):
        if self._tokens is None:
            raise ValueError(f"{what} needs the token store: call enable_token_store() (EmbeddingManager: "
                             f"MMRAG_LATE_STORE=1 or enable_late_store())")
        return self._tokens

    def rows_of_ids(self, ids: Sequence[str]) -> List[int]:
        """the live row of each id, -1 for an id no live row has"""
        with self._lock:
            return [self._row_of.get(i, -1) for i in ids]

    def set_tokens(self, rows: Sequence[int], token_rows, lens: Sequence[int], token_ids=None):
        """Store the token rows of index rows `rows` (TokenStore.set_tokens): row rows[j] gets the next lens[j] rows of
        `token_rows` [sum(lens), dim] (a device or host fp16 array), `token_ids[j]` its token ids for `explain`."""
        with self._lock:
            st = self._need_tokens("set_tokens")
            rows = [int(r) for r in rows]
            if any(not 0 <= r < self._n for r in rows):
                raise ValueError(f"set_tokens: a row outside the {self._n} rows in use")
            st.set_tokens(rows, token_rows, lens, token_ids)

    def ids_without_tokens(self, ids: Sequence[str]) -> List[str]:
        """the ids, in order, that have a live row which keeps no tokens (what an ingest still has to encode)"""
        with self._lock:
            st = self._need_tokens("ids_without_tokens")
            return [i for i in ids if i in self._row_of and st.length(self._row_of[i]) == 0]

    def set_tokens_for_ids(self, ids: Sequence[str], token_rows, lens: Sequence[int], token_ids=None,
                           only_empty: bool = True) -> int:
        """set_tokens by id, resolved and written under ONE lock: rows are renumbered by a compaction, so a row number
        looked up before an encoder forward may name another document after it.  ids[j] owns the next lens[j] rows of
        `token_rows`.  An id without a live row by now (deleted, the collection reset) is dropped with its rows, and --
        `only_empty` -- so is one whose row already keeps tokens: the tokens under a row are those of the document
        under it (add() ignores an id that exists, so its new text is not what is stored).  Returns the ids written."""
        with self._lock:
            st = self._need_tokens("set_tokens_for_ids")
            lens = [int(n) for n in lens]
            if len(lens) != len(ids) or (token_ids is not None and len(token_ids) != len(ids)):
                raise ValueError(f"set_tokens_for_ids: {len(ids)} ids for {len(lens)} lengths")
            rows = [self._row_of.get(i, -1) for i in ids]
            keep, seen = [], set()
            for j, r in enumerate(rows):
                if r >= 0 and r not in seen and not (only_empty and st.length(r) > 0):
                    seen.add(r)
                    keep.append(j)
            if not keep:
                return 0
            as_codes = False
            if len(keep) != len(ids):
                starts = np.concatenate([[0], np.cumsum(lens)])
                pick = np.concatenate([np.arange(starts[j], starts[j + 1]) for j in keep]).astype(np.int64)
                token_rows = st._take(st._as_rows(token_rows), pick)
                as_codes = st.f8          # an FP8 store: the rows are quantised by now
            st.set_tokens([rows[j] for j in keep], token_rows, [lens[j] for j in keep],
                          None if token_ids is None else [token_ids[j] for j in keep], _codes=as_codes)
            return len(keep)

    def token_spans(self, ids_lists: Sequence[Sequence[str]], with_ids: bool = False):
        """One snapshot, under the lock, of where the token rows of these ids lie: (spans, plane, max_doc_tokens) with,
        per id in order, (first plane row, length, token ids if `with_ids` else None), or None for an id without a live
        row or whose row keeps no tokens.  `plane` is the tensor those rows are in: a later fill or compaction swaps a
        new one in and appends write past the rows a snapshot names, so the snapshot stays valid for a launch that
        follows; its dtype says what the rows are (torch.float16, or torch.uint8 for an FP8 store's code rows).
        (None, None, None) without a token store."""
        with self._lock:
            st = self._tokens
            if st is None:
                return None, None, None
            off = st.offsets()
            spans: List[Any] = []
            for ids in ids_lists:
                for i in ids:
                    r = self._row_of.get(i, -1)
                    n = st.length(r) if r >= 0 else 0
                    spans.append((int(off[r]), n, st.token_ids(r) if with_ids else None) if n > 0 else None)
            return spans, st.plane, st.max_doc_tokens

    def token_stats(self) -> Optional[Dict[str, Any]]:
        with self._lock:
            return None if self._tokens is None else self._tokens.stats()

    def late_search(self, q_tokens: torch.Tensor, q_start, q_len, n_results: int,
                    where: Optional[Dict[str, Any]] = None):
        """First-stage late-interaction retrieval (csrc/maxsim_scan.hip, include/mmrag.h mmrag_maxsim_topk): each
        question's exact MaxSim top-k over the token rows of ALL live stored rows that match `where` -- no pooled-vector
        search before it.  Question s is rows q_start[s] .. q_start[s] + q_len[s] of the device fp16 tensor `q_tokens`
        [rows, dim] (unit rows of the encoder that filled the store).  Returns device (scores [Q, k] float32 -- the
        SUM over the question's tokens, descending, ties to the lower row -- and rows [Q, k] int64, -1 = none); a row
        without stored tokens is never returned.  No host synchronisation unless rows_in_use exceeds a question's
        candidate slots."""
        k = int(n_results)
        if not 1 <= k <= _native.MAX_K_DEEP:
            raise ValueError(f"n_results must be in 1..{_native.MAX_K_DEEP} for a late search")
        with self._lock:
            st = self._need_tokens("late_search")
            if q_tokens.dim() != 2 or q_tokens.shape[1] != st.dim:
                raise ValueError(f"late_search: question token rows must be [rows, {st.dim}]")
            bits = self._where_bits(where)
            q_start, q_len = [int(v) for v in q_start], [int(v) for v in q_len]
            tiles = _native.late_question_tiles(q_start, q_len, q_tokens.shape[0])
            need = _native.maxsim_topk_workspace_bytes(len(q_start), self._n, k, st.dim, tiles,
                                                       torch.float8_e4m3fn if st.f8 else torch.float16)
            if self._late_ws is None or _native._nbytes(self._late_ws) < need:
                self._late_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            if st.f8:
                # both operands are codes: the questions' fp16 / fp32 rows are quantised once, here
                q_codes = st._as_rows(q_tokens)
                return _native.maxsim_topk_f8(q_codes, q_start, q_len, st.plane, st.n_rows, st.device_offsets(self._n),
                                              self._n, st.dim, k, alive_bits=bits, workspace=self._late_ws)
            return _native.maxsim_topk(q_tokens, q_start, q_len, st.plane, st.n_rows, st.device_offsets(self._n),
                                       self._n, st.dim, k, alive_bits=bits, workspace=self._late_ws)

    def late_query(self, q_tokens: torch.Tensor, q_start, q_len, n_results: int = 10,
                   where: Optional[Dict[str, Any]] = None,
                   include: Sequence[str] = ("metadatas", "documents", "distances")) -> Dict[str, Any]:
        """late_search as a Chroma-shaped result (the shared result builder): `late_scores` is score / q_len, the mean
        over the question's tokens of each token's best cosine, so it reads like a cosine; `distances` is 1 - that
        (there is no pooled cosine: no pooled search ran)."""
        with self._lock, stage("search"):
            scores, rows = self.late_search(q_tokens, q_start, q_len, n_results, where)
            tables = self._tables()
            emb_src = self._full if "embeddings" in include else None
            q_len_dev = _native._pinned_to_device(torch.as_tensor(q_len, dtype=torch.float32).reshape(-1, 1).cpu(),
                                                  self.device)
            mean = scores / q_len_dev
        with stage("collect"):
            mean_h, rows_h = mean.cpu(), rows.cpu()
            out = self._collect(mean_h, rows_h, include, *tables, emb_src)
            out["late_scores"] = [srow[: len(found)] for srow, found in zip(mean_h.tolist(), out["ids"])]
            return out

    # ------------------------------------------------------------------ lexical / hybrid ----
    def enable_lexical(self):
        """Build the BM25 state (lexical.LexicalIndex) from the stored documents in row order; from then on add,
        add_rows_device, delete, compact and reset keep it current.  Until then they do no lexical work.  Runs by
        itself on the first lexical_query / hybrid_query."""
        with self._lock:
            if self._lex is None:
                from .lexical import LexicalIndex

                lex = LexicalIndex(self.device)
                lex.documents_source = lambda: self._documents[: self._n]    # the positions plane is built from them
                lex.append(self._documents[: self._n])
                if self._n_dead:
                    lex.delete_rows(np.nonzero(self._is_dead(np.arange(self._n, dtype=np.int64)))[0])
                self._lex = lex
            return self._lex

    @property
    def lexical_enabled(self) -> bool:
        return self._lex is not None

    def _lexical_search(self, query_texts: Sequence[str], n_results: int, where, fuzzy=None, phrases=None,
                        slop: int = 0, phrase_mode: str = "require", bitmaps: bool = False):
        """enqueue the BM25 search (caller holds the lock): device (scores, rows), -1 padded, and the corrections
        typo tolerance made (None without `fuzzy`).  With `phrases` two more values: the per-query phrase report and
        (for `bitmaps`, when some query has a phrase) the device bitmaps [B, filter_words(n)] of the rows holding every
        phrase of each query, else None."""
        if isinstance(query_texts, str):
            raise ValueError("query_texts must be a list of strings")
        if n_results < 1 or n_results > _native.MAX_K_DEEP:
            raise ValueError(f"n_results must be in 1..{_native.MAX_K_DEEP} for lexical search")
        lex = self.enable_lexical()
        if phrases:
            scores, rows, corrections, report, info = lex.topk(list(query_texts), n_results, self._where_bits(where),
                                                               fuzzy=fuzzy, phrases=True, slop=slop,
                                                               phrase_mode=phrase_mode, bitmaps=bitmaps)
            return scores, rows, corrections, report, (info["bitmaps"] if info is not None else None)
        got = lex.topk(list(query_texts), n_results, self._where_bits(where), fuzzy=fuzzy)
        return got if len(got) == 3 else got + (None,)

    @property
    def positions_enabled(self) -> bool:
        """True once a phrase query built the lexical leg's positions plane"""
        return self._lex is not None and self._lex.positions_enabled

    def positions_bytes(self) -> int:
        """device bytes of the positions plane (4 per stored token and 8 per posting, with growth room); 0 until a
        phrase query builds it"""
        return self._lex.positions_bytes if self._lex is not None else 0

    def suggest_terms(self, words: Sequence[str], fuzzy="auto", limit: int = 5) -> List[List[Dict[str, Any]]]:
        """"Did you mean": for each word (analysed like a query; its first term counts) up to `limit` (at most 16)
        indexed terms within the edits `fuzzy` allows it, as {"term", "edits", "df"}: fewer edits first, then the
        larger live df, then the term seen first.  Only terms some live row holds are suggested; an indexed word is
        its own first suggestion."""
        from .lexical import FUZZY_MAX_EXPANSIONS, analyze, fuzzy_edits, parse_fuzzy

        if isinstance(words, str):
            raise ValueError("words must be a list of strings")
        if not 1 <= limit <= FUZZY_MAX_EXPANSIONS:
            raise ValueError(f"limit must be in 1..{FUZZY_MAX_EXPANSIONS}")
        mode = parse_fuzzy(fuzzy)
        if mode is None:
            raise ValueError("suggest_terms needs fuzzy: 'auto' or 0..2")
        terms = [(analyze(w) or [""])[0] for w in words]
        with self._lock:
            lex = self.enable_lexical()
            got_t, got_e = lex.fuzzy_terms(terms, [fuzzy_edits(mode, len(t)) for t in terms], limit)
            df = lex.df_host()
            out = []
            for i, t in enumerate(terms):
                ids = [int(x) for x in got_t[i] if x >= 0] if t else []
                out.append([{"term": lex.lexicon.terms(tid, 1)[0], "edits": int(got_e[i, j]), "df": int(df[tid])}
                            for j, tid in enumerate(ids)])
        return out

    # ------------------------------------------------------------------ significant terms ----
    def _group_term_lists(self, group: torch.Tensor, sizes: torch.Tensor, top: int, min_count: int, min_length: int,
                          exclude: Sequence[str]) -> List[List[Dict[str, Any]]]:
        """per group the significant terms of the rows labelled with it (caller holds the lock): LexicalIndex.group_terms
        under label_mask(min_length, exclude), as [{"term", "score", "count", "background" (the live df)}] best first"""
        if not 1 <= int(top) <= _native.MAX_K_DEEP:
            raise ValueError(f"significant terms: top must be in 1..{_native.MAX_K_DEEP} (got {top!r})")
        if int(min_count) < 1 or int(min_length) < 1:
            raise ValueError("significant terms: need min_count >= 1 and min_length >= 1")
        if self._n and not any(self._documents[: self._n]):
            raise ValueError("significant terms need the stored documents: this collection holds none")
        lex = self.enable_lexical()
        scores, terms, counts = lex.group_terms(group, sizes, int(top), int(min_count),
                                                lex.label_mask(min_length, exclude))
        scores_h, terms_h, counts_h = scores.cpu().numpy(), terms.cpu().numpy(), counts.cpu().numpy()
        df = lex.df_host()
        found = np.unique(terms_h[terms_h >= 0])
        known = found[found < len(lex.lexicon)]
        names = {int(t): lex.lexicon.terms(int(t), 1)[0] for t in known.tolist()}
        return [[{"term": names.get(int(t)), "score": float(s), "count": int(c), "background": int(df[t])}
                 for s, t, c in zip(scores_h[g], terms_h[g], counts_h[g]) if t >= 0] for g in range(terms_h.shape[0])]

    def significant_terms(self, where: Optional[Dict[str, Any]] = None, key: Optional[str] = None,
                          values: Optional[Sequence[Any]] = None, labels: Optional[torch.Tensor] = None, top: int = 10,
                          min_count: int = 2, min_length: int = 3, exclude: Sequence[str] = ()) -> List[Dict[str, Any]]:
        """The terms that set groups of rows apart from the rest of the collection (csrc/terms.hip): for every group
        the `top` terms by the JLH score (fgp - bgp) * (fgp / bgp), fgp = the share of the group's rows holding the
        term, bgp = the share of the live rows holding it, among the terms at least `min_count` rows of the group hold,
        of at least `min_length` code points, not digits only and not among the `exclude` words.  Exactly one grouping:
        `where` (one group: the live rows that match), `key` + `values` (one group per value of that metadata key, at
        most 4096 distinct values; a value no live row has gives size 0 and no terms) or `labels` (a device int32
        [rows_in_use]: each row's group 0 .. G-1, or -1 for none; dead rows count for nothing).  Statistics are over the
        live rows.  Builds the lexical index on first use.  Returns [{"group": 0 / the value / the label, "size",
        "terms": [{"term", "score", "count": rows of the group holding it, "background": live rows holding it}]}]."""
        given = (where is not None) + (key is not None or values is not None) + (labels is not None)
        if given != 1 or (key is None) != (values is None):
            raise ValueError("significant_terms takes exactly one of where, key + values and labels")
        with self._lock:
            n, dev = self._n, self.device
            if labels is not None:
                if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.numel() != n:
                    raise ValueError(f"labels must be an int32 device tensor of {n} rows")
                group = labels.to(dev).contiguous()
                if self._n_dead:
                    dead = np.nonzero(self._is_dead(np.arange(n, dtype=np.int64)))[0]
                    group = group.index_fill(0, torch.from_numpy(dead).to(dev), -1)
                G = int(group.max().item()) + 1 if n else 0
                if not 1 <= G <= _native.MAX_TERM_GROUPS:
                    raise ValueError(f"labels must name 1..{_native.MAX_TERM_GROUPS} groups (found {G})")
                sizes = torch.bincount(group.long() + 1, minlength=G + 1)[1:].to(torch.int32)
                names: List[Any] = list(range(G))
            else:
                if key is not None:
                    names = list(values)
                    if isinstance(values, str) or not 1 <= len(names) <= _native.MAX_TERM_GROUPS:
                        raise ValueError(f"values must be a list of 1..{_native.MAX_TERM_GROUPS} values")
                    try:
                        distinct = len(set(names)) == len(names)
                    except TypeError:
                        raise ValueError("values must be hashable") from None
                    if not distinct:
                        raise ValueError("values names a value twice")
                    members = [self._rows_where({key: v}) for v in names]
                else:
                    names, members = [0], [self._rows_where(where)]
                host = np.full(max(n, 1), -1, np.int32)
                for g, rows in enumerate(members):
                    host[rows] = g
                group = torch.from_numpy(host).to(dev)
                sizes = torch.from_numpy(np.asarray([rows.size for rows in members], np.int32)).to(dev)
            lists = self._group_term_lists(group, sizes, top, min_count, min_length, exclude)
            sizes_h = sizes.cpu().tolist()
        return [{"group": name, "size": int(size), "terms": terms} for name, size, terms in zip(names, sizes_h, lists)]

    def lexical_query(self, query_texts: Sequence[str], n_results: int = 10, where: Optional[Dict[str, Any]] = None,
                      include: Sequence[str] = ("metadatas", "documents"), fuzzy=None, phrases=None, slop: int = 0,
                      phrase_mode: str = "require") -> Dict[str, Any]:
        """BM25 search (csrc/lexical.hip): Chroma-shaped lists of lists `ids`, `documents`, `metadatas` and
        `lexical_scores` (descending; ties to the lower row).  Only rows holding at least one query term are returned,
        so a list may be shorter than n_results.  Statistics (N, avgdl, df) are over the live rows; `where` restricts
        the results only.  `fuzzy` ("auto", True or 0..2 edits; csrc/fuzzy.hip): query terms no live row holds are
        replaced by their closest indexed term before scoring, and the result carries `corrections`, per query a list
        of {"term", "matched", "edits"}; corrections are collection-wide like the statistics.  `phrases` (csrc/phrase.hip):
        a segment of the query between two '"' (or between U+201C and U+201D) is a phrase of 1..8 terms, at most 4 per
        query; it occurs in a row where its terms stand in this order with at most `slop` (0..16) other tokens between
        the first and the last, and scores as one more BM25 clause (idf = the sum of its terms' idf, tf = the number of
        starts).  phrase_mode "require" (default): only rows holding every phrase of the query are returned, the terms
        outside the quotes only add score; "prefer": a phrase is an optional clause like a term.  `fuzzy` never rewrites
        a phrase's terms.  The result then carries `phrases`, per query a list of {"text", "terms", "known", "rows"}
        (rows: how many rows the search may return hold the phrase).  The first phrase query builds the positions plane
        (4 bytes per stored token); without `phrases` quotes are punctuation as before."""
        report = None
        with self._lock:
            if phrases:
                scores, rows, corrections, report, _ = self._lexical_search(query_texts, n_results, where, fuzzy, True,
                                                                            slop, phrase_mode)
            else:
                scores, rows, corrections = self._lexical_search(query_texts, n_results, where, fuzzy)
            tables = self._tables()
        scores_h, rows_h = scores.cpu(), rows.cpu()
        out: Dict[str, Any] = {"ids": [], "documents": [] if "documents" in include else None,
                               "metadatas": [] if "metadatas" in include else None, "lexical_scores": []}
        for srow, rrow in zip(scores_h.tolist(), rows_h.tolist()):
            hit = [r for r in rrow if r >= 0]
            self._append_hits(out, tables, hit, include)
            out["lexical_scores"].append(srow[: len(hit)])
        if corrections is not None:
            out["corrections"] = corrections
        if report is not None:
            out["phrases"] = report
        return out

    def hybrid_query(self, query_embeddings, query_texts: Sequence[str], n_results: int = 10,
                     where: Optional[Dict[str, Any]] = None,
                     include: Sequence[str] = ("metadatas", "documents", "distances"),
                     check_norm: bool = True, fuzzy=None, phrases=None, slop: int = 0,
                     phrase_mode: str = "require") -> Dict[str, Any]:
        """Dense + lexical retrieval fused by reciprocal rank (lexical.rrf_fuse).  Each leg takes
        C = max(n_results, MMRAG_HYBRID_CANDIDATES) hits (at most 4096) under the same `where`; a row scores
        sum 1 / (MMRAG_HYBRID_RRF_K + rank) over the legs that returned it.  Returns `ids`, `documents`, `metadatas`,
        `distances`, `hybrid_scores` and `lexical_scores` (0.0 for rows the lexical leg did not return), ordered by
        hybrid score -- so `distances` (1 - cos, the dense leg's own value where it returned the row, else computed on
        the device from the stored row) are NOT ascending.  `fuzzy` makes the lexical leg typo-tolerant as in
        lexical_query; the result then carries `corrections`.  `phrases`, `slop`, `phrase_mode` as in lexical_query, and
        the result carries `phrases`: under "require" a query that has phrases takes its DENSE leg from the same rows --
        those holding every phrase, alive and passing `where` -- by the filtered scan (mmrag_filtered_topk) over the
        match kernel's bitmaps, so every fused hit holds the phrases; queries without phrases share one bitmap, and the
        batch is cut to MMRAG_FILTER_BITMAP_BYTES of bitmaps per launch.  Under "prefer" the dense leg is unchanged."""
        from .config import settings
        from .lexical import parse_phrase_mode, parse_slop, rows_dot, rrf_fuse

        if phrases:
            slop, phrase_mode = parse_slop(slop), parse_phrase_mode(phrase_mode)

        texts = list(query_texts)
        self._need_plane("hybrid_query")
        if n_results < 1:
            raise ValueError("n_results must be >= 1")
        C = min(max(n_results, settings.MMRAG_HYBRID_CANDIDATES), _native.MAX_K_DEEP)
        with self._lock:
            if self._plane is not None:
                # converted and norm-checked once: the search below takes the device tensor as it is
                query_embeddings = self._to_device_f32(query_embeddings, "query", check_norm)
                check_norm = False
                q = self._pack_plane_queries(query_embeddings)
            else:
                q = self._pack_queries(query_embeddings, check_norm)
            if q.shape[0] != len(texts):
                raise ValueError(f"{q.shape[0]} query embeddings for {len(texts)} query texts")
            report = None
            if phrases:
                want = phrase_mode == "require"
                l_scores, l_rows, corrections, report, maps = self._lexical_search(texts, C, where, fuzzy, True, slop,
                                                                                  phrase_mode, bitmaps=want)
                if want and maps is not None:
                    d_scores, d_rows = self._launch_phrase_dense(query_embeddings, q, C, where, check_norm, report, maps)
                else:
                    d_scores, d_rows = self._launch_search(query_embeddings, C, where, check_norm)
            else:
                d_scores, d_rows = self._launch_search(query_embeddings, C, where, check_norm)
                l_scores, l_rows, corrections = self._lexical_search(texts, C, where, fuzzy)
            tables = self._tables()
            d_s, d_r = d_scores.cpu(), d_rows.cpu()
            l_s, l_r = l_scores.cpu().tolist(), l_rows.cpu().tolist()
            dist_dense = (1.0 - d_s).tolist()                    # float32 arithmetic, as query() does
            fused, need = [], []
            for b in range(len(texts)):
                drow = [r for r in d_r[b].tolist() if r >= 0]
                lrow = [r for r in l_r[b] if r >= 0]
                top = rrf_fuse(drow, lrow, settings.MMRAG_HYBRID_RRF_K)[:n_results]
                dpos = {r: i for i, r in enumerate(drow)}
                fused.append((top, dpos, {r: l_s[b][i] for i, r in enumerate(lrow)}))
                need.extend((b, r) for r, _ in top if r not in dpos)
            if need:
                dots = rows_dot(q, self._full, self.dim, torch.tensor([b for b, _ in need], device=self.device),
                                torch.tensor([r for _, r in need], device=self.device))
                extra = dict(zip(need, (1.0 - dots.cpu()).tolist()))
            else:
                extra = {}
        out: Dict[str, Any] = {"ids": [], "distances": [], "hybrid_scores": [], "lexical_scores": [],
                               "documents": [] if "documents" in include else None,
                               "metadatas": [] if "metadatas" in include else None}
        for b, (top, dpos, lex) in enumerate(fused):
            rows = [r for r, _ in top]
            self._append_hits(out, tables, rows, include)
            out["hybrid_scores"].append([s for _, s in top])
            out["lexical_scores"].append([lex.get(r, 0.0) for r in rows])
            out["distances"].append([dist_dense[b][dpos[r]] if r in dpos else extra[(b, r)] for r in rows])
        if corrections is not None:
            out["corrections"] = corrections
        if report is not None:
            out["phrases"] = report
        return out

    def _launch_phrase_dense(self, query_embeddings, q, k: int, where, check_norm: bool, report, maps):
        """the dense leg of a hybrid query under phrase_mode="require" (caller holds the lock): device (scores, rows)
        [B, k].  Query b with phrases is answered from the rows of maps[b] (already alive and passing `where`: the match
        kernel writes no other row); the queries without phrases share ONE bitmap, alive AND `where`.  One filtered scan
        (mmrag_filtered_topk) per MMRAG_FILTER_BITMAP_BYTES of bitmaps."""
        from .config import settings

        B = q.shape[0]
        with_ph = [b for b in range(B) if report[b]]
        without = [b for b in range(B) if not report[b]]
        W = _native.filter_words(self._n)
        per_launch = max(1, int(settings.MMRAG_FILTER_BITMAP_BYTES) // max(4 * W, 1))
        scores = torch.empty((B, k), dtype=torch.float32, device=self.device)
        rows_o = torch.empty((B, k), dtype=torch.int64, device=self.device)
        shared = None
        if without:
            bits = self._where_bits(where)
            if bits is None:
                shared = torch.full((1, W), -1, dtype=torch.int32, device=self.device)
                if self._n % 32 and W:      # bits at and past n stay zero, as mmrag_filter_eval leaves them
                    shared[0, self._n // 32] = (1 << (self._n % 32)) - 1
                shared[0, (self._n + 31) // 32:] = 0
            else:
                shared = torch.zeros((1, W), dtype=torch.int32, device=self.device)
                m = min(W, bits.numel())
                shared[0, :m] = bits[:m]
        # launches: the shared bitmap rides with the first chunk of phrase queries
        order = without + with_ph
        at = 0
        while at < len(order):
            mine, vis, foq = [], [], []
            if at < len(without):
                mine = without[at:]
                vis.append(shared)
                foq = [0] * len(mine)
                at = len(without)
            room = per_launch - len(vis)
            take = order[at: at + max(room, 0 if vis else 1)]
            for b in take:
                foq.append(len(vis))
                vis.append(maps[b: b + 1])
                mine.append(b)
            at += len(take)
            vb = torch.cat(vis, 0).contiguous()
            whole = mine == list(range(B))
            pick = None if whole else torch.tensor(mine, device=self.device)
            need = _native.filtered_topk_workspace_bytes(len(mine), self._n, k)
            ss, rr = _native.filtered_topk(q if whole else q[pick].contiguous(), self._full, self._n, self.dim, k, foq,
                                           vb, workspace=self._workspace("_filtered_ws", need))
            if whole:
                return ss, rr
            scores[pick], rows_o[pick] = ss, rr
        return scores, rows_o

    # ------------------------------------------------------------------ learned sparse ----
    def enable_sparse(self, vocab_size: int):
        """Attach the learned sparse state (sparse.ImpactIndex over a vocabulary of `vocab_size` terms); the rows already
        stored get empty vectors until set_sparse() gives them theirs.  From then on add(sparse=...), compact and
        reset keep it current; a delete needs nothing (the alive bits filter dead rows).  Opt-in: without this call
        the collection does no sparse work."""
        with self._lock:
            if self._sparse is None:
                from .sparse import ImpactIndex

                sp = ImpactIndex(self.device, vocab_size)
                sp.append_empty(self._n)
                self._sparse = sp
            elif self._sparse.n_terms != int(vocab_size):
                raise ValueError(f"the sparse state has {self._sparse.n_terms} terms, not {vocab_size}")
            return self._sparse

    @property
    def sparse_enabled(self) -> bool:
        return self._sparse is not None

    def _need_sparse(self, who: str):
        if self._sparse is None:
            raise RuntimeError(f"{who} needs enable_sparse(vocab_size) first")
        return self._sparse

    def set_sparse(self, rows, off, terms, impacts):
        """Replace the sparse vectors of stored rows `rows` (row numbers; see rows_of_ids) by (off, terms, impacts):
        vector i = terms[off[i] .. off[i + 1]) ascending and distinct, impacts 1..255."""
        with self._lock:
            sp = self._need_sparse("set_sparse")
            rows = np.ascontiguousarray(rows, np.int64)
            if rows.size and (rows.min() < 0 or rows.max() >= self._n):
                raise ValueError("set_sparse: row outside the collection")
            from .sparse import check_sparse_rows

            check_sparse_rows(off, terms, impacts, sp.n_terms, rows.size, _native.MAX_SPARSE_TERMS, "set_sparse")
            sp.set_rows(rows, off, terms, impacts)

    def sparse_search(self, sparse_queries, n_results: int = 10, where: Optional[Dict[str, Any]] = None,
                      cap: int = 0, dbg: int = 0):
        """enqueue the impact search (csrc/sparse_score.hip): device (scores [B, k] float32 = the exact integer score,
        rows [B, k] int64), descending, ties to the lower row, (-inf, -1) padded.  `sparse_queries` = (off, terms,
        impacts): query i's distinct terms[off[i] .. off[i + 1]), at most 64, impacts 1..255.  `cap`, `dbg`: the
        kernel's test hook."""
        with self._lock:
            sp = self._need_sparse("sparse_search")
            return sp.topk(*sparse_queries, n_results, self._where_bits(where), cap, dbg)

    @staticmethod
    def _sparse_norm(scales) -> float:
        from .config import settings

        if scales is None:
            scales = (settings.MMRAG_SPARSE_IMPACT_SCALE, settings.MMRAG_SPARSE_IMPACT_SCALE)
        return float(scales[0]) * float(scales[1])

    def sparse_query(self, sparse_queries, n_results: int = 10, where: Optional[Dict[str, Any]] = None,
                     include: Sequence[str] = ("metadatas", "documents"), scales=None) -> Dict[str, Any]:
        """Learned sparse search as Chroma-shaped lists of lists `ids`, `documents`, `metadatas` and `sparse_scores` =
        integer score / (query scale x document scale), i.e. the dot product of the two un-quantised vectors up to
        rounding (`scales`: the two impact scales, default MMRAG_SPARSE_IMPACT_SCALE for both).  Only rows sharing a
        term with the query are returned, so a list may be shorter than n_results."""
        norm = self._sparse_norm(scales)
        with self._lock:
            scores, rows = self.sparse_search(sparse_queries, n_results, where)
            tables = self._tables()
        scores_h, rows_h = scores.cpu(), rows.cpu()
        out: Dict[str, Any] = {"ids": [], "documents": [] if "documents" in include else None,
                               "metadatas": [] if "metadatas" in include else None, "sparse_scores": [], "rows": []}
        for srow, rrow in zip(scores_h.tolist(), rows_h.tolist()):
            hit = [r for r in rrow if r >= 0]
            self._append_hits(out, tables, hit, include)
            out["sparse_scores"].append([s / norm for s in srow[: len(hit)]])
            out["rows"].append(hit)
        return out

    def sparse_explain(self, q_terms, q_impacts, row: int, scales=None) -> List[Tuple[int, float]]:
        """[(term id, contribution)] of one query against one stored row, best first (ties to the lower term): the
        overlapping terms and their share of sparse_scores, from the host copy of the forward log"""
        norm = self._sparse_norm(scales)
        with self._lock:
            d_terms, d_imp = self._need_sparse("sparse_explain").row_vector(int(row))
        qw = {int(t): int(w) for t, w in zip(q_terms, q_impacts)}
        both = [(int(t), qw[int(t)] * int(w) / norm) for t, w in zip(d_terms, d_imp) if int(t) in qw]
        return sorted(both, key=lambda x: (-x[1], x[0]))

    def sparse_hybrid_query(self, query_embeddings, sparse_queries, n_results: int = 10,
                            where: Optional[Dict[str, Any]] = None,
                            include: Sequence[str] = ("metadatas", "documents", "distances"),
                            check_norm: bool = True, scales=None) -> Dict[str, Any]:
        """Dense + learned sparse retrieval fused by reciprocal rank (lexical.rrf_fuse), as hybrid_query fuses dense +
        BM25: each leg takes C = max(n_results, MMRAG_HYBRID_CANDIDATES) hits (at most 4096) under the same `where`.
        Returns `ids`, `documents`, `metadatas`, `distances`, `hybrid_scores` and `sparse_scores` (0.0 for rows the
        sparse leg did not return), ordered by hybrid score."""
        from .config import settings
        from .lexical import rows_dot, rrf_fuse

        self._need_plane("sparse_hybrid_query")
        if n_results < 1:
            raise ValueError("n_results must be >= 1")
        norm = self._sparse_norm(scales)
        C = min(max(n_results, settings.MMRAG_HYBRID_CANDIDATES), _native.MAX_K_DEEP)
        n_q = len(sparse_queries[0]) - 1
        with self._lock:
            if self._plane is not None:
                query_embeddings = self._to_device_f32(query_embeddings, "query", check_norm)
                check_norm = False
                q = self._pack_plane_queries(query_embeddings)
            else:
                q = self._pack_queries(query_embeddings, check_norm)
            if q.shape[0] != n_q:
                raise ValueError(f"{q.shape[0]} query embeddings for {n_q} sparse queries")
            d_scores, d_rows = self._launch_search(query_embeddings, C, where, check_norm)
            s_scores, s_rows = self.sparse_search(sparse_queries, C, where)
            tables = self._tables()
            d_s, d_r = d_scores.cpu(), d_rows.cpu()
            s_s, s_r = s_scores.cpu().tolist(), s_rows.cpu().tolist()
            dist_dense = (1.0 - d_s).tolist()
            fused, need = [], []
            for b in range(n_q):
                drow = [r for r in d_r[b].tolist() if r >= 0]
                srow = [r for r in s_r[b] if r >= 0]
                top = rrf_fuse(drow, srow, settings.MMRAG_HYBRID_RRF_K)[:n_results]
                dpos = {r: i for i, r in enumerate(drow)}
                fused.append((top, dpos, {r: s_s[b][i] / norm for i, r in enumerate(srow)}))
                need.extend((b, r) for r, _ in top if r not in dpos)
            if need:
                dots = rows_dot(q, self._full, self.dim, torch.tensor([b for b, _ in need], device=self.device),
                                torch.tensor([r for _, r in need], device=self.device))
                extra = dict(zip(need, (1.0 - dots.cpu()).tolist()))
            else:
                extra = {}
        out: Dict[str, Any] = {"ids": [], "distances": [], "hybrid_scores": [], "sparse_scores": [], "rows": [],
                               "documents": [] if "documents" in include else None,
                               "metadatas": [] if "metadatas" in include else None}
        for b, (top, dpos, sp) in enumerate(fused):
            rows = [r for r, _ in top]
            self._append_hits(out, tables, rows, include)
            out["hybrid_scores"].append([s for _, s in top])
            out["sparse_scores"].append([sp.get(r, 0.0) for r in rows])
            out["rows"].append(rows)
            out["distances"].append([dist_dense[b][dpos[r]] if r in dpos else extra[(b, r)] for r in rows])
        return out
