"""The token store: the per-token rows of stored chunks kept on the device, item i being index row i.

Late-interaction re-ranking (late.py) encodes every candidate passage again for every question although the passages
have not changed since they were uploaded.  With the store, ingest keeps their token rows: one fp16 plane [T, dim] in
item order and `item_off`, item i owning plane rows item_off[i] .. item_off[i + 1].  Re-ranking then encodes only the
question, and mmrag_maxsim_topk (csrc/maxsim_scan.hip) scans the whole plane for each question's exact MaxSim top-k.

This module is the bookkeeping: lengths, offsets, the stored token ids (what `explain` names), growth, compaction in the
index's `keep` order and the byte cap.  Every device step is a copy or a gather of rows; the scoring is the HIP kernels'.
With `device=None` the plane is a numpy array: the same bookkeeping, testable without a GPU.

`dtype="float8_e4m3fn"` keeps the plane as rows of E4M3 codes (include/mmrag.h MMRAG_F8E4M3, one byte per element, pad
columns code 0): incoming fp16 / fp32 rows are quantised once, here, and the FP8 kernels (mmrag_maxsim_topk_f8,
mmrag_maxsim_scores_f8) score the codes.  Half the bytes per token, so twice the chunks under the same cap; the scores
are the quantised rows' own.
"""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

logger = logging.getLogger(__name__)

MAX_PLANE_ROWS = (1 << 31) - 1     # mmrag_maxsim_topk: T < 2^31
DTYPES = ("float16", "float8_e4m3fn")


def f8_encode_numpy(x) -> np.ndarray:
    """The E4M3 codes (uint8) of float values x as the storage format defines them: csrc/f8_codec.h's f8_encode
    restated in numpy float32 / uint32 arithmetic (x * 256 rounded to nearest even, subnormals kept, saturation at 448,
    NaN -> +0).  The numpy stand-in of mmrag_f8_encode_rows."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.asarray(x, np.float32) * np.float32(256.0)
        nan = np.isnan(y)
        sign = np.where(nan, 0, (y.view(np.uint32) >> 24) & 0x80).astype(np.uint32)
        a = np.abs(y)
        u = a.view(np.uint32).astype(np.uint64)
        normal = (((u + 0x7FFFF + ((u >> 20) & 1)) >> 20) - (120 << 3)).astype(np.int64)
        sub = np.rint(np.where(a < np.float32(0.015625), a, 0) * np.float32(512.0)).astype(np.int64)   # step 2^-9
        code = np.where(a < np.float32(0.015625), sub, normal)
        code = np.where(a > np.float32(448.0), 0x7E, code)
        code = np.where(nan, 0, code).astype(np.uint32)
    return (sign | code).astype(np.uint8)


class TokenStore:
    """Token rows of items 0 .. n_items.  An item of length 0 has no tokens stored: it is no candidate of the scan and is
    re-encoded by a re-rank."""

    def __init__(self, dim: int, max_doc_tokens: int, device: Any = None, max_bytes: int = 0, capacity: int = 4096,
                 dtype: str = "float16"):
        if dim <= 0 or dim % 64 or dim > 1024:
            raise ValueError(f"token store: dim must be a multiple of 64, at most 1024 (dim={dim})")
        if not 1 <= int(max_doc_tokens) <= 512:
            raise ValueError(f"token store: max_doc_tokens={max_doc_tokens} outside 1..512")
        if dtype not in DTYPES:
            raise ValueError(f"token store: dtype must be one of {DTYPES} (got {dtype!r})")
        self.dim = int(dim)
        self.dtype = dtype
        self.f8 = dtype == "float8_e4m3fn"
        # plane columns and bytes per token row: fp16 rows have no pad (dim % 64 == 0), code rows are whole 128-byte slabs
        self.width = (self.dim + 127) // 128 * 128 if self.f8 else self.dim
        self.bytes_per_row = self.width if self.f8 else self.dim * 2
        self.max_doc_tokens = int(max_doc_tokens)
        self.device = device
        self.max_bytes = int(max_bytes)
        self._plane = self._alloc(max(int(capacity), 256))
        self._T = 0
        self._lens = np.zeros(0, np.int32)
        self._ids: List[Optional[np.ndarray]] = []
        self._off: Optional[np.ndarray] = None            # cumulated lengths, rebuilt on demand
        self._off_dev = None                              # (n, device tensor) of the last device_offsets(n)
        self._warned = False
        self.dropped = 0                                  # items whose tokens the cap kept out

    # ------------------------------------------------------------------ plane helpers --------
    def _alloc(self, rows: int):
        if self.device is None:
            return np.zeros((rows, self.width), np.uint8 if self.f8 else np.float16)
        import torch

        return torch.zeros((rows, self.width), dtype=torch.uint8 if self.f8 else torch.float16, device=self.device)

    def _as_rows(self, token_rows, codes: bool = False):
        """`token_rows` as a [m, width] array of the plane's kind: fp16 rows, or (an FP8 store) their code rows --
        quantised here, on the device by mmrag_f8_encode_rows, in the numpy mode by f8_encode_numpy.  `codes` (internal:
        a caller that hands back what _as_rows returned): the rows already are code rows of the plane's width.  Without
        it integer data is refused: a uint8 array is never taken for codes because its width happens to fit."""
        if self.f8:
            return self._as_code_rows(token_rows, codes)
        if self.device is None:
            rows = np.ascontiguousarray(np.asarray(token_rows, np.float16))
        else:
            import torch

            rows = token_rows if isinstance(token_rows, torch.Tensor) else torch.from_numpy(np.asarray(token_rows))
            rows = rows.to(device=self.device, dtype=torch.float16)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"token store: token rows must be [tokens, {self.dim}] (got {tuple(rows.shape)})")
        return rows

    def _as_code_rows(self, token_rows, codes: bool):
        bad = ValueError(f"token store: token rows must be floating-point [tokens, {self.dim}] (got "
                         f"{tuple(getattr(token_rows, 'shape', ()))})")
        if self.device is None:
            rows = np.asarray(token_rows)
            if codes:
                if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[1] != self.width:
                    raise bad
                return np.ascontiguousarray(rows)
            if rows.ndim != 2 or rows.shape[1] != self.dim or rows.dtype.kind != "f":
                raise bad
            codes = np.zeros((rows.shape[0], self.width), np.uint8)
            codes[:, : self.dim] = f8_encode_numpy(rows.astype(np.float32))
            return codes
        import torch

        from . import _native

        rows = token_rows if isinstance(token_rows, torch.Tensor) else torch.from_numpy(np.asarray(token_rows))
        if codes:
            if rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != self.width:
                raise bad
            return rows.to(self.device).contiguous()
        if rows.dim() != 2 or rows.shape[1] != self.dim or not rows.is_floating_point():
            raise bad
        if rows.dtype not in (torch.float16, torch.float32):
            rows = rows.to(torch.float32)
        return _native.f8_encode_rows(rows.to(self.device).contiguous(), self.dim)

    def _take(self, rows, index: np.ndarray):
        if self.device is None:
            return rows[index]
        import torch

        return rows.index_select(0, torch.from_numpy(np.ascontiguousarray(index, np.int64)).to(self.device))

    GATHER_SLICE = 1 << 20     # rows a rebuild moves per step: the temporary of a gather is one slice, not a plane

    def _gather_into(self, fresh, index: np.ndarray, old, n_old: int, new):
        """fresh[j] = row index[j] of `old` (index[j] < n_old) or row index[j] - n_old of `new`, GATHER_SLICE rows at
        a time and without joining the two sources"""
        for lo in range(0, int(index.size), self.GATHER_SLICE):
            part = index[lo: lo + self.GATHER_SLICE]
            from_new = part >= n_old
            if not from_new.any():
                fresh[lo: lo + part.size] = self._take(old, part)
            elif from_new.all():
                fresh[lo: lo + part.size] = self._take(new, part - n_old)
            else:
                at = lo + np.arange(part.size)
                for src, mask, shift in ((old, ~from_new, 0), (new, from_new, n_old)):
                    dst = at[mask]
                    if self.device is None:
                        fresh[dst] = src[part[mask] - shift]
                    else:
                        import torch

                        fresh.index_copy_(0, torch.from_numpy(dst).to(self.device), self._take(src, part[mask] - shift))

    def _reserve(self, rows: int):
        cap = self._plane.shape[0]
        if rows <= cap:
            return
        new = self._alloc(max(rows, 2 * cap))
        new[: self._T] = self._plane[: self._T]
        self._plane = new

    def _changed(self):
        self._off = None
        self._off_dev = None

    # ------------------------------------------------------------------ reading --------------
    @property
    def plane(self):
        return self._plane

    @property
    def n_rows(self) -> int:
        """T: plane rows in use"""
        return self._T

    @property
    def n_items(self) -> int:
        return int(self._lens.size)

    def offsets(self, n: Optional[int] = None) -> np.ndarray:
        """item_off [n + 1] int32 for items 0 .. n (default: the items the store knows); items the store has not heard
        of have length 0"""
        if self._off is None:
            off = np.zeros(self._lens.size + 1, np.int64)
            np.cumsum(self._lens, out=off[1:])
            self._off = off.astype(np.int32)
        n = self._lens.size if n is None else int(n)
        if n <= self._lens.size:
            return self._off[: n + 1]
        return np.concatenate([self._off, np.full(n - self._lens.size, self._T, np.int32)])

    def device_offsets(self, n: int):
        """offsets(n) on the device, uploaded once per change"""
        if self.device is None:
            return self.offsets(n)
        if self._off_dev is None or self._off_dev[0] != n:
            import torch

            self._off_dev = (n, torch.from_numpy(np.ascontiguousarray(self.offsets(n))).to(self.device))
        return self._off_dev[1]

    def frontier(self) -> int:
        """the item after the last one that keeps tokens: set_tokens of items from here on appends, before it rebuilds"""
        with_tokens = np.nonzero(self._lens > 0)[0]
        return int(with_tokens[-1]) + 1 if with_tokens.size else 0

    def length(self, item: int) -> int:
        return int(self._lens[item]) if 0 <= item < self._lens.size else 0

    def span(self, item: int):
        """(first plane row, length) of an item"""
        return int(self.offsets()[item]) if item < self._lens.size else self._T, self.length(item)

    def token_ids(self, item: int) -> Optional[List[int]]:
        ids = self._ids[item] if 0 <= item < len(self._ids) else None
        return None if ids is None else ids.tolist()

    def stats(self) -> Dict[str, Any]:
        return {"dim": self.dim, "max_doc_tokens": self.max_doc_tokens, "items": int((self._lens > 0).sum()),
                "tokens": self._T, "bytes": self._T * self.bytes_per_row,
                "reserved_bytes": int(self._plane.shape[0]) * self.bytes_per_row, "max_bytes": self.max_bytes,
                "dropped_items": self.dropped, "dtype": self.dtype, "bytes_per_token": self.bytes_per_row}

    # ------------------------------------------------------------------ writing --------------
    def set_tokens(self, rows: Sequence[int], token_rows, lens: Sequence[int],
                   token_ids: Optional[Sequence[Optional[Sequence[int]]]] = None, _codes: bool = False):
        """Store the token rows of items `rows` (distinct): item rows[j] gets the next lens[j] rows of `token_rows`
        [sum(lens), dim].  Items past the last one that has tokens are appended to the plane; any other item (a fill of an
        earlier row, a replacement) rebuilds the plane by one gather.  Past `max_bytes` (0 = no cap) or 2^31 - 1 plane
        rows the remaining items get length 0 and one warning is logged."""
        rows_a = np.asarray(list(rows), np.int64).reshape(-1)
        lens_a = np.asarray(list(lens), np.int64).reshape(-1)
        if rows_a.size != lens_a.size:
            raise ValueError(f"token store: {rows_a.size} rows for {lens_a.size} lengths")
        if token_ids is not None and len(token_ids) != rows_a.size:
            raise ValueError(f"token store: {len(token_ids)} token id lists for {rows_a.size} rows")
        if rows_a.size == 0:
            return
        if rows_a.min() < 0 or np.unique(rows_a).size != rows_a.size:
            raise ValueError("token store: rows must be distinct and non-negative")
        if lens_a.min() < 0 or lens_a.max() > self.max_doc_tokens:
            raise ValueError(f"token store: a length outside 0..{self.max_doc_tokens}")
        new = self._as_rows(token_rows, _codes)      # _codes: VectorIndex.set_tokens_for_ids hands back _as_rows' rows
        if new.shape[0] != int(lens_a.sum()):
            raise ValueError(f"token store: {new.shape[0]} token rows for lengths that sum to {int(lens_a.sum())}")
        src_at = np.zeros(rows_a.size + 1, np.int64)     # where each item's rows start in `new`
        np.cumsum(lens_a, out=src_at[1:])
        ids_in = [None if token_ids is None or token_ids[j] is None else np.asarray(token_ids[j], np.int32)
                  for j in range(rows_a.size)]

        hi = int(rows_a.max()) + 1
        if hi > self._lens.size:
            self._lens = np.concatenate([self._lens, np.zeros(hi - self._lens.size, np.int32)])
            self._ids.extend([None] * (hi - len(self._ids)))
        old_lens = self._lens[rows_a].astype(np.int64)
        # the cap: rows in use after this call = T - what is replaced + what is kept of the new rows, item by item
        keep = lens_a.copy()
        limit = MAX_PLANE_ROWS
        if self.max_bytes > 0:
            limit = min(limit, self.max_bytes // self.bytes_per_row)
        used = self._T - int(old_lens.sum())
        for j in range(rows_a.size):
            if used + keep[j] > limit:
                self.dropped += int((keep[j:] > 0).sum())
                keep[j:] = 0
                if not self._warned:
                    self._warned = True
                    logger.warning("token store: the cap of %d token rows is reached; further items get no tokens and "
                                   "are re-encoded by a re-rank", limit)
                break
            used += int(keep[j])

        with_tokens = np.nonzero(self._lens > 0)[0]
        frontier = int(with_tokens[-1]) + 1 if with_tokens.size else 0
        ascending = bool(np.all(np.diff(rows_a) > 0))
        if ascending and int(rows_a[0]) >= frontier:
            # append: the new items lie after every item that has tokens
            pick = np.concatenate([np.arange(src_at[j], src_at[j] + keep[j]) for j in range(rows_a.size)] or
                                  [np.zeros(0, np.int64)]).astype(np.int64)
            m = int(pick.size)
            self._reserve(self._T + m)
            if m:
                self._plane[self._T: self._T + m] = new if m == new.shape[0] else self._take(new, pick)
            self._T += m
        else:
            # general: every item's rows from the old plane or from `new` (numbered behind the old rows), gathered
            # slice by slice into a fresh plane: old plane + new plane + one slice at once, the old one freed after
            T0 = self._T
            starts = np.zeros(self._lens.size + 1, np.int64)
            np.cumsum(self._lens, out=starts[1:])
            seg_start = starts[:-1].copy()
            seg_len = self._lens.astype(np.int64)
            seg_start[rows_a] = T0 + src_at[:-1]
            seg_len[rows_a] = keep
            index = _ranges(seg_start, seg_len)
            fresh = self._alloc(max(int(self._plane.shape[0]), int(index.size)))
            self._gather_into(fresh, index, self._plane, T0, new)
            self._plane, self._T = fresh, int(index.size)
        self._lens[rows_a] = keep.astype(np.int32)
        for j, r in enumerate(rows_a.tolist()):
            self._ids[r] = ids_in[j] if keep[j] > 0 else None
        self._changed()

    def compact(self, keep: np.ndarray):
        """Keep the items `keep` (ascending old item numbers), in order: item j of the new store is old item keep[j].
        A new plane is swapped in."""
        keep = np.asarray(keep, np.int64).reshape(-1)
        hi = int(keep.max()) + 1 if keep.size else 0
        lens = np.concatenate([self._lens, np.zeros(max(hi - self._lens.size, 0), np.int32)]).astype(np.int64)
        starts = np.zeros(lens.size + 1, np.int64)
        np.cumsum(lens, out=starts[1:])
        seg_start, seg_len = starts[:-1][keep], lens[keep]
        index = _ranges(np.asarray(seg_start, np.int64), seg_len)
        fresh = self._alloc(max(256, int(index.size), int(self._plane.shape[0]) // 2
                                if index.size < self._plane.shape[0] // 4 else int(self._plane.shape[0])))
        self._gather_into(fresh, index, self._plane, self._plane.shape[0], None)
        self._ids = [self._ids[int(r)] if r < len(self._ids) else None for r in keep]
        self._plane, self._T = fresh, int(index.size)
        self._lens = seg_len.astype(np.int32)
        self._changed()

    def reset(self):
        self._T = 0
        self._lens = np.zeros(0, np.int32)
        self._ids = []
        self.dropped = 0
        self._warned = False
        self._changed()


def _ranges(starts: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """the concatenation of arange(starts[i], starts[i] + lens[i]) as int64"""
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    nz = lens > 0
    starts, lens = starts[nz], lens[nz]
    ends = np.cumsum(lens)
    out = np.ones(total, np.int64)
    out[0] = starts[0]
    out[ends[:-1]] = starts[1:] - (starts[:-1] + lens[:-1] - 1)
    return np.cumsum(out)
