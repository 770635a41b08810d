"""Plain-numpy reference of range retrieval (include/mmrag.h mmrag_range_scan): float64 scores of the stored values
up-cast exactly, what the kernels of csrc/range.hip are compared with.

Row r PASSES for query b iff it is visible to b and score(b, r) >= thr[b].  counts[b] is the number of passing rows; the
facet table of column c holds, in slot g < G_c, the passing rows whose code is g and, in slot G_c, those whose code is
outside 0..G_c-1; hits are the `limit` best passing rows, score descending, ties to the lower row, (-inf, -1) padded."""
from typing import List, Optional, Sequence, Tuple

import numpy as np


def scores64(q, rows) -> np.ndarray:
    return np.asarray(q, np.float64) @ np.asarray(rows, np.float64).T


def range_ref(q, rows, thr, limit: int, vis_of_query: Optional[np.ndarray] = None,
              facet_codes: Sequence[np.ndarray] = (), sizes: Sequence[int] = (),
              row_offset: int = 0) -> Tuple[np.ndarray, List[np.ndarray], np.ndarray, np.ndarray]:
    """q [B, d], rows [n, d] (the values as stored), thr: one float or [B]; vis_of_query: bool [B, n] or None (every row);
    facet_codes: int [n] per column, sizes: G per column.  Returns (counts [B] int64, one [B, G + 1] int64 table per
    column, scores [B, limit] float32, rows [B, limit] int64)."""
    q, rows = np.asarray(q), np.asarray(rows)
    B, n = q.shape[0], rows.shape[0]
    thr = np.broadcast_to(np.asarray(thr, np.float64).reshape(-1), (B,))
    s = scores64(q, rows) if n else np.zeros((B, 0))
    ok = s >= thr[:, None]
    if vis_of_query is not None:
        ok &= np.asarray(vis_of_query, bool).reshape(B, n)
    counts = ok.sum(axis=1).astype(np.int64)
    tables = []
    for codes, G in zip(facet_codes, sizes):
        codes = np.asarray(codes)[:n].astype(np.int64)
        slot = np.where((codes >= 0) & (codes < G), codes, G)
        t = np.zeros((B, G + 1), np.int64)
        for b in range(B):
            t[b] = np.bincount(slot[ok[b]], minlength=G + 1)
        tables.append(t)
    out_s = np.full((B, limit), -np.inf, np.float32)
    out_r = np.full((B, limit), -1, np.int64)
    for b in range(B):
        cand = np.nonzero(ok[b])[0]
        order = cand[np.lexsort((cand, -s[b, cand]))][:limit]      # score descending, then the lower row
        out_s[b, : order.size] = s[b, order]
        out_r[b, : order.size] = order + row_offset
    return counts, tables, out_s, out_r


def gap_threshold(scores_b, target: int, gap: float = 4e-4) -> float:
    """The midpoint of the gap of at least `gap` between consecutive sorted scores that lies nearest to `target` passing
    rows.  4e-4 is twice the project's 2e-4 tie margin (oracle/search_oracle.py): 2e-4 on each side of the threshold,
    above the 1e-4 score tolerance, so a correct kernel and the reference agree on the count EXACTLY."""
    s = np.sort(np.asarray(scores_b, np.float64))[::-1]
    assert s.size >= 2
    width = s[:-1] - s[1:]                    # width[i]: between the (i + 1)-th and (i + 2)-th best; i + 1 rows pass
    at = np.nonzero(width >= gap)[0]
    assert at.size, "no gap of the required width between consecutive scores"
    i = at[np.argmin(np.abs(at + 1 - target))]
    return float((s[i] + s[i + 1]) / 2)
