"""Plain numpy reference of document-scoped retrieval (csrc/scoped.hip, VectorIndex.scoped_search): query b sees row r
iff r is alive and group_of_row[r] is in the scope of b; its answer is the exact top-k of the search oracle over the
sub-matrix of the rows it sees, mapped back to global rows and padded with (-inf, -1).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from oracle import search_oracle as O


def visible_rows(group_of_row: np.ndarray, scope: Sequence[int], alive: Optional[np.ndarray] = None) -> np.ndarray:
    """ascending rows whose ordinal is in `scope` (ordinal -1 is in no scope) and that are alive"""
    g = np.asarray(group_of_row)
    keep = np.isin(g, np.asarray(list(scope), dtype=np.int64)) & (g >= 0)
    if alive is not None:
        keep &= np.asarray(alive, dtype=bool)[: g.size]
    return np.nonzero(keep)[0]


def scoped_topk(q: np.ndarray, rows: np.ndarray, k: int, group_of_row: np.ndarray, scope_of_query: Sequence[int],
                scopes: Sequence[Sequence[int]], alive: Optional[np.ndarray] = None,
                row_offset: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """q [B, d], rows [n, d] (the stored values, up-cast exactly); scopes[s] = the ordinals of scope s, query b has scope
    scope_of_query[b].  Returns (scores [B, k] float32 descending, ties to the lower row; rows [B, k] int64 +
    row_offset), (-inf, -1) padded."""
    B = q.shape[0]
    out_s = np.full((B, k), O.NEG_INF, dtype=np.float32)
    out_r = np.full((B, k), -1, dtype=np.int64)
    seen = {}
    for b in range(B):
        s = int(scope_of_query[b])
        if s not in seen:
            seen[s] = visible_rows(group_of_row, scopes[s], alive)
        vis = seen[s]
        if vis.size == 0:
            continue
        ss, rr = O.cosine_topk(q[b: b + 1], rows[vis], k)
        live = rr[0] >= 0
        out_s[b, : live.sum()] = ss[0][live]
        out_r[b, : live.sum()] = vis[rr[0][live]] + row_offset
    return out_s, out_r
