"""Shared pieces of the extractive reader's tests: float64 logits and normalisers, the span selection rule in plain
Python (two independent statements of it), the seeded qa_outputs head the goldens were made with.  numpy only."""
from typing import List, Tuple

import numpy as np

from tests import cross_encoder_ref as R

NEG_INF = float("-inf")


def logits_f64(hidden: np.ndarray, qa_w: np.ndarray, qa_b: np.ndarray) -> np.ndarray:
    """[T, 2] float64 start / end logits of hidden [T, H]"""
    return np.asarray(hidden, np.float64) @ np.asarray(qa_w, np.float64).T + np.asarray(qa_b, np.float64)


def lse_f64(ls: np.ndarray, le: np.ndarray, ctx_start: int, ctx_len: int) -> Tuple[float, float]:
    """log-sum-exp of the start and of the end logits over position 0 and the passage tokens, in float64"""
    at = np.concatenate([[0], np.arange(ctx_start, ctx_start + ctx_len)]).astype(np.int64)
    out = []
    for x in (np.asarray(ls, np.float64)[at], np.asarray(le, np.float64)[at]):
        m = x.max()
        out.append(float(m + np.log(np.exp(x - m).sum())))
    return out[0], out[1]


def select_spans(ls, le, ctx_start: int, ctx_len: int, L: int, n: int):
    """(spans [n, 2] int32, scores [n] float32): n rounds over the candidates (i, j), ctx_start <= i <= j < ctx_start +
    ctx_len, j - i < L, score float32(ls[i]) + float32(le[j]) rounded to float32 and above -inf.  A round takes the
    eligible candidate of highest score, then lowest i, then lowest j; a candidate is eligible while it shares no token
    with a span taken earlier.  Rounds without one give (-1, -1), -inf.  The first r rounds do not depend on n: the
    result for a smaller n is a prefix.  (The walk over j is one float32 numpy row per i, so that a 512-token sequence
    costs milliseconds; finite logits are assumed.)"""
    ls, le = np.asarray(ls, np.float32), np.asarray(le, np.float32)
    end = ctx_start + ctx_len
    taken = [False] * max(end, 1)
    spans = np.full((n, 2), -1, np.int32)
    scores = np.full(n, NEG_INF, np.float32)
    for r in range(n):
        best, at = np.float32(NEG_INF), None
        for i in range(ctx_start, end):
            stop = min(i + L, end)
            for j in range(i, stop):        # a span from i ends before the first taken token
                if taken[j]:
                    stop = j
                    break
            if stop == i:
                continue
            row = ls[i] + le[i:stop]        # float32 + float32
            k = int(np.argmax(row))         # the first of equal scores: the lowest j
            if row[k] > best:               # ascending i: the first of equal scores stays
                best, at = row[k], (i, i + k)
        if at is None:
            break
        spans[r], scores[r] = at, best
        for t in range(at[0], at[1] + 1):
            taken[t] = True
    return spans, scores


def select_spans_brute(ls, le, ctx_start: int, ctx_len: int, L: int, n: int):
    """the same rule stated as: enumerate every candidate, sort by (-score, i, j), keep greedily what is disjoint"""
    ls, le = np.asarray(ls, np.float32), np.asarray(le, np.float32)
    end = ctx_start + ctx_len
    cands: List[Tuple[float, int, int]] = []
    for i in range(ctx_start, end):
        for j in range(i, min(i + L, end)):
            s = np.float32(ls[i] + le[j])
            if s > NEG_INF:
                cands.append((float(s), i, j))
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))
    spans = np.full((n, 2), -1, np.int32)
    scores = np.full(n, NEG_INF, np.float32)
    kept: List[Tuple[int, int]] = []
    for s, i, j in cands:
        if len(kept) == n:
            break
        if all(j < a or b < i for a, b in kept):
            spans[len(kept)], scores[len(kept)] = (i, j), s
            kept.append((i, j))
    return spans, scores


def qa_head(hidden: int, seed: int):
    """qa_outputs of a golden shape: numpy PCG64 seeded with seed + 2000, weight [2, H] / sqrt(H) then bias [2] * 0.05
    (standard normal, float32)"""
    g = np.random.default_rng(seed + 2000)
    return {"qa_outputs.weight": (g.standard_normal((2, hidden)) / np.sqrt(hidden)).astype(np.float32),
            "qa_outputs.bias": (g.standard_normal(2) * 0.05).astype(np.float32)}


def reader_weights(name: str):
    """(shape, weights with BertModel names + the two-row type table + qa_outputs) of a golden shape: the
    cross-encoder goldens' body (tests/cross_encoder_ref.py), its pooler and classifier dropped"""
    shape, _, w = R.cross_weights(name)
    w = {k: v for k, v in w.items() if not k.startswith(("pooler.", "classifier."))}
    w.update(qa_head(shape.hidden, R.SHAPES[name][2]))
    return shape, w
