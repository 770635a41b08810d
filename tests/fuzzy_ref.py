"""Pure-Python reference of the typo-tolerant lexical leg: the optimal-string-alignment
distance by the full dynamic programme, the AUTO rule, the candidate order and the query rewrite.  The tests compare
csrc/fuzzy.hip and lexical.py against it, every element equal."""
from typing import Dict, List, Sequence, Tuple

import numpy as np

FUZZY_MAX_LEN = 64


def osa(a: str, b: str) -> int:
    """optimal string alignment distance over code points: insert, delete, substitute and the transposition of two
    adjacent code points cost 1; no substring is edited twice, so osa("ca", "abc") is 3, not 2"""
    la, lb = len(a), len(b)
    d = [[0] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        d[i][0] = i
    for j in range(lb + 1):
        d[0][j] = j
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            v = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                v = min(v, d[i - 2][j - 2] + 1)
            d[i][j] = v
    return d[la][lb]


def auto_edits(n_code_points: int) -> int:
    """AUTO:3,6 -- 0 edits for 1-2 code points, 1 for 3-5, 2 for 6 or more"""
    return 0 if n_code_points < 3 else 1 if n_code_points < 6 else 2


def edits_for(fuzzy, n_code_points: int) -> int:
    """the budget of a term under fuzzy = "auto" / True / 0..2; terms above FUZZY_MAX_LEN are never corrected"""
    if n_code_points > FUZZY_MAX_LEN:
        return 0
    if fuzzy is True or fuzzy == "auto":
        return auto_edits(n_code_points)
    return int(fuzzy)


def key(dist: int, df: int, term_id: int) -> int:
    """the selection key: smaller distance, then larger df, then lower id, as one integer to maximise"""
    return ((2 - dist) << 62) | (df << 31) | (2 ** 31 - 1 - term_id)


def candidates(pattern: str, edits: int, terms: Sequence[str], df: Sequence[int]) -> List[Tuple[int, int]]:
    """every (term id, distance) within `edits` of `pattern`, best first.  Candidates have df >= 1 and 1..64 code
    points; a pattern above 64 code points has none."""
    if len(pattern) > FUZZY_MAX_LEN or not 0 <= edits <= 2:
        return []
    found = []
    for t, s in enumerate(terms):
        if df[t] < 1 or not 1 <= len(s) <= FUZZY_MAX_LEN or abs(len(s) - len(pattern)) > edits:
            continue
        dist = osa(pattern, s)
        if dist <= edits:
            found.append((key(dist, int(df[t]), t), t, dist))
    found.sort(reverse=True)
    return [(t, dist) for _, t, dist in found]


def fuzzy_terms(terms: Sequence[str], df: Sequence[int], patterns: Sequence[str], edits: Sequence[int],
                max_expansions: int):
    """what mmrag_fuzzy_terms returns: (term ids, edits) [P, E] int32, best first, -1 padded"""
    P, E = len(patterns), max_expansions
    out_t = np.full((P, E), -1, np.int32)
    out_e = np.full((P, E), -1, np.int32)
    for p, (pat, e) in enumerate(zip(patterns, edits)):
        for s, (t, dist) in enumerate(candidates(pat, int(e), terms, df)[:E]):
            out_t[p, s], out_e[p, s] = t, dist
    return out_t, out_e


def rewrite(terms: Sequence[Tuple[int, str]], live: Sequence[bool], best: Dict[str, Tuple[int, int]]):
    """One query under typo tolerance.  terms: its distinct (id, string) in order of first occurrence (id -1: unknown);
    live[i]: the term has live df >= 1; best: string -> (best candidate id, edits).  A term that is not live is
    replaced where it stood by its best candidate, or dropped without one; the list keeps the first of equal ids, so
    it is again "distinct terms in order of first occurrence" -- exactly the list of the corrected text.  Returns
    (ids, [(term, matched id, edits)] for every term that found a candidate)."""
    ids: List[int] = []
    made: List[Tuple[str, int, int]] = []
    for (tid, s), ok in zip(terms, live):
        if not ok:
            if s not in best:
                continue
            tid, e = best[s]
            made.append((s, tid, e))
        if tid not in ids:
            ids.append(tid)
    return ids, made
