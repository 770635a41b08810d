"""float64 reference of answer citations (include/mmrag.h mmrag_attribute), for the tests.

One unit: claims x_0 .. x_{C-1}, evidence e_0 .. e_{E-1} as numbers, a source ordinal per evidence row, n_sources, m.
  S = X E^T;  M_is = max over j with source_j = s of S_ij, J_is = the lowest such j that attains it (-inf, -1 for a
  source without evidence; an ordinal outside 0 .. n_sources - 1 counts for nothing);
  per claim the m best sources with J_is >= 0: M_is descending, ties to the lower s; (-1, -1, -inf) padded.
Everything is float64.
"""
import numpy as np


def similarities(X, E):
    """S [C, E] in float64"""
    X, E = np.asarray(X, np.float64), np.asarray(E, np.float64)
    return X @ E.T if len(E) else np.zeros((len(X), 0))


def support(S, sources, n_sources):
    """(M [C, n_sources] float64, J [C, n_sources] int)"""
    sources = np.asarray(sources, np.int64)
    C = S.shape[0]
    M = np.full((C, n_sources), -np.inf)
    J = np.full((C, n_sources), -1, np.int64)
    for s in range(n_sources):
        rows = np.nonzero(sources == s)[0]              # ascending j
        if rows.size:
            part = S[:, rows]
            best = np.argmax(part, axis=1)              # the first maximum: the lowest j
            M[:, s] = part[np.arange(C), best]
            J[:, s] = rows[best]
    return M, J


def rank(M, J, m):
    """(src [C, m], ev [C, m], score [C, m]): per claim the m best sources with evidence, padded"""
    C, n_sources = M.shape
    src = np.full((C, m), -1, np.int64)
    ev = np.full((C, m), -1, np.int64)
    score = np.full((C, m), -np.inf)
    for i in range(C):
        have = [s for s in range(n_sources) if J[i, s] >= 0]
        have.sort(key=lambda s: (-M[i, s], s))
        for t, s in enumerate(have[:m]):
            src[i, t], ev[i, t], score[i, t] = s, J[i, s], M[i, s]
    return src, ev, score


def attribute(X, E, sources, n_sources, m):
    """the whole definition for one unit: (src, ev, score, M)"""
    M, J = support(similarities(X, E), sources, n_sources)
    return rank(M, J, m) + (M,)


def margins(S, sources, n_sources, picks_src, picks_ev):
    """For one claim's picks (a kernel's source ordinals and evidence positions, best first, -1 padded; S: the
    claim's row [E]), per pick: (the reference value of the picked evidence row, the reference M of the picked source,
    the best reference M among the sources with evidence that no earlier pick took, the margin between that best and
    the second best of them -- inf when only one is left, the reference's own pick at that step, whether the picked row
    belongs to the picked source)"""
    M, J = support(np.asarray(S, np.float64)[None, :], sources, n_sources)
    M, J = M[0], J[0]
    sources = np.asarray(sources, np.int64)
    left = [s for s in range(n_sources) if J[s] >= 0]
    out = []
    for s, j in zip(picks_src, picks_ev):
        if s < 0:
            break
        order = sorted(left, key=lambda t: (-M[t], t))
        best = M[order[0]] if order else -np.inf
        margin = float(M[order[0]] - M[order[1]]) if len(order) > 1 else float("inf")
        mine = 0 <= j < len(sources) and sources[j] == s and s in left
        out.append((float(S[j]) if 0 <= j < len(sources) else -np.inf, float(M[s]) if 0 <= s < n_sources else -np.inf,
                    float(best), margin, order[0] if order else -1, bool(mine)))
        if s in left:
            left.remove(s)
    return out, len(left)
