"""Plain-Python reference of grouping search hits by a per-row key (include/mmrag.h mmrag_group_select, DESIGN.md
section 3.1h) and of the candidate-depth ladder of VectorIndex.grouped_search.  No arithmetic: the result is exact."""
import numpy as np

MAX_CANDIDATES = 4096


def select(rows, group_of_row, n_rows):
    """every group of one query's candidate list, in rank order: [(ordinal, [positions in list order])], and the number
    of valid candidates.  The list ends at its first row < 0; a row >= n_rows or with a negative ordinal has no key and
    is a group of its own, ordinal -1"""
    groups, at, valid = [], {}, 0
    for i, r in enumerate(rows):
        r = int(r)
        if r < 0:
            break
        valid += 1
        g = int(group_of_row[r]) if r < n_rows else -1
        if g < 0:
            groups.append((-1, [i]))
        elif g in at:
            groups[at[g]][1].append(i)
        else:
            at[g] = len(groups)
            groups.append((g, [i]))
    return groups, valid


def select_padded(scores, rows, group_of_row, n_rows, G, S):
    """the five output blocks of one query: scores [G, S] float32 (the input's bits), rows [G, S] int64, positions
    [G, S] int32, ordinals [G] int32, info [2] int32 = (groups found capped at G, valid candidates); unused slots
    (-inf, -1, -1) and -2"""
    scores = np.asarray(scores, np.float32)
    groups, valid = select(rows, group_of_row, n_rows)
    out_s = np.full((G, S), -np.inf, np.float32)
    out_r = np.full((G, S), -1, np.int64)
    out_p = np.full((G, S), -1, np.int32)
    out_g = np.full(G, -2, np.int32)
    for gi, (g, members) in enumerate(groups[:G]):
        out_g[gi] = g
        for slot, i in enumerate(members[:S]):
            out_s[gi, slot] = scores[i]
            out_r[gi, slot] = rows[i]
            out_p[gi, slot] = i
    return out_s, out_r, out_p, out_g, np.array([min(len(groups), G), valid], np.int32)


def first_depth(G, S, base=64):
    return min(max(base, 4 * G * S), MAX_CANDIDATES)


def complete(answer, C, G):
    """a pass at depth C is complete when it found G groups or its list was exhausted (what `exhaustive` reports)"""
    return bool(answer[4][0] >= G or answer[4][1] < C)


def ladder(full_ranked_scores, full_ranked_rows, group_of_row, n_rows, G, S, base=64, fetch_k=None):
    """The depth policy applied to one query's exact full ranking (every live row, best first): returns (C*, answer)
    where answer = select_padded over the first C* candidates (padded to C* with (-inf, -1) when the
    ranking is shorter).  fetch_k: one pass at min(max(fetch_k, G), 4096).  Otherwise C = first_depth, and while the
    pass neither found G groups nor exhausted the list (valid < C) and C < 4096, C = min(4 C, 4096)."""
    scores = np.asarray(full_ranked_scores, np.float32)
    rows = np.asarray(full_ranked_rows, np.int64)

    def at_depth(C):
        s = np.full(C, -np.inf, np.float32)
        r = np.full(C, -1, np.int64)
        m = min(C, len(rows))
        s[:m], r[:m] = scores[:m], rows[:m]
        return select_padded(s, r, group_of_row, n_rows, G, S)

    C = first_depth(G, S, base) if fetch_k is None else min(max(int(fetch_k), G), MAX_CANDIDATES)
    while True:
        ans = at_depth(C)
        if complete(ans, C, G) or fetch_k is not None or C >= MAX_CANDIDATES:
            return C, ans
        C = min(4 * C, MAX_CANDIDATES)
