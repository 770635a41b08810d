"""The definition of related-group retrieval (include/mmrag.h mmrag_related_groups) restated in numpy float64: what the
kernels of csrc/related.hip are compared with.

    dot[a][r]          = <A_a, x_r>
    candidate rows     r < n, alive, 0 <= group_of_row[r] < n_groups
    best[a][g]         = max of dot[a][r] over the candidate rows of g (-0 read as +0); best_row = the LOWEST such row
    similarity[s][g]   = sequential ascending float64 sum of float32(best[a][g]) over the set's columns / the set's size,
                         rounded once to float32
    covered[s][g]      = #{a : float32(best[a][g]) >= float32(threshold)}
    candidate groups   at least one candidate row, and not exclude_group[s]
    winners            similarity descending, ties to the lower ordinal; (-inf, -1, 0) padded, best (-inf, -1) padded
"""
import numpy as np


def best_matches(sets, rows, group_of_row, n_groups, alive=None):
    """(best [M, n_groups] float32 with -inf where the group has no candidate row, best_row [M, n_groups] int64, -1)"""
    sets = np.asarray(sets, np.float64)
    rows = np.asarray(rows, np.float64)
    col = np.asarray(group_of_row, np.int64)
    n, M = rows.shape[0], sets.shape[0]
    ok = (col >= 0) & (col < n_groups)
    if alive is not None:
        ok &= np.asarray(alive, bool)[:n]
    # float32(dot): the kernel's accumulation is float32; on exactly representable data the two are the same number
    dots = (sets @ rows.T).astype(np.float32) + np.float32(0.0) if n else np.zeros((M, 0), np.float32)
    best = np.full((M, n_groups), -np.inf, np.float32)
    best_row = np.full((M, n_groups), -1, np.int64)
    for g in np.unique(col[ok]):
        mine = np.nonzero(ok & (col == g))[0]               # ascending rows
        sub = dots[:, mine]
        at = np.argmax(sub, axis=1)                         # argmax: the first (lowest row) of equal maxima
        best[:, g] = sub[np.arange(M), at]
        best_row[:, g] = mine[at]
    return best, best_row


def related_groups(sets, set_off, rows, group_of_row, n_groups, k, threshold, exclude=None, alive=None):
    """the five outputs of mmrag_related_groups: (similarity [S, k] float32, group [S, k] int32, covered [S, k] int32,
    best [M, k] float32, best_row [M, k] int64) and, for the tests' tolerance, (all_similarity [S, n_groups] float32 with
    -inf where the group is no candidate, best_all [M, n_groups])"""
    sets = np.asarray(sets)
    M, S = sets.shape[0], len(set_off) - 1
    best_all, row_all = best_matches(sets, rows, group_of_row, n_groups, alive)
    thr = np.float32(threshold)
    sim = np.full((S, k), -np.inf, np.float32)
    grp = np.full((S, k), -1, np.int32)
    cov = np.zeros((S, k), np.int32)
    best = np.full((M, k), -np.inf, np.float32)
    best_row = np.full((M, k), -1, np.int64)
    all_sim = np.full((S, n_groups), -np.inf, np.float32)
    for s in range(S):
        lo, hi = int(set_off[s]), int(set_off[s + 1])
        if hi <= lo:
            continue
        for g in range(n_groups):
            if row_all[lo, g] < 0 or (exclude is not None and exclude[s] == g):
                continue
            total = 0.0
            for a in range(lo, hi):                          # sequential, ascending a
                total += float(best_all[a, g])
            all_sim[s, g] = np.float32(total / (hi - lo))
        cand = np.nonzero(all_sim[s] > -np.inf)[0]
        # similarity descending, ties to the lower ordinal (-0 and +0 tie)
        order = sorted(cand.tolist(), key=lambda g: (-float(all_sim[s, g]), g))[:k]
        for j, g in enumerate(order):
            sim[s, j] = all_sim[s, g] + np.float32(0.0)
            grp[s, j] = g
            cov[s, j] = int(np.sum(best_all[lo:hi, g] >= thr))
            best[lo:hi, j] = best_all[lo:hi, g]
            best_row[lo:hi, j] = row_all[lo:hi, g]
    return (sim, grp, cov, best, best_row), (all_sim, best_all)


def chunk_topk_groups(sets, rows, group_of_row, depth, alive=None):
    """the workaround the feature replaces: for each vector of `sets`, the set of groups that own one of its `depth`
    best rows (the groups a merge of per-chunk top-k lists can see at all)"""
    dots = np.asarray(sets, np.float64) @ np.asarray(rows, np.float64).T
    col = np.asarray(group_of_row)
    if alive is not None:
        dots[:, ~np.asarray(alive, bool)] = -np.inf
    dots[:, col < 0] = -np.inf
    seen = []
    for a in range(dots.shape[0]):
        top = np.argsort(-dots[a], kind="stable")[:depth]
        seen.append(set(col[top[np.isfinite(dots[a, top])]].tolist()))
    return seen
