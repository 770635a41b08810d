"""float64 reference of extractive selection by sentence centrality (include/mmrag.h mmrag_summary_select), for the
tests.

One unit: rows x_0 .. x_{n-1} as numbers, integer costs, an integer budget, optionally a bias row q.
  S = X X^T, s = X q;  W_ij = S_ij if i != j and S_ij >= t, else 0;  deg_j = sum_i W_ij, inv_j = 1 / deg_j or 0;
  b = 1 / n, or max(s, 0) / sum(max(s, 0)) when that sum is positive;
  p = b, then exactly T steps of p' = alpha b + (1 - alpha) W (p * inv);  rel = p / max(p);
  selection: among the free i with cost_i <= remaining the largest v_i = lam rel_i - (1 - lam) red_i, ties to the lower
  i; then remaining -= cost_i and red = max(red, max(S_i, 0)).
alpha, 1 - alpha, lam, 1 - lam and t are the float32 values the kernel uses (1 - x is rounded to float32 first),
widened; everything else is float64.
"""
import numpy as np


def weights(x):
    """(x, 1 - x) as the float32 numbers of the definition, widened to float64"""
    x32 = np.float32(x)
    return float(x32), float(np.float32(1.0) - x32)


def similarities(X, q=None):
    """(S [n, n], s [n] or None) in float64"""
    X = np.asarray(X, np.float64)
    return X @ X.T, (None if q is None else X @ np.asarray(q, np.float64))


def prior(n, s=None):
    b = np.full(n, 1.0 / n)
    if s is not None:
        r = np.maximum(s, 0.0)
        if r.sum() > 0:
            b = r / r.sum()
    return b


def centrality(S, s, t, alpha, T):
    """rel [n] of one unit"""
    n = S.shape[0]
    t = float(np.float32(t))
    a, oma = weights(alpha)
    W = np.where((S >= t) & ~np.eye(n, dtype=bool), S, 0.0)
    deg = W.sum(axis=0)
    inv = np.where(deg > 0, 1.0 / np.where(deg > 0, deg, 1.0), 0.0)
    b = prior(n, s)
    p = b.copy()
    for _ in range(int(T)):
        p = a * b + oma * (W @ (p * inv))
    return p / p.max()


def step_values(rel, S, cost, remaining, picked, lam):
    """(v [n] float64, eligible [n] bool) of one selection step, given the positions picked so far (in any order) and
    what is left of the budget after them"""
    rel = np.asarray(rel, np.float64)
    a, b = weights(lam)
    red = np.zeros(len(rel))
    if len(picked):
        red = np.maximum(S[list(picked)], 0.0).max(axis=0)
    free = np.ones(len(rel), bool)
    free[list(picked)] = False
    return a * rel - b * red, free & (np.asarray(cost) <= remaining)


def select(rel, S, cost, budget, k, lam):
    """(positions, values, used): the picks in order, v at each pick, the cost spent"""
    cost = np.asarray(cost)
    remaining, pos, val = int(budget), [], []
    while len(pos) < int(k):
        v, ok = step_values(rel, S, cost, remaining, pos, lam)
        idx = np.nonzero(ok)[0]
        if idx.size == 0:
            break
        i = int(idx[np.argmax(v[idx])])      # argmax returns the first maximum: ties to the lower position
        pos.append(i)
        val.append(float(v[i]))
        remaining -= int(cost[i])
    return pos, val, int(budget) - remaining


def summarize(X, cost, budget, k, t, alpha, T, lam, q=None):
    """the whole definition for one unit: (rel, positions, values, used)"""
    S, s = similarities(X, q)
    rel = centrality(S, s, t, alpha, T)
    pos, val, used = select(rel, S, cost, budget, k, lam)
    return rel, pos, val, used


def margins(rel, S, cost, budget, lam, picks):
    """for every step of `picks` (positions in order, e.g. a kernel's): (v of the pick, best eligible v, the margin
    between the best and the second-best eligible v -- inf when only one is eligible, whether the pick was eligible),
    each step given the earlier picks of the SAME list"""
    cost = np.asarray(cost)
    remaining, out = int(budget), []
    for at, i in enumerate(picks):
        v, ok = step_values(rel, S, cost, remaining, picks[:at], lam)
        idx = np.nonzero(ok)[0]
        order = np.sort(v[idx])[::-1]
        margin = float(order[0] - order[1]) if order.size > 1 else float("inf")
        best = float(order[0]) if order.size else float("-inf")
        out.append((float(v[i]), best, margin, bool(ok[i]), int(idx[np.argmax(v[idx])]) if order.size else -1))
        remaining -= int(cost[i])
    return out, remaining
