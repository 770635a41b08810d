"""NumPy model of semantic chunking (include/mmrag.h mmrag_chunk_boundaries; csrc/chunk.hip): the partition of n
sentences into admissible chunks of greatest total gain.

  chunk [a, b) admissible:  b - a <= W  and  (b - a == 1  or  cost[a:b].sum() <= max_cost)
  gain(a, b) = sum_{a <= i < j < b} (S_ij - tau) - beta
  best[0] = 0;  best[b] = max over admissible a in [b - W, b) of best[a] + gain(a, b);  ties to the lowest a

`segment` follows the kernel's order of operations in the dtype it is given, so with np.float32 it is the kernel bit
for bit on data whose S is exact, and with np.float64 it is the reference the float32 results are bounded against.
Only S_ij with i < j is read.
"""
import itertools

import numpy as np


def similarities(X):
    """S = X X^T in float64 (X: the stored numbers)"""
    X = np.asarray(X, np.float64)
    return X @ X.T


def auto_tau(S, auto_scale, dtype=np.float64):
    """auto_scale * mean adjacent similarity in the kernel's order: one accumulator over ascending i, a division by
    n - 1, a multiplication; 0 for a single sentence"""
    f = np.dtype(dtype).type
    n = len(S)
    if n < 2:
        return f(0.0)
    acc = f(0.0)
    for i in range(n - 1):
        acc = f(acc + f(S[i, i + 1]))
    return f(f(auto_scale) * f(acc / f(n - 1)))


def segment(S, cost, max_cost, W, tau, beta, dtype=np.float64, stats=None):
    """-> (prev [n] int: prev[b - 1] is the start of the best chunk that ends at b, best [n]: best[b - 1] = best[b]).
    `stats` (a dict): stats["peak"] becomes the largest magnitude among the partial sums and differences formed"""
    f = np.dtype(dtype).type
    n = len(S)
    S = np.asarray(S).astype(dtype)
    tau, beta = f(tau), f(beta)
    csum = np.concatenate([[0], np.cumsum(np.asarray(cost, np.int64))])
    # R[a, b] = sum_{j = a+1}^{b-1} (S_aj - tau), ascending j in one accumulator, for b - a <= W
    # (np.cumsum accumulates strictly in order in the dtype it is given; the leading 0 makes the first step 0 + x)
    R = np.zeros((n, n + 1), dtype)
    for a in range(n):
        hi = min(a + W - 1, n - 1)
        if hi > a:
            R[a, a + 2: hi + 2] = np.cumsum(np.concatenate([[f(0.0)], S[a, a + 1: hi + 1] - tau]), dtype=dtype)[1:]
    best = np.zeros(n + 1, dtype)
    prev = np.zeros(n + 1, np.int64)
    peak = max(float(np.abs(R).max()), float(np.abs(np.triu(S, 1) - tau).max()) if n > 1 else 0.0)
    for b in range(1, n + 1):
        cand = np.arange(b - 1, max(b - W, 0) - 1, -1)       # descending a
        g = np.cumsum(R[cand, b], dtype=dtype)               # G(a, b) = G(a + 1, b) + R_a(b); G(b - 1, b) = 0
        v = best[cand] + (g - beta)
        peak = max(peak, float(np.abs(g).max()), float(np.abs(g - beta).max()), float(np.abs(v).max()))
        ok = (cand == b - 1) | (csum[b] - csum[cand] <= max_cost)
        v = np.where(ok, v, f(-np.inf))
        top = v.max()
        at = np.flatnonzero(v == top)[-1]                    # ties: the lowest a
        best[b], prev[b] = top, cand[at]
    if stats is not None:
        stats["peak"] = peak
    return prev[1:], best[1:]


def cuts_of(prev):
    """the chunk starts, ascending, from prev (read from the end)"""
    out, b = [], len(prev)
    while b > 0:
        b = int(prev[b - 1])
        out.append(b)
    return out[::-1]


def objective(S, cuts, tau, beta):
    """the total gain in float64 of the partition whose chunks start at `cuts` (ascending, cuts[0] == 0)"""
    S = np.asarray(S, np.float64)
    n = len(S)
    total = 0.0
    for a, b in zip(cuts, list(cuts[1:]) + [n]):
        iu = np.triu_indices(b - a, 1)
        total += float((S[a:b, a:b][iu] - float(tau)).sum()) - float(beta)
    return total


def admissible(cuts, n, cost, max_cost, W):
    csum = np.concatenate([[0], np.cumsum(np.asarray(cost, np.int64))])
    return all(b - a <= W and (b - a == 1 or csum[b] - csum[a] <= max_cost)
               for a, b in zip(cuts, list(cuts[1:]) + [n]))


def brute_force(S, cost, max_cost, W, tau, beta):
    """the best objective over all 2^(n-1) partitions (n <= 12) and the partitions that reach it"""
    n = len(S)
    assert 1 <= n <= 12
    top, found = None, []
    for bits in itertools.product((0, 1), repeat=n - 1):
        cuts = [0] + [i + 1 for i, bit in enumerate(bits) if bit]
        if not admissible(cuts, n, cost, max_cost, W):
            continue
        v = objective(S, cuts, tau, beta)
        if top is None or v > top:
            top, found = v, [cuts]
        elif v == top:
            found.append(cuts)
    return top, found
