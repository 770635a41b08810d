"""float64 reference of maximal-marginal-relevance selection (include/mmrag.h mmrag_mmr_select), for the tests.

One query: candidates c_0 .. c_{C-1} in the dense order with relevance rel_i; the list ends at its first row < 0.
Step 0 picks c_0; step t >= 1 picks the free i that maximises v_i = lam * rel_i - (1 - lam) * max_{j picked} sim(i, j),
ties to the lower i; sim is the dot product of the two stored rows.  lam and 1 - lam are the float32 values the kernel
multiplies with (1 - lam is rounded to float32 first); everything else is float64.
"""
import numpy as np


def weights(lam):
    """(lam, 1 - lam) as the float32 numbers of the definition, widened to float64"""
    lam32 = np.float32(lam)
    return float(lam32), float(np.float32(1.0) - lam32)


def valid_count(rows):
    rows = np.asarray(rows)
    bad = np.nonzero(rows < 0)[0]
    return int(bad[0]) if bad.size else int(rows.size)


def step_values(rel, vectors, picked, lam):
    """v of every candidate given the picked positions (float64 [C]) and the mask of the free ones"""
    rel = np.asarray(rel, np.float64)
    X = np.asarray(vectors, np.float64)
    a, b = weights(lam)
    maxsim = (X @ X[list(picked)].T).max(axis=1)
    free = np.ones(len(rel), bool)
    free[list(picked)] = False
    return a * rel - b * maxsim, free


def select(rel, rows, matrix, k, lam):
    """(positions, values) of the picks of one query, both of length min(k, valid candidates).
    rel [C], rows [C] (-1 tail allowed), matrix [n, d]: the stored rows as numbers (any float dtype)."""
    rows = np.asarray(rows)
    cnt = valid_count(rows)
    n = min(int(k), cnt)
    if n == 0:
        return [], []
    rel = np.asarray(rel, np.float64)[:cnt]
    X = np.asarray(matrix)[rows[:cnt]].astype(np.float64)
    a, b = weights(lam)
    maxsim = np.full(cnt, -np.inf)
    free = np.ones(cnt, bool)
    pos, val = [0], [float(rel[0])]
    free[0] = False
    while len(pos) < n:
        maxsim = np.maximum(maxsim, X @ X[pos[-1]])
        v = a * rel - b * maxsim
        idx = np.nonzero(free)[0]
        i = int(idx[np.argmax(v[idx])])      # argmax returns the first maximum: ties to the lower position
        pos.append(i)
        val.append(float(v[i]))
        free[i] = False
    return pos, val


def select_padded(rel, rows, matrix, k, lam):
    """the kernel's four output rows for one query: (scores f32 [k], rows i64 [k], positions i32 [k], values f32 [k]),
    unused slots (-inf, -1, -1, -inf)"""
    pos, val = select(rel, rows, matrix, k, lam)
    out_s = np.full(k, -np.inf, np.float32)
    out_r = np.full(k, -1, np.int64)
    out_p = np.full(k, -1, np.int32)
    out_v = np.full(k, -np.inf, np.float32)
    m = len(pos)
    out_s[:m] = np.asarray(rel, np.float32)[pos]
    out_r[:m] = np.asarray(rows, np.int64)[pos]
    out_p[:m] = pos
    out_v[:m] = np.asarray(val, np.float64).astype(np.float32)
    return out_s, out_r, out_p, out_v
