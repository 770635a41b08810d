"""Plain numpy float64 reference of topic clustering (csrc/kmeans.hip, VectorIndex.cluster): the nearest-centroid
assignment with its margin, the per-cluster sums, the Lloyd loop of VectorIndex.cluster step for step, and the data
recipes the GPU tests share.  Everything is computed in float64 from the rows as stored.

How a set-valued result is compared.  The kernel's scores are float32 sums, each within TOL of the float64 dot.  Two
scores that are each within TOL of the truth can swap order only if their true values are closer than 2 * TOL = BAND,
so a row whose float64 margin (best minus second best) is at least BAND must get the reference's centroid, and a row
inside the band may get any centroid whose float64 score is within BAND of the best.

MAX_BAND_SHARE caps the share of rows inside the band so that the band cannot hide a failure; it is a cap, not a
measurement.  Measured on a CPU with random unit rows, centroids drawn from the rows and fp16 / bf16 / fp32 storage:
the share of rows whose float64 margin is below 2e-3 was at most 0.13 (at d=768, k=300); the share grows linearly with
the band width, so at 2e-4 it is about 0.013.  Every case picks its seed as tests/test_dedup_gpu.py::case does -- the
first of a fixed sequence for which the reference alone stays under the cap -- and asserts the cap again where the
data is used."""
import numpy as np

from tests import dedup_ref

TORCH_DT = dedup_ref.TORCH_DT
stored = dedup_ref.stored
TOL = dedup_ref.TOL          # 1e-4: the project's score tolerance, every dtype
BAND = 2 * TOL
MAX_BAND_SHARE = 0.05


# ---------------------------------------------------------------- the two device steps
def assign(x64: np.ndarray, c64: np.ndarray, alive=None):
    """(arg, best, margin) per row: the LOWEST index at the maximum of x . c^T, that maximum, and best minus second best
    (+inf for k = 1).  A dead row holds (-1, -inf, +inf)."""
    n, k = len(x64), len(c64)
    s = x64 @ c64.T
    arg = np.argmax(s, axis=1).astype(np.int64) if n else np.zeros(0, np.int64)     # argmax: the first maximum
    best = s[np.arange(n), arg] if n else np.zeros(0)
    if k > 1 and n:
        rest = s.copy()
        rest[np.arange(n), arg] = -np.inf
        margin = best - rest.max(axis=1)
    else:
        margin = np.full(n, np.inf)
    if alive is not None:
        dead = ~np.asarray(alive, bool)
        arg[dead], best[dead], margin[dead] = -1, -np.inf, np.inf
    return arg, best, margin


def sums(x64: np.ndarray, labels: np.ndarray, k: int) -> np.ndarray:
    """[k, d] float64 sum of the rows of each label 0 .. k-1 (labels < 0 are left out)"""
    out = np.zeros((k, x64.shape[1]))
    keep = labels >= 0
    np.add.at(out, labels[keep], x64[keep])
    return out


def band_share(margin: np.ndarray, alive=None) -> float:
    m = margin if alive is None else margin[np.asarray(alive, bool)]
    return float(np.mean(m < BAND)) if len(m) else 0.0


# ---------------------------------------------------------------- the loop of VectorIndex.cluster
def lloyd(x: np.ndarray, dtype: str, init_rows, alive=None, max_iter: int = 25, tol: float = 1e-3):
    """Spherical k-means exactly as VectorIndex.cluster runs it, in float64 over the rows as stored.  Each iteration:
    round the master centroids to `dtype`, assign, count the rows that changed cluster; stop (converged) when at most
    tol * live rows changed and no cluster is empty; else every centroid becomes sum / |sum| of its members, and an
    empty (or zero-sum) cluster, in index order, takes the alive row with the lowest score (ties to the lower row,
    distinct rows).  After max_iter iterations without convergence one more assign follows.
    Returns {"labels": the labels of every assign, "objective", "iterations", "converged", "centroids" (master),
    "min_margin": the smallest margin of an alive row in any assign (to centroids that differ from the winner),
    "min_reseed_gap": the smallest gap between
    consecutive scores among the (re-seeded + 1) lowest wherever a re-seed happened (+inf if none did)}."""
    x64 = stored(x, dtype)
    n = len(x64)
    alive = np.ones(n, bool) if alive is None else np.asarray(alive, bool)
    m = int(alive.sum())
    k = len(init_rows)
    C = x64[np.asarray(init_rows, np.int64)].copy()
    prev = np.full(n, -1, np.int64)
    out = {"labels": [], "objective": [], "converged": False, "min_margin": np.inf, "min_reseed_gap": np.inf}

    def step():
        cs = stored(C.astype(np.float32), dtype)
        arg, best, _ = assign(x64, cs, alive)
        out["labels"].append(arg.copy())
        out["objective"].append(float(best[alive].mean()))
        # the margin to the best centroid that is not a copy of the winner: a copy scores the same in any arithmetic,
        # so between the two the tie rule decides, not the rounding
        s = x64[alive] @ cs.T
        s[(cs[arg[alive]][:, None, :] == cs[None, :, :]).all(axis=2)] = -np.inf
        out["min_margin"] = min(out["min_margin"], float((best[alive] - s.max(axis=1)).min()))
        return arg, best

    for _ in range(max_iter):
        arg, best = step()
        changed = int((arg != prev).sum())
        prev = arg
        S = sums(x64, arg, k)
        nrm = np.linalg.norm(S, axis=1)
        bad = (np.bincount(arg[alive], minlength=k) == 0) | (nrm == 0)
        if changed <= tol * m and not bad.any():
            out["converged"] = True
            break
        C = S / np.where(nrm > 0, nrm, 1.0)[:, None]
        if bad.any():
            rows = np.nonzero(alive)[0]
            order = rows[np.lexsort((rows, best[rows]))]          # score ascending, ties to the lower row
            nb = int(bad.sum())
            lowest = best[order[: nb + 1]]
            if len(lowest) > 1:
                out["min_reseed_gap"] = min(out["min_reseed_gap"], float(np.diff(lowest).min()))
            C[np.nonzero(bad)[0]] = x64[order[:nb]]
    out["iterations"] = len(out["labels"])
    if not out["converged"]:
        step()
    out["centroids"] = C
    return out


# ---------------------------------------------------------------- data recipes
def unit_rows(n: int, d: int, seed: int, dtype: str) -> np.ndarray:
    """float32 unit Gaussian rows already rounded to `dtype`"""
    x = np.random.default_rng(seed).standard_normal((n, d))
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
    return stored(x, dtype).astype(np.float32)


def centroids_of(x: np.ndarray, k: int, seed: int, dtype: str) -> np.ndarray:
    """k of the rows (distinct), re-normalised and rounded to `dtype`, float32"""
    picks = np.random.default_rng(seed + 7919).choice(len(x), k, replace=False)
    c = x[picks].astype(np.float64)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    return stored(c, dtype).astype(np.float32)


def blobs(n_blobs: int, per: int, d: int, seed: int, dtype: str, min_cos: float = 0.95, max_between: float = 0.3):
    """(rows float32 rounded to dtype [n_blobs * per, d], blob of each row, centres): unit centres whose pairwise
    cosine is at most max_between, members at cosine >= min_cos to their own centre; blob b owns rows b * per ..."""
    g = np.random.default_rng(seed)
    while True:
        centres = g.standard_normal((n_blobs, d))
        centres /= np.linalg.norm(centres, axis=1, keepdims=True)
        gram = centres @ centres.T - np.eye(n_blobs)
        if np.abs(gram).max() <= max_between:
            break
    rows, owner = [], []
    for b in range(n_blobs):
        for _ in range(per):
            u = g.standard_normal(d)
            u -= (u @ centres[b]) * centres[b]
            u /= np.linalg.norm(u)
            c = g.uniform(min_cos + 0.01, 0.995)
            rows.append(c * centres[b] + np.sqrt(1 - c * c) * u)
            owner.append(b)
    x = stored(np.asarray(rows), dtype).astype(np.float32)
    return x, np.asarray(owner), centres
