"""Plain numpy reference of near-duplicate detection (csrc/simjoin.hip, VectorIndex.near_duplicates / add(dedup_threshold)):
the brute-force threshold self-join, the connected components of its pair graph, the greedy ingest rule, and the data
recipe the GPU tests share.  Everything is computed in float64 from the rows as stored."""
import numpy as np
import torch

TORCH_DT = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
T_JOIN = 0.95            # the threshold every pair-set comparison joins at
BAND = 2e-3              # no pair's float64 cosine may lie this close to the threshold (asserted on the reference)
TOL = 1e-4               # tests/test_search_gpu.py: cosine scores within 1e-4, every dtype
COSINES = (1.0, 0.99, 0.97, 0.93, 0.90)


def stored(x: np.ndarray, dtype: str) -> np.ndarray:
    """float32 rows rounded to the storage dtype, back as float64 (what the kernel's dot is over)"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TORCH_DT[dtype]).to(torch.float64).numpy()


def planted_pairs(n: int, extra=()):
    want = [(0, 1), (n // 2 - 1, n // 2), (127, 128), (126, 129), (255, 256), (5, n - 2)] + list(extra)
    out, used = [], set()
    for i, j in want:
        if 0 <= i < j < n and i not in used and j not in used:
            used.update((i, j))
            out.append((i, j))
    return out


def make_rows(n: int, d: int, seed: int, dtype: str, extra=()):
    """(float32 rows [n, d] already rounded to `dtype`, the planted (i, j, c)).  Unit Gaussian rows; partner
    x_j = c x_i + sqrt(1 - c^2) u with u unit and orthogonal to x_i, c cycling through COSINES; then rounded."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d))
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
    planted = []
    for at, (i, j) in enumerate(planted_pairs(n, extra)):
        c = COSINES[at % len(COSINES)]
        u = g.standard_normal(d)
        u -= (u @ x[i]) * x[i]
        u /= np.linalg.norm(u)
        x[j] = c * x[i] + np.sqrt(max(0.0, 1.0 - c * c)) * u
        planted.append((i, j, c))
    rounded = torch.from_numpy(x.astype(np.float32)).to(TORCH_DT[dtype]).to(torch.float32).numpy()
    return rounded, planted


def gram(x64: np.ndarray) -> np.ndarray:
    return x64 @ x64.T


def pairs(x64: np.ndarray, alive, t: float):
    """{(i, j): float64 dot} for i < j, both alive (None = all), dot >= t -- brute force over the stored rows"""
    n = len(x64)
    if n < 2:
        return {}
    g = gram(x64)
    ok = np.triu(np.ones((n, n), bool), 1) & (g >= t)
    if alive is not None:
        a = np.asarray(alive, bool)
        ok &= a[:, None] & a[None, :]
    return {(int(i), int(j)): float(g[i, j]) for i, j in zip(*np.nonzero(ok))}


def band_is_empty(x64: np.ndarray, t: float, band: float = BAND) -> bool:
    """no pair i < j (dead rows included: the stricter statement) has a cosine within `band` of t"""
    n = len(x64)
    if n < 2:
        return True
    g = gram(x64)[np.triu_indices(n, 1)]
    return not bool(np.any(np.abs(g - t) < band))


def components(pair_list):
    """connected components of the pair graph: members ascending, the first (lowest row) is the keeper; components in
    keeper order"""
    adj = {}
    for a, b in pair_list:
        adj.setdefault(a, set()).add(b)
        adj.setdefault(b, set()).add(a)
    seen, out = set(), []
    for start in sorted(adj):
        if start in seen:
            continue
        comp, todo = [], [start]
        seen.add(start)
        while todo:
            v = todo.pop()
            comp.append(v)
            for w in adj[v]:
                if w not in seen:
                    seen.add(w)
                    todo.append(w)
        out.append(sorted(comp))
    return out


def greedy(existing_best, batch_pairs, m: int):
    """the ingest rule, in input order.  existing_best[j]: the stored row that duplicates batch row j, or None;
    batch_pairs: the (i, j), i < j, of the batch's own join.  Returns (kept positions, {skipped j: ("stored", row) or
    ("batch", i)}): j is skipped for a stored duplicate, else for the LOWEST earlier i that pairs with it and is kept."""
    by_j = {}
    for i, j in batch_pairs:
        by_j.setdefault(j, []).append(i)
    kept, skipped, is_kept = [], {}, [False] * m
    for j in range(m):
        if existing_best[j] is not None:
            skipped[j] = ("stored", existing_best[j])
            continue
        first = next((i for i in sorted(by_j.get(j, ())) if is_kept[i]), None)
        if first is not None:
            skipped[j] = ("batch", first)
            continue
        is_kept[j] = True
        kept.append(j)
    return kept, skipped
