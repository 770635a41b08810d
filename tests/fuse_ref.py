"""Reference of multi-query fusion: a numpy float32 restatement of the definition in include/mmrag.h at
mmrag_fuse_select (one plain dict per group, sequential float32 adds in list order, np.float32 division), and a float64
brute force that checks the ordering logic only."""
import numpy as np

MAX_LISTS, MAX_CANDIDATES, MAX_RESULTS = 16, 256, 4096
RRF, MAX = 0, 1
METHODS = {"rrf": RRF, "max": MAX}


def fuse_group(scores, rows, weights, method, rrf_k, n):
    """one group: scores [nl, C] float32, rows [nl, C] int64, weights [nl] float32 or None.  Returns (fused [n] float32,
    rows [n] int64, best [n] float32, best_list [n] int32, count [n] int32, info [2] int32), padded with
    (-inf, -1, -inf, -1, 0)"""
    scores, rows = np.asarray(scores, np.float32), np.asarray(rows, np.int64)
    acc, valid = {}, 0                                       # row -> [fused, best, best_list, count]
    for l in range(len(rows)):
        w = np.float32(1.0) if weights is None else np.float32(weights[l])
        seen = set()
        for p in range(rows.shape[1]):
            r = int(rows[l, p])
            if r < 0:
                break                                        # the list ends at its first row < 0
            valid += 1
            if r in seen:
                continue                                     # only a row's first occurrence in a list counts
            seen.add(r)
            s = scores[l, p]
            c = w / np.float32(rrf_k + p + 1) if method == RRF else w * s
            assert type(c) is np.float32
            cur = acc.get(r)
            if cur is None:
                acc[r] = [c, s, l, 1]
                continue
            if method == RRF:
                cur[0] = cur[0] + c                          # float32, in ascending list order
            elif c > cur[0]:
                cur[0] = c
            if s > cur[1]:
                cur[1], cur[2] = s, l
            cur[3] += 1
    # negation swaps -0.0 and 0.0, which compare equal: such a pair falls through to the next key
    order = sorted(acc, key=lambda r: (-float(acc[r][0]), -float(acc[r][1]), r))[:n]
    fused = np.full(n, -np.inf, np.float32)
    out_rows = np.full(n, -1, np.int64)
    best = np.full(n, -np.inf, np.float32)
    best_list = np.full(n, -1, np.int32)
    count = np.zeros(n, np.int32)
    for j, r in enumerate(order):
        fused[j], best[j], best_list[j], count[j] = acc[r]
        out_rows[j] = r
    return fused, out_rows, best, best_list, count, np.array([len(acc), valid], np.int32)


def fuse_select(scores, rows, list_off, n, weights=None, method="rrf", rrf_k=60):
    """all groups of a call: the six outputs stacked [G, n] / [G, 2]"""
    m = METHODS[method] if isinstance(method, str) else method
    outs = []
    for g in range(len(list_off) - 1):
        lo, hi = int(list_off[g]), int(list_off[g + 1])
        outs.append(fuse_group(scores[lo:hi], rows[lo:hi], None if weights is None else weights[lo:hi], m, rrf_k, n))
    return tuple(np.stack(col) for col in zip(*outs))


def brute_force(scores, rows, weights, method, rrf_k):
    """order free and in float64: {row: (fused, best, best_list, count)} of one group.  The fused value is exact up to
    float64 rounding, so it agrees with the float32 definition only to float32 accuracy: for the ordering logic"""
    scores, rows = np.asarray(scores, np.float64), np.asarray(rows, np.int64)
    out = {}
    for l in reversed(range(len(rows))):                     # any order will do
        w = 1.0 if weights is None else float(np.float32(weights[l]))
        neg = np.nonzero(rows[l] < 0)[0]
        end = int(neg[0]) if len(neg) else rows.shape[1]
        uniq, first = np.unique(rows[l, :end], return_index=True)
        for r, p in zip(uniq.tolist(), first.tolist()):
            c = w / (rrf_k + p + 1) if method == RRF else float(np.float32(w) * np.float32(scores[l, p]))
            out.setdefault(r, []).append((l, c, float(scores[l, p])))
    res = {}
    for r, got in out.items():
        got.sort()
        fused = sum(c for _, c, _ in got) if method == RRF else max(c for _, c, _ in got)
        top = max(s for _, _, s in got)
        res[r] = (fused, top, min(l for l, _, s in got if s == top), len(got))
    return res
