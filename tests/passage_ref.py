"""The numpy definition of windowed MaxSim (include/mmrag.h mmrag_maxsim_windows), twice.

`windows` is the contract as written: block maxima, windows of whole blocks, float32 sums in ascending i, the lowest
start of the largest sum, the tight span.  `windows_by_tokens` is an independent formulation with no block table: per
window a brute-force maximum over the TOKENS 16 s .. 16 (s + w) clipped to d_len, and a tight span found from token
positions.  tests/test_passages_cpu.py holds the two equal.

Both take the similarity matrix S [q_len, d_len]; `sims` forms it from rows in float64 (exact for the integer rows of the
tests; the GPU tests that need the kernel's own float32 bits pass their own S)."""
import numpy as np

BLOCK = 16          # MMRAG_LATE_WINDOW_TOKENS
SLOTS = 32          # MMRAG_MAX_LATE_WINDOWS


def sims(q, d):
    """S[i][j] = <q_i, d_j> in float64"""
    return np.asarray(q, np.float64) @ np.asarray(d, np.float64).T


def _sum_f32(values):
    """the float32 sum in ascending order starting from 0.0f"""
    # cumsum adds one element after the other in the dtype given
    return np.cumsum(np.concatenate([[0.0], np.asarray(values, np.float64)]).astype(np.float32), dtype=np.float32)[-1]


def windows(S, w):
    """-> (out_sum float32, out_win [32] float32, out_best (start, first, last)) of one pair, by blocks"""
    S = np.asarray(S)
    q_len, d_len = S.shape
    assert 1 <= w <= SLOTS and 1 <= d_len <= BLOCK * SLOTS and q_len >= 1
    nb = -(-d_len // BLOCK)
    bm = np.stack([S[:, BLOCK * g: min(BLOCK * g + BLOCK, d_len)].max(axis=1) for g in range(nb)], axis=1)
    out_sum = _sum_f32(bm.max(axis=1))
    out_win = np.full(SLOTS, -np.inf, np.float32)
    for s in range(max(nb - w, 0) + 1):
        out_win[s] = _sum_f32(bm[:, s: min(s + w, nb)].max(axis=1))
    start = int(np.argmax(out_win))             # argmax: the first (lowest) of equal maxima
    inside = bm[:, start: min(start + w, nb)]
    lowest = start + np.argmax(inside == inside.max(axis=1, keepdims=True), axis=1)
    return out_sum, out_win, (start, int(lowest.min()), int(lowest.max()))


def windows_by_tokens(S, w):
    """the same outputs without a block table: every window is a range of tokens"""
    S = np.asarray(S)
    q_len, d_len = S.shape
    out_sum = _sum_f32([S[i].max() for i in range(q_len)])
    out_win = np.full(SLOTS, -np.inf, np.float32)
    s, best, best_s = 0, None, -1
    while True:
        lo, hi = BLOCK * s, min(BLOCK * (s + w), d_len)
        out_win[s] = _sum_f32([S[i, lo:hi].max() for i in range(q_len)])
        if best is None or out_win[s] > best:       # strictly greater: the first of equal sums stays
            best, best_s = out_win[s], s
        if hi >= d_len:
            break
        s += 1
    lo, hi = BLOCK * best_s, min(BLOCK * (best_s + w), d_len)
    # per query token the FIRST token of the window that attains its maximum there, as a block
    blocks = [(lo + int(np.flatnonzero(S[i, lo:hi] == S[i, lo:hi].max())[0])) // BLOCK for i in range(q_len)]
    return out_sum, out_win, (best_s, min(blocks), max(blocks))


def windows_of_tables(q_rows, d_rows, q_start, q_len, d_start, d_len, pair_q, pair_d, w):
    """`windows` for every pair of maxsim_scores-style tables over float rows: a list of (out_sum, out_win, out_best)"""
    out = []
    for a, b in zip(pair_q, pair_d):
        q = q_rows[q_start[a]: q_start[a] + q_len[a]]
        d = d_rows[d_start[b]: d_start[b] + d_len[b]]
        out.append(windows(sims(q, d), w))
    return out
