"""Plain numpy definition of late-interaction (MaxSim) scoring (csrc/maxsim.hip, multimodal_rag_amd/late.py), in float64
from the rows as stored: per query token the maximum dot product over the passage's tokens and the LOWEST passage token
that attains it, their sum in ascending query-token order, and the mean."""
import numpy as np


def maxsim(q_rows: np.ndarray, d_rows: np.ndarray):
    """q_rows [q_len, dim], d_rows [d_len, dim] -> (best_sim [q_len] float64, best_idx [q_len] int, sum, mean)"""
    q = np.asarray(q_rows, np.float64)
    d = np.asarray(d_rows, np.float64)
    sims = q @ d.T                               # [q_len, d_len]
    best_idx = np.argmax(sims, axis=1)           # numpy's argmax returns the first (lowest) index of the maximum
    best_sim = sims[np.arange(len(q)), best_idx]
    total = 0.0
    for v in best_sim:                           # ascending i, starting from 0.0
        total += float(v)
    return best_sim, best_idx.astype(np.int64), total, total / len(q)


def sims(q_rows: np.ndarray, d_rows: np.ndarray) -> np.ndarray:
    """the whole [q_len, d_len] float64 similarity matrix (for checks that accept any index within a tolerance)"""
    return np.asarray(q_rows, np.float64) @ np.asarray(d_rows, np.float64).T


def score_tables(q_tok, d_tok, q_start, q_len, d_start, d_len, pair_q, pair_d):
    """the reference over the kernel's own tables: a list with one maxsim(...) tuple per pair"""
    out = []
    for a, b in zip(pair_q, pair_d):
        qs, ql, ds, dl = int(q_start[a]), int(q_len[a]), int(d_start[b]), int(d_len[b])
        out.append(maxsim(q_tok[qs: qs + ql], d_tok[ds: ds + dl]))
    return out
