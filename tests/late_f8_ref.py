"""The float64 definition of MaxSim over FP8 token rows (include/mmrag.h mmrag_maxsim_scores_f8 / mmrag_maxsim_topk_f8):
both sides are rows of E4M3 codes (tests/f8_ref.py); a similarity is the dot product of the decoded values times 2^-16,
and everything else is tests/late_ref.py's and tests/late_store_ref.py's definition applied to the decoded rows."""
import numpy as np

from tests import f8_ref, late_ref, late_store_ref


def encode_rows(x, ld=None):
    """code rows [m, ld] (uint8) of float rows x [m, d]: f8_ref.encode, pad columns code 0; ld defaults to the padded dim"""
    x = np.asarray(x, np.float32)
    d = x.shape[1]
    ld = (d + 127) // 128 * 128 if ld is None else ld
    out = np.zeros((x.shape[0], ld), np.uint8)
    out[:, :d] = f8_ref.encode(x)
    return out


def values(codes):
    """what a code row stands for: decode / 256 (exact in float64), so plain dot products are the similarities"""
    return f8_ref.decode(codes) / f8_ref.SCALE


def score_matrix(q_codes, q_start, q_len, codes, item_off, alive=None):
    return late_store_ref.score_matrix(values(q_codes), q_start, q_len, values(codes), item_off, alive)


def topk(q_codes, q_start, q_len, codes, item_off, k, alive=None):
    return late_store_ref.topk_of_scores(score_matrix(q_codes, q_start, q_len, codes, item_off, alive), k)


def score_tables(q_codes, d_codes, q_start, q_len, d_start, d_len, pair_q, pair_d):
    """late_ref.score_tables over the decoded rows: one (best_sim, best_idx, sum, mean) per pair"""
    return late_ref.score_tables(values(q_codes), values(d_codes), q_start, q_len, d_start, d_len, pair_q, pair_d)
