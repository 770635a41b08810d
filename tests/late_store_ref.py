"""Plain numpy definition of exact MaxSim retrieval over a token plane (csrc/maxsim_scan.hip, include/mmrag.h
mmrag_maxsim_topk): item i owns rows item_off[i] .. item_off[i + 1] of the plane; a question's score against an item is
tests/late_ref.maxsim's sum (float64 from the rows as stored, ascending query-token order); its winners are the k
candidate items of highest score, descending, ties to the LOWER item, (-inf, -1) padded."""
import numpy as np

from tests import late_ref

MAX_QUERY_TOKENS = 128
MAX_DOC_TOKENS = 512


def candidates(item_off, alive=None, max_doc_tokens=MAX_DOC_TOKENS):
    """bool [n_items]: length in 1..max_doc_tokens and, with `alive` (bool per item), alive"""
    off = np.asarray(item_off, np.int64)
    lens = off[1:] - off[:-1]
    ok = (lens >= 1) & (lens <= max_doc_tokens)
    if alive is not None:
        ok &= np.asarray(alive, bool)[: len(ok)]
    return ok


def score_matrix(q_tok, q_start, q_len, tok, item_off, alive=None):
    """float64 [Q, n_items]: the MaxSim sum of every (question, candidate item), -inf for an item that is no candidate
    and for every item of a bad question (length outside 1..128 or rows outside q_tok)"""
    q_tok, tok = np.asarray(q_tok, np.float64), np.asarray(tok, np.float64)
    off = np.asarray(item_off, np.int64)
    ok = candidates(off, alive)
    out = np.full((len(q_start), len(off) - 1), -np.inf)
    for q, (s, n) in enumerate(zip(q_start, q_len)):
        s, n = int(s), int(n)
        if not 1 <= n <= MAX_QUERY_TOKENS or s < 0 or s + n > len(q_tok):
            continue
        sims = q_tok[s: s + n] @ tok.T                       # [n, T]
        for i in np.nonzero(ok)[0]:
            best = sims[:, off[i]: off[i + 1]].max(axis=1)
            total = 0.0
            for v in best:                                   # ascending i, starting from 0.0
                total += float(v)
            out[q, i] = total
    return out


def topk_of_scores(scores, k):
    """(float64 [Q, k], int64 [Q, k]) of a [Q, n_items] score matrix in which -inf marks "no candidate": score
    descending, ties to the lower item, (-inf, -1) padded"""
    Q, n = scores.shape
    out_s = np.full((Q, k), -np.inf)
    out_i = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        items = [i for i in range(n) if scores[q, i] != -np.inf]
        items.sort(key=lambda i: (-scores[q, i], i))
        items = items[:k]
        out_s[q, : len(items)] = scores[q, items]
        out_i[q, : len(items)] = items
    return out_s, out_i


def topk(q_tok, q_start, q_len, tok, item_off, k, alive=None):
    return topk_of_scores(score_matrix(q_tok, q_start, q_len, tok, item_off, alive), k)


def topk_by_pairs(q_tok, q_start, q_len, tok, item_off, k, alive=None):
    """the same answer from a loop over late_ref.score_tables, one (question, item) pair at a time"""
    off = np.asarray(item_off, np.int64)
    ok = candidates(off, alive)
    scores = np.full((len(q_start), len(off) - 1), -np.inf)
    for q in range(len(q_start)):
        if not 1 <= int(q_len[q]) <= MAX_QUERY_TOKENS or q_start[q] < 0 or q_start[q] + q_len[q] > len(q_tok):
            continue
        items = np.nonzero(ok)[0]
        ref = late_ref.score_tables(np.asarray(q_tok), np.asarray(tok), q_start, q_len, off[:-1], off[1:] - off[:-1],
                                    [q] * len(items), items)
        for i, (_, _, total, _) in zip(items, ref):
            scores[q, i] = total
    return topk_of_scores(scores, k)
