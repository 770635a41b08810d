"""numpy reference of boosted retrieval (csrc/boosted.hip): cosine plus a per-row score prior, ranked in one pass.

    final[b][r] = float32(dot64(q_b, x_r) + float64(w_b) * float64(prior[r]))

over the float32 inputs; ranked by (-final, row); (-inf, -1) padded.  Also the boosts float32(w_b * prior[r]) of the hits
(0.0 in padding)."""
import numpy as np


def boosted_topk(q, c, k, prior, weight, alive=None, row_offset=0):
    q = np.asarray(q, np.float32)
    c = np.asarray(c, np.float32)
    prior = np.asarray(prior, np.float32)
    B, n = q.shape[0], c.shape[0]
    weight = np.broadcast_to(np.asarray(weight, np.float32), (B,))
    dots = q.astype(np.float64) @ c.astype(np.float64).T if n else np.zeros((B, 0))
    final = (dots + weight.astype(np.float64)[:, None] * prior.astype(np.float64)[None, :]).astype(np.float32)
    live = np.ones(n, bool) if alive is None else np.asarray(alive, bool)
    rows = np.nonzero(live)[0]
    scores = np.full((B, k), -np.inf, np.float32)
    out_rows = np.full((B, k), -1, np.int64)
    boosts = np.zeros((B, k), np.float32)
    for b in range(B):
        order = rows[np.lexsort((rows, -final[b, rows]))][:k]
        m = order.size
        scores[b, :m] = final[b, order]
        out_rows[b, :m] = order + row_offset
        boosts[b, :m] = weight[b] * prior[order]        # float32 * float32, rounded once
    return scores, out_rows, boosts
