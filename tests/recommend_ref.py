"""numpy reference of recommend retrieval (csrc/recommend.hip): positive and negative examples, ranked in one pass.

A request owns 16 example slots with a sign each (+1 positive, -1 negative, 0 unused).  For a live row x, with float64
dots of the float32 inputs:

    pos   = max over the positive examples of <e, x>
    neg   = max over the negative examples of <e, x>        (no negatives: 0)
    final = float32(pos - float64(w) * max(neg, 0))

ranked by (-final, row); (-inf, -1) padded.  Also the explain outputs of the hits: float32(pos), float32(neg) and the
slots 0..15 that gave them (the lowest slot on equal dots, -1 for none); 0 / -1 in padding."""
import numpy as np

E = 16


def pack(positives, negatives, d):
    """ragged float32 example lists -> (examples [16 R, d] float32, sign int8 [16 R]): positives first, then negatives"""
    R = len(positives)
    ex = np.zeros((E * R, d), np.float32)
    sign = np.zeros(E * R, np.int8)
    for g in range(R):
        pos = list(positives[g])
        neg = list(negatives[g]) if negatives is not None and negatives[g] is not None else []
        assert pos and len(pos) + len(neg) <= E
        for j, e in enumerate(pos + neg):
            ex[E * g + j] = e
            sign[E * g + j] = 1 if j < len(pos) else -1
    return ex, sign


def recommend_topk(examples, sign, weight, c, k, alive=None, row_offset=0):
    examples = np.asarray(examples, np.float32)
    c = np.asarray(c, np.float32)
    sign = np.asarray(sign).reshape(-1, E)
    R, n = sign.shape[0], c.shape[0]
    weight = np.broadcast_to(np.asarray(weight, np.float32), (R,))
    live = np.ones(n, bool) if alive is None else np.asarray(alive, bool)
    rows = np.nonzero(live)[0]
    scores = np.full((R, k), -np.inf, np.float32)
    out_rows = np.full((R, k), -1, np.int64)
    pos_o, neg_o = np.zeros((R, k), np.float32), np.zeros((R, k), np.float32)
    pa_o, na_o = np.full((R, k), -1, np.int32), np.full((R, k), -1, np.int32)
    for g in range(R):
        ex = examples[E * g: E * (g + 1)].astype(np.float64)
        dots = ex @ c.astype(np.float64).T if n else np.zeros((E, 0))      # [16, n]
        ps, ns = np.nonzero(sign[g] > 0)[0], np.nonzero(sign[g] < 0)[0]
        assert ps.size
        pos = dots[ps].max(axis=0)
        p_arg = ps[dots[ps].argmax(axis=0)]              # the first (lowest) slot on equal dots
        if ns.size:
            neg = dots[ns].max(axis=0)
            n_arg = ns[dots[ns].argmax(axis=0)]
        else:
            neg, n_arg = np.zeros(n), np.full(n, -1)
        final = (pos - np.float64(weight[g]) * np.maximum(neg, 0.0)).astype(np.float32)
        order = rows[np.lexsort((rows, -final[rows]))][:k]
        m = order.size
        scores[g, :m] = final[order]
        out_rows[g, :m] = order + row_offset
        pos_o[g, :m], neg_o[g, :m] = pos[order], neg[order]
        pa_o[g, :m], na_o[g, :m] = p_arg[order], n_arg[order]
    return scores, out_rows, pos_o, neg_o, pa_o, na_o
