"""NumPy float64 restatements of the learned sparse leg (csrc/sparse_expand.hip, csrc/sparse_score.hip, the MLM head
of csrc/encoder.hip), computed from the same fp16-rounded inputs the device reads.  Test infrastructure only."""
import math

import numpy as np

MAX_CHUNK_TOKENS = 512
MAX_TERMS = 256
MAX_QUERY_TERMS = 64


# ---- pool -------------------------------------------------------------------------------------------------------------
def chunk_ok(s: int, e: int, T: int) -> bool:
    return s >= 0 and e > s and e - s <= MAX_CHUNK_TOKENS and e <= T


def pool(tok: np.ndarray, cu, E: np.ndarray) -> np.ndarray:
    """pooled [n_chunks, V] float64: max over the rows of chunk c of <tok_t, E_v>; -inf rows for bad chunks"""
    tok64, E64 = tok.astype(np.float64), E.astype(np.float64)
    cu = [int(x) for x in cu]
    out = np.full((len(cu) - 1, E.shape[0]), -np.inf, np.float64)
    for c in range(len(cu) - 1):
        if chunk_ok(cu[c], cu[c + 1], tok.shape[0]):
            out[c] = (tok64[cu[c]: cu[c + 1]] @ E64.T).max(axis=0)
    return out


def pool_with_bound(tok: np.ndarray, cu, E: np.ndarray):
    """(pooled float64, bound): bound[c][v] = the largest sum_k |h_k e_k| over the chunk's rows -- what the float32
    accumulation error of any of its logits is measured against"""
    tok64, E64 = tok.astype(np.float64), E.astype(np.float64)
    cu = [int(x) for x in cu]
    out = np.full((len(cu) - 1, E.shape[0]), -np.inf, np.float64)
    bound = np.zeros_like(out)
    for c in range(len(cu) - 1):
        if chunk_ok(cu[c], cu[c + 1], tok.shape[0]):
            out[c] = (tok64[cu[c]: cu[c + 1]] @ E64.T).max(axis=0)
            bound[c] = (np.abs(tok64[cu[c]: cu[c + 1]]) @ np.abs(E64).T).max(axis=0)
    return out, bound


# ---- transform + head ---------------------------------------------------------------------------------------------------
_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(x: np.ndarray) -> np.ndarray:
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def layer_norm(x: np.ndarray, g: np.ndarray, b: np.ndarray, eps: float) -> np.ndarray:
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def mlm_transform(hidden: np.ndarray, w: dict, eps: float) -> np.ndarray:
    """cls.predictions.transform: LayerNorm(gelu(hidden . W^T + b)), float64"""
    f = lambda k: np.asarray(w[k], np.float64)  # noqa: E731
    y = gelu(hidden @ f("cls.predictions.transform.dense.weight").T + f("cls.predictions.transform.dense.bias"))
    return layer_norm(y, f("cls.predictions.transform.LayerNorm.weight"), f("cls.predictions.transform.LayerNorm.bias"), eps)


def bert_hidden(w: dict, ids, n_layers: int, n_heads: int, eps: float) -> np.ndarray:
    """last hidden state [S, H] of one un-padded sequence, float64 (HF BertModel semantics, token type 0)"""
    f = lambda k: np.asarray(w[k], np.float64)  # noqa: E731
    ids = np.asarray(ids, np.int64)
    S = ids.size
    x = (f("embeddings.word_embeddings.weight")[ids] + f("embeddings.position_embeddings.weight")[:S]
         + f("embeddings.token_type_embeddings.weight")[0])
    x = layer_norm(x, f("embeddings.LayerNorm.weight"), f("embeddings.LayerNorm.bias"), eps)
    H = x.shape[1]
    dh = H // n_heads
    for l in range(n_layers):
        p = f"encoder.layer.{l}."
        q = x @ f(p + "attention.self.query.weight").T + f(p + "attention.self.query.bias")
        k = x @ f(p + "attention.self.key.weight").T + f(p + "attention.self.key.bias")
        v = x @ f(p + "attention.self.value.weight").T + f(p + "attention.self.value.bias")
        a = np.empty_like(x)
        for h in range(n_heads):
            sl = slice(h * dh, (h + 1) * dh)
            s = q[:, sl] @ k[:, sl].T / math.sqrt(dh)
            s = np.exp(s - s.max(axis=1, keepdims=True))
            a[:, sl] = (s / s.sum(axis=1, keepdims=True)) @ v[:, sl]
        a = a @ f(p + "attention.output.dense.weight").T + f(p + "attention.output.dense.bias")
        x = layer_norm(x + a, f(p + "attention.output.LayerNorm.weight"), f(p + "attention.output.LayerNorm.bias"), eps)
        mid = gelu(x @ f(p + "intermediate.dense.weight").T + f(p + "intermediate.dense.bias"))
        o = mid @ f(p + "output.dense.weight").T + f(p + "output.dense.bias")
        x = layer_norm(x + o, f(p + "output.LayerNorm.weight"), f(p + "output.LayerNorm.bias"), eps)
    return x


def round_matrices_fp16(w: dict) -> dict:
    """what the device stores: matrices in fp16, vectors float32"""
    return {k: (np.asarray(v).astype(np.float16).astype(np.float64) if np.asarray(v).ndim == 2
                else np.asarray(v, np.float32).astype(np.float64)) for k, v in w.items()}


def decoder_rows(w: dict) -> np.ndarray:
    k = "cls.predictions.decoder.weight"
    return np.asarray(w[k] if k in w else w["embeddings.word_embeddings.weight"])


def expand(w: dict, sequences, n_layers: int, n_heads: int, eps: float) -> np.ndarray:
    """pooled [B, V] float64 of whole sequences: max over tokens of the MLM logits WITHOUT the vocabulary bias (the
    bias joins in `weights`, as on the device)"""
    E = np.asarray(decoder_rows(w), np.float64)
    out = []
    for ids in sequences:
        t = mlm_transform(bert_hidden(w, ids, n_layers, n_heads, eps), w, eps)
        out.append((t @ E.T).max(axis=0))
    return np.stack(out)


# ---- activation, quantisation, select -----------------------------------------------------------------------------------
def weights(pooled: np.ndarray, bias: np.ndarray, scale: float) -> np.ndarray:
    """w * scale, float64: log1p(max(pooled + bias, 0)) * scale.  The maximum is fmaxf's: a NaN logit gives
    fmax(NaN, 0) = 0, weight 0 and impact 0; +inf gives an infinite weight and the clamped impact 255; -inf gives 0"""
    x = np.fmax(np.asarray(pooled, np.float64) + np.asarray(bias, np.float64), 0.0)
    return np.log1p(x) * float(scale)


def impacts(pooled, bias, scale: float) -> np.ndarray:
    """min(255, rint(w * scale)) (rint: half to even, as rintf)"""
    return np.minimum(np.rint(weights(pooled, bias, scale)), 255).astype(np.int64)


def select(imp_row: np.ndarray, m: int, skip=None):
    """(terms ascending, their impacts) of one chunk: the m terms of highest impact >= 1, ties to the LOWER term id;
    `skip`: boolean [V] of dropped terms"""
    imp = np.asarray(imp_row, np.int64).copy()
    if skip is not None:
        imp[np.asarray(skip, bool)] = 0
    cand = np.nonzero(imp >= 1)[0]
    order = cand[np.lexsort((cand, -imp[cand]))][:m]       # impact descending, then term ascending
    order = np.sort(order)
    return order.astype(np.int64), imp[order]


def select_batch(imp: np.ndarray, m: int, skip=None):
    """(cnt [n], terms [n, m] padded -1, impacts [n, m] padded 0): mmrag_sparse_select's outputs"""
    n = imp.shape[0]
    cnt = np.zeros(n, np.int32)
    terms = np.full((n, m), -1, np.int32)
    imps = np.zeros((n, m), np.int32)
    for c in range(n):
        t, q = select(imp[c], m, skip)
        cnt[c] = t.size
        terms[c, : t.size] = t
        imps[c, : t.size] = q
    return cnt, terms, imps


def bits_to_bool(words: np.ndarray, V: int) -> np.ndarray:
    w = np.asarray(words).astype(np.uint32)
    return ((w[np.arange(V) >> 5] >> (np.arange(V) & 31).astype(np.uint32)) & 1).astype(bool)


def bool_to_bits(flags: np.ndarray) -> np.ndarray:
    f = np.zeros((len(flags) + 31) // 32 * 32, bool)
    f[: len(flags)] = flags
    return np.packbits(f, bitorder="little").view(np.int32)


# ---- integer impact scoring ---------------------------------------------------------------------------------------------
def scores(off, terms, imps, n_terms: int, q_terms, q_imps) -> np.ndarray:
    """score [n] int64 of one query over a forward log (off [n + 1], terms, imps): sum q_imp * d_imp over shared terms"""
    off = np.asarray(off, np.int64)
    n = off.size - 1
    qw = np.zeros(n_terms, np.int64)
    for t, w in zip(q_terms, q_imps):
        if 0 <= t < n_terms and 1 <= w <= 255:
            qw[t] = w
    contrib = qw[np.asarray(terms, np.int64)] * np.asarray(imps, np.int64)
    row = np.repeat(np.arange(n), np.diff(off))
    return np.bincount(row, weights=contrib.astype(np.float64), minlength=n).astype(np.int64)


def topk(score: np.ndarray, k: int, allowed=None):
    """(scores [k] float32, rows [k] int64): score descending, ties to the lower row, rows with score > 0 and allowed;
    (-inf, -1) padding"""
    ok = score > 0
    if allowed is not None:
        ok &= np.asarray(allowed, bool)
    cand = np.nonzero(ok)[0]
    order = cand[np.lexsort((cand, -score[cand]))][:k]
    s = np.full(k, -np.inf, np.float32)
    r = np.full(k, -1, np.int64)
    s[: order.size] = score[order].astype(np.float32)
    r[: order.size] = order
    return s, r
