"""Float64 references for the CLIP towers and their kernels.  TEST INFRASTRUCTURE ONLY.

The architecture is the one oracle/clip_oracle.py restates (and pins against transformers.CLIPModel); this module widens
it to float64, batches it (sequences of one length run as one batched matmul, so an ingest-sized batch costs seconds),
and can emulate the device's fp16 STORAGE: with `store=True` every tensor the HIP forward writes to memory as fp16 is
rounded to fp16 at that point, and nothing else changes (all arithmetic stays float64):

    embedding output | LayerNorm outputs | QKV | attention P (before P.V) and attention output |
    each GEMM output before the residual add, and the sum after it (csrc/encoder.hip, linear_kernel: "the activated
    value is rounded to fp16 before the residual add") | FFN hidden | pooled row | projected row

`e_store` = |forward(store=False) - forward(store=True)| is then the error that fp16 storage alone causes on a given
input; the GPU tests bound the device's error by a small multiple of it (tests/test_clip_gpu.py).

The host-side rules of DeviceClip.encode_text_ids are restated here too: a sequence is cut to t_max_pos tokens, and the
pooled token is the first EOS, or arg-max of the ids where the (cut) sequence holds none.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

from oracle import clip_oracle as C

# a ViT-B/16-like shape (197 tokens per image, 12 heads of 64, G = 14) with two layers and a tiny text tower
VITB16_2L = C.ClipShape(2, 128, 4, 256, 1000, 32, 999, 2, 768, 12, 3072, 224, 16, 512)

MEAN64 = C.CLIP_MEAN.astype(np.float64)
STD64 = C.CLIP_STD.astype(np.float64)


def r16(x) -> np.ndarray:
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _keep(x):
    return x


# ---- single kernels ---------------------------------------------------------------------------------------------------
def patchify(pixels_chw: np.ndarray, patch: int) -> np.ndarray:
    """[B, 3, I, I] -> [B, (I/P)^2, 3 P P]: patch index = grid row * G + grid column, vector order (c, ph, pw)"""
    B, _, I, _ = pixels_chw.shape
    G = I // patch
    x = pixels_chw.reshape(B, 3, G, patch, G, patch).transpose(0, 2, 4, 1, 3, 5)
    return np.ascontiguousarray(x.reshape(B, G * G, 3 * patch * patch))


def normalize_u8(tiles_hwc: np.ndarray) -> np.ndarray:
    """uint8 [B, I, I, 3] -> float64 [B, 3, I, I]: (v / 255 - mean_c) / std_c with clip_oracle's float32 constants widened"""
    x = (tiles_hwc.astype(np.float64) / 255.0 - MEAN64) / STD64
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def layer_norm(x: np.ndarray, g, b, eps: float) -> np.ndarray:
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def vit_assemble(emb: np.ndarray, cls: np.ndarray, pos: np.ndarray) -> np.ndarray:
    """emb [B, S-1, H], cls [H], pos [S, H] -> concat(cls, emb[b]) + pos, [B * S, H] (before the LayerNorm)"""
    B, _, H = emb.shape
    x = np.concatenate([np.broadcast_to(cls, (B, 1, H)), emb], axis=1) + pos
    return x.reshape(-1, H)


def clamp_index(i: np.ndarray, n: int) -> np.ndarray:
    """embed_ln_kernel's documented handling of ids / positions outside their table"""
    return np.clip(i, 0, n - 1)


def normalize_rows(x: np.ndarray) -> np.ndarray:
    return x / np.maximum(np.sqrt((x * x).sum(axis=-1, keepdims=True)), 1e-12)


def quick_gelu(x: np.ndarray) -> np.ndarray:
    return x / (1.0 + np.exp(-1.702 * x))


# ---- towers -----------------------------------------------------------------------------------------------------------
def eos_index(ids: Sequence[int], eos_id: int) -> int:
    ids = np.asarray(ids)
    hit = np.nonzero(ids == eos_id)[0]
    return int(hit[0]) if hit.size else int(np.argmax(ids))


def cut_sequences(s: C.ClipShape, sequences) -> List[np.ndarray]:
    return [np.asarray(q[:s.t_max_pos], np.int64) for q in sequences]


def _attention(q, k, v, lens, heads, causal, st):
    """packed [T, H] rows; sequences of equal length run as one batch.  P is stored (st) before P.V, as the kernel
    does with its un-normalised exp(s - max)"""
    T, H = q.shape
    dh = H // heads
    out = np.empty_like(q)
    lens = np.asarray(lens)
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    for S in np.unique(lens):
        rows = (starts[lens == S][:, None] + np.arange(S)[None, :]).reshape(-1)
        n = rows.size // S
        qq, kk, vv = (a[rows].reshape(n, S, heads, dh).transpose(0, 2, 1, 3) for a in (q, k, v))
        sc = qq @ kk.transpose(0, 1, 3, 2) / np.sqrt(dh)
        if causal:
            sc = np.where(np.tril(np.ones((S, S), bool)), sc, -np.inf)
        p = np.exp(sc - sc.max(axis=-1, keepdims=True))
        o = (st(p) @ vv) / p.sum(axis=-1, keepdims=True)
        out[rows] = o.transpose(0, 2, 1, 3).reshape(n * S, H)
    return out


def _blocks(x, w, tower, n_layers, heads, eps, causal, lens, st):
    for l in range(n_layers):
        p = f"{tower}.encoder.layers.{l}."
        a = st(layer_norm(x, w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], eps))
        q, k, v = (st(a @ w[p + f"self_attn.{n}.weight"].T + w[p + f"self_attn.{n}.bias"]) for n in ("q_proj", "k_proj", "v_proj"))
        o = st(_attention(q, k, v, lens, heads, causal, st))
        x = st(st(o @ w[p + "self_attn.out_proj.weight"].T + w[p + "self_attn.out_proj.bias"]) + x)
        b = st(layer_norm(x, w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], eps))
        hm = st(quick_gelu(b @ w[p + "mlp.fc1.weight"].T + w[p + "mlp.fc1.bias"]))
        x = st(st(hm @ w[p + "mlp.fc2.weight"].T + w[p + "mlp.fc2.bias"]) + x)
    return x


def widen(w: Dict[str, np.ndarray], tower: str) -> Dict[str, np.ndarray]:
    """the "text" or "vision" tower's weights (and its projection) as float64"""
    pre = {"text": "text_", "vision": "vis"}[tower]
    return {k: np.asarray(v, np.float64) for k, v in w.items() if k.startswith(pre)}


def text_embed(s: C.ClipShape, w: Dict[str, np.ndarray], sequences, store: bool = False) -> np.ndarray:
    """token-id sequences -> [B, proj] float64, L2-normalised; `w` as float64 (widen)"""
    st = r16 if store else _keep
    seqs = cut_sequences(s, sequences)
    lens = [len(q) for q in seqs]
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    ids = np.concatenate(seqs)
    pos = np.concatenate([np.arange(n) for n in lens])
    x = st(w["text_model.embeddings.token_embedding.weight"][ids] + w["text_model.embeddings.position_embedding.weight"][pos])
    x = _blocks(x, w, "text_model", s.t_layers, s.t_heads, s.ln_eps, True, lens, st)
    x = st(layer_norm(x, w["text_model.final_layer_norm.weight"], w["text_model.final_layer_norm.bias"], s.ln_eps))
    pooled = x[starts + np.array([eos_index(q, s.eos_id) for q in seqs])]
    return normalize_rows(st(pooled @ w["text_projection.weight"].T))


def image_embed(s: C.ClipShape, w: Dict[str, np.ndarray], pixels_chw: np.ndarray, store: bool = False) -> np.ndarray:
    """[B, 3, image, image] normalised pixels (float64) -> [B, proj] float64, L2-normalised; `w` as float64 (widen)"""
    st = r16 if store else _keep
    B = pixels_chw.shape[0]
    S = s.n_patches + 1
    wp = w["vision_model.embeddings.patch_embedding.weight"].reshape(s.v_hidden, -1)
    emb = st(patchify(np.asarray(pixels_chw, np.float64), s.patch) @ wp.T)
    x = vit_assemble(emb, w["vision_model.embeddings.class_embedding"], w["vision_model.embeddings.position_embedding.weight"])
    x = st(layer_norm(x, w["vision_model.pre_layrnorm.weight"], w["vision_model.pre_layrnorm.bias"], s.ln_eps))
    x = _blocks(x, w, "vision_model", s.v_layers, s.v_heads, s.ln_eps, False, [S] * B, st)
    x = st(layer_norm(x, w["vision_model.post_layernorm.weight"], w["vision_model.post_layernorm.bias"], s.ln_eps))
    return normalize_rows(st(x[::S] @ w["visual_projection.weight"].T))


def store_error(plain: np.ndarray, stored: np.ndarray):
    """(e_store, 1 - cos_store): the largest elementwise distance and the largest cosine distance over the batch that
    fp16 storage alone causes"""
    return float(np.abs(plain - stored).max()), float(one_minus_cos(plain, stored).max())


def one_minus_cos(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """per row, float64, without cancellation: 1 - cos = |a/|a| - b/|b||^2 / 2"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    d = a / np.linalg.norm(a, axis=1, keepdims=True) - b / np.linalg.norm(b, axis=1, keepdims=True)
    return 0.5 * (d * d).sum(axis=1)
