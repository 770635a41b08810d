"""Shared pieces of the cross-encoder tests: the golden shapes, the seeded weights the goldens were made with, packed
pair layouts and a float64 head.  numpy only (the GPU box regenerates the weights from here bit for bit)."""
import dataclasses
from typing import Dict, List, Tuple

import numpy as np

from oracle import encoder_oracle as E

# name -> (BertShape, n_labels, layer seed)
SHAPES = {
    "tiny": (E.TINY, 2, 21),
    "minilm": (dataclasses.replace(E.MINILM_L6, pool="cls"), 1, 22),      # cross-encoder/ms-marco-MiniLM-L-6-v2 shape
    "dh64": (E.BertShape(2, 256, 4, 512, vocab=2000, max_pos=512, pool="cls"), 3, 23),
}


def head_weights(shape: E.BertShape, n_labels: int, seed: int) -> Dict[str, np.ndarray]:
    """Token-type table, pooler and classifier: numpy PCG64 seeded with seed + 1000, drawn in this order:
    type [2, H] * 0.05, pooler W [H, H] / sqrt(H), pooler b [H] * 0.05, classifier W [n_labels, H] / sqrt(H),
    classifier b [n_labels] * 0.05 (all standard normal, float32)."""
    g = np.random.default_rng(seed + 1000)
    H = shape.hidden
    f = lambda shp, s: (g.standard_normal(shp) * s).astype(np.float32)  # noqa: E731
    return {"embeddings.token_type_embeddings.weight": f((2, H), 0.05),
            "pooler.dense.weight": f((H, H), 1.0 / np.sqrt(H)), "pooler.dense.bias": f((H,), 0.05),
            "classifier.weight": f((n_labels, H), 1.0 / np.sqrt(H)), "classifier.bias": f((n_labels,), 0.05)}


def cross_weights(name: str):
    """(shape, n_labels, weights with BertModel names + pooler / classifier) of a golden shape"""
    shape, nl, seed = SHAPES[name]
    w = E.make_bert_weights(shape, seed)
    w.update(head_weights(shape, nl, seed))
    return shape, nl, w


def pair_rows(shape: E.BertShape, seed: int, pair_lens: List[Tuple[int, int]]):
    """padded (ids, type_ids) [B, S] int32 and lens [B] of random pairs [CLS] a [SEP] b [SEP] with |a|, |b| given"""
    g = np.random.default_rng(seed)
    lens = np.array([a + b + 3 for a, b in pair_lens], np.int32)
    S = int(lens.max())
    ids = np.zeros((len(pair_lens), S), np.int32)
    types = np.zeros_like(ids)
    lo = min(1000, shape.vocab // 2)
    for i, (a, b) in enumerate(pair_lens):
        row = [101] + g.integers(lo, shape.vocab, a).tolist() + [102] + g.integers(lo, shape.vocab, b).tolist() + [102]
        ids[i, : len(row)] = row
        types[i, a + 2: len(row)] = 1
    return ids, types, lens


def head_f64(cls: np.ndarray, wp, bp, wc, bc) -> np.ndarray:
    c = np.asarray(cls, np.float64)
    pooled = np.tanh(c @ np.asarray(wp, np.float64).T + np.asarray(bp, np.float64))
    return pooled @ np.asarray(wc, np.float64).T + np.asarray(bc, np.float64)
