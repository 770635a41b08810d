#!/usr/bin/env python3
"""Goldens of the extractive reader (BUILD container only: needs `transformers`; the files written here travel, the
library need not exist on the GPU box).

    python tests/golden/make_reader_golden.py

tests/golden/reader_<shape>.npz: start / end logits of `transformers.BertForQuestionAnswering` (float32, eager) built
from a local config with the weights of tests/reader_ref.py (body and type table: the cross-encoder goldens' of
tests/cross_encoder_ref.py; qa_outputs: reader_ref.qa_head), over padded pair rows with attention masks.  Stored: ids,
type_ids, lens, ctx_start, ctx_len, group (0: a pair of <= 64 tokens meant to be read alone -- the folded-LayerNorm
path; 1: the mixed batch), logits [B, S, 2] (start, end; zero past a row's length).  No weights are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import cross_encoder_ref as R  # noqa: E402
from tests import reader_ref as Q  # noqa: E402

# (question tokens, passage tokens) of the row read alone, and of the mixed batch
PAIRS = {
    "tiny": ([(20, 30)], [(3, 5), (10, 40), (25, 25), (1, 0), (4, 1), (0, 7)]),
    "minilm": ([(10, 40)], [(9, 120), (20, 230), (12, 300), (30, 470), (5, 60), (2, 1)]),
    "dh64": ([(8, 30)], [(16, 250), (10, 490), (7, 80), (40, 100)]),
}


def hf_qa_model(shape, w):
    from transformers import BertConfig, BertForQuestionAnswering

    cfg = BertConfig(vocab_size=shape.vocab, hidden_size=shape.hidden, num_hidden_layers=shape.n_layers,
                     num_attention_heads=shape.n_heads, intermediate_size=shape.intermediate,
                     max_position_embeddings=shape.max_pos, hidden_act="gelu", layer_norm_eps=shape.ln_eps,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, type_vocab_size=2)
    m = BertForQuestionAnswering(cfg)
    sd = m.state_dict()
    for k, v in w.items():
        key = k if k.startswith("qa_outputs.") else "bert." + k
        assert key in sd and tuple(sd[key].shape) == v.shape, key
        sd[key] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.eval()


def logits_of(m, ids, types, lens):
    mask = (np.arange(ids.shape[1])[None, :] < lens[:, None]).astype(np.int64)
    with torch.no_grad():
        o = m(input_ids=torch.from_numpy(ids.astype(np.int64)), token_type_ids=torch.from_numpy(types.astype(np.int64)),
              attention_mask=torch.from_numpy(mask))
    lg = torch.stack([o.start_logits, o.end_logits], -1).numpy().astype(np.float32)
    return lg * mask[:, :, None].astype(np.float32)


def one(name):
    shape, w = Q.reader_weights(name)
    single, mixed = PAIRS[name]
    m = hf_qa_model(shape, w)
    ids, types, lens = R.pair_rows(shape, R.SHAPES[name][2] + 11, single + mixed)
    group = np.array([0] * len(single) + [1] * len(mixed), np.int32)
    n1 = len(single)
    S1 = int(lens[:n1].max())
    logits = np.zeros(ids.shape + (2,), np.float32)
    logits[:n1, :S1] = logits_of(m, ids[:n1, :S1], types[:n1, :S1], lens[:n1])
    logits[n1:] = logits_of(m, ids[n1:], types[n1:], lens[n1:])
    np.savez_compressed(os.path.join(HERE, f"reader_{name}.npz"), ids=ids, type_ids=types, lens=lens, group=group,
                        ctx_start=np.array([a + 2 for a, _ in single + mixed], np.int32),
                        ctx_len=np.array([b for _, b in single + mixed], np.int32), logits=logits)
    print(f"{name}: T = {lens.tolist()}, logits range [{logits.min():.3f}, {logits.max():.3f}]")


if __name__ == "__main__":
    for n in PAIRS:
        one(n)
