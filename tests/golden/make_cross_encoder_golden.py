#!/usr/bin/env python3
"""Goldens of the cross-encoder (BUILD container only: needs `transformers` / `tokenizers`; the files written here
travel, the libraries need not exist on the GPU box).

    python tests/golden/make_cross_encoder_golden.py

1. tests/golden/cross_encoder_<shape>.npz: logits of `transformers.BertForSequenceClassification` (float32, eager)
   built from a local config with the weights of tests/cross_encoder_ref.py (layers: oracle make_bert_weights; type
   table, pooler, classifier: head_weights), over padded pair rows with attention masks.  Stored: ids, type_ids, lens,
   group (0: a pair of <= 64 tokens meant to be scored alone -- the folded-LayerNorm path; 1: the mixed batch), logits.
   No weights are stored.
2. tests/golden/cross_encoder_pairs.json: `BertTokenizerFast` pair encodings (truncation="longest_first", batch call
   as CrossEncoder.predict makes it) over the small vocabulary tests/golden/cross_encoder_vocab.txt.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import cross_encoder_ref as R  # noqa: E402

PAIRS = {
    "tiny": ([(20, 30)], [(3, 5), (10, 40), (25, 25), (1, 0), (0, 7)]),
    "minilm": ([(10, 40)], [(9, 120), (20, 230), (12, 300), (30, 470), (5, 60), (2, 1)]),
    "dh64": ([(8, 30)], [(16, 250), (10, 490), (7, 80), (40, 100)]),
}

VOCAB = (["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(".,?!'-") + [str(d) for d in range(10)]
         + [chr(c) for c in range(ord("a"), ord("z") + 1)] + ["##" + chr(c) for c in range(ord("a"), ord("z") + 1)]
         + ["the", "quick", "brown", "fox", "jump", "##ed", "##ing", "over", "lazy", "dog", "what", "is",
            "machine", "learn", "cafe", "naive", "re", "##rank", "query", "passage"]
         + list("中文日本語"))

TEXT_CASES = [
    # (a, b, max_length)
    ("what is machine learning?", "machine learning is the quick fox.", 32),          # fits
    ("what is it", "the quick brown fox jumped over the lazy dog " * 6, 24),           # shorter side fits
    ("the quick brown fox " * 5, "the lazy dog jumps over " * 5, 16),                  # both overflow
    ("the quick brown fox " * 5, "the lazy dog jumps over " * 5, 17),                  # odd budget
    ("a b c d e f g h", "h g f e d c b a", 11),                                        # equal lengths, odd budget
    ("a b c d e f g h", "h g f e d c b a", 12),                                        # equal lengths, even budget
    ("", "the quick brown fox", 16),                                                   # empty first
    ("what is it", "", 16),                                                            # empty second
    ("", "", 8),
    ("Café naïve RE-RANKING", "中文 日本語 text, with 'quotes'!", 20),               # accents, CJK, punctuation
    ("the quick brown fox jumps", "over the lazy dog again", 5),                       # budget 2: one token a side
    ("the quick brown fox jumps", "over the lazy dog again", 4),                       # budget 1
    ("the quick", "over the lazy dog again", 3),                                       # budget 0
    ("zzzz xylophone", "qqq", 10),
]


def hf_cls_model(shape, n_labels, w):
    from transformers import BertConfig, BertForSequenceClassification

    cfg = BertConfig(vocab_size=shape.vocab, hidden_size=shape.hidden, num_hidden_layers=shape.n_layers,
                     num_attention_heads=shape.n_heads, intermediate_size=shape.intermediate,
                     max_position_embeddings=shape.max_pos, hidden_act="gelu", layer_norm_eps=shape.ln_eps,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_labels=n_labels,
                     type_vocab_size=2)
    m = BertForSequenceClassification(cfg)
    sd = m.state_dict()
    for k, v in w.items():
        key = k if k.startswith("classifier.") else "bert." + k
        assert key in sd and tuple(sd[key].shape) == v.shape, key
        sd[key] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=False)
    return m.eval()


def logits_of(m, ids, types, lens):
    mask = (np.arange(ids.shape[1])[None, :] < lens[:, None]).astype(np.int64)
    with torch.no_grad():
        return m(input_ids=torch.from_numpy(ids.astype(np.int64)), token_type_ids=torch.from_numpy(types.astype(np.int64)),
                 attention_mask=torch.from_numpy(mask)).logits.numpy().astype(np.float32)


def one(name):
    shape, nl, w = R.cross_weights(name)
    single, mixed = PAIRS[name]
    m = hf_cls_model(shape, nl, w)
    ids, types, lens = R.pair_rows(shape, R.SHAPES[name][2] + 7, single + mixed)
    group = np.array([0] * len(single) + [1] * len(mixed), np.int32)
    logits = np.concatenate([logits_of(m, ids[:1], types[:1], lens[:1]), logits_of(m, ids[1:], types[1:], lens[1:])])
    np.savez_compressed(os.path.join(HERE, f"cross_encoder_{name}.npz"), ids=ids, type_ids=types, lens=lens, group=group,
                        logits=logits, n_labels=np.int32(nl))
    print(f"{name}: T = {lens.tolist()}, logits range [{logits.min():.3f}, {logits.max():.3f}]")


def pairs_golden():
    from transformers import BertTokenizerFast

    vocab_path = os.path.join(HERE, "cross_encoder_vocab.txt")
    with open(vocab_path, "w", encoding="utf-8") as f:
        f.write("\n".join(VOCAB) + "\n")
    tk = BertTokenizerFast(vocab_path, do_lower_case=True)
    cases = []
    for a, b, ml in TEXT_CASES:
        e = tk([a], [b], truncation="longest_first", max_length=ml)
        cases.append({"a": a, "b": b, "max_length": ml, "ids": e["input_ids"][0], "type_ids": e["token_type_ids"][0]})
    with open(os.path.join(HERE, "cross_encoder_pairs.json"), "w", encoding="utf-8") as f:
        json.dump({"cases": cases}, f, ensure_ascii=False, indent=1)
    print(f"pairs: {len(cases)} cases")


if __name__ == "__main__":
    pairs_golden()
    for n in PAIRS:
        one(n)
