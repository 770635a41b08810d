"""GPU: the cross-encoder (mmrag_cross_encoder_forward / _f32) -- its embedding kernel with segment ids, its float32
classification head, and the whole forward against transformers.BertForSequenceClassification goldens
(tests/golden/make_cross_encoder_golden.py).  Tolerances are documented in DESIGN.md."""
import asyncio
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import encoder_oracle as E
from tests import cross_encoder_ref as R

pytestmark = pytest.mark.gpu

# fp16: 2x the largest error measured over the goldens (1.46e-3, dh64), rounded up; DESIGN.md section 3.2c
TOL = {"fp32": 1e-4, "fp16": 3e-3}


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def r16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("H,T", [(128, 37), (384, 300), (768, 5)])
def test_embed_types_kernel(N, prec, H, T):
    g = np.random.default_rng(H + T)
    V, P = 500, 64
    tok, pos, typ = (g.standard_normal((n, H)).astype(np.float32) * 0.5 for n in (V, P, 2))
    gam = (1.0 + 0.1 * g.standard_normal(H)).astype(np.float32)
    bet = (0.1 * g.standard_normal(H)).astype(np.float32)
    ids = g.integers(-3, V + 3, T).astype(np.int32)          # out-of-range ids are clamped
    pids = g.integers(0, P + 2, T).astype(np.int32)
    tids = g.integers(-1, 3, T).astype(np.int32)               # type ids too
    if prec == "fp16":
        tok, pos, typ = r16(tok), r16(pos), r16(typ)
    dt = torch.float16 if prec == "fp16" else torch.float32
    d = lambda x, t=dt: torch.from_numpy(x).cuda().to(t)  # noqa: E731
    out = N.embed_types_ln(d(ids, torch.int32), d(tids, torch.int32), d(pids, torch.int32), d(tok), d(pos), d(typ),
                           d(gam, torch.float32), d(bet, torch.float32), 1e-12)
    torch.cuda.synchronize()
    x = (tok[np.clip(ids, 0, V - 1)].astype(np.float64) + pos[np.clip(pids, 0, P - 1)] + typ[np.clip(tids, 0, 1)])
    mu = x.mean(1, keepdims=True)
    ref = (x - mu) / np.sqrt(((x - mu) ** 2).mean(1, keepdims=True) + 1e-12) * gam + bet
    err = float(np.abs(out.float().cpu().numpy() - ref).max())
    assert err <= (4e-3 if prec == "fp16" else 1e-5), err


@pytest.mark.parametrize("B,H,NL", [(1, 128, 1), (20, 384, 1), (100, 384, 1), (37, 768, 3), (16, 1024, 16),
                                    (33, 256, 2)])
def test_head_kernel_vs_float64(N, B, H, NL):
    g = np.random.default_rng(B * H + NL)
    cls = g.standard_normal((B, H)).astype(np.float32)
    wp = (g.standard_normal((H, H)) / np.sqrt(H)).astype(np.float32)
    bp = (0.1 * g.standard_normal(H)).astype(np.float32)
    wc = (g.standard_normal((NL, H)) / np.sqrt(H)).astype(np.float32)
    bc = (0.1 * g.standard_normal(NL)).astype(np.float32)
    d = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    got = N.cls_head_f32(d(cls), d(wp), d(bp), d(wc), d(bc))
    again = N.cls_head_f32(d(cls), d(wp), d(bp), d(wc), d(bc))
    torch.cuda.synchronize()
    ref = R.head_f64(cls, wp, bp, wc, bc)
    rel = float(np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max())
    assert rel <= 1e-5, rel
    assert torch.equal(got, again)                                       # deterministic: no float atomics
    sub = N.cls_head_f32(d(cls[B // 2: B // 2 + 1]), d(wp), d(bp), d(wc), d(bc))
    assert torch.equal(sub[0], got[B // 2])                              # a sequence's logits ignore its batch


def _encoder(name, prec):
    from multimodal_rag_amd.encoder import EncoderConfig
    from multimodal_rag_amd.reranker import DeviceCrossEncoder

    shape, nl, w = R.cross_weights(name)
    cfg = EncoderConfig(name, shape.n_layers, shape.hidden, shape.n_heads, shape.intermediate, shape.vocab,
                        shape.max_pos, shape.max_pos, "cls", shape.ln_eps)
    return DeviceCrossEncoder(cfg, w, "cuda:0", prec), nl


def _golden(name):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"cross_encoder_{name}.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def measured():
    out = {}
    yield out
    print("\n[cross-encoder] max |dlogit| vs transformers:", json.dumps(out))


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["tiny", "minilm", "dh64"])
def test_forward_vs_golden(N, name, prec, measured):
    enc, nl = _encoder(name, prec)
    z = _golden(name)
    ids, types, lens, ref = z["ids"], z["type_ids"], z["lens"], z["logits"]
    alone = z["group"] == 0
    got = np.concatenate([enc.score_ids(ids[alone], types[alone], lens[alone]).cpu().numpy(),
                          enc.score_ids(ids[~alone], types[~alone], lens[~alone]).cpu().numpy()])
    ref = np.concatenate([ref[alone], ref[~alone]])
    assert got.shape == (len(lens), nl)
    err = float(np.abs(got - ref).max())
    measured[f"{name}/{prec}"] = err
    tol = TOL[prec]
    assert err <= tol, err
    # ordering: wherever the golden separates two pairs by more than 2 tol, so does the GPU
    for c in range(nl):
        o = np.argsort(-ref[:, c], kind="stable")
        for i, j in zip(o[:-1], o[1:]):
            if ref[i, c] - ref[j, c] > 2 * tol:
                assert got[i, c] > got[j, c]
    # the same pair inside the mixed batch and alone; identical calls give identical bits
    one = enc.score_ids(ids[~alone][:1], types[~alone][:1], lens[~alone][:1]).cpu().numpy()
    assert np.abs(one[0] - got[int(alone.sum())]).max() <= tol
    a = enc.score_ids(ids, types, lens)
    b = enc.score_ids(ids, types, lens)
    assert torch.equal(a, b)


def test_type_ids_matter(N):
    """segment 1 embeddings are really read: flipping the type ids changes the logits"""
    enc, _ = _encoder("tiny", "fp32")
    z = _golden("tiny")
    a = enc.score_ids(z["ids"], z["type_ids"], z["lens"]).cpu().numpy()
    b = enc.score_ids(z["ids"], np.zeros_like(z["type_ids"]), z["lens"]).cpu().numpy()
    assert np.abs(a - b).max() > 1e-3


def _write_checkpoint(path, name, vocab):
    from safetensors.numpy import save_file

    shape, nl, w = R.cross_weights(name)
    sd = {(k if k.startswith("classifier.") else "bert." + k): np.ascontiguousarray(v) for k, v in w.items()}
    save_file(sd, os.path.join(path, "model.safetensors"))
    cfg = {"architectures": ["BertForSequenceClassification"], "model_type": "bert", "vocab_size": shape.vocab,
           "hidden_size": shape.hidden, "num_hidden_layers": shape.n_layers, "num_attention_heads": shape.n_heads,
           "intermediate_size": shape.intermediate, "max_position_embeddings": shape.max_pos,
           "layer_norm_eps": shape.ln_eps, "type_vocab_size": 2, "hidden_act": "gelu",
           "id2label": {str(i): f"LABEL_{i}" for i in range(nl)}}
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    with open(os.path.join(path, "vocab.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(vocab) + "\n")


def test_end_to_end_local_checkpoint_and_rerank(N, tmp_path, monkeypatch):
    from multimodal_rag_amd import embedder as emb_mod
    from multimodal_rag_amd.embedder import EmbeddingManager
    from multimodal_rag_amd.reranker import DeviceCrossEncoder

    words = ["the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "what", "is", "machine", "learning",
             "retrieval", "gpu", "kernel", "cat"]
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words + [f"w{i}" for i in range(1000 - 5 - len(words))]
    _write_checkpoint(str(tmp_path), "tiny", vocab)
    enc = DeviceCrossEncoder.from_local_dir(str(tmp_path), "cuda:0", precision="fp32")
    assert enc.n_labels == 2 and enc.max_length == 64
    g = np.random.default_rng(5)
    docs = [" ".join(g.choice(words, int(n))) for n in g.integers(1, 30, 12)] + [None]
    q = "what is machine learning"
    s = enc.predict([(q, d or "") for d in docs], batch_size=5)
    assert s.shape == (13, 2)
    np.testing.assert_array_equal(s, enc.predict([(q, d or "") for d in docs], batch_size=13))

    monkeypatch.setattr(emb_mod.settings, "MMRAG_RERANKER_DIR", str(tmp_path))
    m = EmbeddingManager(engine=types.SimpleNamespace(device="cuda:0"))
    res = {"ids": [f"id{i}" for i in range(13)], "distances": [0.1 * i for i in range(13)],
           "metadatas": [{"i": i} for i in range(13)], "documents": docs}
    out = asyncio.run(m.rerank_results(q, res, top_k=5))        # loads the cross-encoder from the directory
    assert isinstance(m._reranker, DeviceCrossEncoder)
    s = m._reranker.predict([(q, d or "") for d in docs])
    want = np.argsort(-s[:, 0], kind="stable")[:5]
    assert out["ids"] == [f"id{i}" for i in want]
    np.testing.assert_allclose(out["rerank_scores"], s[want, 0], rtol=0, atol=0)

    # a single-label checkpoint: predict applies the sigmoid by default
    p1 = tmp_path / "one"
    p1.mkdir()
    _write_checkpoint(str(p1), "minilm", vocab[:1000] + [f"x{i}" for i in range(30522 - 1000)])
    one = DeviceCrossEncoder.from_local_dir(str(p1), "cuda:0", precision="fp16")
    raw = one.predict([(q, d or "") for d in docs[:4]], apply_sigmoid=False)
    sig = one.predict([(q, d or "") for d in docs[:4]])
    assert raw.shape == (4,) and np.allclose(sig, 1 / (1 + np.exp(-raw.astype(np.float64))), atol=1e-6)
