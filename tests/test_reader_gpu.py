"""GPU: the extractive reader -- the span head alone against an exact reference (mmrag_span_select on integer-valued
data), its normalisers against float64, batch independence and repeatability, the whole forward
(mmrag_reader_forward) against transformers.BertForQuestionAnswering goldens (tests/golden/make_reader_golden.py),
and reader.DeviceReader / EmbeddingManager.read_answers end to end on a checkpoint written here.  Tolerances are
documented in DESIGN.md."""
import asyncio
import functools
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import reader_ref as Q

pytestmark = pytest.mark.gpu

# fp16 forward vs the float32 goldens: 2x the largest error measured over them (3.20e-3, minilm; the maximum over up
# to 2 x 503 logits of a sequence), rounded up to one significant digit; DESIGN.md section 3.2d
TOL_LOGITS = 7e-3
# lse vs float64: derived, not measured -- 513 float32 terms put a relative error of at most 513 * 2^-24 = 3.1e-5 on
# the sum, the same absolute error on its log, plus a few ulp of a result below 64
TOL_LSE = 1e-4


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


# (len, ctx_start, ctx_len) of the 37-sequence batch: the edge sequences first, then mixed lengths
def batch_layout():
    g = np.random.default_rng(37)
    rows = [(3, 2, 0), (4, 2, 1), (20, 5, 12), (512, 6, 505), (5, 2, 2), (512, 1, 511), (64, 10, 53), (65, 33, 31)]
    while len(rows) < 37:
        n = int(g.integers(6, 300))
        cs = int(g.integers(1, n - 2))
        rows.append((n, cs, int(g.integers(0, n - cs))))
    return rows


@functools.lru_cache(maxsize=None)
def exact_case(H):
    """integer-valued fp16 rows in -4..4, qa_w and qa_b in multiples of 1/8: every partial sum is exact in float32, so
    any summation order gives the float64 result"""
    g = np.random.default_rng(H)
    rows = batch_layout()
    T = sum(n for n, _, _ in rows)
    hidden = g.integers(-4, 5, (T, H)).astype(np.float16)
    w = (g.integers(-8, 9, (2, H)) / 8.0).astype(np.float32)
    b = (g.integers(-8, 9, 2) / 8.0).astype(np.float32)
    logits = Q.logits_f64(hidden, w, b)
    assert np.array_equal(logits, logits.astype(np.float32).astype(np.float64))
    cu = np.concatenate([[0], np.cumsum([n for n, _, _ in rows])]).astype(np.int32)
    return rows, hidden, w, b, logits.astype(np.float32), cu


@functools.lru_cache(maxsize=None)
def exact_ref(H, L):
    """the reference's 8 rounds of every sequence of exact_case(H) (fewer rounds are a prefix)"""
    rows, _, _, _, logits, cu = exact_case(H)
    return [Q.select_spans(logits[cu[b]: cu[b + 1], 0], logits[cu[b]: cu[b + 1], 1], cs, cl, L, 8)
            for b, (_, cs, cl) in enumerate(rows)]


def check_exact(got, logits, cu, rows, ref, n, which=None):
    span, score, null, lse, lg = (t.cpu().numpy() for t in got)
    which = range(len(rows)) if which is None else which
    assert span.shape == (len(which), n, 2) and score.shape == (len(which), n)
    at = 0
    for k, b in enumerate(which):
        want = logits[cu[b]: cu[b + 1]]
        assert np.array_equal(lg[at: at + len(want)].view(np.uint32), want.view(np.uint32)), b
        at += len(want)
        assert np.array_equal(span[k], ref[b][0][:n]), (b, rows[b], span[k], ref[b][0][:n])
        assert np.array_equal(score[k].view(np.uint32), ref[b][1][:n].view(np.uint32)), b
        assert null[k].view(np.uint32) == np.float32(want[0, 0] + want[0, 1]).view(np.uint32)
        lo = Q.lse_f64(want[:, 0], want[:, 1], rows[b][1], rows[b][2])
        assert abs(lse[k, 0] - lo[0]) <= max(TOL_LSE, 4 * np.spacing(np.float32(abs(lo[0]))))
        assert abs(lse[k, 1] - lo[1]) <= max(TOL_LSE, 4 * np.spacing(np.float32(abs(lo[1]))))


@pytest.mark.parametrize("H", [128, 384, 768, 1024])
def test_span_head_exact(N, H):
    rows, hidden, w, b, logits, cu = exact_case(H)
    d_h, d_w, d_b, d_cu = dev(hidden), dev(w), dev(b), dev(cu)
    d_cs, d_cl = dev(np.array([r[1] for r in rows], np.int32)), dev(np.array([r[2] for r in rows], np.int32))
    for L in (1, 30, 64):
        ref = exact_ref(H, L)
        for n in (1, 3, 8):
            got = N.span_select(d_h, d_w, d_b, d_cu, d_cs, d_cl, L, n, logits=True)
            check_exact(got, logits, cu, rows, ref, n)
    # ctx_len 0: nothing; ctx_len 1: one span; ctx_len 2: at most two real spans (one when the best covers both
    # tokens); the rest (-1, -1, -inf)
    span, score = (t.cpu().numpy() for t in N.span_select(d_h, d_w, d_b, d_cu, d_cs, d_cl, 64, 8)[:2])
    assert (span[0] == -1).all() and (score[0] == -np.inf).all()
    assert span[1, 0].tolist() == [2, 2] and (span[1, 1:] == -1).all() and (score[1, 1:] == -np.inf).all()
    assert (span[4, 0] >= 2).all() and (span[4, 2:] == -1).all() and (score[4, 2:] == -np.inf).all()
    assert np.array_equal(span[4], exact_ref(H, 64)[4][0])
    # B = 1: the 512-token sequence alone, a view into the same rows
    b1 = 3
    one = N.span_select(d_h[cu[b1]: cu[b1 + 1]], d_w, d_b, dev(np.array([0, 512], np.int32)), d_cs[b1: b1 + 1],
                        d_cl[b1: b1 + 1], 30, 8, logits=True)
    check_exact(one, logits, cu, rows, exact_ref(H, 30), 8, which=[b1])
    # out_logits is optional: the same spans without it
    a = N.span_select(d_h, d_w, d_b, d_cu, d_cs, d_cl, 30, 3, logits=True)
    c = N.span_select(d_h, d_w, d_b, d_cu, d_cs, d_cl, 30, 3)
    assert c[4] is None and all(torch.equal(x, y) for x, y in zip(a[:4], c[:4]))


def identity_case(ls, le, H=128):
    """hidden rows and a head for which the logits ARE (ls, le): small integers in columns 0 and 1"""
    hidden = np.zeros((len(ls), H), np.float16)
    hidden[:, 0], hidden[:, 1] = ls, le
    w = np.zeros((2, H), np.float32)
    w[0, 0] = w[1, 1] = 1.0
    return dev(hidden), dev(w), dev(np.zeros(2, np.float32))


def test_ties_go_to_the_lowest_start_then_end(N):
    g = np.random.default_rng(9)
    lens = [40, 300, 512]
    ls, le = g.integers(0, 2, sum(lens)).astype(np.float32), g.integers(0, 2, sum(lens)).astype(np.float32)
    h, w, b = identity_case(ls, le)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cs, cl = np.array([1, 7, 2], np.int32), np.array([38, 290, 509], np.int32)
    for L, n in ((5, 8), (64, 8), (1, 8)):
        span, score, _, _, lg = (t.cpu().numpy() for t in N.span_select(h, w, b, dev(cu), dev(cs), dev(cl), L, n, logits=True))
        assert np.array_equal(lg[:, 0], ls) and np.array_equal(lg[:, 1], le)
        for k in range(3):
            want = Q.select_spans(ls[cu[k]: cu[k + 1]], le[cu[k]: cu[k + 1]], int(cs[k]), int(cl[k]), L, n)
            assert np.array_equal(span[k], want[0]) and np.array_equal(score[k], want[1]), (L, k)
    # all logits equal: one token at a time from the left
    h, w, b = identity_case(np.zeros(12, np.float32), np.zeros(12, np.float32))
    span = N.span_select(h, w, b, dev(np.array([0, 12], np.int32)), dev(np.array([3], np.int32)),
                         dev(np.array([8], np.int32)), 4, 3)[0].cpu().numpy()
    assert span[0].tolist() == [[3, 3], [4, 4], [5, 5]]


def test_an_overlapping_runner_up_is_skipped(N):
    ls = np.array([0, 0, 0, 4, 0, -3, 1, 0, 0], np.float32)
    le = np.array([0, 0, 0, 0, 4, 3, 2, 0, 0], np.float32)
    h, w, b = identity_case(ls, le)
    span, score, null, lse, _ = N.span_select(h, w, b, dev(np.array([0, 9], np.int32)), dev(np.array([1], np.int32)),
                                              dev(np.array([7], np.int32)), 4, 3)
    # (3, 4) = 8 wins; (3, 5) = 7 is the best of the rest but shares tokens with it; (6, 6) = 3 is next
    assert span[0, :2].tolist() == [[3, 4], [6, 6]]
    assert score[0, :2].tolist() == [8.0, 3.0] and float(null[0]) == 0.0
    want = Q.select_spans(ls, le, 1, 7, 4, 3)
    assert np.array_equal(span[0].cpu().numpy(), want[0]) and np.array_equal(score[0].cpu().numpy(), want[1])
    assert np.array_equal(want[0], Q.select_spans_brute(ls, le, 1, 7, 4, 3)[0])


def test_sequences_outside_their_tables_read_nothing(N):
    g = np.random.default_rng(2)
    lens = [10, 10, 600, 10]
    hidden = g.integers(-4, 5, (sum(lens), 128)).astype(np.float16)
    w, b = (g.integers(-8, 9, (2, 128)) / 8.0).astype(np.float32), np.zeros(2, np.float32)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cs, cl = np.array([2, 5, 2, 0], np.int32), np.array([7, 6, 100, 3], np.int32)      # ok, past the end, > 512, no [CLS]
    span, score, null, lse, _ = (t.cpu().numpy() for t in N.span_select(dev(hidden), dev(w), dev(b), dev(cu), dev(cs),
                                                                        dev(cl), 30, 3, logits=True))
    assert (span[0, 0] >= 2).all() and np.isfinite(null[0]) and np.isfinite(lse[0]).all()
    for k in (1, 2, 3):
        assert (span[k] == -1).all() and (score[k] == -np.inf).all() and np.isnan(null[k]) and np.isnan(lse[k]).all()


@functools.lru_cache(maxsize=None)
def real_case(H=384):
    g = np.random.default_rng(H + 1)
    rows = batch_layout()
    T = sum(n for n, _, _ in rows)
    hidden = g.standard_normal((T, H)).astype(np.float16)
    w = (g.standard_normal((2, H)) / np.sqrt(H)).astype(np.float32)
    b = (g.standard_normal(2) * 0.1).astype(np.float32)
    cu = np.concatenate([[0], np.cumsum([n for n, _, _ in rows])]).astype(np.int32)
    return rows, hidden, w, b, cu


def test_normalisers_vs_float64(N):
    rows, hidden, w, b, cu = real_case()
    cs, cl = np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.int32)
    span, score, null, lse, lg = (t.cpu().numpy() for t in N.span_select(dev(hidden), dev(w), dev(b), dev(cu), dev(cs),
                                                                         dev(cl), 30, 3, logits=True))
    ref = Q.logits_f64(hidden, w, b)
    # a float32 dot of H terms plus the bias: at most (H + 2) * 2^-24 * sum |x_k w_k| away from the exact one
    bound = (hidden.shape[1] + 2) * 2.0 ** -24 * (np.abs(hidden.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
                                                  + np.abs(b))
    assert (np.abs(lg - ref) <= bound).all()
    worst = 0.0
    for k, (_, s, c) in enumerate(rows):
        a, e = Q.lse_f64(lg[cu[k]: cu[k + 1], 0], lg[cu[k]: cu[k + 1], 1], s, c)     # of the kernel's own logits
        worst = max(worst, abs(lse[k, 0] - a), abs(lse[k, 1] - e))
        assert abs(a) < 64 and abs(e) < 64
        want = Q.select_spans(lg[cu[k]: cu[k + 1], 0], lg[cu[k]: cu[k + 1], 1], s, c, 30, 3)
        assert np.array_equal(span[k], want[0]) and np.array_equal(score[k].view(np.uint32), want[1].view(np.uint32))
    print(f"\n[reader] max |lse - float64| = {worst:.3g}")
    assert worst <= TOL_LSE, worst


def test_batch_independence_and_repeatability(N):
    rows, hidden, w, b, cu = real_case()
    cs, cl = np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.int32)
    d_h, d_w, d_b = dev(hidden), dev(w), dev(b)
    args = (d_h, d_w, d_b, dev(cu), dev(cs), dev(cl), 30, 8)
    first, again = N.span_select(*args, logits=True), N.span_select(*args, logits=True)
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    for k in (0, 3, 5, 17, 36):
        lo, hi = int(cu[k]), int(cu[k + 1])
        one = N.span_select(d_h[lo:hi].contiguous(), d_w, d_b, dev(np.array([0, hi - lo], np.int32)),
                            dev(cs[k: k + 1]), dev(cl[k: k + 1]), 30, 8, logits=True)
        assert torch.equal(one[0][0], first[0][k]) and torch.equal(one[1][0], first[1][k]), k
        assert torch.equal(one[2][0], first[2][k]) and torch.equal(one[3][0], first[3][k]), k
        assert torch.equal(one[4], first[4][lo:hi]), k


# ---------------------------------------------------------------- the whole forward
def _reader(name):
    from multimodal_rag_amd.encoder import EncoderConfig
    from multimodal_rag_amd.reader import DeviceReader

    shape, w = Q.reader_weights(name)
    cfg = EncoderConfig(name, shape.n_layers, shape.hidden, shape.n_heads, shape.intermediate, shape.vocab,
                        shape.max_pos, shape.max_pos, "cls", shape.ln_eps)
    return DeviceReader(cfg, w, "cuda:0")


def _golden(name):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"reader_{name}.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def measured():
    out = {}
    yield out
    print("\n[reader] max |dlogit| vs transformers:", json.dumps(out))


@pytest.mark.parametrize("name", ["tiny", "minilm", "dh64"])
def test_forward_vs_golden(N, name, measured):
    enc = _reader(name)
    z = _golden(name)
    alone = z["group"] == 0
    assert int(z["lens"][alone].max()) <= 64                 # the folded-LayerNorm path
    worst = 0.0
    for pick in (alone, ~alone):
        ids, types, lens, cs, cl, ref = (z[k][pick] for k in ("ids", "type_ids", "lens", "ctx_start", "ctx_len", "logits"))
        span, score, null, lse, lg = (t.cpu().numpy() for t in enc.read_ids(ids, types, lens, cs, cl, 30, 8, logits=True))
        cu = np.concatenate([[0], np.cumsum(lens)])
        for k in range(len(lens)):
            mine = lg[cu[k]: cu[k + 1]]
            worst = max(worst, float(np.abs(mine - ref[k, : lens[k]]).max()))
            # the spans through the kernel's own logits: exact, near-ties included
            want = Q.select_spans(mine[:, 0], mine[:, 1], int(cs[k]), int(cl[k]), 30, 8)
            assert np.array_equal(span[k], want[0]) and np.array_equal(score[k].view(np.uint32), want[1].view(np.uint32))
            assert null[k].view(np.uint32) == np.float32(mine[0, 0] + mine[0, 1]).view(np.uint32)
            a, e = Q.lse_f64(mine[:, 0], mine[:, 1], int(cs[k]), int(cl[k]))
            assert abs(lse[k, 0] - a) <= TOL_LSE and abs(lse[k, 1] - e) <= TOL_LSE
        again = enc.read_ids(ids, types, lens, cs, cl, 30, 8, logits=True)
        assert torch.equal(again[0], torch.from_numpy(span).cuda()) and torch.equal(again[4], torch.from_numpy(lg).cuda())
    measured[name] = worst
    print(f"\n[reader] {name}: max |dlogit| = {worst:.3e}")
    assert worst <= TOL_LOGITS, worst


def test_type_ids_matter(N):
    """segment 1 embeddings are really read: zeroing the type ids changes the logits"""
    enc = _reader("tiny")
    z = _golden("tiny")
    args = (z["lens"], z["ctx_start"], z["ctx_len"], 30, 3)
    a = enc.read_ids(z["ids"], z["type_ids"], *args, logits=True)[4].cpu().numpy()
    b = enc.read_ids(z["ids"], np.zeros_like(z["type_ids"]), *args, logits=True)[4].cpu().numpy()
    assert np.abs(a - b).max() > 1e-3


def test_precision_fp32_is_refused(N):
    from multimodal_rag_amd.encoder import EncoderConfig
    from multimodal_rag_amd.reader import DeviceReader

    shape, w = Q.reader_weights("tiny")
    cfg = EncoderConfig("tiny", shape.n_layers, shape.hidden, shape.n_heads, shape.intermediate, shape.vocab,
                        shape.max_pos, shape.max_pos, "cls", shape.ln_eps)
    with pytest.raises(ValueError, match="fp16 is the only"):
        DeviceReader(cfg, w, "cuda:0", precision="fp32")
    r = DeviceReader.random_init(cfg, seed=3)
    out = r.read_ids([[101, 7, 102, 8, 9, 102]], [[0, 0, 0, 1, 1, 1]], None, [3], [2], 30, 3)
    assert out[0].shape == (1, 3, 2) and (out[0][0, 0] >= 3).all()


# ---------------------------------------------------------------- end to end
WORDS = ["the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "what", "is", "machine", "learning",
         "retrieval", "gpu", "kernel", "cat", "paris", "march", "2019", "capital"]


def _write_checkpoint(path, name, vocab):
    from safetensors.numpy import save_file

    shape, w = Q.reader_weights(name)
    sd = {(k if k.startswith("qa_outputs.") else "bert." + k): np.ascontiguousarray(v) for k, v in w.items()}
    save_file(sd, os.path.join(path, "model.safetensors"))
    cfg = {"architectures": ["BertForQuestionAnswering"], "model_type": "bert", "vocab_size": shape.vocab,
           "hidden_size": shape.hidden, "num_hidden_layers": shape.n_layers, "num_attention_heads": shape.n_heads,
           "intermediate_size": shape.intermediate, "max_position_embeddings": shape.max_pos,
           "layer_norm_eps": shape.ln_eps, "type_vocab_size": 2, "hidden_act": "gelu"}
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    with open(os.path.join(path, "vocab.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(vocab) + "\n")


def test_end_to_end_local_checkpoint_and_read_answers(N, tmp_path, monkeypatch):
    from multimodal_rag_amd import embedder as emb_mod
    from multimodal_rag_amd.embedder import EmbeddingManager
    from multimodal_rag_amd.reader import DeviceReader

    shape, _ = Q.reader_weights("tiny")
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", ".", ","] + WORDS
    vocab += [f"w{i}" for i in range(shape.vocab - len(vocab))]
    _write_checkpoint(str(tmp_path), "tiny", vocab)
    enc = DeviceReader.from_local_dir(str(tmp_path), "cuda:0")
    assert enc.max_length == shape.max_pos == 64
    g = np.random.default_rng(6)
    passages = [" ".join(g.choice(WORDS, int(n))) + "." for n in g.integers(1, 40, 6)] + [""]
    passages.append("  ".join(g.choice(WORDS, 150)))                  # does not fit: several windows
    q = "what is the capital"
    out, rows, (span, score, null, lse) = enc.read(q, passages, n_best=3, max_answer_tokens=10, doc_stride=16,
                                                   details=True)
    assert len(out) == len(passages) and sum(r["passage"] == len(passages) - 1 for r in rows) >= 3
    assert out == enc.read(q, passages, n_best=3, max_answer_tokens=10, doc_stride=16)
    # the spans of every row are the reference's on that row's logits
    got = enc.read_ids([r["ids"] for r in rows], [r["type_ids"] for r in rows], None, [r["ctx_start"] for r in rows],
                       [r["ctx_len"] for r in rows], 10, 3, logits=True)
    assert np.array_equal(got[0].cpu().numpy(), span)
    lg = got[4].cpu().numpy()
    cu = np.concatenate([[0], np.cumsum([len(r["ids"]) for r in rows])])
    probs = {}
    for k, r in enumerate(rows):
        mine = lg[cu[k]: cu[k + 1]]
        want = Q.select_spans(mine[:, 0], mine[:, 1], r["ctx_start"], r["ctx_len"], 10, 3)
        assert np.array_equal(span[k], want[0]) and np.array_equal(score[k], want[1])
        for (i, j), s in zip(span[k], score[k]):
            if i >= 0:
                p = min(1.0, math.exp(float(s) - float(lse[k, 0]) - float(lse[k, 1])))
                probs.setdefault((r["passage"], float(s)), []).append(p)
    for p, (text, found) in enumerate(zip(passages, out)):
        mine = [k for k, r in enumerate(rows) if r["passage"] == p]
        assert found["null_score"] == min(float(null[k]) for k in mine)
        assert len(found["spans"]) <= 3 and (found["spans"] or not text)
        for a, b in zip(found["spans"], found["spans"][1:]):
            assert a["score"] >= b["score"] and (a["end"] <= b["start"] or b["end"] <= a["start"])
        for s in found["spans"]:
            assert s["text"] == text[s["start"]: s["end"]] and s["text"]
            assert 0.0 < s["probability"] <= 1.0
            assert any(s["probability"] == pytest.approx(x, rel=1e-12) for x in probs[(p, s["score"])])

    monkeypatch.setattr(emb_mod.settings, "MMRAG_READER_DIR", str(tmp_path))
    monkeypatch.setattr(emb_mod.settings, "MMRAG_READER_MAX_ANSWER_TOKENS", 10)
    monkeypatch.setattr(emb_mod.settings, "MMRAG_READER_DOC_STRIDE", 16)
    monkeypatch.setattr(emb_mod.settings, "MMRAG_READER_NULL_THRESHOLD", -1e9)
    m = EmbeddingManager(engine=types.SimpleNamespace(device="cuda:0"))
    res = {"ids": [f"id{i}" for i in range(len(passages))], "distances": [0.1] * len(passages),
           "metadatas": [{} for _ in passages], "documents": [p or None for p in passages]}
    ans = asyncio.run(m.read_answers(q, res, n_answers=3))          # loads the reader from the directory
    assert isinstance(m._reader, DeviceReader)
    flat = sorted(((s["score"], p) for p, f in enumerate(out) for s in f["spans"]), key=lambda t: -t[0])
    assert ans["answers"][0]["score"] == flat[0][0] and ans["answers"][0]["hit"] == flat[0][1]
    for a in ans["answers"]:
        assert a["text"] == passages[a["hit"]][a["start"]: a["end"]]
    assert len({a["text"] for a in ans["answers"]}) == len(ans["answers"]) == 3
    assert ans["null_score"] == min(f["null_score"] for f in out)
    assert [[s["text"] for s in per] for per in ans["answer_spans"]] == [[s["text"] for s in f["spans"]] for f in out]
    assert ans["answerable"] is True                                 # best - null > -1e9
    monkeypatch.setattr(emb_mod.settings, "MMRAG_READER_NULL_THRESHOLD", 1e9)
    assert asyncio.run(m.read_answers(q, res))["answerable"] is False
    gap = ans["answers"][0]["score"] - ans["null_score"]
    assert asyncio.run(m.read_answers(q, res, null_threshold=gap - 1e-3))["answerable"] is True
    assert asyncio.run(m.read_answers(q, res, null_threshold=gap))["answerable"] is False
