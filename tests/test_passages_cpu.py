"""CPU: answer passages -- the two formulations of tests/passage_ref.py against each other, the C-ABI surface and its
argument checks (nothing is launched), the tokenizers' character spans, the MMRAG_PASSAGE_TOKENS setting, and the host
layers above the kernel (EmbeddingManager.extract_passages, late_rerank(passages=...), POST /query "passages") over a
fake scorer."""
import asyncio
import ctypes
import os
import random
import re
import types
import unicodedata

import numpy as np
import pytest
import torch
from starlette.testclient import TestClient

from multimodal_rag_amd import _native
from multimodal_rag_amd import embedder as emb_mod
from multimodal_rag_amd.embedder import RESULT_KEYS, EmbeddingManager
from multimodal_rag_amd.late import LateInteractionScorer
from multimodal_rag_amd.tokenizer import (HashTokenizer, NativeWordPieceTokenizer, WordPieceTokenizer, basic_tokenize,
                                          basic_tokenize_spans)
from tests import passage_ref
from tests.fakes import FakeEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
D_LENS = (1, 15, 16, 17, 128, 129, 300, 512)
Q_LENS = (1, 5, 128)
WIDTHS = (1, 2, 4, 32)


# ---------------------------------------------------------------- the reference, twice
def test_the_two_reference_formulations_agree():
    g = np.random.default_rng(0)
    q_seqs = {n: g.integers(-2, 3, (n, 64)).astype(np.float32) for n in Q_LENS}
    d_seqs = {n: g.integers(-2, 3, (n, 64)).astype(np.float32) for n in D_LENS}
    cases = ties = 0
    for d_len in D_LENS:
        for q_len in Q_LENS:
            S = passage_ref.sims(q_seqs[q_len], d_seqs[d_len])
            for w in WIDTHS:
                a_sum, a_win, a_best = passage_ref.windows(S, w)
                b_sum, b_win, b_best = passage_ref.windows_by_tokens(S, w)
                assert a_sum.dtype == np.float32 and a_win.dtype == np.float32 and a_win.shape == (32,)
                assert a_sum.tobytes() == b_sum.tobytes() and a_win.tobytes() == b_win.tobytes(), (d_len, q_len, w)
                assert a_best == b_best, (d_len, q_len, w, a_best, b_best)
                nb = -(-d_len // 16)
                n_win = max(nb - w, 0) + 1
                assert np.isfinite(a_win[:n_win]).all() and np.isneginf(a_win[n_win:]).all()
                if w >= nb:
                    assert a_win[0].tobytes() == a_sum.tobytes() and a_best[0] == 0
                start, first, last = a_best
                assert 0 <= start < n_win and start <= first <= last < min(start + w, nb)
                assert a_win[start] == a_win[:n_win].max() and (a_win[:start] < a_win[start]).all()
                cases += 1
                ties += int((a_win[:n_win] == a_win[start]).sum() > 1)
    assert cases == 96 and ties >= 1, (cases, ties)      # the lowest-start rule is exercised by the data as it is
    print(f"{ties} of {cases} cases have tied best windows")


def test_reference_tie_and_span_rules_by_hand():
    # two query tokens, 48 passage tokens (3 blocks): token 0 matches block 2 best, token 1 matches blocks 0 and 2 alike
    S = np.zeros((2, 48))
    S[0, 40], S[0, 3] = 5.0, 4.0
    S[1, 2], S[1, 33] = 3.0, 3.0
    out_sum, win, best = passage_ref.windows(S, 1)
    assert out_sum == 8.0 and win[:3].tolist() == [7.0, 0.0, 8.0] and best == (2, 2, 2)
    _, win, best = passage_ref.windows(S, 2)
    assert win[:2].tolist() == [7.0, 8.0] and np.isneginf(win[2:]).all() and best == (1, 2, 2)
    _, win, best = passage_ref.windows(S, 3)          # one window; token 1's LOWEST best block is 0
    assert win[0] == 8.0 and best == (0, 0, 2)
    S[0, 40] = 4.0                                      # windows 0 and 2 of width 1 tie at 7: the lowest start
    assert passage_ref.windows(S, 1)[2] == (0, 0, 0) and passage_ref.windows_by_tokens(S, 1)[2] == (0, 0, 0)


# ---------------------------------------------------------------- the C ABI
WINDOWS_ARGS = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def test_header_constants_and_symbols():
    with open(os.path.join(ROOT, "include", "mmrag.h")) as f:
        header = f.read()
    assert re.search(r"#define MMRAG_LATE_WINDOW_TOKENS 16\b", header)
    assert re.search(r"#define MMRAG_MAX_LATE_WINDOWS 32\b", header)
    assert "int mmrag_maxsim_windows(" in header and "int mmrag_maxsim_windows_f8(" in header
    assert (_native.LATE_WINDOW_TOKENS, _native.MAX_LATE_WINDOWS) == (16, 32)
    assert _native.LATE_WINDOW_TOKENS * _native.MAX_LATE_WINDOWS == _native.MAX_LATE_DOC_TOKENS
    lib = _native.lib()
    for name in ("mmrag_maxsim_windows", "mmrag_maxsim_windows_f8"):
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == WINDOWS_ARGS
    assert lib.mmrag_abi_version() == 1


@pytest.mark.parametrize("name", ["mmrag_maxsim_windows", "mmrag_maxsim_windows_f8"])
def test_bad_arguments_need_no_gpu(name):
    lib = _native.lib()
    fn = getattr(lib, name)
    p = ctypes.c_void_p(256)   # never dereferenced: the arguments are refused first
    ld = 128 if name.endswith("_f8") else 64

    def call(w=2, dim=64, P=1, out_sum=p, out_win=p, out_best=p, ld=ld, q_tok=p):
        return fn(q_tok, 10, ld, p, 10, ld, dim, p, p, 1, p, p, 1, p, p, P, w, out_sum, out_win, out_best, None)

    for w in (0, 33, -1):
        assert call(w=w) == EINVAL
        assert "window_blocks" in lib.mmrag_last_error().decode()
    for which in ("out_sum", "out_win", "out_best", "q_tok"):
        assert call(**{which: None}) == EINVAL
        assert "null pointer" in lib.mmrag_last_error().decode()
    assert call(dim=96) == EINVAL and "multiple of 64" in lib.mmrag_last_error().decode()
    assert call(dim=0) == EINVAL and call(dim=1088) == EINVAL
    assert call(P=0) == EINVAL and call(P=65536) == EINVAL
    assert call(ld=32) == EINVAL        # narrower than dim
    assert name[len("mmrag_"):] + ":" in lib.mmrag_last_error().decode()      # reported under its own name


def test_wrapper_refuses_before_the_device():
    rows = torch.zeros((8, 64), dtype=torch.float16)
    with pytest.raises(_native.MMRagNativeError, match="device"):       # no CPU path
        _native.maxsim_windows(rows, rows, 64, [0], [4], [4], [4], [0], [0], 2)
    with pytest.raises(_native.MMRagNativeError, match="device"):
        _native.maxsim_windows_f8(rows.view(torch.uint8), rows.view(torch.uint8), 64, [0], [4], [4], [4], [0], [0], 2)


# ---------------------------------------------------------------- character spans of tokens
from tests.test_tokenizer import VOCAB as BASE_VOCAB  # noqa: E402

EXTRA = ["σ", "ς", "##σ", "ας", "e", "##e", "a", "##a", "b", "##b", "c", "##c", "d", "##d", "ß", "ss", "i", "##i",
         "viet", "##nam", "tieng", "##1", "1", "x", "##x", "中", "文", "(", ")", "'", "\"", "…", "—", "istanbul", "##stanbul"]
SPAN_VOCAB = {w: i for i, w in enumerate(BASE_VOCAB + [e for e in EXTRA if e not in BASE_VOCAB])}


def span_cases():
    with open(os.path.join(ROOT, "tests", "golden", "sample_document.txt"), encoding="utf-8") as f:
        sample = f.read()
    cases = [sample, sample[:400], "", "   ", "Machine learning là gì?", "unaffable running, naïve café!",
             "state-of-the-art embeddingly 你好", "Tiếng Việt Nam", "Tiếng Việt", "İstanbul İİ aİb",
             "ΑΣ ΑΣΑ Σ ΑΣ. ΑΣ'Α", "ab\x00cd\x07e �f", "a" * 101 + " abc " + "b" * 100, "x" * 250,
             "!!!...???,,, --- (a)(b)", "中文abc中d文", "가나다 한글 ab", "ﬁ ǅ ẞ ß", "a b c d　e"]
    alphabet = list("abcdeABCDE xX.,!?-'\"()1 \t\n") + ["Σ", "σ", "İ", "I", "é", "É", "ü", "Å", "ß", "你", "好", "中", "文",
                                                      "́", "̣", "̀", "­", "​", " ",
                                                      "　", "\x00", "�", "\x1c", "\x85", "—", "…", "ế", "ệ"]
    rng = random.Random(7)
    cases += ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 80))) for _ in range(400)]
    return cases


def normalised(s, lower=True):
    """what the tokenizer makes of a stretch of text that holds one token or a part of one, character by character:
    cleaned, lower-cased, decomposed, marks dropped (no rule that looks at a character's neighbours, such as the
    word-final sigma's: the words where that matters are the fallback's)"""
    out = []
    for ch in s:
        if ord(ch) in (0, 0xFFFD) or (unicodedata.category(ch) in ("Cc", "Cf") and ch not in "\t\n\r"):
            continue
        ch = unicodedata.normalize("NFD", ch.lower()) if lower else ch
        out.append("".join(c for c in ch if not lower or unicodedata.category(c) != "Mn"))
    return "".join(out)


def whole_word(s, lower=True):
    """the tokenizer's own normalisation of a whole whitespace-delimited word, its tokens joined"""
    return "".join(basic_tokenize(s, lower))


@pytest.mark.parametrize("lower", [True, False])
def test_basic_tokenize_spans(lower):
    fallbacks = 0
    for text in span_cases():
        got = basic_tokenize_spans(text, lower)
        assert [w for w, _ in got] == basic_tokenize(text, lower), repr(text)
        starts = [a for _, (a, _) in got]
        assert starts == sorted(starts) and all(0 <= a < b <= len(text) for _, (a, b) in got), repr(text)
        for word, (a, b) in got:
            if normalised(text[a:b], lower) != word:        # the whole-word fallback: the word holds the token
                fallbacks += 1
                assert word in whole_word(text[a:b], lower), (repr(text), word, a, b)
    assert fallbacks > 0 or not lower       # a word-final sigma is in the cases


@pytest.mark.parametrize("max_length", [512, 16, 3, 2])
def test_wordpiece_encode_with_spans(max_length):
    tk = WordPieceTokenizer(SPAN_VOCAB)
    id2tok = {i: t for t, i in SPAN_VOCAB.items()}
    exact = 0
    for text in span_cases():
        ids, spans = tk.encode_with_spans(text, max_length)
        assert ids == tk.encode(text, max_length), repr(text)
        assert len(spans) == len(ids) and spans[0] == (0, 0) and spans[-1] == (0, 0)
        inner = spans[1:-1]
        assert [a for a, _ in inner] == sorted(a for a, _ in inner), repr(text)
        assert all(0 <= a < b <= len(text) for a, b in inner), repr(text)
        words = {(a, b) for _, (a, b) in basic_tokenize_spans(text)}
        for pid, (a, b) in zip(ids[1:-1], inner):
            piece = id2tok[pid]
            if piece == "[UNK]":
                assert (a, b) in words, (repr(text), a, b)      # the whole word's span
            elif normalised(text[a:b]) == piece[2:] if piece.startswith("##") else normalised(text[a:b]) == piece:
                exact += 1
            else:       # the fallback: every piece of such a word carries the whole word's span
                assert (a, b) in words and piece.lstrip("#") in whole_word(text[a:b]), (repr(text), piece, a, b)
    assert exact > 0 or max_length <= 2


def test_fallback_words_and_the_other_tokenizers():
    tk = WordPieceTokenizer(SPAN_VOCAB)
    # "ας": the final sigma lower-cases by its place in the WORD, so the word's characters cannot be told apart
    ids, spans = tk.encode_with_spans("ab ΑΣ ab", 32)
    assert ids[1:-1] == [SPAN_VOCAB["a"], SPAN_VOCAB["##b"], SPAN_VOCAB["ας"], SPAN_VOCAB["a"], SPAN_VOCAB["##b"]]
    assert spans[1:-1] == [(0, 1), (1, 2), (3, 5), (6, 7), (7, 8)]
    # combining marks are dropped: the span of a piece ends at its last kept character; CJK characters stand alone
    text = "Việtnam中文"
    ids, spans = tk.encode_with_spans(text, 32)
    assert ids[1:-1] == [SPAN_VOCAB["viet"], SPAN_VOCAB["##nam"], SPAN_VOCAB["中"], SPAN_VOCAB["文"]]
    assert spans[1:-1] == [(0, 6), (6, 9), (9, 10), (10, 11)]
    # an [UNK] word: one id over the whole word
    ids, spans = tk.encode_with_spans("the zzz fox", 32)
    assert ids[2] == SPAN_VOCAB["[UNK]"] and spans[2] == (4, 7)
    # the hash tokenizer: one id per word
    ht = HashTokenizer(3000)
    for text in span_cases()[:60]:
        for ml in (512, 5):
            ids, spans = ht.encode_with_spans(text, ml)
            assert ids == ht.encode(text, ml) and len(spans) == len(ids)
            assert spans[1:-1] == [s for _, s in basic_tokenize_spans(text)][: ml - 2]
    # the native tokenizer answers through the Python one over the same vocabulary
    nat = NativeWordPieceTokenizer(SPAN_VOCAB, n_threads=2)
    for text in span_cases()[:80]:
        ids, spans = nat.encode_with_spans(text, 24)
        assert ids == nat.encode(text, 24) and (ids, spans) == tk.encode_with_spans(text, 24), repr(text)


# ---------------------------------------------------------------- the setting
def test_passage_tokens_setting(monkeypatch):
    from multimodal_rag_amd.config import Settings

    monkeypatch.delenv("MMRAG_PASSAGE_TOKENS", raising=False)
    assert Settings().MMRAG_PASSAGE_TOKENS == 64 and Settings().passage_tokens() == 64
    for good in (16, 64, 512):
        monkeypatch.setenv("MMRAG_PASSAGE_TOKENS", str(good))
        assert Settings().passage_tokens() == good
    for bad in (0, 8, 24, 100, 528, -16):
        monkeypatch.setenv("MMRAG_PASSAGE_TOKENS", str(bad))
        with pytest.raises(ValueError, match="MMRAG_PASSAGE_TOKENS must be a multiple of 16 in 16..512"):
            Settings()
    monkeypatch.delenv("MMRAG_PASSAGE_TOKENS")
    s = Settings()
    s.MMRAG_PASSAGE_TOKENS = 40         # changed after start-up: the accessor checks again
    with pytest.raises(ValueError, match="MMRAG_PASSAGE_TOKENS"):
        s.passage_tokens()


def test_scorer_rounds_the_window_to_blocks():
    wb = LateInteractionScorer.window_blocks
    assert [wb(n) for n in (-5, 0, 1, 16, 17, 64, 100, 512, 513, 10000)] == [1, 1, 1, 1, 2, 4, 7, 32, 32, 32]


# ---------------------------------------------------------------- EmbeddingManager and POST /query over a fake scorer
class FakeTokenEncoder:
    """stands where DeviceEncoder stands: the limits the scorer reads, no device"""

    def __init__(self, max_seq_length=256, max_pos=512, hidden=64):
        self.cfg = types.SimpleNamespace(max_seq_length=max_seq_length, max_pos=max_pos, hidden=hidden)


class FakePassages(LateInteractionScorer):
    """stands where LateInteractionScorer stands, with its tokenizer and trimming: a pair's score is the number of the
    query's words the passage contains, and its best window is the 16-token block of the first such word"""

    def __init__(self):
        super().__init__(FakeTokenEncoder(), HashTokenizer(3000))
        self.calls = []
        self.other_ids = set()       # documents reported with other token ids than their text gives

    def _words(self, text):
        return basic_tokenize(text)[: self.max_doc_tokens]

    def score_pairs(self, queries, docs, pairs, explain=False, **stored):
        self.calls.append(("score", list(queries), list(docs), list(pairs)))
        return np.array([float(sum(1 for t in set(queries[a].split()) if t in self._words(docs[b])))
                         for a, b in pairs], np.float32)

    def explain_pairs(self, queries, docs, pairs, **stored):
        self.calls.append(("explain", list(queries), list(docs), list(pairs)))
        recs = [[{"query_token": t, "doc_token": t, "doc_index": 0, "similarity": 1.0} for t in queries[a].split()]
                for a, b in pairs]
        scores = self.score_pairs(queries, docs, pairs)
        self.calls.pop()
        return scores, recs

    def best_passages(self, queries, docs, pairs, window_tokens, **stored):
        self.calls.append(("passages", list(queries), list(docs), list(pairs), int(window_tokens)))
        out = []
        for a, b in pairs:
            wanted, words = set(queries[a].split()), self._words(docs[b])
            ids = self.tokenizer.encode(docs[b], self.max_doc_tokens + 2)
            ids = ids[1:-1] if len(ids) > 2 else ids[:1]
            at = [k for k, w in enumerate(words) if w in wanted]
            start = 16 * (at[0] // 16) if at else 0
            end = min(start + 16, len(ids))
            whole = float(len({words[k] for k in at}))
            inside = float(len({words[k] for k in at if start <= k < end}))
            out.append({"score": whole, "window_score": inside, "sum": whole, "window_sum": inside,
                        "window_start": start, "window_end": end, "token_start": start, "token_end": end,
                        "window_scores": [inside], "doc_ids": ids[::-1] if docs[b] in self.other_ids else ids})
        return out


LONG = "filler " * 20 + "alpha beta" + " tail" * 3       # words 20, 21 answer "alpha beta": block 1 = words 16 .. 24
DOCS = ["x y", LONG, None, "beta z", "alpha " + "pad " * 17 + "beta"]


def results(docs):
    n = len(docs)
    return {"ids": [f"id{i}" for i in range(n)], "distances": [0.1 * i for i in range(n)],
            "metadatas": [{"i": i} for i in range(n)], "documents": list(docs)}


def manager(monkeypatch):
    m = EmbeddingManager(engine=FakeEngine())
    assert not m.supports_passages()        # FakeEngine has no encoder / tokenizer
    m._late = FakePassages()
    monkeypatch.setattr(m, "has_late_reranker", lambda: True)
    assert m.supports_passages()
    return m


def test_extract_passages_columns(monkeypatch):
    m = manager(monkeypatch)
    res = results(DOCS)
    out = asyncio.run(m.extract_passages("alpha beta", res, window_tokens=16))
    assert {k: out[k] for k in RESULT_KEYS} == {k: res[k] for k in RESULT_KEYS}        # the hits, in their order
    assert set(out) == set(RESULT_KEYS) | {"passages"} and len(out["passages"]) == 5
    assert m._late.calls == [("passages", ["alpha beta"], ["x y", LONG, "", "beta z", DOCS[4]],
                              [(0, i) for i in range(5)], 16)]
    keys = {"text", "char_start", "char_end", "token_start", "token_end", "score", "share"}
    assert all(set(p) == keys for p in out["passages"])
    none, long, gone, short, split = out["passages"]
    assert none == {"text": "x y", "char_start": 0, "char_end": 3, "token_start": 0, "token_end": 2, "score": 0.0,
                    "share": None}                                  # a whole sum that is not positive: no share
    assert long["text"] == LONG[16 * 7:] and (long["char_start"], long["char_end"]) == (112, len(LONG))
    assert (long["token_start"], long["token_end"], long["score"], long["share"]) == (16, 25, 2.0, 1.0)
    assert gone["text"] is None and gone["char_start"] is None and gone["char_end"] is None     # a None document
    assert short["text"] == "beta z" and short["share"] == 1.0
    assert split["text"] == ("alpha " + "pad " * 15).rstrip() and split["share"] == 0.5        # beta is word 18
    assert all(isinstance(p["share"], float) or p["share"] is None for p in out["passages"])
    # the default window is the setting's
    monkeypatch.setattr(emb_mod.settings, "MMRAG_PASSAGE_TOKENS", 48)
    asyncio.run(m.extract_passages("alpha", results(["alpha"])))
    assert m._late.calls[-1][4] == 48
    # other ids than the text's (the document changed since its tokens were stored): the span, but no text
    m._late.other_ids.add(LONG)
    changed = asyncio.run(m.extract_passages("alpha beta", res, window_tokens=16))["passages"][1]
    assert changed["text"] is None and changed["char_start"] is None
    assert (changed["token_start"], changed["token_end"], changed["share"]) == (16, 25, 1.0)
    # the batch form: ONE scoring call, the answers of the single calls
    m._late.other_ids.clear()
    many, qs = [results(DOCS[:2]), results([]), results(DOCS[3:])], ["alpha beta", "zzz", "beta"]
    n_before = len(m._late.calls)
    got = asyncio.run(m.batch_extract_passages(qs, many, window_tokens=32))
    assert len(m._late.calls) == n_before + 1 and m._late.calls[-1][3] == [(0, 0), (0, 1), (2, 2), (2, 3)]
    assert got == [asyncio.run(m.extract_passages(q, r, window_tokens=32)) for q, r in zip(qs, many)]
    assert got[1]["passages"] == []
    with pytest.raises(ValueError, match="result dicts"):
        asyncio.run(m.batch_extract_passages(["a"], many))
    bare = EmbeddingManager(engine=FakeEngine())
    with pytest.raises(ValueError, match="answer passages need"):
        asyncio.run(bare.extract_passages("q", res))


def test_late_rerank_with_passages_keeps_the_order(monkeypatch):
    m = manager(monkeypatch)
    res = results(DOCS)
    plain = asyncio.run(m.late_rerank("alpha beta", res, top_k=4))
    assert "passages" not in plain and m._late.calls[-1][0] == "score"
    n_before = len(m._late.calls)
    out = asyncio.run(m.late_rerank("alpha beta", res, top_k=4, passages=16))
    assert [c[0] for c in m._late.calls[n_before:]] == ["passages"]          # in place of the scores call
    assert {k: out[k] for k in plain} == plain and set(out) == set(plain) | {"passages"}
    assert out["ids"] == ["id1", "id4", "id3", "id0"]
    alone = asyncio.run(m.extract_passages("alpha beta", res, window_tokens=16))["passages"]
    assert out["passages"] == [alone[i] for i in (1, 4, 3, 0)]               # in the new order
    # through rerank_results; with explain a second call gives the matches
    via = asyncio.run(m.rerank_results("alpha beta", res, top_k=4, method="late", passages=16))
    assert via == out
    n_before = len(m._late.calls)
    both = asyncio.run(m.rerank_results("alpha beta", res, top_k=2, method="late", explain=True, passages=16))
    assert [c[0] for c in m._late.calls[n_before:]] == ["explain", "passages"]
    assert both["passages"] == out["passages"][:2] and len(both["late_matches"]) == 2
    got = asyncio.run(m.batch_late_rerank(["alpha beta", "beta"], [res, results(DOCS[3:])], top_k=2, passages=16))
    assert got[0] == {k: v[:2] for k, v in out.items()} and [p["text"] for p in got[1]["passages"]][0] == "beta z"
    with pytest.raises(ValueError, match="late-interaction re-ranking"):
        asyncio.run(m.rerank_results("alpha beta", res, method="cross", passages=16))


class WithoutPassages:
    """an embedder of an older build: everything but extract_passages / supports_passages"""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        if name in ("extract_passages", "supports_passages", "batch_extract_passages"):
            raise AttributeError(name)
        return getattr(self._inner, name)


def test_query_route_passages(monkeypatch):
    from multimodal_rag_amd import server

    monkeypatch.setattr(server.settings, "MMRAG_RERANK_CANDIDATES", 20)
    monkeypatch.setattr(server.settings, "MMRAG_RERANKER_DIR", "")
    monkeypatch.setattr(server.settings, "MMRAG_RERANK_METHOD", "cross")
    m = EmbeddingManager(engine=FakeEngine())
    with TestClient(server.create_app(embedder=m)) as c:
        for i, body in enumerate(["alpha beta gamma. " * 3, "delta epsilon. " * 30, "zeta eta theta. " * 3]):
            r = c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
        q = {"query": "delta epsilon", "top_k": 2}
        plain = c.post("/query", json=q).json()
        # the two refusals
        r = c.post("/query", json={**q, "passage_tokens": 32})
        assert r.status_code == 400 and "`passages`" in r.json()["detail"]
        r = c.post("/query", json={**q, "passages": True})
        assert r.status_code == 400 and r.json()["detail"] == server.PASSAGES_NEEDS[2]
        assert "not available with this embedder: they need" in server.PASSAGES_NEEDS[2]
        for bad in (8, 513):
            assert c.post("/query", json={**q, "passages": True, "passage_tokens": bad}).status_code == 422
        # an engine that can
        m._late = FakePassages()
        monkeypatch.setattr(m, "has_late_reranker", lambda: True)
        r = c.post("/query", json={**q, "passages": True})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert [{k: v for k, v in s.items() if k != "passage"} for s in src] == plain["sources"]
        assert m._late.calls[-1][0] == "passages" and m._late.calls[-1][4] == 64     # MMRAG_PASSAGE_TOKENS
        for s in src:
            assert set(s["passage"]) == {"text", "char_start", "char_end", "score", "share"}
            stored = m.collection.get(ids=[s["doc_id"]])["documents"][0]
            if s["passage"]["text"] is not None:
                assert s["passage"]["text"] == stored[s["passage"]["char_start"]: s["passage"]["char_end"]]
        r = c.post("/query", json={**q, "passages": True, "passage_tokens": 32})
        assert r.status_code == 200 and m._late.calls[-1][4] == 32
        # with a late re-rank it rides on the re-rank call: no scores call, no second passages call
        n_before = len(m._late.calls)
        r = c.post("/query", json={**q, "passages": True, "rerank": True, "rerank_method": "late"})
        assert r.status_code == 200, r.text
        assert [call[0] for call in m._late.calls[n_before:]] == ["passages"]
        src = r.json()["sources"]
        assert all("passage" in s and "rerank_score" in s for s in src)
        assert "delta" in src[0]["passage"]["text"].lower() and src[0]["passage"]["share"] == 1.0
        assert [s["rerank_score"] for s in src] == sorted((s["rerank_score"] for s in src), reverse=True)
        # a cross re-rank (here the placeholder's refusal aside) does not carry them: extract_passages on its hits
        n_before = len(m._late.calls)
        r = c.post("/query", json={**q, "passages": True, "rerank": True, "rerank_method": "late", "explain": True})
        assert r.status_code == 200, r.text
        assert [call[0] for call in m._late.calls[n_before:]] == ["explain", "passages"]
        assert all("passage" in s and "matches" in s for s in r.json()["sources"])
        # a request without passages is what it was
        assert c.post("/query", json=q).json()["sources"] == plain["sources"]
    with TestClient(server.create_app(embedder=WithoutPassages(m))) as c:
        r = c.post("/query", json={"query": "delta", "passages": True})
        assert r.status_code == 400 and r.json()["detail"] == server.PASSAGES_NEEDS[2]
