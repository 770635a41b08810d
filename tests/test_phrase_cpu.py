"""Host side of phrase queries (no GPU): the query language against tests/phrase_ref.py, mmrag_lexicon_analyze_positions
against the pure-Python analyzer, the reference's greedy match against brute force, the exported symbols, the argument
errors that return before any launch, the kernels' resource usage, the settings and POST /query with "phrases"."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from fastapi.testclient import TestClient

from multimodal_rag_amd import lexical as L
from multimodal_rag_amd.embedder import EmbeddingManager
from multimodal_rag_amd.server import create_app
from tests import phrase_ref as R
from tests.fakes import FakeCollection, FakeEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ, RQ = "“", "”"


# ---- the query language ----------------------------------------------------------------------------------------------
QUERIES = [
    'plain words only',
    'say "new york" twice "New  York!" and "los angeles"',
    f'curly {LQ}force majeure{RQ} and "straight ones"',
    'an "unbalanced quote stays punctuation',
    f'a closing {RQ} alone and an opening {LQ} alone',
    f'"outer {LQ}inner{RQ} rest" tail',            # the straight pair wins: curly quotes inside are punctuation
    f'{LQ}curly "inner{RQ} rest" tail',             # the curly pair wins: the straight quote after it has no partner
    '"" " " "..." empty segments',
    '"a" b "a b" a',                                # a term inside and outside quotes
    '"one two three four five six seven eight"',
    '"p1" "p2" "p3" "p4"',
    '"to be or not to be"',
    '"東京 tower" 東京',
    None,
    '',
]


def test_parser_matches_the_reference():
    for q in QUERIES:
        loose, phrases = L.query_phrases(q)
        want_loose, want = R.parse(q)
        assert loose == want_loose and [t for _, t in phrases] == want, q
        assert L.split_phrases(q) == R.split(q), q


def test_parser_fixed_points():
    assert L.split_phrases('say "new york" now') == ("say   now", ["new york"])
    assert L.split_phrases(f"{LQ}force majeure{RQ}") == (" ", ["force majeure"])
    assert L.split_phrases('an "open quote') == ('an "open quote', [])
    assert L.split_phrases(f"{RQ}x{LQ}") == (f"{RQ}x{LQ}", [])
    assert L.split_phrases(f'"a {LQ}b{RQ} c"') == (" ", [f"a {LQ}b{RQ} c"])
    assert L.split_phrases(f'{LQ}a "b{RQ} c"') == ('  c"', ['a "b'])
    loose, phrases = L.query_phrases('"a" b "a b" a "A"')
    assert [t for _, t in phrases] == [["a"], ["a", "b"]] and L.analyze(loose) == ["b", "a"]
    assert L.query_phrases('"" " " "..."')[1] == []
    assert [t for _, t in L.query_phrases('"to be or not to be"')[1]] == [["to", "be", "or", "not", "to", "be"]]
    assert [s for s, _ in L.query_phrases('"New  York!" x "new york"')[1]] == ["New  York!"]      # equal terms: one
    eight = " ".join(f"w{i}" for i in range(8))
    assert len(L.query_phrases(f'"{eight}"')[1][0][1]) == 8
    with pytest.raises(ValueError):
        L.query_phrases(f'"{eight} w8"')
    assert len(L.query_phrases('"p1" "p2" "p3" "p4" "p1"')[1]) == 4
    with pytest.raises(ValueError):
        L.query_phrases('"p1" "p2" "p3" "p4" "p5"')
    assert (L.MAX_PHRASE_TERMS, L.MAX_QUERY_PHRASES, L.MAX_PHRASE_SLOP) == \
        (R.MAX_PHRASE_TERMS, R.MAX_QUERY_PHRASES, R.MAX_PHRASE_SLOP) == (8, 4, 16)
    for ok in (0, 1, 16, np.int64(3)):
        assert L.parse_slop(ok) == int(ok)
    for bad in (-1, 17, 1.0, "1", True, None):
        with pytest.raises(ValueError):
            L.parse_slop(bad)
    assert L.parse_phrase_mode("require") == "require" and L.parse_phrase_mode("prefer") == "prefer"
    with pytest.raises(ValueError):
        L.parse_phrase_mode("must")


def test_parse_phrases_gives_ids_with_repeats():
    lx = L.Lexicon()
    lx.analyze_batch(["to be or not", "new york city"], L.LEX_DOCUMENTS)
    idx = L.LexicalIndex.__new__(L.LexicalIndex)      # parse_phrases reads the lexicon only: no device
    idx.lexicon = lx
    known = lx.terms(0, len(lx))
    (loose, phrases), (_, none) = idx.parse_phrases(['x "to be or not to be" "New York" "new jersey"', "no quotes"])
    assert none == [] and loose.split() == ["x"]
    assert [ids for _, _, ids in phrases] == [tuple(known.index(t) for t in "to be or not to be".split()),
                                              (known.index("new"), known.index("york")), (known.index("new"), -1)]
    assert len(lx) == len(known)                      # nothing was added


# ---- positions from the analyzer ---------------------------------------------------------------------------------------
def _seeded_texts(n=300, seed=11):
    g = np.random.default_rng(seed)
    pool = (["alpha", "beta", "Gamma", "the", "THE", "học", "hoc", "İstanbul", "ß", "x-ray", "a.b", "C++", "naïve"]
            + list("東京都中文") + ["é", "ọ̈", "...", "!!", "--", "(", ")", "​", "\t", "\n", "  "])
    out = []
    for _ in range(n):
        k = int(g.integers(0, 40))
        out.append("".join(pool[int(i)] + (" " if g.random() < 0.7 else "") for i in g.integers(0, len(pool), k)))
    return out + ["", None, "   ", "...!!!", "a", "a a a a"]


def _check_positions(texts, n_threads):
    lx, plain = L.Lexicon(n_threads), L.Lexicon(n_threads)
    off, ids, tfs, dl, pos = lx.analyze_positions(texts)
    off2, ids2, tfs2, dl2 = plain.analyze_batch(texts, L.LEX_DOCUMENTS)
    assert np.array_equal(off, off2) and np.array_equal(ids, ids2) and np.array_equal(tfs, tfs2)
    assert np.array_equal(dl, dl2) and len(lx) == len(plain) and lx.terms(0, len(lx)) == plain.terms(0, len(plain))
    assert pos.dtype == np.int32 and pos.size == int(dl.sum()) == int(tfs.sum())
    names = lx.terms(0, len(lx))
    at = 0
    for i, t in enumerate(texts):
        want = L.analyze(t)
        assert dl[i] == len(want)
        seq = [None] * len(want)
        for j in range(off[i], off[i + 1]):
            mine = pos[at: at + tfs[j]]
            assert np.all(np.diff(mine) > 0)                      # ascending within a pair
            for p in mine:
                assert seq[p] is None
                seq[p] = names[ids[j]]
            at += int(tfs[j])
        assert seq == want, t                                     # the positions rebuild the token sequence
    assert at == pos.size


def test_analyze_positions_matches_the_python_analyzer():
    with open(os.path.join(ROOT, "tests", "golden", "sample_document.txt"), encoding="utf-8") as f:
        doc = f.read()
    paragraphs = [p for p in doc.split("\n\n")] + [doc]
    for n_threads in (1, 4):
        _check_positions(paragraphs, n_threads)
        _check_positions(_seeded_texts(), n_threads)
    _check_positions([], 1)


def test_analyze_positions_small_capacities():
    lx = L.Lexicon()
    texts = ["alpha beta alpha gamma alpha", "İİ ǅ", ""]
    cps, offs = L._utf32(texts)
    out_off, dl, needed = np.zeros(4, np.int64), np.zeros(3, np.int32), ctypes.c_int64(-1)
    ids, tfs, pos = np.full(16, -7, np.int32), np.full(16, -7, np.int32), np.full(16, -7, np.int32)

    def call(cap, pos_cap):
        return lx._lib.mmrag_lexicon_analyze_positions(lx._h, cps.ctypes.data, offs.ctypes.data, 3, out_off.ctypes.data,
                                                       ids.ctypes.data, tfs.ctypes.data, dl.ctypes.data, cap,
                                                       pos.ctypes.data, pos_cap, ctypes.byref(needed), 1)
    assert call(4, 16) == 2 and out_off.tolist() == [0, 3, 5, 5] and needed.value == 7      # pairs do not fit
    assert call(16, 6) == 2 and out_off[3] == 5 and needed.value == 7 and dl.tolist() == [5, 2, 0]   # positions do not
    assert (pos == -7).all() and (ids == -7).all()                                          # nothing was written
    assert call(5, 7) == 0                                                                   # the retry fits exactly
    assert ids[:5].tolist() == [0, 1, 2, 3, 4] and tfs[:5].tolist() == [3, 1, 1, 1, 1]
    assert pos[:7].tolist() == [0, 2, 4, 1, 3, 0, 1] and pos[7] == -7 and len(lx) == 5                     # adding twice is harmless
    assert call(16, 0) == 2 and call(0, 0) == 2
    assert lx._lib.mmrag_lexicon_analyze_positions(None, cps.ctypes.data, offs.ctypes.data, 3, out_off.ctypes.data,
                                                   ids.ctypes.data, tfs.ctypes.data, dl.ctypes.data, 16,
                                                   pos.ctypes.data, 16, ctypes.byref(needed), 1) == 1
    assert lx._lib.mmrag_lexicon_analyze_positions(lx._h, cps.ctypes.data, offs.ctypes.data, 3, out_off.ctypes.data,
                                                   ids.ctypes.data, tfs.ctypes.data, dl.ctypes.data, 16,
                                                   pos.ctypes.data, 16, None, 1) == 1
    got = L.Lexicon().analyze_positions(texts)
    assert got[4].tolist() == pos[:7].tolist()


# ---- the reference's greedy match is the definition ---------------------------------------------------------------------
def test_reference_greedy_equals_brute_force():
    g = np.random.default_rng(5)
    for _ in range(1500):
        T = g.integers(0, 3, int(g.integers(0, 10))).tolist()
        ph = g.integers(0, 3, int(g.integers(1, 5))).tolist()
        for slop in range(5):
            assert R.tf_greedy(T, ph, slop) == R.tf_brute(T, ph, slop), (T, ph, slop)
    assert R.tf_greedy([0, 0, 0], [0, 0], 0) == 2                                     # overlaps count
    assert R.tf_greedy([0, 1, 0, 1, 0], [0, 1, 0], 0) == 2
    assert R.tf_greedy([0, 2, 1], [0, 1], 0) == 0 and R.tf_greedy([0, 2, 1], [0, 1], 1) == 1
    assert R.tf_greedy([0] + [2] * 16 + [1], [0, 1], 15) == 0 and R.tf_greedy([0] + [2] * 16 + [1], [0, 1], 16) == 1
    assert R.tf_greedy([5, 5, 5], [5], 0) == 3 and R.tf_greedy([], [5], 0) == 0


def test_reference_scores_and_hits():
    ref = R.PhraseRef([[0, 1, 2], [1, 0], [0, 1, 0, 1], [], [3]])
    live = np.array([True, True, True, True, False])
    acc, hit = ref.scores([2], [[0, 1]], live, 0, "require")
    assert hit.tolist() == [True, False, True, False, False] and acc[0] > acc[2] > 0 and acc[1] == 0
    acc_p, hit_p = ref.scores([2], [[0, 1]], live, 0, "prefer")
    assert np.array_equal(acc, acc_p) and hit_p.tolist() == [True, False, True, False, False]
    assert not ref.scores([0], [[0, 3]], live)[1].any()                     # 3 lives in a dead row only: unknown
    assert not ref.scores([0], [[0, -1]], live)[1].any()
    assert ref.scores([0], [[0, 3]], live, 0, "prefer")[1].tolist() == [True, True, True, False, False]
    assert R.bitmap([True, False, True], 4).tolist() == [5, 0, 0, 0]


# ---- the library ---------------------------------------------------------------------------------------------------------
def test_header_symbols_are_exported():
    with open(os.path.join(ROOT, "include", "mmrag.h"), encoding="utf-8") as f:
        header = f.read()
    lib = L._native.lib()
    for name in ("mmrag_lexicon_analyze_positions", "mmrag_phrase_match", "mmrag_bm25_phrase_topk_workspace_bytes",
                 "mmrag_bm25_phrase_topk"):
        assert re.search(rf"\b{name}\(", header), name
        assert hasattr(lib, name), name
    for macro, value in (("MMRAG_MAX_PHRASE_TERMS", 8), ("MMRAG_MAX_QUERY_PHRASES", 4), ("MMRAG_MAX_PHRASE_SLOP", 16)):
        assert re.search(rf"#define {macro} {value}\b", header), macro
    assert hasattr(lib, "mmrag_internal_phrase_limits") and "mmrag_internal_phrase_limits" not in header
    assert lib.mmrag_abi_version() == 1
    lim = L.phrase_limits()
    assert lim["wave_lanes"] == 64 and lim["score_rows"] == L.lexical_limits()["score_rows"]
    assert lim["match_block"] >= 64 and lim["lane_starts"] >= 1


def test_workspace_size_without_gpu():
    lib = L._native.lib()
    for B, n, k in ((1, 0, 1), (3, 4099, 21), (130, 10**6, 4096)):
        assert L.bm25_phrase_workspace_bytes(B, n, k) == L.bm25_workspace_bytes(B, n, k) > 0
    assert lib.mmrag_bm25_phrase_topk_workspace_bytes(0, 10, 1) == 0
    assert lib.mmrag_bm25_phrase_topk_workspace_bytes(1, -1, 1) == 0
    assert lib.mmrag_bm25_phrase_topk_workspace_bytes(1, 10, 0) == 0
    assert lib.mmrag_bm25_phrase_topk_workspace_bytes(1, 10, 4097) == 0


def test_argument_errors_return_before_any_launch():
    """every call below is refused with MMRAG_EINVAL (1) on a machine without a GPU: nothing was launched"""
    lib = L._native.lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data

    def match(**kw):
        a = dict(fwd_off=p, fwd_term=p, pos_off=p, pos=p, n=8, term_off=p, post_row=p, ph_off=p, ph_terms=p, ph_driver=p,
                 ptf_off=p, n_phrases=1, max_terms=2, longest=4, slop=0, alive=None, ptf=p, ph_rows=p, q_ph_off=p, q_ph=p,
                 B=1, max_phrases=1, bitmaps=p, stream=None)
        a.update(kw)
        return lib.mmrag_phrase_match(*a.values())

    for bad in (dict(slop=-1), dict(slop=17), dict(max_terms=9), dict(max_terms=-1), dict(max_phrases=5),
                dict(n_phrases=-1), dict(B=-1), dict(n=-1), dict(n=2**31), dict(longest=-1), dict(ph_off=None),
                dict(ph_terms=None), dict(ph_driver=None), dict(ptf_off=None), dict(ph_rows=None), dict(fwd_off=None),
                dict(fwd_term=None), dict(pos_off=None), dict(pos=None), dict(term_off=None), dict(post_row=None),
                dict(ptf=None), dict(q_ph_off=None), dict(q_ph=None)):
        assert match(**bad) == 1, bad
        assert "phrase_match" in L._native.lib().mmrag_last_error().decode()

    def topk(**kw):
        a = dict(term_off=p, post_row=p, post_tf=p, dl=p, df=p, n_terms=4, n=8, q_off=p, q_terms=p, B=1, q_ph_off=p,
                 q_ph=p, ph_off=p, ph_terms=p, ph_driver=p, ptf_off=p, ptf=p, n_phrases=1, max_terms=2, max_phrases=1,
                 require=1, n_live=8, sum_dl=8, k1=1.2, b=0.75, k=5, alive=None, out_s=p, out_r=p, ws=p, ws_bytes=512,
                 stream=None)
        a.update(kw)
        return lib.mmrag_bm25_phrase_topk(*a.values())

    for bad in (dict(B=0), dict(k=0), dict(k=4097), dict(n=-1), dict(n=2**31), dict(n_terms=-1), dict(n_live=9),
                dict(sum_dl=-1), dict(k1=-1.0), dict(b=1.5), dict(n_phrases=-1), dict(max_terms=9), dict(max_phrases=5),
                dict(max_phrases=-1), dict(out_s=None), dict(out_r=None), dict(q_off=None), dict(q_ph_off=None),
                dict(q_ph=None), dict(ph_off=None), dict(ph_terms=None), dict(ph_driver=None), dict(ptf_off=None),
                dict(ptf=None), dict(term_off=None), dict(post_row=None), dict(post_tf=None), dict(dl=None),
                dict(df=None), dict(q_terms=None)):
        assert topk(**bad) == 1, bad
        assert "bm25_phrase_topk" in L._native.lib().mmrag_last_error().decode()
    assert topk(ws=None) == 2 and topk(ws_bytes=16) == 2          # MMRAG_EWORKSPACE, also before any launch


def test_phrase_kernels_no_scratch_no_spills():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c", "-I",
                        os.path.join(ROOT, "include"), os.path.join(ROOT, "multimodal_rag_amd", "csrc", "phrase.hip"),
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern in ("phrase_match_kernel", "phrase_bitmap_kernel", "bm25_phrase_score_kernel"):
        assert any(kern in n for n in names), kern
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(x) for x in re.findall(r"[VS]GPRs Spill: (\d+)", r.stderr)]
    assert scratch and not any(scratch) and not any(spills)
    # (the translation unit also instantiates deep_select.h's select, which keeps its key cache in LDS)
    for block in r.stderr.split("Function Name: ")[1:]:
        if any(kern in block.split()[0] for kern in ("phrase_match_kernel", "phrase_bitmap_kernel", "bm25_phrase_score")):
            assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", block).group(1)) <= 64 * 1024, block[:80]


# ---- settings and the service layers ---------------------------------------------------------------------------------------
def test_settings_are_checked(monkeypatch):
    from multimodal_rag_amd.config import Settings, settings

    assert settings.MMRAG_LEXICAL_PHRASES is False and settings.MMRAG_LEXICAL_SLOP == 0 and settings.lexical_slop() == 0
    monkeypatch.setenv("MMRAG_LEXICAL_PHRASES", "1")
    monkeypatch.setenv("MMRAG_LEXICAL_SLOP", "16")
    s = Settings()
    assert s.MMRAG_LEXICAL_PHRASES is True and s.MMRAG_LEXICAL_SLOP == 16
    for bad in ("17", "-1", "two"):
        monkeypatch.setenv("MMRAG_LEXICAL_SLOP", bad)
        with pytest.raises(ValueError):
            Settings()


class PhraseCollection(FakeCollection):
    """the fake collection plus a hybrid_query that takes `phrases` / `slop` and says what it got"""

    def hybrid_query(self, query_embeddings, query_texts, n_results=10, where=None, include=(), fuzzy=None,
                     phrases=None, slop=0, phrase_mode="require"):
        res = self.query(query_embeddings, n_results=n_results, where=where)
        res["hybrid_scores"] = [[1.0 / (61 + i) for i in range(len(ids))] for ids in res["ids"]]
        res["lexical_scores"] = [[0.0] * len(ids) for ids in res["ids"]]
        if phrases:
            res["phrases"] = [[{"text": seg, "terms": terms, "known": True, "rows": slop}
                               for seg, terms in L.query_phrases(t)[1]] for t in query_texts]
        return res


def _phrase_engine(monkeypatch):
    eng = FakeEngine()
    orig = eng.new_collection

    def new_collection(*a, **kw):
        c = orig(*a, **kw)
        c.__class__ = PhraseCollection
        return c

    monkeypatch.setattr(eng, "new_collection", new_collection)
    return eng


def test_query_endpoint_phrases_schema_and_400s(monkeypatch):
    m = EmbeddingManager(engine=_phrase_engine(monkeypatch))
    with TestClient(create_app(embedder=m)) as c:
        for i, body in enumerate(["alpha beta gamma. " * 3, "delta epsilon. " * 3, "zeta eta theta. " * 3]):
            assert c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")}).status_code == 200
        q = 'find "delta epsilon" please'
        plain = c.post("/query", json={"query": q, "top_k": 2, "hybrid": True})
        assert plain.status_code == 200 and "phrases" not in plain.json()
        r = c.post("/query", json={"query": q, "top_k": 2, "hybrid": True, "phrases": True})
        assert r.status_code == 200, r.text
        assert r.json()["phrases"] == [{"text": "delta epsilon", "terms": ["delta", "epsilon"], "known": True, "rows": 0}]
        assert r.json()["sources"] == plain.json()["sources"]
        r = c.post("/query", json={"query": q, "top_k": 2, "hybrid": True, "phrases": True, "slop": 3,
                                   "hybrid_leg": "lexical"})
        assert r.status_code == 200 and r.json()["phrases"][0]["rows"] == 3
        r = c.post("/query", json={"query": q, "top_k": 2, "hybrid": True, "phrases": True, "rerank": False, "fuzzy": 1})
        assert r.status_code == 200 and "phrases" in r.json()
        off = c.post("/query", json={"query": q, "top_k": 2, "hybrid": True, "phrases": False})
        assert off.status_code == 200 and "phrases" not in off.json()
        # the two refusals, each with its one-line reason, as `fuzzy` is refused
        r = c.post("/query", json={"query": q, "top_k": 2, "phrases": True})
        assert r.status_code == 400 and "`phrases`" in r.json()["detail"] and "`hybrid`" in r.json()["detail"]
        r = c.post("/query", json={"query": q, "top_k": 2, "hybrid": True, "hybrid_leg": "sparse", "phrases": True})
        assert r.status_code == 400 and "lexical leg" in r.json()["detail"] and "\n" not in r.json()["detail"]
        r = c.post("/query", json={"query": q, "top_k": 2, "slop": 1})
        assert r.status_code == 400
        for bad in (17, -1):
            r = c.post("/query", json={"query": q, "top_k": 2, "hybrid": True, "phrases": True, "slop": bad})
            assert r.status_code == 400 and "slop" in r.json()["detail"], r.text
        nine = " ".join(f"w{i}" for i in range(9))
        r = c.post("/query", json={"query": f'"{nine}"', "top_k": 2, "hybrid": True, "phrases": True})
        assert r.status_code == 400 and "8" in r.json()["detail"]
        r = c.post("/query", json={"query": '"a" "b" "c" "d" "e"', "top_k": 2, "hybrid": True, "phrases": True})
        assert r.status_code == 400 and "4" in r.json()["detail"]


def test_settings_turn_phrases_on_by_default(monkeypatch):
    import asyncio

    from multimodal_rag_amd.config import settings

    m = EmbeddingManager(engine=_phrase_engine(monkeypatch))

    async def go():
        await m.initialize()
        await m.embed_and_store([{"id": f"t{i}", "type": "text", "summary": d}
                                 for i, d in enumerate(["alpha beta", "gamma delta"])], "doc")
        q = 'the "gamma delta" one'
        assert "phrases" not in await m.hybrid_query(q, n_results=1)
        got = await m.hybrid_query(q, n_results=1, phrases=True, slop=2)
        assert got["phrases"] == [{"text": "gamma delta", "terms": ["gamma", "delta"], "known": True, "rows": 2}]
        monkeypatch.setattr(settings, "MMRAG_LEXICAL_PHRASES", True)
        monkeypatch.setattr(settings, "MMRAG_LEXICAL_SLOP", 5)
        assert (await m.hybrid_query(q, n_results=1))["phrases"][0]["rows"] == 5
        assert (await m.hybrid_query(q, n_results=1, slop=1))["phrases"][0]["rows"] == 1
        assert "phrases" not in await m.hybrid_query(q, n_results=1, phrases=False)
        with pytest.raises(ValueError):
            await m.hybrid_query(q, n_results=1, leg="sparse", phrases=True)
        with pytest.raises(ValueError):
            await m.hybrid_query(q, n_results=1, phrases=True, slop=17)
        # the positions plane is reported once it exists
        assert "lexical_positions_bytes" not in await m.get_collection_stats()
        m.collection.positions_enabled, m.collection.positions_bytes = True, lambda: 4096
        assert (await m.get_collection_stats())["lexical_positions_bytes"] == 4096

    asyncio.run(go())
