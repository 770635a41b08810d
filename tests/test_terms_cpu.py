"""Significant terms without a GPU: the NumPy reference on corpora worked by hand, the label rules on strings, the
library's argument checks through ctypes, and that the overflow corpus of the GPU tests really overflows."""
import ctypes
from fractions import Fraction

import numpy as np

from tests import terms_ref as R


def jlh(fg, size, bg, n):
    fgp, bgp = Fraction(fg, size), Fraction(bg, n)
    return float((fgp - bgp) * (fgp / bgp))


# ---------------------------------------------------------------- 1. the reference
def hand_corpus():
    # rows 0 1 | 2 | 3 4 5 ; term 0 everywhere, 1 in rows 0 1, 2 in rows 0 1 2, 3 in rows 3 4 5, 4 in rows 0 and 3
    rows = [[0, 1, 2, 4], [0, 1, 2], [0, 2], [0, 3, 4], [0, 3], [0, 3]]
    off, ids, _, _ = R.postings(rows)
    group = np.asarray([0, 0, -1, 1, 1, 1])
    return off, ids, group, np.asarray([2, 3]), R.live_df(off, ids, np.ones(6, bool), 5)


def test_reference_on_a_hand_worked_corpus():
    off, ids, group, sizes, df = hand_corpus()
    assert df.tolist() == [6, 2, 3, 3, 2]
    s, t, c = R.group_terms(off, ids, group, sizes, df, 6, None, 1, 4)
    # group 0 (2 rows): term 1 fg 2 of bg 2: (1 - 1/3) * 3; term 2 fg 2 of bg 3: (1 - 1/2) * 2; term 4 fg 1 of bg 2:
    # (1/2 - 1/3) * (3/2); term 0 has fgp == bgp == 1 and does not qualify
    assert t[0].tolist() == [1, 2, 4, -1] and c[0].tolist() == [2, 2, 1, 0]
    want = [jlh(2, 2, 2, 6), jlh(2, 2, 3, 6), jlh(1, 2, 2, 6)]
    assert want == [2.0, 1.0, 0.25]
    np.testing.assert_allclose(s[0, :3], want, rtol=3e-7)
    assert s[0, 3] == -np.inf and s.dtype == np.float32 and t.dtype == np.int64 and c.dtype == np.int32
    # group 1 (3 rows): term 3, fg 3 of bg 3: (1 - 1/2) * 2; term 4 has fgp == bgp == 1/3 (1/3 and 2/6 round alike)
    assert t[1].tolist() == [3, -1, -1, -1] and c[1].tolist() == [3, 0, 0, 0]
    np.testing.assert_allclose(s[1, 0], jlh(3, 3, 3, 6), rtol=3e-7)
    # min_count drops term 4; a mask drops term 1 and term 2 moves up; top cuts
    assert R.group_terms(off, ids, group, sizes, df, 6, None, 2, 4)[1][0].tolist() == [1, 2, -1, -1]
    mask = np.asarray([True, False, True, True, True])
    assert R.group_terms(off, ids, group, sizes, df, 6, mask, 2, 4)[1][0].tolist() == [2, -1, -1, -1]
    assert R.group_terms(off, ids, group, sizes, df, 6, None, 1, 1)[1].tolist() == [[1], [3]]


def test_reference_ties_padding_and_empty_groups():
    # terms 0 .. 5 are held by exactly the rows of group 0: one tie class; the lower ids win
    rows = [list(range(6)), list(range(6)), [6], [6]]
    off, ids, _, _ = R.postings(rows)
    df = R.live_df(off, ids, np.ones(4, bool), 7)
    group = np.asarray([0, 0, 2, 9])          # label 9 is outside 0 .. G-1; group 1 is empty
    s, t, c = R.group_terms(off, ids, group, [2, 0, 1], df, 4, None, 1, 4)
    assert t[0].tolist() == [0, 1, 2, 3] and len(set(s[0].tolist())) == 1 and c[0].tolist() == [2, 2, 2, 2]
    assert t[1].tolist() == [-1] * 4 and np.all(s[1] == -np.inf) and not c[1].any()
    assert t[2].tolist() == [6, -1, -1, -1] and c[2].tolist() == [1, 0, 0, 0]
    np.testing.assert_allclose(s[2, 0], jlh(1, 1, 2, 4), rtol=3e-7)
    # nothing live, no rows
    assert np.all(R.group_terms(np.zeros(1), [], [], [0, 0], np.zeros(3), 0, None, 1, 2)[1] == -1)


def test_stop_word_scores_below_theme_words():
    from multimodal_rag_amd.lexical import LEX_DOCUMENTS, Lexicon

    docs, theme = R.three_theme_corpus()
    lex = Lexicon()
    off, ids, _, _ = lex.analyze_batch(docs, LEX_DOCUMENTS)
    words = lex.terms(0, len(lex))
    df = R.live_df(off, ids, np.ones(len(docs), bool), len(lex))
    s, t, _ = R.group_terms(off, ids, theme, np.bincount(theme), df, len(docs), None, 2, len(lex))
    assert df[words.index("the")] == len(docs)
    for g, name in enumerate(R.THEMES):
        found = [words[i] for i in t[g] if i >= 0]
        assert set(found[:8]) == set(R.THEMES[name])              # the theme's words lead
        assert "the" not in found                                  # fgp == bgp: never qualifies
        function = [s[g, j] for j, w in enumerate(found) if w in R.FUNCTION_WORDS]
        assert not function or max(function) < 0.5 * s[g, 7]       # a function word is far below the weakest theme word


# ---------------------------------------------------------------- 2. which terms may be labels
def test_label_rules_on_strings():
    from multimodal_rag_amd.lexical import LEX_DOCUMENTS, LexicalIndex, analyze, label_allowed

    assert not label_allowed("ab") and label_allowed("abc") and label_allowed("ab", 2)
    assert not label_allowed("2019") and label_allowed("x86") and not label_allowed("42") and label_allowed("1st")
    acute, e_acute = chr(0x301), chr(0xE9)      # analysed terms are NFD: an accent is a code point of its own
    assert analyze("N" + e_acute) == ["ne" + acute] and label_allowed("ne" + acute)
    assert not label_allowed("n" + e_acute) and not label_allowed("")
    cafe = "caf" + "e" + acute
    lex = LexicalIndex("cpu")                  # the mask's host half needs no device
    lex.lexicon.analyze_batch(["ab 2019 x86 caf" + e_acute + " inverter Sourdough", "the"], LEX_DOCUMENTS)
    words = lex.lexicon.terms(0, len(lex.lexicon))

    def allowed(mask):
        bits = np.unpackbits(mask.numpy().view(np.uint8), bitorder="little")
        return {w for i, w in enumerate(words) if bits[i]}

    base = lex.label_mask(3)
    assert allowed(base) == {"x86", cafe, "inverter", "sourdough", "the"}
    assert lex.label_mask(3) is base                                           # kept per min_length
    assert allowed(lex.label_mask(3, exclude=["The", "SOURDOUGH!", "unknownword"])) == {"x86", cafe, "inverter"}
    assert allowed(lex.label_mask(4)) == {cafe, "inverter", "sourdough"}
    lex.lexicon.analyze_batch(["of gambit"], LEX_DOCUMENTS)                    # the lexicon grew: the mask follows
    words = lex.lexicon.terms(0, len(lex.lexicon))
    assert allowed(lex.label_mask(3)) == {"x86", cafe, "inverter", "sourdough", "the", "gambit"}
    lex._max_term = len(words) + 40                                            # synthetic terms: always allowed
    grown = np.unpackbits(lex.label_mask(3).numpy().view(np.uint8), bitorder="little")
    assert grown[len(words): len(words) + 41].all() and grown.size >= lex.n_terms


# ---------------------------------------------------------------- 3. the library's argument checks
def test_argument_checks_need_no_device():
    from multimodal_rag_amd import _native

    L = _native.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)       # never dereferenced: every call below returns before anything is launched
    EINVAL, EWORKSPACE = 1, 2

    def call(term_off=p, post_row=p, df=p, n_terms=100, n=50, group=p, sizes=p, G=3, n_live=40, bits=None,
             min_count=2, top=5, out_s=p, out_t=p, out_c=p, ws=p, ws_bytes=1 << 40):
        return L.mmrag_group_terms(term_off, post_row, df, n_terms, n, group, sizes, G, n_live, bits, min_count, top,
                                   out_s, out_t, out_c, ws, ws_bytes, None)

    for name in ("term_off", "post_row", "df", "group", "sizes", "out_s", "out_t", "out_c"):
        assert call(**{name: None}) == EINVAL, name
    assert b"null pointer" in L.mmrag_last_error()
    assert call(G=0) == EINVAL and call(G=4097) == EINVAL and call(G=-1) == EINVAL
    assert call(top=0) == EINVAL and call(top=_native.MAX_K_DEEP + 1) == EINVAL
    assert call(min_count=0) == EINVAL and call(min_count=-2) == EINVAL
    assert call(n=-1) == EINVAL and call(n_terms=-1) == EINVAL and call(n_live=-1) == EINVAL
    assert call(n_live=51) == EINVAL
    need = L.mmrag_group_terms_workspace_bytes(3, 100, 5)
    assert need > 0
    assert call(ws=None) == EWORKSPACE and call(ws_bytes=need - 1) == EWORKSPACE and call(ws_bytes=0) == EWORKSPACE
    assert b"workspace" in L.mmrag_last_error()

    size = L.mmrag_group_terms_workspace_bytes
    assert size(0, 100, 5) == 0 and size(4097, 100, 5) == 0 and size(3, -1, 5) == 0
    assert size(3, 100, 0) == 0 and size(3, 100, _native.MAX_K_DEEP + 1) == 0
    tops = [size(256, 1 << 20, k) for k in (1, 10, 512, 513, 2000, 4096)]
    assert tops == sorted(tops) and tops[-1] > tops[0]
    terms = [size(256, v, 10) for v in (0, 1, 256, 257, 5000, 16384, 16385, 1 << 20)]
    assert terms == sorted(terms) and terms[-1] > terms[0]
    # sized for one launch's window, not for n_groups
    lim = _native.terms_limits()
    assert size(lim["groups"], 5000, 10) == size(4096, 5000, 10) > size(lim["groups"] - 1, 5000, 10)
    assert lim["groups"] == 256 and lim["block_stride"] % 64 == 0 and lim["wave_limit"] >= 64
    assert lim["block_terms"] >= 1 and _native.MAX_TERM_GROUPS == 4096


def test_overflow_corpus_overflows_the_candidate_buffer():
    from multimodal_rag_amd import _native

    off, ids, _, _, group, sizes = R.overflow_corpus()
    V = R.OVERFLOW_TERMS + 1
    cap = min(_native.candidate_capacity(R.OVERFLOW_TOP), (V + 255) // 256 * 256)
    df = R.live_df(off, ids, np.ones(R.OVERFLOW_ROWS, bool), V)
    s, t, c = R.group_terms(off, ids, group, sizes, df, R.OVERFLOW_ROWS, None, 2, V)
    qualifying = int((t[0] >= 0).sum())
    assert qualifying == R.OVERFLOW_TERMS > cap == 16384
    assert t[0, : R.OVERFLOW_TOP].tolist() == list(range(R.OVERFLOW_TERMS - 5, R.OVERFLOW_TERMS))
    assert s[0, 4] > s[0, 5] and np.all(c[0, : R.OVERFLOW_TERMS] == 2)
