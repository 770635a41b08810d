"""NumPy restatement of the significant-terms aggregation (csrc/terms.hip, LexicalIndex.group_terms), plus the small
corpora its tests share.

For group g and term t, with fg = the rows labelled g that hold t (a posting counts once), size = group_size[g],
bg = df[t] and N = n_live, the pair qualifies when size > 0, bg > 0, fg >= min_count, t is set in the mask and
fgp > bgp for fgp = float32(fg) / float32(size), bgp = float32(bg) / float32(N); its score is (fgp - bgp) * (fgp / bgp)
in float32, one rounding per operation.  A group's result: its `top` qualifying terms by score descending, ties to the
lower term id, padded with (-inf, -1, 0)."""
import numpy as np


def group_terms(off, ids, group, group_size, df, n_live, mask, min_count, top):
    """(scores [G, top] float32, terms [G, top] int64, counts [G, top] int32) from the forward log (off [n + 1], the
    rows' term ids), the labels group [n] (-1 or anything outside 0 .. G-1: in no group), group_size [G], the live
    df [V], n_live, a bool mask [V] or None, min_count and top"""
    off = np.asarray(off, np.int64)
    ids = np.asarray(ids, np.int64)
    group = np.asarray(group, np.int64)
    group_size = np.asarray(group_size, np.int64)
    df = np.asarray(df, np.int64)
    G, V, n = group_size.size, df.size, off.size - 1
    out_s = np.full((G, top), -np.inf, np.float32)
    out_t = np.full((G, top), -1, np.int64)
    out_c = np.zeros((G, top), np.int32)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    g = group[rows] if n else np.zeros(0, np.int64)
    inside = (g >= 0) & (g < G)
    pair, fg = np.unique(g[inside] * V + ids[: rows.size][inside], return_counts=True)
    pg, pt = pair // V, pair % V
    size, bg = group_size[pg], df[pt]
    ok = (size > 0) & (bg > 0) & (fg >= min_count) & (n_live > 0)
    if mask is not None:
        ok &= np.asarray(mask, bool)[pt]
    with np.errstate(divide="ignore", invalid="ignore"):
        fgp = fg.astype(np.float32) / size.astype(np.float32)
        bgp = bg.astype(np.float32) / np.float32(n_live)
        ok &= fgp > bgp
        score = (fgp - bgp) * (fgp / bgp)
    assert score.dtype == np.float32
    for c in range(G):
        at = np.nonzero(ok & (pg == c))[0]
        order = at[np.lexsort((pt[at], -score[at]))][:top]
        out_s[c, : order.size] = score[order]
        out_t[c, : order.size] = pt[order]
        out_c[c, : order.size] = fg[order]
    return out_s, out_t, out_c


def live_df(off, ids, live, n_terms):
    """df over the live rows of a forward log"""
    off = np.asarray(off, np.int64)
    rows = np.repeat(np.arange(off.size - 1), np.diff(off))
    return np.bincount(np.asarray(ids, np.int64)[: rows.size][np.asarray(live, bool)[rows]], minlength=n_terms)


def postings(row_terms):
    """append_postings' arrays (off, ids, tfs, dl) of rows given as collections of distinct term ids"""
    lists = [np.sort(np.asarray(list(t), np.int32)) for t in row_terms]
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([t.size for t in lists], out=off[1:])
    ids = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return off, ids, np.ones(ids.size, np.int32), np.diff(off).astype(np.int32)


# ---- the three-theme corpus: short documents of theme words among function words
THEMES = {
    "solar": ["inverter", "photovoltaic", "panel", "kilowatt", "battery", "grid", "rooftop", "irradiance"],
    "bread": ["sourdough", "starter", "flour", "knead", "crumb", "proofing", "oven", "gluten"],
    "chess": ["gambit", "endgame", "bishop", "castling", "checkmate", "opening", "rook", "zugzwang"],
}
FUNCTION_WORDS = ["the", "and", "with", "for", "that", "this", "from", "have"]


def three_theme_corpus(n_docs=120, seed=0, theme=None):
    """(documents, theme index per document): document i is about theme[i] (default i % 3) -- five distinct words of
    its theme among six function words, "the" in every one"""
    g = np.random.default_rng(seed)
    names = list(THEMES)
    theme = np.arange(n_docs) % 3 if theme is None else np.asarray(theme)
    docs = []
    for t in theme.tolist():
        words = list(g.choice(THEMES[names[t]], 5, replace=False)) + ["the"] + list(g.choice(FUNCTION_WORDS, 5))
        docs.append(" ".join(words[j] for j in g.permutation(len(words))).capitalize() + ".")
    return docs, theme


# ---- the overflow corpus: more qualifying pairs in one group than a candidate buffer holds
OVERFLOW_TERMS, OVERFLOW_TOP, OVERFLOW_ROWS = 20000, 5, 8


def overflow_corpus():
    """(off, ids, tfs, dl, group, group_size): 8 live rows; group 0 is rows 0 and 1, which both hold terms
    0 .. 19999; row 2, outside the group, holds all but the five highest of them; rows 3 .. 7 hold one filler term.
    Every one of the 20000 terms qualifies (fgp = 1 > bgp), and the five that row 2 lacks have the lower bgp (2 / 8
    against 3 / 8): they alone are the top five, in id order."""
    T = OVERFLOW_TERMS
    every = np.arange(T)
    rows = [every, every, every[: T - OVERFLOW_TOP]] + [[T]] * (OVERFLOW_ROWS - 3)
    group = np.full(OVERFLOW_ROWS, -1, np.int32)
    group[:2] = 0
    return postings(rows) + (group, np.asarray([2], np.int32))
