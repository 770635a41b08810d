"""float64 restatement of the phrase-query contract (multimodal_rag_amd/lexical.py, csrc/phrase.hip, include/mmrag.h):
the query language, the match under a slop, the phrase clause of the BM25 score and the two hit rules.  Pure Python /
NumPy; nothing is imported from the package, so the device path is checked against a second statement of the rules."""
import itertools
import math

import numpy as np

from tests import bm25_ref

MAX_PHRASE_TERMS = 8
MAX_QUERY_PHRASES = 4
MAX_PHRASE_SLOP = 16
_CLOSING = {'"': '"', "“": "”"}


def split(text):
    """(loose text, segments): a segment stands between two '"' or between U+201C and U+201D; an opening quote without
    its closing one is ordinary punctuation; left to right, a segment ends at the first closing quote of its kind"""
    text = text or ""
    loose, segments, i = [], [], 0
    while i < len(text):
        close = _CLOSING.get(text[i])
        j = text.find(close, i + 1) if close else -1
        if j < 0:
            loose.append(text[i])
            i += 1
        else:
            segments.append(text[i + 1: j])
            loose.append(" ")
            i = j + 1
    return "".join(loose), segments


def parse(text):
    """(loose text, [term lists]): the distinct phrases in order of appearance, repeats inside a phrase kept"""
    loose, segments = split(text)
    phrases = []
    for seg in segments:
        terms = bm25_ref.analyze(seg)
        if not terms or terms in phrases:
            continue
        if len(terms) > MAX_PHRASE_TERMS:
            raise ValueError("phrase too long")
        phrases.append(terms)
    if len(phrases) > MAX_QUERY_PHRASES:
        raise ValueError("too many phrases")
    return loose, phrases


def tf_greedy(T, phrase, slop):
    """starts i with T[i] = phrase[0] from which the earliest next position of every following term keeps the span
    within the slop"""
    count, m = 0, len(phrase)
    for i, t in enumerate(T):
        if t != phrase[0]:
            continue
        prev, ok = i, True
        for j in range(1, m):
            nxt = next((p for p in range(prev + 1, len(T)) if T[p] == phrase[j]), None)
            if nxt is None:
                ok = False
                break
            prev = nxt
        count += ok and prev - i - (m - 1) <= slop
    return count


def tf_brute(T, phrase, slop):
    """the definition itself: starts i for which SOME increasing positions i = p0 < p1 < .. exist"""
    count, m = 0, len(phrase)
    for i, t in enumerate(T):
        if t != phrase[0]:
            continue
        found = False
        for rest in itertools.combinations(range(i + 1, len(T)), m - 1):
            if all(T[p] == phrase[j + 1] for j, p in enumerate(rest)) and (rest[-1] if rest else i) - i - (m - 1) <= slop:
                found = True
                break
        count += found
    return count


class PhraseRef:
    """rows as term-id sequences; BM25 with phrase clauses in float64"""

    def __init__(self, seqs):
        self.seqs = [list(map(int, s)) for s in seqs]
        self.n = len(self.seqs)
        off, ids, tfs, dl = [0], [], [], []
        self.holders = {}
        for r, s in enumerate(self.seqs):
            counts = {}
            for t in s:
                counts[t] = counts.get(t, 0) + 1
            for t in sorted(counts):
                ids.append(t)
                tfs.append(counts[t])
                self.holders.setdefault(t, []).append(r)
            off.append(len(ids))
            dl.append(len(s))
        self.bm25 = bm25_ref.RefIndex(off, ids, tfs, dl)
        self._tf = {}

    def df(self, t, live):
        rows = self.holders.get(t, [])
        return int(np.asarray(live, bool)[rows].sum()) if rows else 0

    def known(self, phrase, live):
        return all(t >= 0 and self.df(t, live) >= 1 for t in phrase)

    def tf(self, phrase, slop):
        """tf_p of every row [n] (dead rows included: the caller masks them)"""
        key = (tuple(phrase), slop)
        if key not in self._tf:
            out = np.zeros(self.n, np.int64)
            rows = set(self.holders.get(phrase[0], []))
            for t in phrase[1:]:
                rows &= set(self.holders.get(t, []))
            for r in rows:
                out[r] = tf_greedy(self.seqs[r], phrase, slop)
            self._tf[key] = out
        return self._tf[key]

    def scores(self, q_ids, phrases, live, slop=0, mode="require", k1=1.2, b=0.75, visible=None):
        """(score [n] float64, hit [n] bool) before `allowed`: the loose terms in order, then the phrases in order.
        `visible` (default: live): the rows the match may see -- alive and passing `where`; tf_p is 0 elsewhere."""
        live = np.asarray(live, bool)
        visible = live if visible is None else np.asarray(visible, bool)
        acc, matched = self.bm25.scores(q_ids, live, k1, b)
        N = int(live.sum())
        total = self.bm25.dl[live].sum()
        avgdl = total / N if N and total else 1.0
        holds_all = np.ones(self.n, bool)
        for ph in phrases:
            if not self.known(ph, live):
                holds_all[:] = False
                continue
            tf = np.where(visible, self.tf(ph, slop), 0).astype(np.float64)
            idf = 0.0
            for t in ph:
                df = self.df(t, live)
                idf += math.log(1.0 + (N - df + 0.5) / (df + 0.5))
            rows = tf > 0
            acc[rows] += idf * tf[rows] * (k1 + 1) / (tf[rows] + k1 * (1 - b + b * self.bm25.dl[rows] / avgdl))
            matched = matched | rows
            holds_all &= rows
        if phrases and mode == "require":
            return acc, holds_all
        return acc, matched


def bitmap(flags, words):
    """bit r & 31 of word r >> 5, `words` uint32 words"""
    bits = np.zeros(words * 32, bool)
    bits[: len(flags)] = flags
    return np.packbits(bits, bitorder="little").view(np.uint32)
