"""BM25 lexical retrieval on the device, and reciprocal-rank fusion with the dense leg.

The reference's Chroma store keeps every document in a full-text index beside its vector index; this module is that
leg for `VectorIndex`.  Analysis is host code (csrc/tokenizer.cpp, with `analyze` below as its
pure-Python twin); postings, statistics and scoring live on the device (csrc/lexical.hip).

Scoring contract (the tests pin it against tests/bm25_ref.py):
  score(q, d) = sum over the distinct known terms t of q, in order of first occurrence, of
                idf_t * tf (k1 + 1) / (tf + k1 (1 - b + b dl / avgdl)),   idf_t = ln(1 + (N - df_t + 0.5) / (df_t + 0.5))
  with N, avgdl = sum(dl) / N and df over the LIVE rows (a `where` filter restricts results, not statistics), float32 on
  the device.  Rows with score > 0, alive and passing `where`, ordered by score, ties to the lower row.

Typo tolerance (opt-in, `fuzzy=`; the tests pin it against tests/fuzzy_ref.py): a query term no live row holds is
replaced by its closest indexed term -- optimal-string-alignment distance within 0..2 edits, then larger live df, then
lower id -- found on the device over the lexicon's strings (csrc/fuzzy.hip); the list then goes to the same scoring.

Phrase queries (opt-in, `phrases=`; the tests pin them against tests/phrase_ref.py): a quoted segment of the query is a
phrase, matched against the token positions of every row (the positions plane, built by the first phrase query) by
csrc/phrase.hip and scored as one more BM25 clause; under phrase_mode="require" only rows holding every phrase are hits.
"""
from __future__ import annotations

import os
import unicodedata
from ctypes import byref, c_float, c_int, c_int64, c_size_t, c_void_p
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .tokenizer import _is_cjk, _is_punct, _utf32

LEX_DOCUMENTS, LEX_QUERIES = 0, 1   # mmrag_lexicon_analyze_batch modes (include/mmrag.h)


def analyze(text: Optional[str]) -> List[str]:
    """The BM25 terms of `text` (pure Python; csrc/tokenizer.cpp analyze_text is the native twin): BERT's cleaning,
    CJK spacing and whitespace split, then per word str.lower() and NFD keeping the combining marks, split at
    punctuation, which is dropped.  No stemming, no stop words.  None is empty."""
    if not text:
        return []
    out = []
    for ch in text:
        cp = ord(ch)
        if cp == 0 or cp == 0xFFFD or (unicodedata.category(ch) in ("Cc", "Cf") and ch not in "\t\n\r"):
            continue
        if _is_cjk(cp):
            out.append(f" {ch} ")
        elif ch in " \t\n\r" or unicodedata.category(ch) == "Zs":
            out.append(" ")
        else:
            out.append(ch)
    terms: List[str] = []
    for w in "".join(out).split():
        cur = ""
        for ch in unicodedata.normalize("NFD", w.lower()):
            if _is_punct(ch):
                if cur:
                    terms.append(cur)
                cur = ""
            else:
                cur += ch
        if cur:
            terms.append(cur)
    return terms


def rrf_fuse(dense_rows: Sequence[int], lexical_rows: Sequence[int], k: int = 60) -> List[Tuple[int, float]]:
    """Reciprocal-rank fusion of one query's two ranked row lists: every row of either list with score
    sum 1 / (k + rank) over the lists it is in (ranks 1-based, the dense term added first), ordered by score
    descending, ties to the better dense rank (absent = worst), then to the lower row."""
    dense_rank = {int(r): i + 1 for i, r in enumerate(dense_rows)}
    score: Dict[int, float] = {r: 1.0 / (k + rank) for r, rank in dense_rank.items()}
    for i, r in enumerate(lexical_rows):
        r = int(r)
        score[r] = score.get(r, 0.0) + 1.0 / (k + i + 1)
    worst = len(dense_rank) + 1
    order = sorted(score, key=lambda r: (-score[r], dense_rank.get(r, worst), r))
    return [(r, score[r]) for r in order]


class Lexicon:
    """term string -> int32 id in first-seen order (libmmrag.so's native lexicon).  Host only: works without a GPU."""

    def __init__(self, n_threads: int = 0):
        self._lib = _native.lib()
        self._h = self._lib.mmrag_lexicon_create()
        self.n_threads = n_threads or min(16, os.cpu_count() or 1)

    def __len__(self) -> int:
        return int(self._lib.mmrag_lexicon_size(self._h))

    def analyze_batch(self, texts: Sequence[Optional[str]], mode: int):
        """(offsets int64 [n+1], term_ids int32, tfs int32, dl int32 [n]) of `texts`; pairs of text i at
        offsets[i] .. offsets[i+1].  LEX_DOCUMENTS adds unseen terms (pairs sorted by id); LEX_QUERIES drops unknown
        terms (pairs in order of first occurrence)."""
        cps, offs = _utf32([t or "" for t in texts])
        n = len(texts)
        out_off = np.zeros(n + 1, np.int64)
        dl = np.zeros(n, np.int32)
        cap = int(cps.size) + 1
        while True:
            ids = np.empty(cap, np.int32)
            tfs = np.empty(cap, np.int32)
            st = self._lib.mmrag_lexicon_analyze_batch(self._h, cps.ctypes.data, offs.ctypes.data, n, mode,
                                                       out_off.ctypes.data, ids.ctypes.data, tfs.ctypes.data,
                                                       dl.ctypes.data, cap, self.n_threads)
            if st == 2 and int(out_off[n]) > cap:      # MMRAG_EWORKSPACE: more pairs than code points (rare)
                cap = int(out_off[n])
                continue
            _native._check(st, "mmrag_lexicon_analyze_batch")
            total = int(out_off[n])
            return out_off, ids[:total], tfs[:total], dl

    def analyze_positions(self, texts: Sequence[Optional[str]]):
        """analyze_batch(texts, LEX_DOCUMENTS) and a fifth array: every pair's token positions (0-based token indices),
        ascending, concatenated in pair order -- sum(dl) int32 (mmrag_lexicon_analyze_positions)"""
        cps, offs = _utf32([t or "" for t in texts])
        n = len(texts)
        out_off = np.zeros(n + 1, np.int64)
        dl = np.zeros(n, np.int32)
        needed = c_int64(0)
        cap = pos_cap = int(cps.size) + 1
        while True:
            ids = np.empty(cap, np.int32)
            tfs = np.empty(cap, np.int32)
            pos = np.empty(pos_cap, np.int32)
            st = self._lib.mmrag_lexicon_analyze_positions(self._h, cps.ctypes.data, offs.ctypes.data, n,
                                                           out_off.ctypes.data, ids.ctypes.data, tfs.ctypes.data,
                                                           dl.ctypes.data, cap, pos.ctypes.data, pos_cap, byref(needed),
                                                           self.n_threads)
            if st == 2 and (int(out_off[n]) > cap or int(needed.value) > pos_cap):   # MMRAG_EWORKSPACE (rare)
                cap, pos_cap = max(cap, int(out_off[n])), max(pos_cap, int(needed.value))
                continue
            _native._check(st, "mmrag_lexicon_analyze_positions")
            total = int(out_off[n])
            return out_off, ids[:total], tfs[:total], dl, pos[: int(needed.value)]

    def export(self, first_id: int, count: int):
        """(offsets int64 [count+1] from 0, code points uint32) of terms first_id .. first_id + count"""
        offs = np.zeros(count + 1, np.int64)
        cps = np.empty(max(8 * count, 1), np.uint32)
        while True:
            st = self._lib.mmrag_lexicon_export(self._h, first_id, count, offs.ctypes.data, cps.ctypes.data, cps.size)
            if st == 2 and int(offs[count]) > cps.size:        # MMRAG_EWORKSPACE: offsets say how much
                cps = np.empty(int(offs[count]), np.uint32)
                continue
            _native._check(st, "mmrag_lexicon_export")
            return offs, cps[: int(offs[count])]

    def terms(self, first_id: int, count: int) -> List[str]:
        """the term strings of ids first_id .. first_id + count"""
        offs, cps = self.export(first_id, count)
        return [_str_of(cps[offs[i]: offs[i + 1]]) for i in range(count)]

    def analyze_terms(self, texts: Sequence[Optional[str]]):
        """(offsets int64 [n+1], term_ids int32, cp_offsets int64 [total+1], cps uint32): every distinct term of each
        text in order of first occurrence, unknown ones (id -1) included; term j of the batch is
        cps[cp_offsets[j] .. cp_offsets[j+1])"""
        cps, offs = _utf32([t or "" for t in texts])
        n = len(texts)
        out_off = np.zeros(n + 1, np.int64)
        needed = np.zeros(2, np.int64)
        t_cap, c_cap = int(cps.size) + 1, 2 * int(cps.size) + 16
        while True:
            ids = np.empty(t_cap, np.int32)
            cp_off = np.zeros(t_cap + 1, np.int64)
            out = np.empty(c_cap, np.uint32)
            st = self._lib.mmrag_lexicon_analyze_terms(self._h, cps.ctypes.data, offs.ctypes.data, n,
                                                       out_off.ctypes.data, ids.ctypes.data, cp_off.ctypes.data,
                                                       out.ctypes.data, t_cap, c_cap, needed.ctypes.data,
                                                       self.n_threads)
            if st == 2 and (int(needed[0]) > t_cap or int(needed[1]) > c_cap):   # decompositions outgrew the guess
                t_cap, c_cap = max(t_cap, int(needed[0])), max(c_cap, int(needed[1]))
                continue
            _native._check(st, "mmrag_lexicon_analyze_terms")
            total = int(needed[0])
            return out_off, ids[:total], cp_off[: total + 1], out[: int(needed[1])]

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.mmrag_lexicon_destroy(h)


def _str_of(cps: np.ndarray) -> str:
    return np.ascontiguousarray(cps, np.uint32).tobytes().decode("utf-32-le", "surrogatepass")


FUZZY_MAX_LEN = 64          # MMRAG_FUZZY_MAX_LEN: longer terms are neither corrected nor corrected to
FUZZY_MAX_EXPANSIONS = 16   # MMRAG_FUZZY_MAX_EXPANSIONS


def parse_fuzzy(fuzzy):
    """None (off), "auto" or an int 0..2 from what callers pass: None / "" / False, True / "auto", 0..2 / "0".."2" """
    if fuzzy is None or fuzzy is False or fuzzy == "":
        return None
    if fuzzy is True:
        return "auto"
    if isinstance(fuzzy, str):
        s = fuzzy.strip().lower()
        if s == "auto":
            return "auto"
        if s in ("0", "1", "2"):
            return int(s)
    elif isinstance(fuzzy, (int, np.integer)) and 0 <= int(fuzzy) <= 2:
        return int(fuzzy)
    raise ValueError(f"fuzzy must be 'auto', True or an integer 0..2, not {fuzzy!r}")


def fuzzy_edits(fuzzy, n_code_points: int) -> int:
    """the edits allowed to a term of n_code_points under `fuzzy` (parse_fuzzy's value, not None).  "auto" is the
    AUTO:3,6 rule: 0 for 1-2 code points, 1 for 3-5, 2 for 6 or more.  Terms above FUZZY_MAX_LEN get 0."""
    if n_code_points > FUZZY_MAX_LEN:
        return 0
    if fuzzy == "auto":
        return 0 if n_code_points < 3 else 1 if n_code_points < 6 else 2
    return int(fuzzy)


def rewrite_terms(terms: Sequence[Tuple[int, str]], live: Sequence[bool], best: Dict[str, Tuple[int, int]]):
    """One query's term list under typo tolerance (pure Python; tests/fuzzy_ref.py restates it).  `terms` are its
    distinct (id, string) in order of first occurrence, id -1 when unknown; live[i] says the term is in the lexicon with
    live df >= 1; best maps a term string to its best candidate (term id, edits).  A term that is not live is replaced
    at the place it stood by its best candidate, or dropped when it has none; of equal ids the first stays.  Returns
    (ids, corrections) with corrections [(term, matched id, edits)] for every term that found a candidate."""
    ids: List[int] = []
    corrections: List[Tuple[str, int, int]] = []
    for (tid, s), ok in zip(terms, live):
        if not ok:
            if s not in best:
                continue
            tid, e = best[s]
            corrections.append((s, int(tid), int(e)))
        if tid not in ids:
            ids.append(int(tid))
    return ids, corrections


MAX_PHRASE_TERMS = 8       # MMRAG_MAX_PHRASE_TERMS
MAX_QUERY_PHRASES = 4      # MMRAG_MAX_QUERY_PHRASES
MAX_PHRASE_SLOP = 16       # MMRAG_MAX_PHRASE_SLOP
PHRASE_MODES = ("require", "prefer")


def split_phrases(text: Optional[str]) -> Tuple[str, List[str]]:
    """(the text outside the quotes, the quoted segments in order) of a query under `phrases`: a segment between two
    '"' (U+0022), or between U+201C and U+201D, is a phrase; an opening quote without its closing one is ordinary
    punctuation.  The scan runs left to right and a segment ends at the first closing quote of its own kind, so quotes
    do not nest.  Each segment leaves a space in the loose text."""
    text = text or ""
    loose: List[str] = []
    segments: List[str] = []
    i = 0
    while i < len(text):
        ch = text[i]
        close = '"' if ch == '"' else "\u201d" if ch == "\u201c" else None
        j = text.find(close, i + 1) if close else -1
        if j < 0:
            loose.append(ch)
            i += 1
            continue
        segments.append(text[i + 1: j])
        loose.append(" ")
        i = j + 1
    return "".join(loose), segments


def query_phrases(text: Optional[str]) -> Tuple[str, List[Tuple[str, List[str]]]]:
    """(loose text, [(segment text, its terms)]) of one query under `phrases` (pure Python): the distinct phrases in
    order of appearance, each segment analysed like a document with repeats kept.  An empty segment is ignored and equal
    term sequences are one phrase; a segment of more than MAX_PHRASE_TERMS terms or more than MAX_QUERY_PHRASES distinct
    phrases raise ValueError."""
    loose, segments = split_phrases(text)
    mine: List[Tuple[str, List[str]]] = []
    for seg in segments:
        terms = analyze(seg)
        if not terms or any(terms == t for _, t in mine):
            continue
        if len(terms) > MAX_PHRASE_TERMS:
            raise ValueError(f"a phrase holds at most {MAX_PHRASE_TERMS} terms: {seg!r} has {len(terms)}")
        mine.append((seg, terms))
    if len(mine) > MAX_QUERY_PHRASES:
        raise ValueError(f"a query holds at most {MAX_QUERY_PHRASES} distinct phrases, not {len(mine)}")
    return loose, mine


def parse_slop(slop) -> int:
    if isinstance(slop, bool) or not isinstance(slop, (int, np.integer)) or not 0 <= int(slop) <= MAX_PHRASE_SLOP:
        raise ValueError(f"slop must be an integer in 0..{MAX_PHRASE_SLOP}, not {slop!r}")
    return int(slop)


def parse_phrase_mode(mode) -> str:
    if mode not in PHRASE_MODES:
        raise ValueError(f"phrase_mode must be 'require' or 'prefer', not {mode!r}")
    return mode


def label_allowed(term: str, min_length: int = 3) -> bool:
    """may an analysed term stand in a topic label or a keyword list (LexicalIndex.label_mask): at least `min_length`
    code points (as analysed: NFD, so an accent counts as one) and not decimal digits only"""
    return len(term) >= min_length and not term.isdecimal()


def _grow(t: torch.Tensor, need: int) -> torch.Tensor:
    if t.numel() >= need:
        return t
    out = torch.zeros(max(need, 2 * t.numel()), dtype=t.dtype, device=t.device)
    out[: t.numel()].copy_(t)
    return out


class LexicalIndex:
    """The device lexical state of one `VectorIndex` (its owner holds the lock around every call).

    Forward log (row-major postings, grown like the matrix) and per-row dl on the device; df per term kept by integer
    kernels; N and sum(dl) as host integers.  The term-major CSR is rebuilt on the device (counting sort) by the first
    search after adds; deletes only update df, N and sum(dl) -- the alive bits filter dead rows."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.reset()

    def reset(self):
        dev = self.device
        self.n = 0
        self.n_live = 0
        self.sum_dl = 0
        self._off_host = np.zeros(1, np.int64)
        self._dl_host = np.zeros(0, np.int32)
        self._fwd_off = torch.zeros(257, dtype=torch.int64, device=dev)
        self._fwd_term = torch.zeros(4096, dtype=torch.int32, device=dev)
        self._fwd_tf = torch.zeros(4096, dtype=torch.int32, device=dev)
        self._dl = torch.zeros(256, dtype=torch.int32, device=dev)
        self._df = torch.zeros(1024, dtype=torch.int32, device=dev)
        self._csr = None                  # (term_off, post_row, post_tf) of rows [0, _csr_n), n_terms = _csr_terms
        self._csr_n = self._csr_terms = -1
        self._csr_ws = None
        self._search_ws = None
        self.csr_builds = 0               # how many times the CSR was rebuilt (tests, tools)
        self.lexicon = Lexicon()
        self._max_term = -1               # largest term id appended (synthetic postings bypass the lexicon)
        # the term plane (fuzzy matching): the lexicon's strings on the device, synchronised by the first fuzzy call
        # after adds.  Terms of synthetic postings have no strings and are not in it.
        self._tp_off = torch.zeros(1025, dtype=torch.int32, device=dev)    # [_tp_n + 1] code point offsets
        self._tp_cps = torch.zeros(8192, dtype=torch.int32, device=dev)    # uint32 code points (bit pattern)
        self._tp_n = 0
        self._tp_total = 0
        self._fuzzy_ws = None
        self.term_plane_syncs = 0         # how many times terms were uploaded (tests, tools)
        # the positions plane (phrase queries): built by enable_positions(), None until then
        self._pos_off = None              # int64 [n_postings + 1]: prefix sum of tf over the forward postings
        self._pos = None                  # int32 [sum(dl)]: each forward posting's token positions, ascending
        self._pos_total = 0
        self._counts_host = None          # postings per term of the current CSR (driver choice), read once per build
        self._counts_build = -1
        self._phrase_ws = None
        self.position_builds = 0          # how many times the plane was built from documents (tests, tools)
        # significant terms (group_terms / label_mask)
        self._terms_ws = None
        self._label_masks: Dict[int, Dict[str, object]] = {}   # min_length -> the rule's verdicts and their bitmap

    @property
    def n_terms(self) -> int:
        return max(len(self.lexicon), self._max_term + 1)

    @property
    def n_postings(self) -> int:
        return int(self._off_host[-1])

    def _stream(self) -> int:
        return _native._stream_ptr(self.device)

    def append(self, documents: Sequence[Optional[str]]):
        """analyse and append rows n .. n + len(documents), all alive"""
        m = len(documents)
        if m == 0:
            return
        if self.positions_enabled:
            off, ids, tfs, dl, pos = self.lexicon.analyze_positions(documents)
            self.append_postings(off, ids, tfs, dl, pos)
            return
        off, ids, tfs, dl = self.lexicon.analyze_batch(documents, LEX_DOCUMENTS)
        self.append_postings(off, ids, tfs, dl)

    def append_postings(self, off: np.ndarray, ids: np.ndarray, tfs: np.ndarray, dl: np.ndarray,
                        positions: Optional[np.ndarray] = None):
        """append already analysed rows (offsets [m+1] from 0, term ids sorted within each row, distinct): the form
        `Lexicon.analyze_batch(..., LEX_DOCUMENTS)` returns; tools feed synthetic corpora through it.  `positions`
        (the fifth array of `Lexicon.analyze_positions`) is needed once the positions plane exists."""
        m = int(dl.size)
        p0 = self.n_postings
        if self.positions_enabled:
            if positions is None:
                raise ValueError("the positions plane is enabled: rows need their token positions (append_sequences)")
            self._append_positions(p0, np.asarray(tfs, np.int64), np.ascontiguousarray(positions, np.int32))
        if ids.size:
            self._max_term = max(self._max_term, int(ids.max()))
        new_off = p0 + np.asarray(off, np.int64)
        self._fwd_off = _grow(self._fwd_off, self.n + m + 1)
        self._fwd_term = _grow(self._fwd_term, p0 + int(ids.size))
        self._fwd_tf = _grow(self._fwd_tf, p0 + int(ids.size))
        self._dl = _grow(self._dl, self.n + m)
        self._df = _grow(self._df, max(self.n_terms, 1))
        self._fwd_off[self.n: self.n + m + 1].copy_(torch.from_numpy(new_off))
        if ids.size:
            self._fwd_term[p0: p0 + ids.size].copy_(torch.from_numpy(np.ascontiguousarray(ids, np.int32)))
            self._fwd_tf[p0: p0 + ids.size].copy_(torch.from_numpy(np.ascontiguousarray(tfs, np.int32)))
        self._dl[self.n: self.n + m].copy_(torch.from_numpy(np.ascontiguousarray(dl, np.int32)))
        self._off_host = np.concatenate([self._off_host[:-1], new_off])
        self._dl_host = np.concatenate([self._dl_host, np.asarray(dl, np.int32)])
        with torch.cuda.device(self.device):
            _native._check(_native.lib().mmrag_lexical_df_update(self._fwd_off.data_ptr(), self._fwd_term.data_ptr(),
                                                                 None, self.n, m, 1, self._df.data_ptr(),
                                                                 self._stream()), "mmrag_lexical_df_update")
        self.n += m
        self.n_live += m
        self.sum_dl += int(np.asarray(dl, np.int64).sum())

    def delete_rows(self, rows: np.ndarray):
        """rows (live, distinct) became dead: df, N and sum(dl) drop them; the CSR stays valid"""
        rows = np.ascontiguousarray(rows, np.int64)
        if rows.size == 0:
            return
        dev_rows = torch.from_numpy(rows).to(self.device)
        with torch.cuda.device(self.device):
            _native._check(_native.lib().mmrag_lexical_df_update(self._fwd_off.data_ptr(), self._fwd_term.data_ptr(),
                                                                 dev_rows.data_ptr(), 0, rows.size, -1,
                                                                 self._df.data_ptr(), self._stream()),
                           "mmrag_lexical_df_update")
        self.n_live -= int(rows.size)
        self.sum_dl -= int(self._dl_host[rows].astype(np.int64).sum())

    def compact(self, keep: np.ndarray):
        """keep only rows `keep` (ascending, the live ones), renumbered 0 .. len(keep): df, N and sum(dl) are
        unchanged (the dropped rows were already subtracted); the CSR is rebuilt by the next search"""
        keep = np.asarray(keep, np.int64)
        P = self.n_postings
        off = self._off_host
        term = self._fwd_term[:P].cpu().numpy()
        tf = self._fwd_tf[:P].cpu().numpy()
        lens = off[keep + 1] - off[keep]
        new_off = np.zeros(keep.size + 1, np.int64)
        np.cumsum(lens, out=new_off[1:])
        src = (np.repeat(off[keep] - new_off[:-1], lens) + np.arange(int(new_off[-1]), dtype=np.int64))
        self._off_host = new_off
        self._dl_host = self._dl_host[keep]
        self.n = int(keep.size)
        self._fwd_off[: self.n + 1].copy_(torch.from_numpy(new_off))
        if src.size:
            self._fwd_term[: src.size].copy_(torch.from_numpy(term[src]))
            self._fwd_tf[: src.size].copy_(torch.from_numpy(tf[src]))
        if self.n:
            self._dl[: self.n].copy_(torch.from_numpy(self._dl_host))
        if self.positions_enabled:
            pos_off = self._pos_off[: P + 1].cpu().numpy()
            pos = self._pos[: self._pos_total].cpu().numpy()
            plens = pos_off[src + 1] - pos_off[src]
            new_pos_off = np.zeros(src.size + 1, np.int64)
            np.cumsum(plens, out=new_pos_off[1:])
            psrc = np.repeat(pos_off[src] - new_pos_off[:-1], plens) + np.arange(int(new_pos_off[-1]), dtype=np.int64)
            self._pos_off[: src.size + 1].copy_(torch.from_numpy(new_pos_off))
            if psrc.size:
                self._pos[: psrc.size].copy_(torch.from_numpy(pos[psrc]))
            self._pos_total = int(new_pos_off[-1])
        self._csr_n = -1

    def _ensure_csr(self):
        V, n, P = self.n_terms, self.n, self.n_postings
        if self._csr is not None and self._csr_n == n and self._csr_terms == V:
            return self._csr
        L = _native.lib()
        term_off = torch.empty(V + 1, dtype=torch.int64, device=self.device)
        post_row = torch.empty(max(P, 1), dtype=torch.int32, device=self.device)
        post_tf = torch.empty(max(P, 1), dtype=torch.int32, device=self.device)
        need = int(L.mmrag_lexical_csr_build_workspace_bytes(n, V))
        if self._csr_ws is None or self._csr_ws.numel() < need:
            self._csr_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _native._check(L.mmrag_lexical_csr_build(self._fwd_off.data_ptr(), self._fwd_term.data_ptr(),
                                                     self._fwd_tf.data_ptr(), n, P, V, term_off.data_ptr(),
                                                     post_row.data_ptr(), post_tf.data_ptr(), self._csr_ws.data_ptr(),
                                                     self._csr_ws.numel(), self._stream()), "mmrag_lexical_csr_build")
        self._csr, self._csr_n, self._csr_terms = (term_off, post_row, post_tf), n, V
        self.csr_builds += 1
        return self._csr

    def analyze_queries(self, query_texts: Sequence[str]):
        """(q_off int32 [B+1], q_terms int32) on the host: each query's distinct known terms, first occurrence first"""
        off, ids, _, _ = self.lexicon.analyze_batch(list(query_texts), LEX_QUERIES)
        return off.astype(np.int32), ids

    def _sync_term_plane(self):
        """upload the terms the lexicon gained since the last fuzzy call (ids are append-only, so this is a suffix)"""
        V = len(self.lexicon)
        if V > self._tp_n:
            offs, cps = self.lexicon.export(self._tp_n, V - self._tp_n)
            total = self._tp_total + int(cps.size)
            if total >= 2 ** 31:
                raise ValueError(f"the lexicon's {total} code points exceed the term plane's 2^31 - 1")
            self._tp_off = _grow(self._tp_off, V + 1)
            self._tp_cps = _grow(self._tp_cps, max(total, 1))
            self._tp_off[self._tp_n: V + 1].copy_(torch.from_numpy((offs + self._tp_total).astype(np.int32)))
            if cps.size:
                self._tp_cps[self._tp_total: total].copy_(torch.from_numpy(cps.view(np.int32)))
            self._tp_n, self._tp_total = V, total
            self.term_plane_syncs += 1
        self._df = _grow(self._df, max(V, 1))

    def fuzzy_terms(self, terms: Sequence[str], edits: Sequence[int], max_expansions: int = 1):
        """For each analysed term string the best lexicon terms within edits[i] (0..2) optimal-string-alignment edits
        (csrc/fuzzy.hip): (term ids [P, E] int32, edits [P, E] int32) on the host, best first (fewer edits, then
        larger live df, then lower id), -1 padded.  Candidates have live df >= 1 and at most FUZZY_MAX_LEN code
        points; a longer term string has none."""
        P, E = len(terms), int(max_expansions)
        if not 1 <= E <= FUZZY_MAX_EXPANSIONS:
            raise ValueError(f"max_expansions must be in 1..{FUZZY_MAX_EXPANSIONS}")
        if len(edits) != P:
            raise ValueError(f"{len(edits)} edit budgets for {P} terms")
        pe = np.ascontiguousarray(edits, np.int32)
        if P and (pe.min() < 0 or pe.max() > 2):
            raise ValueError("edits must be 0, 1 or 2")
        if P == 0:
            return np.zeros((0, E), np.int32), np.zeros((0, E), np.int32)
        self._sync_term_plane()
        cps, offs = _utf32(list(terms))
        return self.fuzzy_ids(self._tp_off, self._tp_cps, self._df, self._tp_n, offs.astype(np.int32), cps, pe, E)

    def fuzzy_ids(self, term_off: torch.Tensor, term_cps: torch.Tensor, df: torch.Tensor, n_terms: int,
                  pat_off: np.ndarray, pat_cps: np.ndarray, pat_edits: np.ndarray, max_expansions: int):
        """mmrag_fuzzy_terms over an explicit term plane (device int32 offsets, code points, df) and host patterns"""
        P, E = int(pat_off.size) - 1, int(max_expansions)
        dev = self.device
        d_off = torch.from_numpy(np.ascontiguousarray(pat_off, np.int32)).to(dev)
        d_cps = torch.from_numpy(np.concatenate([np.ascontiguousarray(pat_cps, np.uint32).view(np.int32),
                                                 np.zeros(1, np.int32)])).to(dev)
        d_ed = torch.from_numpy(np.ascontiguousarray(pat_edits, np.int32)).to(dev)
        L = _native.lib()
        need = int(L.mmrag_fuzzy_terms_workspace_bytes(n_terms, P, E))
        if self._fuzzy_ws is None or self._fuzzy_ws.numel() < need:
            self._fuzzy_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        out_t = torch.empty((P, E), dtype=torch.int32, device=dev)
        out_e = torch.empty((P, E), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _native._check(L.mmrag_fuzzy_terms(term_off.data_ptr(), term_cps.data_ptr(), df.data_ptr(), n_terms,
                                               d_off.data_ptr(), d_cps.data_ptr(), d_ed.data_ptr(), P, E,
                                               out_t.data_ptr(), out_e.data_ptr(), self._fuzzy_ws.data_ptr(),
                                               self._fuzzy_ws.numel(), self._stream()), "mmrag_fuzzy_terms")
        return out_t.cpu().numpy(), out_e.cpu().numpy()

    def analyze_queries_fuzzy(self, query_texts: Sequence[str], fuzzy):
        """analyze_queries under typo tolerance: (q_off, q_terms, corrections).  Only terms that contribute nothing
        today -- unknown, or known with live df == 0 -- are corrected, each to its single best candidate
        (rewrite_terms); corrections[i] lists query i's {"term", "matched", "edits"}.  Collection-wide, like df."""
        fuzzy = parse_fuzzy(fuzzy)
        off, ids, cp_off, cps = self.lexicon.analyze_terms(list(query_texts))
        strings = [_str_of(cps[cp_off[j]: cp_off[j + 1]]) for j in range(int(ids.size))]
        self._sync_term_plane()
        live = np.zeros(ids.size, bool)
        known = ids >= 0
        if known.any():
            df = self._df[torch.from_numpy(ids[known].astype(np.int64)).to(self.device)].cpu().numpy()
            live[known] = df >= 1
        want: Dict[str, int] = {}
        for j in np.nonzero(~live)[0]:
            e = fuzzy_edits(fuzzy, int(cp_off[j + 1] - cp_off[j]))
            if e > 0 and cp_off[j + 1] - cp_off[j] <= FUZZY_MAX_LEN:
                want.setdefault(strings[j], e)
        best: Dict[str, Tuple[int, int]] = {}
        if want and self._tp_n:
            pats = list(want)
            got_t, got_e = self.fuzzy_terms(pats, [want[p] for p in pats], 1)
            best = {p: (int(got_t[i, 0]), int(got_e[i, 0])) for i, p in enumerate(pats) if got_t[i, 0] >= 0}
        q_off = np.zeros(off.size, np.int32)
        q_terms: List[int] = []
        corrections: List[List[Dict[str, object]]] = []
        names: Dict[int, str] = {}
        for i in range(off.size - 1):
            lo, hi = int(off[i]), int(off[i + 1])
            kept, made = rewrite_terms([(int(ids[j]), strings[j]) for j in range(lo, hi)], live[lo:hi], best)
            q_terms.extend(kept)
            q_off[i + 1] = len(q_terms)
            for _, tid, _ in made:
                if tid not in names:
                    names[tid] = self.lexicon.terms(tid, 1)[0]
            corrections.append([{"term": s, "matched": names[tid], "edits": e} for s, tid, e in made])
        return q_off, np.asarray(q_terms, np.int32), corrections

    def topk(self, query_texts: Sequence[str], k: int, alive_bits: Optional[torch.Tensor] = None,
             k1: Optional[float] = None, b: Optional[float] = None, fuzzy=None, phrases=None, slop: int = 0,
             phrase_mode: str = "require", bitmaps: bool = False):
        """(scores [B, k] float32 desc, rows [B, k] int64; (-inf, -1) padding) on the device.  With `fuzzy`
        ("auto", True or 0..2) the query terms BM25 would drop are corrected first (analyze_queries_fuzzy) and the
        corrections come back as a third value.  With `phrases` quoted segments are phrases (parse_phrases) and the
        call returns topk_phrases' five values: scores, rows, corrections (None without `fuzzy`), the per-query phrase
        report and, for `bitmaps`, the per-query row bitmaps inside the last value."""
        if len(query_texts) == 0:
            raise ValueError("no query texts")
        if not 1 <= k <= _native.MAX_K_DEEP:
            raise ValueError(f"n_results must be in 1..{_native.MAX_K_DEEP} for lexical search")
        if phrases:
            return self.topk_phrases(query_texts, k, alive_bits, k1, b, fuzzy, slop, phrase_mode, bitmaps)
        if parse_fuzzy(fuzzy) is not None:
            q_off, q_terms, corrections = self.analyze_queries_fuzzy(query_texts, fuzzy)
            return self.topk_ids(q_off, q_terms, k, alive_bits, k1, b) + (corrections,)
        q_off, q_terms = self.analyze_queries(query_texts)
        return self.topk_ids(q_off, q_terms, k, alive_bits, k1, b)

    def topk_ids(self, q_off: np.ndarray, q_terms: np.ndarray, k: int, alive_bits: Optional[torch.Tensor] = None,
                 k1: Optional[float] = None, b: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """topk over already analysed queries: query i's distinct term ids q_terms[q_off[i] .. q_off[i+1])"""
        from .config import settings

        k1 = settings.MMRAG_BM25_K1 if k1 is None else k1
        b = settings.MMRAG_BM25_B if b is None else b
        B = int(q_off.size) - 1
        q_off = np.ascontiguousarray(q_off, np.int32)
        q_terms = np.ascontiguousarray(q_terms, np.int32)
        if q_terms.size and (q_terms.min() < 0 or q_terms.max() >= self.n_terms):
            raise ValueError("query term id outside the lexicon")
        term_off, post_row, post_tf = self._ensure_csr()
        dq_off = torch.from_numpy(q_off).to(self.device)
        dq_terms = torch.from_numpy(np.concatenate([q_terms, np.zeros(1, np.int32)])).to(self.device)
        L = _native.lib()
        need = int(L.mmrag_bm25_topk_workspace_bytes(B, self.n, k))
        if self._search_ws is None or self._search_ws.numel() < need:
            self._search_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        out_s = torch.empty((B, k), dtype=torch.float32, device=self.device)
        out_r = torch.empty((B, k), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _native._check(L.mmrag_bm25_topk(term_off.data_ptr(), post_row.data_ptr(), post_tf.data_ptr(),
                                             self._dl.data_ptr(), self._df.data_ptr(), self.n_terms, self.n,
                                             dq_off.data_ptr(), dq_terms.data_ptr(), B, self.n_live, self.sum_dl,
                                             float(k1), float(b), k,
                                             alive_bits.data_ptr() if alive_bits is not None else None,
                                             out_s.data_ptr(), out_r.data_ptr(), self._search_ws.data_ptr(),
                                             self._search_ws.numel(), self._stream()), "mmrag_bm25_topk")
        return out_s, out_r

    def df_host(self) -> np.ndarray:
        """live df per term (tests)"""
        return self._df[: self.n_terms].cpu().numpy()

    # ------------------------------------------------------------------ significant terms ----
    def group_terms(self, group: torch.Tensor, group_size, top: int, min_count: int = 2,
                    term_bits: Optional[torch.Tensor] = None):
        """Each group's significant terms (csrc/terms.hip; the tests pin it against tests/terms_ref.py): `group` is an
        int32 device tensor [>= n] labelling every row 0 .. G-1 or -1 (dead rows -1), `group_size` [G] the rows per
        label.  Returns device (scores [G, top] float32, terms [G, top] int64, counts [G, top] int32): per group the
        terms with the highest JLH score (fgp - bgp) * (fgp / bgp) among those at least `min_count` of its rows hold,
        set in `term_bits` (label_mask's bitmap; None: every term) and more frequent in the group than in the live
        collection; ties to the lower term id, (-inf, -1, 0) padding."""
        if not isinstance(group, torch.Tensor) or group.dtype != torch.int32 or group.numel() < self.n:
            raise ValueError(f"group must be an int32 device tensor of at least {self.n} labels")
        if not isinstance(group_size, torch.Tensor):
            group_size = torch.from_numpy(np.ascontiguousarray(group_size, np.int32))
        group_size = group_size.to(device=self.device, dtype=torch.int32).contiguous()
        G = int(group_size.numel())
        if not 1 <= G <= _native.MAX_TERM_GROUPS:
            raise ValueError(f"significant terms take 1..{_native.MAX_TERM_GROUPS} groups, not {G}")
        if not 1 <= int(top) <= _native.MAX_K_DEEP:
            raise ValueError(f"top must be in 1..{_native.MAX_K_DEEP}")
        if int(min_count) < 1:
            raise ValueError("min_count must be at least 1")
        term_off, post_row, _ = self._ensure_csr()
        self._df = _grow(self._df, max(self.n_terms, 1))      # the kernel reads df of every term of the vocabulary
        need = _native.group_terms_workspace_bytes(G, self.n_terms, int(top))
        if self._terms_ws is None or self._terms_ws.numel() < need:
            self._terms_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        return _native.group_terms(term_off, post_row, self._df, self.n_terms, self.n, group.contiguous(), group_size,
                                   self.n_live, int(top), int(min_count), term_bits, self._terms_ws)

    def label_mask(self, min_length: int = 3, exclude: Sequence[str] = ()) -> torch.Tensor:
        """The device bitmap (int32 words, bit t & 31 of word t >> 5) of the terms allowed as labels: at least
        `min_length` code points and not digits only (label_allowed); the terms of the `exclude` words, analysed like
        a document, are cleared.  Terms of synthetic postings have no strings and are always allowed.  The rule's
        verdicts are kept per min_length and extended by the terms the lexicon gained, as the term plane is."""
        min_length = int(min_length)
        if isinstance(exclude, str):
            raise ValueError("exclude must be a list of words")
        V, L = self.n_terms, len(self.lexicon)
        entry = self._label_masks.setdefault(min_length, {"allowed": np.zeros(0, bool), "dev": None, "terms": -1})
        known = int(entry["allowed"].size)
        if L > known:
            fresh = self.lexicon.terms(known, L - known)
            entry["allowed"] = np.concatenate([entry["allowed"],
                                               np.fromiter((label_allowed(s, min_length) for s in fresh), bool, L - known)])
            entry["dev"] = None
        drop = [int(t) for t in self.lexicon.analyze_terms(list(exclude))[1] if t >= 0] if len(exclude) else []
        if not drop and entry["dev"] is not None and entry["terms"] == V:
            return entry["dev"]
        bits = np.ones(32 * max((V + 31) // 32, 1), bool)
        bits[:L] = entry["allowed"]
        bits[drop] = False
        dev = torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32).copy()).to(self.device)
        if not drop:
            entry["dev"], entry["terms"] = dev, V
        return dev

    # ------------------------------------------------------------------ positions plane / phrase queries ----
    documents_source = None   # set by the owner: a callable returning the stored documents in row order

    @property
    def positions_enabled(self) -> bool:
        return self._pos_off is not None

    @property
    def positions_bytes(self) -> int:
        """device bytes of the positions plane (0 until it exists)"""
        if not self.positions_enabled:
            return 0
        return self._pos_off.numel() * 8 + self._pos.numel() * 4

    def enable_positions(self):
        """Build the positions plane: re-analyse the stored documents in row order (dead rows included, so the rows
        stay aligned with the forward log; the lexicon already holds every term, so the pairs come out as they stand
        there).  From then on append, compact and reset keep it current; a delete needs nothing.  Runs by itself on
        the first phrase query; an index that never sees one allocates none of it."""
        if self.positions_enabled:
            return
        dev = self.device
        self._pos_off = torch.zeros(4097, dtype=torch.int64, device=dev)
        self._pos = torch.zeros(4096, dtype=torch.int32, device=dev)
        self._pos_total = 0
        if self.n == 0:
            return
        docs = self.documents_source() if self.documents_source is not None else None
        if docs is None or len(docs) != self.n:
            self._pos_off = self._pos = None
            raise ValueError("the positions plane needs the stored documents of every row: rows appended as bare "
                             "postings have no positions (use append_sequences from the start)")
        step = 65536
        p0 = 0
        for lo in range(0, self.n, step):
            off, ids, tfs, dl, pos = self.lexicon.analyze_positions(docs[lo: lo + step])
            hi = lo + int(dl.size)
            if (not np.array_equal(off + self._off_host[lo], self._off_host[lo: hi + 1])
                    or not np.array_equal(dl, self._dl_host[lo:hi])):
                self._pos_off = self._pos = None
                raise ValueError("the stored documents do not match the forward log")
            self._append_positions(p0, tfs.astype(np.int64), pos)
            p0 += int(ids.size)
        self.position_builds += 1

    def _append_positions(self, p0: int, tfs: np.ndarray, positions: np.ndarray):
        """forward postings p0 .. p0 + len(tfs) stand at `positions` (tf each, in posting order)"""
        if int(tfs.sum()) != int(positions.size):
            raise ValueError(f"{positions.size} positions for postings with {int(tfs.sum())} occurrences")
        ends = self._pos_total + np.cumsum(tfs, dtype=np.int64)
        total = int(ends[-1]) if ends.size else self._pos_total
        if total >= 2 ** 31:
            raise ValueError(f"{total} stored tokens exceed the positions plane's 2^31 - 1")
        self._pos_off = _grow(self._pos_off, p0 + tfs.size + 1)
        self._pos = _grow(self._pos, max(total, 1))
        if ends.size:
            self._pos_off[p0 + 1: p0 + 1 + ends.size].copy_(torch.from_numpy(ends))
        if positions.size:
            self._pos[self._pos_total: total].copy_(torch.from_numpy(positions))
        self._pos_total = total

    def append_sequences(self, seqs: Sequence[Sequence[int]]):
        """append rows given as raw term-id sequences (token order, repeats kept): postings and positions are derived
        on the host and the lexicon is bypassed -- append_postings' twin for tests and tools.  Enables the positions
        plane on an empty index; a non-empty one must have it already."""
        if not self.positions_enabled:
            if self.n:
                raise ValueError("append_sequences needs the positions plane from the first row on")
            self.enable_positions()
        lens = np.fromiter((len(s) for s in seqs), np.int64, len(seqs))
        m = int(lens.size)
        flat = (np.concatenate([np.asarray(s, np.int64).reshape(-1) for s in seqs]) if m else np.zeros(0, np.int64))
        if flat.size and (flat.min() < 0 or flat.max() >= 2 ** 31 - 1):
            raise ValueError("term ids must be in 0..2^31-2")
        starts = np.zeros(m + 1, np.int64)
        np.cumsum(lens, out=starts[1:])
        rows = np.repeat(np.arange(m, dtype=np.int64), lens)
        where = np.arange(flat.size, dtype=np.int64) - np.repeat(starts[:-1], lens)
        order = np.lexsort((where, flat, rows))
        rows_s, terms_s = rows[order], flat[order]
        first = np.ones(flat.size, bool)
        first[1:] = (rows_s[1:] != rows_s[:-1]) | (terms_s[1:] != terms_s[:-1])
        at = np.nonzero(first)[0]
        tfs = np.diff(np.append(at, flat.size)).astype(np.int32)
        off = np.zeros(m + 1, np.int64)
        np.cumsum(np.bincount(rows_s[at], minlength=m), out=off[1:])
        self.append_postings(off, terms_s[at].astype(np.int32), tfs, lens.astype(np.int32),
                             where[order].astype(np.int32))

    def _posting_counts(self) -> np.ndarray:
        """postings per term of the current CSR on the host (read once per CSR build): the driver choice"""
        term_off, _, _ = self._ensure_csr()
        if self._counts_build != self.csr_builds:
            self._counts_host = np.diff(term_off.cpu().numpy())
            self._counts_build = self.csr_builds
        return self._counts_host

    def parse_phrases(self, query_texts: Sequence[Optional[str]]):
        """The query language of `phrases` (query_phrases) with the lexicon's ids: per query (loose text,
        [(segment text, [term strings], (term ids))]), id -1 for a term the lexicon does not hold.  The string -> id map
        comes from the native analyzer (mmrag_lexicon_analyze_terms); nothing is added to the lexicon."""
        split = [query_phrases(t) for t in query_texts]
        segs = [seg for _, mine in split for seg, _ in mine]
        ids_of: Dict[str, int] = {}
        if segs:
            off, ids, cp_off, cps = self.lexicon.analyze_terms(segs)
            for j in range(int(ids.size)):
                ids_of[_str_of(cps[cp_off[j]: cp_off[j + 1]])] = int(ids[j])
        return [(loose, [(seg, terms, tuple(ids_of.get(t, -1) for t in terms)) for seg, terms in mine])
                for loose, mine in split]

    def match_phrases(self, phrases: Sequence[Sequence[int]], slop: int = 0,
                      alive_bits: Optional[torch.Tensor] = None, q_phrases: Optional[Sequence[Sequence[int]]] = None,
                      bitmaps: bool = False) -> Dict[str, object]:
        """mmrag_phrase_match for `phrases` (term-id sequences, -1 = unknown term): a dict with
          known     [NP] bool (host): every term in the lexicon with live df >= 1
          drivers   [NP] int32 (host): the driver term of each known phrase (fewest postings, ties to the earlier
                    position), -1 for the others
          ptf_off   [NP + 1] int64 (host) and ptf (device int32): tf_p per posting of each driver's CSR list
          rows      [NP] int32 (device): rows with tf_p >= 1
          bitmaps   with `bitmaps`, device int32 [B, filter_words(n)]: query i's rows holding every phrase of
                    q_phrases[i] (indices into `phrases`); all rows below n for a query without phrases
        and the device tables ("tables") that topk_phrase_ids hands to the scoring call."""
        slop = parse_slop(slop)
        if not self.positions_enabled:
            raise ValueError("phrase matching needs the positions plane (enable_positions)")
        phrases = [tuple(int(t) for t in ph) for ph in phrases]
        NP = len(phrases)
        for ph in phrases:
            if not 1 <= len(ph) <= MAX_PHRASE_TERMS:
                raise ValueError(f"a phrase holds 1..{MAX_PHRASE_TERMS} terms, not {len(ph)}")
            if max(ph) >= self.n_terms:
                raise ValueError("phrase term id outside the lexicon")
        q_phrases = [list(q) for q in (q_phrases if q_phrases is not None else [])]
        B = len(q_phrases)
        for q in q_phrases:
            if len(q) > MAX_QUERY_PHRASES or len(set(q)) != len(q) or any(not 0 <= i < NP for i in q):
                raise ValueError(f"a query holds at most {MAX_QUERY_PHRASES} distinct phrases of the batch")
        counts = self._posting_counts()
        term_off, post_row, _ = self._csr
        dev = self.device
        flat = np.asarray([t for ph in phrases for t in ph], np.int64)
        known_t = flat >= 0
        if known_t.any():
            df = self._df[torch.from_numpy(flat[known_t]).to(dev)].cpu().numpy()
            known_t[known_t] = df >= 1
        ph_off = np.zeros(NP + 1, np.int32)
        np.cumsum([len(ph) for ph in phrases], out=ph_off[1:])
        known = np.asarray([bool(known_t[ph_off[i]: ph_off[i + 1]].all()) for i in range(NP)], bool)
        drivers = np.full(NP, -1, np.int32)
        ptf_off = np.zeros(NP + 1, np.int64)
        for i, ph in enumerate(phrases):
            if known[i]:
                drivers[i] = ph[int(np.argmin([counts[t] for t in ph]))]     # argmin: ties to the earlier position
            ptf_off[i + 1] = ptf_off[i] + (int(counts[drivers[i]]) if known[i] else 0)
        longest = int(max((counts[d] for d in drivers if d >= 0), default=0))
        q_off = np.zeros(B + 1, np.int32)
        np.cumsum([len(q) for q in q_phrases], out=q_off[1:])
        blob = np.concatenate([ph_off, np.maximum(flat, 0).astype(np.int32), np.zeros(1, np.int32), drivers, q_off,
                               np.asarray([i for q in q_phrases for i in q], np.int32), np.zeros(1, np.int32)])
        d_blob = torch.from_numpy(blob).to(dev)
        d_ptf_off = torch.from_numpy(ptf_off).to(dev)
        base = d_blob.data_ptr()
        at_terms = 4 * (NP + 1)
        at_drv = at_terms + 4 * (int(flat.size) + 1)
        at_qoff = at_drv + 4 * NP
        at_qph = at_qoff + 4 * (B + 1)
        tables = {"blob": d_blob, "ph_off": base, "ph_terms": base + at_terms, "ph_driver": base + at_drv,
                  "q_ph_off": base + at_qoff, "q_ph": base + at_qph, "ptf_off": d_ptf_off, "n_phrases": NP,
                  "max_terms": max((len(ph) for ph in phrases), default=0),
                  "max_phrases": max((len(q) for q in q_phrases), default=0)}
        ptf = torch.empty(max(int(ptf_off[-1]), 1), dtype=torch.int32, device=dev)
        rows = torch.zeros(max(NP, 1), dtype=torch.int32, device=dev)
        maps = None
        if bitmaps:
            maps = torch.zeros((B, _native.filter_words(self.n)), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _native._check(_native.lib().mmrag_phrase_match(
                self._fwd_off.data_ptr(), self._fwd_term.data_ptr(), self._pos_off.data_ptr(), self._pos.data_ptr(),
                self.n, term_off.data_ptr(), post_row.data_ptr(), tables["ph_off"], tables["ph_terms"],
                tables["ph_driver"], d_ptf_off.data_ptr(), NP, tables["max_terms"], longest, slop,
                alive_bits.data_ptr() if alive_bits is not None else None, ptf.data_ptr(), rows.data_ptr(),
                tables["q_ph_off"], tables["q_ph"], B if bitmaps else 0, tables["max_phrases"],
                maps.data_ptr() if maps is not None and maps.numel() else None, self._stream()), "mmrag_phrase_match")
        return {"known": known, "drivers": drivers, "ptf_off": ptf_off, "ptf": ptf, "rows": rows[:NP], "bitmaps": maps,
                "tables": tables}

    def topk_phrase_ids(self, q_off: np.ndarray, q_terms: np.ndarray, q_phrases: Sequence[Sequence[Sequence[int]]],
                        k: int, alive_bits: Optional[torch.Tensor] = None, k1: Optional[float] = None,
                        b: Optional[float] = None, slop: int = 0, phrase_mode: str = "require",
                        bitmaps: bool = False):
        """topk_ids with phrases: q_phrases[i] lists query i's phrases as term-id sequences (repeats kept, -1 = unknown
        term).  Equal phrases of the batch are matched once.  Returns (scores, rows, info): info is match_phrases'
        dict plus "phrases" (the distinct id sequences) and "q_phrases" (per query, indices into them)."""
        from .config import settings

        k1 = settings.MMRAG_BM25_K1 if k1 is None else k1
        b = settings.MMRAG_BM25_B if b is None else b
        mode = parse_phrase_mode(phrase_mode)
        B = int(q_off.size) - 1
        if len(q_phrases) != B:
            raise ValueError(f"{len(q_phrases)} phrase lists for {B} queries")
        if not 1 <= k <= _native.MAX_K_DEEP:
            raise ValueError(f"n_results must be in 1..{_native.MAX_K_DEEP} for lexical search")
        q_off = np.ascontiguousarray(q_off, np.int32)
        q_terms = np.ascontiguousarray(q_terms, np.int32)
        if q_terms.size and (q_terms.min() < 0 or q_terms.max() >= self.n_terms):
            raise ValueError("query term id outside the lexicon")
        index_of: Dict[Tuple[int, ...], int] = {}
        per_query: List[List[int]] = []
        for phs in q_phrases:
            mine: List[int] = []
            for ph in phs:
                i = index_of.setdefault(tuple(int(t) for t in ph), len(index_of))
                if i not in mine:
                    mine.append(i)
            per_query.append(mine)
        info = self.match_phrases(list(index_of), slop, alive_bits, per_query, bitmaps)
        t = info["tables"]
        term_off, post_row, post_tf = self._csr
        dq_off = torch.from_numpy(q_off).to(self.device)
        dq_terms = torch.from_numpy(np.concatenate([q_terms, np.zeros(1, np.int32)])).to(self.device)
        L = _native.lib()
        need = int(L.mmrag_bm25_phrase_topk_workspace_bytes(B, self.n, k))
        if self._phrase_ws is None or self._phrase_ws.numel() < need:
            self._phrase_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        out_s = torch.empty((B, k), dtype=torch.float32, device=self.device)
        out_r = torch.empty((B, k), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _native._check(L.mmrag_bm25_phrase_topk(
                term_off.data_ptr(), post_row.data_ptr(), post_tf.data_ptr(), self._dl.data_ptr(), self._df.data_ptr(),
                self.n_terms, self.n, dq_off.data_ptr(), dq_terms.data_ptr(), B, t["q_ph_off"], t["q_ph"], t["ph_off"],
                t["ph_terms"], t["ph_driver"], t["ptf_off"].data_ptr(), info["ptf"].data_ptr(), t["n_phrases"],
                t["max_terms"], t["max_phrases"], 1 if mode == "require" else 0, self.n_live, self.sum_dl, float(k1),
                float(b), k, alive_bits.data_ptr() if alive_bits is not None else None, out_s.data_ptr(),
                out_r.data_ptr(), self._phrase_ws.data_ptr(), self._phrase_ws.numel(), self._stream()),
                "mmrag_bm25_phrase_topk")
        info["phrases"] = list(index_of)
        info["q_phrases"] = per_query
        return out_s, out_r, info

    def topk_phrases(self, query_texts: Sequence[str], k: int, alive_bits: Optional[torch.Tensor] = None,
                     k1: Optional[float] = None, b: Optional[float] = None, fuzzy=None, slop: int = 0,
                     phrase_mode: str = "require", bitmaps: bool = False):
        """topk under `phrases` (see topk): (scores, rows, corrections or None, report, info).  report[i] lists query
        i's phrases as {"text", "terms", "known", "rows"}; info is None when no query of the batch has a phrase (the
        call is then topk's, and the positions plane is not touched), else topk_phrase_ids' dict."""
        slop, mode = parse_slop(slop), parse_phrase_mode(phrase_mode)
        parsed = self.parse_phrases(query_texts)
        loose = [t for t, _ in parsed]
        corrections = None
        if parse_fuzzy(fuzzy) is not None:     # quoting means "exactly this": only the loose terms are rewritten
            q_off, q_terms, corrections = self.analyze_queries_fuzzy(loose, fuzzy)
        else:
            q_off, q_terms = self.analyze_queries(loose)
        if not any(phs for _, phs in parsed):
            scores, rows = self.topk_ids(q_off, q_terms, k, alive_bits, k1, b)
            return scores, rows, corrections, [[] for _ in parsed], None
        self.enable_positions()
        scores, rows, info = self.topk_phrase_ids(q_off, q_terms, [[ids for _, _, ids in phs] for _, phs in parsed], k,
                                                  alive_bits, k1, b, slop, mode, bitmaps)
        held = info["rows"].cpu().numpy()
        report = [[{"text": seg, "terms": list(terms), "known": bool(info["known"][i]), "rows": int(held[i])}
                   for (seg, terms, _), i in zip(phs, mine)] for (_, phs), mine in zip(parsed, info["q_phrases"])]
        return scores, rows, corrections, report, info


def rows_dot(q: torch.Tensor, corpus: torch.Tensor, d: int, qi: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """out[i] = <q[qi[i]], corpus[rows[i]]> over the first d columns, float32 (mmrag_rows_dot)"""
    _native._dev_check(q, corpus, qi, rows)
    qi = qi.to(torch.int32).contiguous()
    rows = rows.to(torch.int64).contiguous()
    out = torch.empty(rows.numel(), dtype=torch.float32, device=corpus.device)
    with torch.cuda.device(corpus.device):
        _native._check(_native.lib().mmrag_rows_dot(q.data_ptr(), corpus.data_ptr(), corpus.shape[1],
                                                    _native._TORCH2DT[corpus.dtype], d, qi.data_ptr(), rows.data_ptr(),
                                                    rows.numel(), out.data_ptr(), _native._stream_ptr(corpus.device)),
                       "mmrag_rows_dot")
    return out


def bm25_workspace_bytes(B: int, n: int, k: int) -> int:
    return int(_native.lib().mmrag_bm25_topk_workspace_bytes(B, n, k))


def csr_build_workspace_bytes(n: int, n_terms: int) -> int:
    return int(_native.lib().mmrag_lexical_csr_build_workspace_bytes(n, n_terms))


def fuzzy_limits() -> Dict[str, int]:
    """csrc/fuzzy.hip's tile sizes (mmrag_internal_fuzzy_limits; tests put their seams on them)"""
    v = [c_int(0) for _ in range(5)]
    _native._check(_native.lib().mmrag_internal_fuzzy_limits(*[byref(x) for x in v]), "mmrag_internal_fuzzy_limits")
    return dict(zip(("term_tile", "pattern_tile", "max_len", "max_expansions", "stage_cps"), (int(x.value) for x in v)))


def phrase_limits() -> Dict[str, int]:
    """csrc/phrase.hip's partition sizes (mmrag_internal_phrase_limits; tests put their seams on them)"""
    v = [c_int(0) for _ in range(4)]
    _native._check(_native.lib().mmrag_internal_phrase_limits(*[byref(x) for x in v]), "mmrag_internal_phrase_limits")
    return dict(zip(("match_block", "lane_starts", "wave_lanes", "score_rows"), (int(x.value) for x in v)))


def bm25_phrase_workspace_bytes(B: int, n: int, k: int) -> int:
    return int(_native.lib().mmrag_bm25_phrase_topk_workspace_bytes(B, n, k))


def lexical_limits() -> Dict[str, int]:
    """csrc/lexical.hip's path thresholds (mmrag_internal_lexical_limits; tests restate them and compare)"""
    v = [c_int(0) for _ in range(5)]
    _native._check(_native.lib().mmrag_internal_lexical_limits(*[byref(x) for x in v]), "mmrag_internal_lexical_limits")
    return dict(zip(("score_rows", "score_terms", "sort_lds", "sort_grid", "scan_terms"), (int(x.value) for x in v)))


def declare(lib):
    """ctypes signatures of the lexical entry points (called from _native._declare)"""
    lib.mmrag_lexicon_create.restype = c_void_p
    lib.mmrag_lexicon_create.argtypes = []
    lib.mmrag_lexicon_destroy.restype = None
    lib.mmrag_lexicon_destroy.argtypes = [c_void_p]
    lib.mmrag_lexicon_size.restype = c_int64
    lib.mmrag_lexicon_size.argtypes = [c_void_p]
    lib.mmrag_lexicon_analyze_batch.restype = c_int
    lib.mmrag_lexicon_analyze_batch.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                                c_void_p, c_void_p, c_int64, c_int]
    lib.mmrag_lexical_df_update.restype = c_int
    lib.mmrag_lexical_df_update.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]
    lib.mmrag_lexical_csr_build_workspace_bytes.restype = c_size_t
    lib.mmrag_lexical_csr_build_workspace_bytes.argtypes = [c_int64, c_int]
    lib.mmrag_lexical_csr_build.restype = c_int
    lib.mmrag_lexical_csr_build.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mmrag_bm25_topk_workspace_bytes.restype = c_size_t
    lib.mmrag_bm25_topk_workspace_bytes.argtypes = [c_int, c_int64, c_int]
    lib.mmrag_bm25_topk.restype = c_int
    lib.mmrag_bm25_topk.argtypes = [c_void_p] * 5 + [c_int, c_int64, c_void_p, c_void_p, c_int, c_int64, c_int64,
                                                     c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                     c_size_t, c_void_p]
    lib.mmrag_lexicon_export.restype = c_int
    lib.mmrag_lexicon_export.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int64]
    lib.mmrag_lexicon_analyze_terms.restype = c_int
    lib.mmrag_lexicon_analyze_terms.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_int64, c_int64, c_void_p, c_int]
    lib.mmrag_fuzzy_terms_workspace_bytes.restype = c_size_t
    lib.mmrag_fuzzy_terms_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.mmrag_fuzzy_terms.restype = c_int
    lib.mmrag_fuzzy_terms.argtypes = [c_void_p] * 3 + [c_int] + [c_void_p] * 3 + [c_int, c_int, c_void_p, c_void_p,
                                                                                  c_void_p, c_size_t, c_void_p]
    lib.mmrag_internal_fuzzy_limits.restype = c_int
    lib.mmrag_internal_fuzzy_limits.argtypes = [c_void_p] * 5
    # test-only export (not in include/mmrag.h): the sizes at which the kernels change path
    lib.mmrag_internal_lexical_limits.restype = c_int
    lib.mmrag_internal_lexical_limits.argtypes = [c_void_p] * 5
    lib.mmrag_internal_phrase_limits.restype = c_int
    lib.mmrag_internal_phrase_limits.argtypes = [c_void_p] * 4
    lib.mmrag_lexicon_analyze_positions.restype = c_int
    lib.mmrag_lexicon_analyze_positions.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int]
    lib.mmrag_phrase_match.restype = c_int
    lib.mmrag_phrase_match.argtypes = [c_void_p] * 4 + [c_int64] + [c_void_p] * 6 + [c_int, c_int, c_int64, c_int] + \
        [c_void_p] * 5 + [c_int, c_int, c_void_p, c_void_p]
    lib.mmrag_bm25_phrase_topk_workspace_bytes.restype = c_size_t
    lib.mmrag_bm25_phrase_topk_workspace_bytes.argtypes = [c_int, c_int64, c_int]
    lib.mmrag_bm25_phrase_topk.restype = c_int
    lib.mmrag_bm25_phrase_topk.argtypes = [c_void_p] * 5 + [c_int, c_int64, c_void_p, c_void_p, c_int] + \
        [c_void_p] * 7 + [c_int] * 4 + [c_int64, c_int64, c_float, c_float, c_int] + [c_void_p] * 4 + \
        [c_size_t, c_void_p]
    lib.mmrag_rows_dot.restype = c_int
    lib.mmrag_rows_dot.argtypes = [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p,
                                   c_void_p]
