"""Extractive summaries and answers without a language model: split a text into sentences, embed them, and keep a
non-redundant set of the most CENTRAL sentences under a length budget -- LexRank centrality with MMR selection, all of
it after the encoder in one kernel launch (csrc/summarize.hip, include/mmrag.h mmrag_summary_select; DESIGN.md section
3.1w).  Biased toward a question's embedding the same kernel gives a query-focused answer that quotes its sources.

  split_sentences / split_lines   text -> character spans (host, deterministic, no language tables)
  DeviceSummarizer                spans -> one encode_device call -> one summary_select launch -> one copy back
  ExtractiveSummarizer            the summariser stage of the pipeline (PassthroughSummarizer's contract) on top of it

Opt-in (MMRAG_SUMMARIZER=extractive, POST /query "extractive_answer"): the defaults are ingest.py's stand-ins.
"""
from __future__ import annotations

import re
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

from .config import settings
from .ingest import fallback_summary

Span = Tuple[int, int]

# A sentence ends at a run of . ? ! or the ellipsis character that is followed by whitespace or the end of the text,
# and at a blank line.  Nothing else: abbreviations are NOT special-cased ("e.g. this" is cut after "e.g."), numbers
# like 3.14 and dotted names are safe because no whitespace follows their dot.  One exception, which names no language
# either: a run right after a word of digits only that begins the span or a line ("1. first item") is an enumerator,
# not an end ("in 1999. Then" is one).  Single line breaks do not end a sentence: a list without punctuation is one
# span.
_SENTENCE_END = re.compile(r"[.?!…]+(?=\s|$)|\n[ \t\r\f\v]*\n")


def _is_enumerator(text: str, lo: int, at: int) -> bool:
    """text[lo:at] ends in a word of digits only that begins the span or a line"""
    first = at
    while first > lo and text[first - 1].isdigit():
        first -= 1
    if first == at:
        return False
    while first > lo and text[first - 1] in " \t":
        first -= 1
    return first == lo or text[first - 1] in "\r\n"


def _stripped(text: str, lo: int, hi: int) -> Optional[Span]:
    while lo < hi and text[lo].isspace():
        lo += 1
    while hi > lo and text[hi - 1].isspace():
        hi -= 1
    return (lo, hi) if hi > lo else None


def _cut_long(text: str, span: Span, max_chars: Optional[int]) -> List[Span]:
    """`span` in pieces of at most max_chars characters, each cut at the last whitespace before the limit (at the limit
    itself when the piece has none)"""
    lo, hi = span
    if max_chars is None or max_chars < 1 or hi - lo <= max_chars:
        return [span]
    out: List[Span] = []
    while hi - lo > max_chars:
        cut = next((at for at in range(lo + max_chars, lo, -1) if text[at].isspace()), lo + max_chars)
        piece = _stripped(text, lo, cut)
        if piece:
            out.append(piece)
        rest = _stripped(text, cut, hi)
        if rest is None:
            return out
        lo = rest[0]
    out.append((lo, hi))
    return out


def split_sentences(text: str, max_chars: Optional[int] = None) -> List[Span]:
    """The sentences of `text` as (start, end) character spans: stripped, non-empty, in order, not overlapping.  With
    `max_chars`, a longer span is cut at the last whitespace before the limit so that every span fits it."""
    spans: List[Span] = []
    lo = 0
    for m in _SENTENCE_END.finditer(text or ""):
        end = m.start() if m.group().startswith("\n") else m.end()
        if end == m.end() and _is_enumerator(text, lo, m.start()):
            continue
        piece = _stripped(text, lo, end)
        if piece:
            spans.extend(_cut_long(text, piece, max_chars))
        lo = m.end()
    piece = _stripped(text or "", lo, len(text or ""))
    if piece:
        spans.extend(_cut_long(text, piece, max_chars))
    return spans


def split_lines(text: str, max_chars: Optional[int] = None) -> List[Span]:
    """The non-empty lines of `text` as spans (a table's rows are its sentences), cut like split_sentences'"""
    spans: List[Span] = []
    lo = 0
    for line in (text or "").splitlines(keepends=True):
        piece = _stripped(text, lo, lo + len(line))
        if piece:
            spans.extend(_cut_long(text, piece, max_chars))
        lo += len(line)
    return spans


def summary_parameters() -> Dict[str, Any]:
    """the kernel's parameters from the settings, checked (the C entry refuses them too, with less to go on)"""
    t, alpha = float(settings.MMRAG_SUMMARY_EDGE_THRESHOLD), float(settings.MMRAG_SUMMARY_ALPHA)
    iters, lam = int(settings.MMRAG_SUMMARY_ITERATIONS), float(settings.MMRAG_SUMMARY_LAMBDA)
    if not t >= 0.0 or not 0.0 < alpha <= 1.0 or not 0 <= iters <= 64 or not 0.0 <= lam <= 1.0:
        raise ValueError("MMRAG_SUMMARY_EDGE_THRESHOLD must be >= 0, MMRAG_SUMMARY_ALPHA in (0, 1], "
                         f"MMRAG_SUMMARY_ITERATIONS in 0..64, MMRAG_SUMMARY_LAMBDA in [0, 1] (got {t}, {alpha}, {iters}, "
                         f"{lam})")
    return {"edge_threshold": t, "alpha": alpha, "iterations": iters, "lam": lam}


class DeviceSummarizer:
    """Sentence selection on the device for an engine with `encode_device` (engines.HipEngine).  A call makes ONE
    encode_device call over all sentences (sorted by length, so a packed batch wastes little), casts the rows to
    `dtype` (the collection's; float16 for an FP8 one) into one padded plane, launches summary_select once and copies
    the picks back once."""

    def __init__(self, engine, dtype=None):
        import torch

        self.engine = engine
        if dtype is None:
            dtype = settings.index_dtype()
        self.dtype = torch.float16 if dtype == torch.float8_e4m3fn else dtype

    # ---- the device part: units of sentences -> picks
    def select(self, units: Sequence[Sequence[str]], budgets: Sequence[int], k: int,
               questions: Optional[Sequence[Optional[str]]] = None) -> List[Dict[str, Any]]:
        """One entry per unit (1..MAX_SUMMARY_SENTENCES sentences each; cost = len + 1): {"picks": positions in pick
        order, "rel": the centrality of every sentence, "used": the cost spent}.  questions[u] (None: none) biases
        unit u toward that text's embedding."""
        import numpy as np
        import torch

        from . import _native

        most = _native.MAX_SUMMARY_SENTENCES
        if not units or any(not 1 <= len(u) <= most for u in units):
            raise ValueError(f"a unit holds 1..{most} sentences")
        flat = [s for u in units for s in u]
        lens = [len(u) for u in units]
        asked = [] if questions is None else sorted({q for q in questions if q is not None})
        texts = flat + asked
        order = sorted(range(len(texts)), key=lambda i: len(texts[i]))
        emb = self.engine.encode_device([texts[i] for i in order])           # [len(texts), dim] float32, on the device
        dev, dim = emb.device, int(emb.shape[1])
        ld = _native.padded_dim(dim, self.dtype)
        plane = torch.zeros((len(texts), ld), dtype=self.dtype, device=dev)
        where = torch.from_numpy(np.asarray(order, np.int64)).to(dev)
        plane[where, :dim] = emb.to(self.dtype)
        rows, bias = plane[: len(flat)], (plane[len(flat):] if asked else None)
        n_units = len(units)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        parts = [starts, lens, list(budgets), [len(s) + 1 for s in flat]]
        if asked:
            parts.append([-1 if q is None else asked.index(q) for q in questions])
        table = _native._pinned_to_device(torch.from_numpy(np.concatenate(parts).astype(np.int32)), dev)
        at = [0, n_units, 2 * n_units, 3 * n_units, 3 * n_units + len(flat)]
        k = max(1, min(int(k), most, max(lens)))
        pos, val, rel, used = _native.summary_select(
            rows, dim, table[at[0]: at[1]], table[at[1]: at[2]], table[at[3]: at[4]], table[at[2]: at[3]], k,
            bias_rows=bias, unit_bias=table[at[4]:] if asked else None, **summary_parameters())
        back = torch.cat([pos.reshape(-1), used, rel.view(torch.int32)]).cpu().numpy()       # the one copy back
        pos_h = back[: n_units * k].reshape(n_units, k)
        used_h = back[n_units * k: n_units * k + n_units]
        rel_h = back[n_units * k + n_units:].view(np.float32)
        out = []
        for u, (lo, n) in enumerate(zip(starts, lens)):
            out.append({"picks": [int(p) for p in pos_h[u] if p >= 0], "rel": [float(r) for r in rel_h[lo: lo + n]],
                        "used": int(used_h[u])})
        return out

    # ---- summaries
    def summarize(self, texts: Sequence[str], max_length: int = 300, questions: Optional[Sequence[Optional[str]]] = None,
                  by_lines: bool = False) -> List[Dict[str, Any]]:
        """Per text {"summary", "spans": [(start, end) ...], "scores": [rel ...]}: the picked sentences in document
        order joined by one space, at most max_length characters.  A text no longer than max_length is its own summary
        (fallback_summary's string, no launch); a text of more than MAX_SUMMARY_SENTENCES sentences is cut into
        consecutive sections that share the budget in proportion to their characters; when nothing fits, the summary
        is fallback_summary's.  `by_lines`: lines instead of sentences (tables)."""
        from . import _native

        most = _native.MAX_SUMMARY_SENTENCES
        max_length = int(max_length)
        if max_length < 1:
            raise ValueError("max_length must be positive")
        if questions is not None and len(questions) != len(texts):
            raise ValueError(f"{len(questions)} questions for {len(texts)} texts")
        split = split_lines if by_lines else split_sentences
        out: List[Optional[Dict[str, Any]]] = [None] * len(texts)
        units, budgets, asked, owner = [], [], [], []       # owner: (text, its spans of this section)
        for t, text in enumerate(texts):
            text = text or ""
            whole = _stripped(text, 0, len(text))
            if whole is None or whole[1] - whole[0] <= max_length:
                out[t] = {"summary": fallback_summary(text, max_length), "spans": [whole] if whole else [],
                          "scores": [1.0] if whole else []}
                continue
            spans = split(text, max_length)
            sections = [spans[lo: lo + most] for lo in range(0, len(spans), most)]
            chars = [sum(b - a + 1 for a, b in sec) for sec in sections]
            for sec, c in zip(sections, chars):
                units.append([text[a:b] for a, b in sec])
                budgets.append((max_length + 1) * c // sum(chars))
                asked.append(None if questions is None else questions[t])
                owner.append((t, sec))
        if units:
            found = self.select(units, budgets, most, asked if any(q is not None for q in asked) else None)
            for (t, sec), got in zip(owner, found):
                entry = out[t] or {"summary": "", "spans": [], "scores": []}
                for p in sorted(got["picks"]):
                    entry["spans"].append(sec[p])
                    entry["scores"].append(got["rel"][p])
                out[t] = entry
            for t in {t for t, _ in owner}:
                text, entry = texts[t], out[t]
                if entry["spans"]:
                    entry["summary"] = " ".join(text[a:b] for a, b in entry["spans"])
                else:
                    entry["summary"] = fallback_summary(text, max_length)
        return out

    # ---- answers
    def answer(self, question: str, passages: Sequence[str], max_chars: int = 600,
               top_sentences: int = 8) -> Dict[str, Any]:
        """A query-focused extract of `passages` (in rank order): one unit of their sentences, at most
        MAX_SUMMARY_SENTENCES (later ones are dropped; "considered" says how many took part), biased by the encoded
        question.  {"answer", "quotes": [{"passage", "start", "end", "text", "score"} ...] ordered by (passage,
        start), "considered"}."""
        from . import _native

        most = _native.MAX_SUMMARY_SENTENCES
        max_chars = int(max_chars)
        if max_chars < 1 or not 1 <= int(top_sentences) <= most:
            raise ValueError(f"max_chars must be positive, top_sentences in 1..{most}")
        where = [(i, a, b) for i, text in enumerate(passages) for a, b in split_sentences(text or "", max_chars)][:most]
        if not where:
            return {"answer": "", "quotes": [], "considered": 0}
        got = self.select([[passages[i][a:b] for i, a, b in where]], [max_chars + 1], int(top_sentences), [question])[0]
        quotes = [{"passage": where[p][0], "start": where[p][1], "end": where[p][2],
                   "text": passages[where[p][0]][where[p][1]: where[p][2]], "score": got["rel"][p]}
                  for p in sorted(got["picks"])]
        return {"answer": " ".join(q["text"] for q in quotes), "quotes": quotes, "considered": len(where)}


class ExtractiveSummarizer:
    """The summariser stage (PassthroughSummarizer's contract: the same ids and keys) with extractive summaries: text
    chunks by their sentences, tables by their lines, images unchanged.  `embedder`: an object with
    `summarize_texts(texts, max_length, ...)` (EmbeddingManager), or a callable that returns one -- the pipeline
    creates its embedder after its summariser, so it is resolved at the first document."""

    def __init__(self, embedder: Any):
        self._embedder = embedder
        self.stats = {"total_summaries": 0}

    def _resolve(self):
        if not hasattr(self._embedder, "summarize_texts") and callable(self._embedder):
            self._embedder = self._embedder()
        return self._embedder

    async def summarize_parsed_document(self, parsed_result: Dict[str, Any], max_length: int = 300,
                                        show_progress: bool = True) -> List[Dict[str, Any]]:
        embedder = self._resolve()
        chunks = parsed_result.get("text_chunks", [])
        tables = parsed_result.get("tables", [])
        text_sums = await embedder.summarize_texts([c["content"] for c in chunks], max_length) if chunks else []
        table_sums = (await embedder.summarize_texts([t.get("content", "") for t in tables], max_length, by_lines=True)
                      if tables else [])
        out: List[Dict[str, Any]] = []
        for idx, (chunk, got) in enumerate(zip(chunks, text_sums)):
            out.append({"id": f"text_{idx}", "summary": got["summary"], "raw": chunk["content"], "type": "text",
                        "metadata": chunk.get("metadata", {})})
        for table, got in zip(tables, table_sums):
            out.append({"id": table.get("id", "table_0"), "summary": got["summary"], "raw": table.get("content", ""),
                        "type": "table"})
        for image in parsed_result.get("images", []):
            out.append({"id": image.get("id", "image_0"),
                        "summary": image.get("description") or f"Image: {image.get('id', 'image_0')}",
                        "raw": image.get("base64", ""), "path": image.get("path", ""), "type": "image"})
        self.stats["total_summaries"] += len(out)
        return out

    async def get_stats(self) -> Dict[str, Any]:
        return {"total_summaries": self.stats["total_summaries"], "cache": {"hit_rate": 0}}


def make_summarizer(get_embedder: Callable[[], Any]):
    """the summariser MMRAG_SUMMARIZER names, None for "fallback" (the caller keeps its default)"""
    return ExtractiveSummarizer(get_embedder) if settings.summarizer() == "extractive" else None
