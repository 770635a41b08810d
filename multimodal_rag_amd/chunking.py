"""Semantic chunking: cut a text where its topic changes instead of every CHUNK_SIZE characters.  The text is split
into sentences, the sentences are embedded, and one kernel launch finds the partition into chunks of greatest total
within-chunk similarity above a threshold tau, under the size limits -- exactly, by dynamic programming over the
similarities at distance < 64 (csrc/chunk.hip, include/mmrag.h mmrag_chunk_boundaries).

  semantic_costs            sentence spans -> the characters each sentence adds to a chunk
  DeviceChunker             texts -> one encode_device call -> one chunk_boundaries launch -> one copy back -> chunks
  SemanticDocumentParser    the parser stage of the pipeline (TextDocumentParser's contract) on top of it

Opt-in (MMRAG_CHUNKER=semantic, POST /chunk): the default is ingest.basic_chunk_text.
"""
from __future__ import annotations

import uuid
from typing import Any, Callable, Dict, List, Optional, Sequence

from .config import settings
from .summarize import Span, split_sentences


def semantic_costs(text: str, spans: Sequence[Span]) -> List[int]:
    """What each sentence adds to a chunk's length: the distance to the next sentence's start (the sentence and the
    gap after it); the last sentence costs its own length.  The slice text[start of a chunk's first sentence : end of
    its last] is then never longer than the chunk's cost sum."""
    starts = [a for a, _ in spans]
    return [nxt - a for a, nxt in zip(starts, starts[1:])] + ([spans[-1][1] - spans[-1][0]] if spans else [])


class DeviceChunker:
    """Topic-boundary segmentation on the device for an engine with `encode_device` (engines.HipEngine), the twin of
    summarize.DeviceSummarizer.  A call makes ONE encode_device call over all sentences of all documents (sorted by
    length, so a packed batch wastes little), casts the rows to `dtype` (the collection's; float16 for an FP8 one)
    into one padded plane, launches chunk_boundaries once and copies the answer back once."""

    def __init__(self, engine, dtype=None):
        import torch

        self.engine = engine
        if dtype is None:
            dtype = settings.index_dtype()
        self.dtype = torch.float16 if dtype == torch.float8_e4m3fn else dtype

    # ---- the device part: documents of sentences -> chunks as runs of sentences
    def segment(self, units: Sequence[Sequence[str]], costs: Sequence[Sequence[int]], max_cost: int,
                max_sentences: int, threshold: Optional[float] = None, auto_scale: float = 0.5,
                penalty: float = 0.0) -> List[Dict[str, Any]]:
        """One entry per document (any number >= 1 of sentences, costs[u][i] >= 1 each): {"runs": [(first sentence,
        one past the last, gain) ...] in order, "tau": the threshold used, "score": the total gain}.  `threshold`
        None: tau is auto_scale times the document's mean adjacent similarity."""
        import numpy as np
        import torch

        from . import _native

        if not units or any(len(u) < 1 or len(u) != len(c) for u, c in zip(units, costs)) or len(units) != len(costs):
            raise ValueError("a document holds at least one sentence, with one cost per sentence")
        flat = [s for u in units for s in u]
        lens = [len(u) for u in units]
        order = sorted(range(len(flat)), key=lambda i: len(flat[i]))
        emb = self.engine.encode_device([flat[i] for i in order])            # [len(flat), dim] float32, on the device
        dev, dim = emb.device, int(emb.shape[1])
        ld = _native.padded_dim(dim, self.dtype)
        plane = torch.zeros((len(flat), ld), dtype=self.dtype, device=dev)
        where = torch.from_numpy(np.asarray(order, np.int64)).to(dev)
        plane[where, :dim] = emb.to(self.dtype)
        n_docs = len(units)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        parts = [starts, lens, [int(c) for cs in costs for c in cs]]
        table = _native._pinned_to_device(torch.from_numpy(np.concatenate(parts).astype(np.int32)), dev)
        prev, best, tau, score = _native.chunk_boundaries(
            plane, dim, table[:n_docs], table[n_docs: 2 * n_docs], table[2 * n_docs:], int(max_cost),
            int(max_sentences), threshold=0.0 if threshold is None else float(threshold),
            auto_scale=float(auto_scale) if threshold is None else 0.0, penalty=float(penalty))
        back = torch.cat([prev, best.view(torch.int32), tau.view(torch.int32), score.view(torch.int32)]).cpu().numpy()
        n_rows = len(flat)                                                   # (the one copy back)
        prev_h, best_h = back[:n_rows], back[n_rows: 2 * n_rows].view(np.float32)
        tau_h, score_h = (back[2 * n_rows + i * n_docs: 2 * n_rows + (i + 1) * n_docs].view(np.float32) for i in (0, 1))
        out = []
        for u, (lo, n) in enumerate(zip(starts, lens)):
            runs, b = [], n
            while b > 0:        # O(chunks): from the end, each chunk names where it starts
                a = int(prev_h[lo + b - 1])
                if not 0 <= a < b:
                    raise RuntimeError(f"chunk_boundaries: document {u} has no valid segmentation (prev[{b}] = {a})")
                gain = float(best_h[lo + b - 1]) - (float(best_h[lo + a - 1]) if a else 0.0)
                runs.append((a, b, gain))
                b = a
            out.append({"runs": runs[::-1], "tau": float(tau_h[u]), "score": float(score_h[u])})
        return out

    # ---- texts -> chunks
    def chunk_texts(self, texts: Sequence[str], chunk_size: Optional[int] = None,
                    overlap: Optional[int] = None) -> List[List[Dict[str, Any]]]:
        """Per text its chunks, in order: {"content", "start", "end", "sentences", "gain"} with content ==
        text[start:end] (stripped), chunks that do not overlap and together hold every sentence of
        split_sentences(text, chunk_size), none longer than chunk_size characters.  A text of one sentence, or of
        none, takes no launch.  `overlap` (default: CHUNK_OVERLAP under MMRAG_CHUNK_SEMANTIC_OVERLAP=1, else 0) > 0:
        each chunk after the first is prefixed with the trailing whole sentences of its predecessor that fit in
        `overlap` characters and in what the chunk leaves of chunk_size; `start` / `end` keep naming the chunk's own
        span, the prefix begins at `overlap_start` and content == text[overlap_start:end]."""
        params = settings.chunk_parameters()
        chunk_size = int(settings.CHUNK_SIZE if chunk_size is None else chunk_size)
        configured = params.pop("overlap")
        overlap = int(configured if overlap is None else overlap)
        if chunk_size < 1 or not 0 <= overlap < chunk_size:
            raise ValueError(f"chunk_size must be positive and 0 <= overlap < chunk_size (got {chunk_size}, {overlap})")
        all_spans = [split_sentences(text or "", max_chars=chunk_size) for text in texts]
        many = [t for t, spans in enumerate(all_spans) if len(spans) > 1]
        found: Dict[int, List] = {t: [(0, len(all_spans[t]), -params["penalty"])] for t in range(len(texts))
                                  if len(all_spans[t]) == 1}
        if many:
            got = self.segment([[texts[t][a:b] for a, b in all_spans[t]] for t in many],
                               [semantic_costs(texts[t], all_spans[t]) for t in many], chunk_size - overlap, **params)
            found.update({t: g["runs"] for t, g in zip(many, got)})
        out: List[List[Dict[str, Any]]] = []
        for t, (text, spans) in enumerate(zip(texts, all_spans)):
            chunks: List[Dict[str, Any]] = []
            for first, past, gain in found.get(t, []):
                start, end = spans[first][0], spans[past - 1][1]
                entry = {"content": text[start:end], "start": start, "end": end, "sentences": past - first,
                         "gain": gain}
                if overlap and chunks:
                    room = min(overlap, chunk_size - (end - start))
                    at = first
                    while at > found[t][len(chunks) - 1][0] and start - spans[at - 1][0] <= room:
                        at -= 1
                    if at < first:
                        entry["overlap_start"] = spans[at][0]
                        entry["content"] = text[spans[at][0]: end]
                chunks.append(entry)
            out.append(chunks)
        return out


class SemanticDocumentParser:
    """The parser stage (ingest.TextDocumentParser's contract: the same keys, ids and refusal text) with semantic
    chunks.  Each chunk's metadata additionally carries `char_start` / `char_end` (content == text[char_start:
    char_end]), `sentence_count` and "chunker": "semantic".  `embedder`: an object with `chunk_texts(texts,
    chunk_size)` (EmbeddingManager), or a callable that returns one -- the pipeline creates its embedder after its
    parser, so it is resolved at the first document."""

    def __init__(self, embedder: Any):
        self._embedder = embedder
        self.chunk_size = settings.CHUNK_SIZE

    def _resolve(self):
        if not hasattr(self._embedder, "chunk_texts") and callable(self._embedder):
            self._embedder = self._embedder()
        return self._embedder

    async def parse_document(self, content: bytes, filename: str, content_type: Optional[str] = None,
                             doc_id: Optional[str] = None) -> Dict[str, Any]:
        name = (filename or "").lower()
        if not name.endswith((".txt", ".md", ".markdown", ".text")) and not (content_type or "").startswith("text/"):
            raise ValueError(f"Unsupported file type for this build: {filename} (text/markdown only)")
        try:
            text = content.decode("utf-8")
        except UnicodeDecodeError:
            text = content.decode("latin-1", errors="ignore")
        chunks = []
        for chunk_id, got in enumerate((await self._resolve().chunk_texts([text], self.chunk_size))[0]):
            unique_id = str(uuid.uuid4())[:8]
            chunks.append({
                "chunk_id": f"{doc_id}_chunk_{chunk_id}_{unique_id}",
                "content": got["content"],
                "metadata": {"char_count": len(got["content"]), "filename": filename, "doc_type": "text",
                             "doc_id": doc_id, "char_start": got.get("overlap_start", got["start"]),
                             "char_end": got["end"], "sentence_count": got["sentences"], "chunker": "semantic"},
            })
        return {"doc_type": "text", "text_chunks": chunks, "tables": [], "images": [], "document_structure": {}}


def make_parser(get_embedder: Callable[[], Any]):
    """the parser MMRAG_CHUNKER names, None for "basic" (the caller keeps its default)"""
    return SemanticDocumentParser(get_embedder) if settings.chunker() == "semantic" else None
