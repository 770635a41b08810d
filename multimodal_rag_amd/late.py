"""Late-interaction re-ranking (ColBERT's MaxSim) with the bi-encoder that is already resident on the GPU.

The encoder's per-token outputs are kept instead of pooled (mmrag_encoder_forward_tokens); a (query, passage) pair
scores the mean, over the query's tokens, of each token's best cosine against the passage's tokens
(mmrag_maxsim_scores, csrc/maxsim.hip).  The arg-max also says WHY a passage was a hit: which of its tokens each query
token matched, and how well.

This module tokenises, trims the special tokens and builds the sequence and pair tables; both device steps are HIP
kernels in libmmrag.so.  There is no eager / CPU scoring here.  Loading ColBERT checkpoints is not built: `projection`
takes the [out_dim, hidden] tensor of such a checkpoint's `linear` when the caller has one.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .config import settings


class LateInteractionScorer:
    """MaxSim scores of (query, passage) pairs from ONE encoder forward and ONE MaxSim launch.

    `encoder`: a DeviceEncoder in fp16 mode (anything with `encode_tokens(ids2d, lens, proj)` and a `cfg` with
    `max_seq_length` / `max_pos`).  `tokenizer`: one of tokenizer.py's BERT tokenizers (rows are [CLS] ... [SEP]).
    `projection`: optional [out_dim, hidden] tensor applied to the final hidden states before the normalisation."""

    def __init__(self, encoder, tokenizer, projection=None):
        if tokenizer is None:
            raise ValueError("late interaction needs a tokenizer")
        self.encoder = encoder
        self.tokenizer = tokenizer
        self.projection = projection
        vocab = getattr(tokenizer, "vocab", None)
        self._id2tok: Optional[Dict[int, str]] = {i: t for t, i in vocab.items()} if isinstance(vocab, dict) else None

    # ------------------------------------------------------------------ limits --------------
    @property
    def encoder_max_length(self) -> int:
        cfg = self.encoder.cfg
        return int(min(cfg.max_seq_length, cfg.max_pos))

    @property
    def max_query_tokens(self) -> int:
        """query tokens scored, [CLS] / [SEP] not counted"""
        return min(_native.MAX_LATE_QUERY_TOKENS, self.encoder_max_length - 2)

    @property
    def max_doc_tokens(self) -> int:
        """passage tokens scored, [CLS] / [SEP] not counted: min(MMRAG_LATE_MAX_DOC_TOKENS, the encoder's, 512)"""
        cap = int(settings.MMRAG_LATE_MAX_DOC_TOKENS) or self.encoder_max_length
        return max(1, min(cap, self.encoder_max_length - 2, _native.MAX_LATE_DOC_TOKENS))

    # ------------------------------------------------------------------ host side -----------
    def _tokenize(self, texts: List[str], max_length: int) -> Tuple[np.ndarray, np.ndarray]:
        """(ids [n, W] int32, lens [n]) of `texts`, rows [CLS] ... [SEP] of at most max_length ids"""
        if hasattr(self.tokenizer, "encode_batch_arrays"):
            ids, lens = self.tokenizer.encode_batch_arrays(texts, max_length)
            return np.asarray(ids, np.int32), np.asarray(lens, np.int32)
        rows = [self.tokenizer.encode(t, max_length) for t in texts]
        ids = np.zeros((len(rows), max(max_length, 1)), np.int32)
        for i, r in enumerate(rows):
            ids[i, : len(r)] = r
        return ids, np.array([len(r) for r in rows], np.int32)

    def plan(self, queries: Sequence[str], docs: Sequence[str], pairs: Sequence[Tuple[int, int]],
             stored: Optional[Sequence[bool]] = None):
        """The host half of score_pairs: tokenise the distinct texts that some pair uses and lay out one encoder batch.
        Returns a dict: ids [B, W] / lens [B] (queries first, then passages), the six tables of mmrag_maxsim_scores
        relative to the packed token rows (q_start, q_len, d_start, d_len, pair_q, pair_d; [CLS] and the final [SEP]
        trimmed through start / len), and q_ids / d_ids, the scored token ids of each sequence.
        `stored` (one flag per passage; the token store): a flagged passage is neither tokenised nor encoded -- its
        pairs get pair_d = -1 and the caller scores them from the stored rows."""
        pairs = [(int(a), int(b)) for a, b in pairs]
        if not pairs:
            raise ValueError("score_pairs: no pairs")
        for a, b in pairs:
            if not 0 <= a < len(queries) or not 0 <= b < len(docs):
                raise ValueError(f"score_pairs: pair ({a}, {b}) outside {len(queries)} queries x {len(docs)} passages")
        # distinct texts, in order of first use: a query or passage shared between pairs is encoded once
        q_slot: Dict[str, int] = {}
        d_slot: Dict[str, int] = {}
        pair_q, pair_d = [], []
        for a, b in pairs:
            qt = queries[a] if queries[a] is not None else ""
            dt = docs[b] if docs[b] is not None else ""
            pair_q.append(q_slot.setdefault(qt, len(q_slot)))
            pair_d.append(-1 if stored is not None and stored[b] else d_slot.setdefault(dt, len(d_slot)))
        q_texts, d_texts = list(q_slot), list(d_slot)
        q_max, d_max = self.max_query_tokens + 2, self.max_doc_tokens + 2
        q_ids, q_lens = self._tokenize(q_texts, q_max)
        if d_texts:
            d_ids, d_lens = self._tokenize(d_texts, d_max)
        else:       # every passage is stored: the batch is the queries alone
            d_ids, d_lens = np.zeros((0, 1), np.int32), np.zeros(0, np.int32)
        q_lens, d_lens = np.minimum(q_lens, q_max), np.minimum(d_lens, d_max)
        W = max(q_ids.shape[1], d_ids.shape[1])
        ids = np.zeros((len(q_texts) + len(d_texts), W), np.int32)
        ids[: len(q_texts), : q_ids.shape[1]] = q_ids
        ids[len(q_texts):, : d_ids.shape[1]] = d_ids
        lens = np.concatenate([q_lens, d_lens]).astype(np.int32)
        cu = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=cu[1:])
        # a sequence is [CLS] t_1 .. t_m [SEP]: score t_1 .. t_m.  A text without a single token keeps its [CLS] row, so
        # that every sequence has a token to score
        inner = np.maximum(lens - 2, 0)
        start = np.where(inner > 0, cu[:-1] + 1, cu[:-1])
        length = np.where(inner > 0, inner, 1)
        nq = len(q_texts)
        seq_ids = [ids[s, (1 if inner[s] > 0 else 0): (1 if inner[s] > 0 else 0) + int(length[s])].tolist()
                   for s in range(len(lens))]
        return {"ids": ids, "lens": lens, "q_start": start[:nq].astype(np.int32), "q_len": length[:nq].astype(np.int32),
                "d_start": start[nq:].astype(np.int32), "d_len": length[nq:].astype(np.int32),
                "pair_q": np.asarray(pair_q, np.int32), "pair_d": np.asarray(pair_d, np.int32),
                "q_ids": seq_ids[:nq], "d_ids": seq_ids[nq:]}

    # A forward of at most this many tokens takes the encoder's single-query GEMM kernels (csrc/encoder.hip
    # takes_small16_kernel: M <= 64), which split K over the waves of a workgroup: the same sequence then gets other
    # low bits than in any larger batch, where every tile kernel adds a row's K products in one order.
    SMALL_FORWARD_TOKENS = 64

    def _encode_stable(self, ids: np.ndarray, lens: np.ndarray):
        """encode_tokens whose rows' bits depend on each sequence alone: a forward that would hold at most
        SMALL_FORWARD_TOKENS tokens is filled up past them with filler sequences (copies of the first id), whose rows
        are dropped.  What the token store keeps and what is scored against it go through here, so a stored row equals
        the row any re-encoding forward of more than SMALL_FORWARD_TOKENS tokens computes.  Returns (tokens, cu) of the
        real sequences."""
        lens = np.asarray(lens, np.int32)
        total, n = int(lens.sum()), len(lens)
        if total > self.SMALL_FORWARD_TOKENS:
            return self.encoder.encode_tokens(ids, lens, self.projection)
        fill, most = [], self.encoder_max_length
        short = self.SMALL_FORWARD_TOKENS + 1 - total
        while short > 0:
            fill.append(min(short, most))
            short -= fill[-1]
        W = max(ids.shape[1], max(fill))
        padded = np.full((n + len(fill), W), int(ids[0, 0]), np.int32)
        padded[:n, : ids.shape[1]] = ids
        tokens, cu = self.encoder.encode_tokens(padded, np.concatenate([lens, np.asarray(fill, np.int32)]),
                                                self.projection)
        return tokens[:total], cu[: n + 1]

    def trimmed(self, lens: np.ndarray):
        """(first scored token, scored tokens) of sequences [CLS] t_1 .. t_m [SEP] of `lens` ids, relative to each
        sequence's first id -- plan()'s rule: t_1 .. t_m, or the [CLS] row alone for a text without a single token"""
        inner = np.maximum(np.asarray(lens, np.int64) - 2, 0)
        return np.where(inner > 0, 1, 0), np.where(inner > 0, inner, 1)

    def encode_documents(self, texts: Sequence[Optional[str]], batch: int = 64):
        """What the token store keeps of `texts`: (token rows [sum(lens), dim] device fp16, lens [n], token ids per
        text) -- each text tokenised and truncated as plan() does a passage, encoded `batch` texts per forward, [CLS]
        and the final [SEP] trimmed as plan() trims them.  A token row's bits depend on its own sequence alone, so these
        are the rows a re-rank would compute again (_encode_stable says for which forwards that holds)."""
        import torch

        texts = [t if t is not None else "" for t in texts]
        parts, lens_out, ids_out = [], [], []
        for lo in range(0, len(texts), batch):
            ids, lens = self._tokenize(texts[lo: lo + batch], self.max_doc_tokens + 2)
            lens = np.minimum(lens, self.max_doc_tokens + 2).astype(np.int32)
            tokens, _ = self._encode_stable(ids, lens)
            cu = np.zeros(len(lens) + 1, np.int64)
            np.cumsum(lens, out=cu[1:])
            first, count = self.trimmed(lens)
            pick = np.concatenate([np.arange(cu[s] + first[s], cu[s] + first[s] + count[s]) for s in range(len(lens))])
            parts.append(tokens.index_select(0, torch.from_numpy(pick).to(tokens.device)))
            lens_out.extend(int(c) for c in count)
            ids_out.extend(ids[s, first[s]: first[s] + count[s]].tolist() for s in range(len(lens)))
        dim = int(self.projection.shape[0]) if self.projection is not None else int(self.encoder.cfg.hidden)
        rows = torch.cat(parts) if parts else torch.zeros((0, dim), dtype=torch.float16)
        return rows, np.asarray(lens_out, np.int32), ids_out

    def encode_questions(self, texts: Sequence[str]):
        """(token rows device fp16, q_start, q_len, token ids per question) of questions alone: ONE forward, trimmed as
        plan() trims a query"""
        ids, lens = self._tokenize([t if t is not None else "" for t in texts], self.max_query_tokens + 2)
        lens = np.minimum(lens, self.max_query_tokens + 2).astype(np.int32)
        tokens, _ = self._encode_stable(ids, lens)
        cu = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=cu[1:])
        first, count = self.trimmed(lens)
        q_ids = [ids[s, first[s]: first[s] + count[s]].tolist() for s in range(len(lens))]
        return tokens, (cu[:-1] + first).astype(np.int32), count.astype(np.int32), q_ids

    def _launch(self, q_tok, d_tok, dim, tables, want_best: bool, f8: bool, window_blocks: int):
        """One MaxSim launch; its outputs side by side as raw 32-bit words, a device int32 tensor [P, width]: the sums,
        then best_sim | best_idx (`want_best`) -- or, with `window_blocks`, the windows launch in place of the scores
        launch (mmrag_maxsim_windows): the sums, then the 32 window sums | (start, first, last)."""
        import torch

        if window_blocks:
            fn = _native.maxsim_windows_f8 if f8 else _native.maxsim_windows
            sums, win, best = fn(q_tok, d_tok, dim, *tables, window_blocks)
            cols = [sums.view(torch.int32).reshape(-1, 1), win.view(torch.int32), best]
        else:
            fn = _native.maxsim_scores_f8 if f8 else _native.maxsim_scores
            sums, best_sim, best_idx = fn(q_tok, d_tok, dim, *tables, want_best=want_best)
            cols = [sums.view(torch.int32).reshape(-1, 1)]
            if want_best:
                cols += [best_sim.view(torch.int32), best_idx]
        return cols[0] if len(cols) == 1 else torch.cat(cols, dim=1)

    @staticmethod
    def _width(want_best: bool, window_blocks: int) -> int:
        """columns of _launch's tensor"""
        if window_blocks:
            return 1 + _native.MAX_LATE_WINDOWS + 3
        return 1 + 2 * _native.MAX_LATE_QUERY_TOKENS if want_best else 1

    def _run_stored(self, queries, docs, pairs, spans, plane, want_best: bool, plane_f8: bool = False,
                    window_blocks: int = 0):
        """_run with a token store: `spans[b]` is (first plane row, length, token ids) of passage b's stored rows, or
        None.  ONE forward over the queries and the passages that are not stored, then one MaxSim launch for the
        stored passages' pairs (against `plane`) and one for the others.  Returns _run's tuple; the plan's d_ids /
        pair_d are rewritten so that pair p's passage ids are plan["d_ids"][plan["pair_d"][p]] as in _run.
        An FP8 store (`plane_f8`: `plane` holds E4M3 code rows): the encoded rows -- the questions' AND those of the passages that
        had to be encoded -- are quantised once and both launches are mmrag_maxsim_scores_f8, so every candidate of the
        call is scored in the plane's arithmetic and a passage scores the same from the plane as re-encoded."""
        stored = [s is not None for s in spans]
        plan = self.plan(queries, docs, pairs, stored=stored)
        tokens, _ = self._encode_stable(plan["ids"], plan["lens"])
        dim = int(self.projection.shape[0]) if self.projection is not None else int(self.encoder.cfg.hidden)
        P = len(plan["pair_q"])
        if plane_f8:
            tokens = _native.f8_encode_rows(tokens, dim)
        from_store = np.array([stored[int(b)] for _, b in pairs], bool)
        packed = np.zeros((P, self._width(want_best, window_blocks)), np.int32)
        d_ids = list(plan["d_ids"])
        pair_d = plan["pair_d"].copy()
        for mask, d_tok in ((from_store, plane), (~from_store, tokens)):
            at = np.nonzero(mask)[0]
            if at.size == 0:
                continue
            if d_tok is plane:
                used = sorted({int(pairs[p][1]) for p in at})
                slot = {b: i for i, b in enumerate(used)}
                d_start = np.array([spans[b][0] for b in used], np.int32)
                d_len = np.array([spans[b][1] for b in used], np.int32)
                pd = np.array([slot[int(pairs[p][1])] for p in at], np.int32)
                for b in used:
                    pair_of = len(d_ids)
                    d_ids.append(list(spans[b][2]) if spans[b][2] is not None else [0] * int(spans[b][1]))
                    pair_d[[p for p in at if int(pairs[p][1]) == b]] = pair_of
            else:
                d_start, d_len, pd = plan["d_start"], plan["d_len"], plan["pair_d"][at]
            out = self._launch(tokens, d_tok, dim, (plan["q_start"], plan["q_len"], d_start, d_len, plan["pair_q"][at],
                                                    pd), want_best, plane_f8, window_blocks)
            packed[at] = out.cpu().numpy()
        plan["d_ids"], plan["pair_d"] = d_ids, pair_d
        if window_blocks:
            plan["d_len_of_pair"] = np.array([spans[int(b)][1] if stored[int(b)] else plan["d_len"][plan["pair_d"][p]]
                                              for p, (_, b) in enumerate(pairs)], np.int32)
        return self._unpack(packed, plan, want_best, window_blocks)

    @staticmethod
    def _unpack(packed: np.ndarray, plan, want_best: bool, window_blocks: int):
        """_run's tuple from the host copy of _launch's columns"""
        W = _native.MAX_LATE_WINDOWS if window_blocks else _native.MAX_LATE_QUERY_TOKENS
        q_len = plan["q_len"][plan["pair_q"]].astype(np.float32)
        scores = packed[:, 0].copy().view(np.float32) / q_len
        if window_blocks:
            plan["sums"] = packed[:, 0].copy().view(np.float32)
        elif not want_best:
            return scores, None, None, plan
        sims = np.ascontiguousarray(packed[:, 1: 1 + W]).view(np.float32)
        return scores, sims, np.ascontiguousarray(packed[:, 1 + W:]), plan

    def _token(self, token_id: int) -> Any:
        if self._id2tok is None:
            return int(token_id)
        return self._id2tok.get(int(token_id), int(token_id))

    # ------------------------------------------------------------------ scoring -------------
    def _run(self, queries, docs, pairs, want_best: bool, spans=None, plane=None, plane_f8: bool = False,
             window_blocks: int = 0):
        """(scores [P] float32, best_sim [P, 128] float32 | None, best_idx [P, 128] int32 | None, plan): one tokenise
        of the distinct texts, ONE encoder forward over queries and passages together, ONE MaxSim launch, one copy back.
        `window_blocks` (best_passages): the windows launch in place of the scores launch -- the tuple is then (scores,
        window sums [P, 32] float32, (start, first, last) [P, 3] int32, plan) and plan["d_len_of_pair"] [P] holds each
        pair's passage length."""
        if spans is not None and (plane_f8 or any(s is not None for s in spans)):     # an FP8 store: always
            return self._run_stored(queries, docs, pairs, spans, plane, want_best, plane_f8, window_blocks)
        plan = self.plan(queries, docs, pairs)
        tokens, _ = self.encoder.encode_tokens(plan["ids"], plan["lens"], self.projection)
        dim = int(self.projection.shape[0]) if self.projection is not None else int(self.encoder.cfg.hidden)
        # one copy back: the outputs side by side as raw 32-bit words
        packed = self._launch(tokens, tokens, dim, (plan["q_start"], plan["q_len"], plan["d_start"], plan["d_len"],
                                                    plan["pair_q"], plan["pair_d"]), want_best, False,
                              window_blocks).cpu().numpy()
        if window_blocks:
            plan["d_len_of_pair"] = plan["d_len"][plan["pair_d"]].astype(np.int32)
        return self._unpack(packed, plan, want_best, window_blocks)

    def score_pairs(self, queries: List[str], docs: List[str], pairs: List[Tuple[int, int]], explain: bool = False,
                    spans=None, plane=None, plane_f8: bool = False):
        """MaxSim score of every pair (i, j) = (queries[i], docs[j]): float32 [len(pairs)], out_sum / q_len -- the mean
        over the query's tokens of each token's best cosine against the passage's tokens, so it reads like a cosine.
        `explain`: returns (scores, matches) with, per pair, [(query_token, doc_token, sim)] in query-token order:
        token strings from the tokenizer's `vocab` where it has one, ids otherwise.
        `spans`, `plane` (the token store): spans[b] = (first row, length, token ids) of passage b's rows in the device
        plane, or None -- such a passage is scored from those rows instead of being encoded again, with the same bits."""
        if not explain:
            return self._run(queries, docs, pairs, False, spans, plane, plane_f8)[0]
        scores, records = self.explain_pairs(queries, docs, pairs, spans, plane, plane_f8)
        return scores, [[(m["query_token"], m["doc_token"], m["similarity"]) for m in rec] for rec in records]

    @staticmethod
    def window_blocks(window_tokens: int) -> int:
        """a window width in tokens as whole blocks: rounded up to a multiple of LATE_WINDOW_TOKENS, clamped to
        16..512 tokens"""
        blocks = -(-int(window_tokens) // _native.LATE_WINDOW_TOKENS)
        return max(1, min(blocks, _native.MAX_LATE_WINDOWS))

    def best_passages(self, queries: List[str], docs: List[str], pairs: List[Tuple[int, int]], window_tokens: int,
                      spans=None, plane=None, plane_f8: bool = False):
        """The best window of each pair's passage by windowed MaxSim (mmrag_maxsim_windows): plan, forward and stored
        spans exactly as score_pairs, with the windows launch in place of the scores launch.  One dict per pair:
          score          out_sum / q_len, the number score_pairs gives
          window_score   the best window's sum / q_len
          sum, window_sum   the two float32 sums themselves
          window_start, window_end   the best window in scored tokens of the passage: whole blocks, the end clipped
          token_start, token_end     the tight span inside it: the blocks that hold some query token's best match
          window_scores  every window's sum / q_len, by start block
          doc_ids        the passage's scored token ids (plan()'s d_ids; a stored passage's are the store's)
        `window_tokens` is rounded up to whole blocks of 16 and clamped to 16..512."""
        w = self.window_blocks(window_tokens)
        scores, win, best, plan = self._run(queries, docs, pairs, False, spans, plane, plane_f8, window_blocks=w)
        block = _native.LATE_WINDOW_TOKENS
        out = []
        for p in range(len(scores)):
            d_len, q_len = int(plan["d_len_of_pair"][p]), float(plan["q_len"][plan["pair_q"][p]])
            start, first, last = (int(v) for v in best[p])
            valid = win[p, : max(-(-d_len // block) - w, 0) + 1]
            out.append({"score": float(scores[p]), "window_score": float(win[p, start] / np.float32(q_len)),
                        "sum": float(plan["sums"][p]), "window_sum": float(win[p, start]),
                        "window_start": block * start, "window_end": min(block * (start + w), d_len),
                        "token_start": block * first, "token_end": min(block * (last + 1), d_len),
                        "window_scores": [float(v / np.float32(q_len)) for v in valid],
                        "doc_ids": plan["d_ids"][plan["pair_d"][p]]})
        return out

    def explain_pairs(self, queries: List[str], docs: List[str], pairs: List[Tuple[int, int]], spans=None, plane=None,
                      plane_f8: bool = False):
        """(scores, records): per pair one dict per query token -- query_token, doc_token (as score_pairs names them),
        doc_index (the matched token's 0-based position among the passage's scored tokens) and similarity"""
        scores, sims, idx, plan = self._run(queries, docs, pairs, True, spans, plane, plane_f8)
        records = []
        for p in range(len(scores)):
            qi, di = plan["q_ids"][plan["pair_q"][p]], plan["d_ids"][plan["pair_d"][p]]
            records.append([{"query_token": self._token(qi[i]), "doc_token": self._token(di[int(idx[p, i])]),
                             "doc_index": int(idx[p, i]), "similarity": float(sims[p, i])} for i in range(len(qi))])
        return scores, records
