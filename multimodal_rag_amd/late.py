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

    def plan(self, queries: Sequence[str], docs: Sequence[str], pairs: Sequence[Tuple[int, int]]):
        """The host half of score_pairs: tokenise the distinct texts that some pair uses and lay out one encoder batch.
        Returns a dict: ids [B, W] / lens [B] (queries first, then passages), the six tables of mmrag_maxsim_scores
        relative to the packed token rows (q_start, q_len, d_start, d_len, pair_q, pair_d; [CLS] and the final [SEP]
        trimmed through start / len), and q_ids / d_ids, the scored token ids of each sequence."""
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
            pair_d.append(d_slot.setdefault(dt, len(d_slot)))
        q_texts, d_texts = list(q_slot), list(d_slot)
        q_max, d_max = self.max_query_tokens + 2, self.max_doc_tokens + 2
        q_ids, q_lens = self._tokenize(q_texts, q_max)
        d_ids, d_lens = self._tokenize(d_texts, d_max)
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

    def _token(self, token_id: int) -> Any:
        if self._id2tok is None:
            return int(token_id)
        return self._id2tok.get(int(token_id), int(token_id))

    # ------------------------------------------------------------------ scoring -------------
    def _run(self, queries, docs, pairs, want_best: bool):
        """(scores [P] float32, best_sim [P, 128] float32 | None, best_idx [P, 128] int32 | None, plan): one tokenise
        of the distinct texts, ONE encoder forward over queries and passages together, ONE MaxSim launch, one copy back"""
        import torch

        plan = self.plan(queries, docs, pairs)
        tokens, _ = self.encoder.encode_tokens(plan["ids"], plan["lens"], self.projection)
        dim = int(self.projection.shape[0]) if self.projection is not None else int(self.encoder.cfg.hidden)
        sums, best_sim, best_idx = _native.maxsim_scores(
            tokens, tokens, dim, plan["q_start"], plan["q_len"], plan["d_start"], plan["d_len"], plan["pair_q"],
            plan["pair_d"], want_best=want_best)
        P = len(plan["pair_q"])
        q_len = plan["q_len"][plan["pair_q"]].astype(np.float32)
        if not want_best:
            return sums.cpu().numpy() / q_len, None, None, plan
        # one copy back: the three outputs side by side as raw 32-bit words
        W = _native.MAX_LATE_QUERY_TOKENS
        packed = torch.cat([sums.view(torch.int32).reshape(P, 1), best_sim.view(torch.int32), best_idx],
                           dim=1).cpu().numpy()
        scores = packed[:, 0].copy().view(np.float32) / q_len
        sims = np.ascontiguousarray(packed[:, 1: 1 + W]).view(np.float32)
        return scores, sims, np.ascontiguousarray(packed[:, 1 + W:]), plan

    def score_pairs(self, queries: List[str], docs: List[str], pairs: List[Tuple[int, int]], explain: bool = False):
        """MaxSim score of every pair (i, j) = (queries[i], docs[j]): float32 [len(pairs)], out_sum / q_len -- the mean
        over the query's tokens of each token's best cosine against the passage's tokens, so it reads like a cosine.
        `explain`: returns (scores, matches) with, per pair, [(query_token, doc_token, sim)] in query-token order:
        token strings from the tokenizer's `vocab` where it has one, ids otherwise."""
        if not explain:
            return self._run(queries, docs, pairs, False)[0]
        scores, records = self.explain_pairs(queries, docs, pairs)
        return scores, [[(m["query_token"], m["doc_token"], m["similarity"]) for m in rec] for rec in records]

    def explain_pairs(self, queries: List[str], docs: List[str], pairs: List[Tuple[int, int]]):
        """(scores, records): per pair one dict per query token -- query_token, doc_token (as score_pairs names them),
        doc_index (the matched token's 0-based position among the passage's scored tokens) and similarity"""
        scores, sims, idx, plan = self._run(queries, docs, pairs, True)
        records = []
        for p in range(len(scores)):
            qi, di = plan["q_ids"][plan["pair_q"][p]], plan["d_ids"][plan["pair_d"][p]]
            records.append([{"query_token": self._token(qi[i]), "doc_token": self._token(di[int(idx[p, i])]),
                             "doc_index": int(idx[p, i]), "similarity": float(sims[p, i])} for i in range(len(qi))])
        return scores, records
