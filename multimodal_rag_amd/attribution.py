"""Answer citations: which source stands behind which sentence of an answer, and whether a sentence has any source
behind it.  The answer is split into sentences (the claims), the sources' passages into sentences (the evidence); all
of them are embedded in one call and one kernel launch finds, for every claim and source, the best-supporting sentence
of that source and ranks the sources per claim (csrc/attribute.hip, include/mmrag.h mmrag_attribute; DESIGN.md section
3.1y).

This is similarity-based attribution with the bi-encoder that is already on the device: a citation says "this source
says something very close to this sentence".  It is NOT entailment: a source that says the opposite in the same words
scores high.

  DeviceAttributor    texts -> one encode_device call -> one attribute launch -> one copy back

Opt-in (POST /query "citations", POST /attribute, MMRAG_CITATIONS=1 for the flag's default).
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

from .config import settings
from .summarize import split_sentences


def citation_parameters(threshold: Optional[float] = None, max_citations: Optional[int] = None) -> Dict[str, Any]:
    """a call's threshold and citation count, the settings' where None, checked"""
    base = settings.citation_parameters()
    t = base["threshold"] if threshold is None else threshold
    most = base["max_citations"] if max_citations is None else max_citations
    if (isinstance(t, bool) or not isinstance(t, (int, float)) or not -1.0 < float(t) <= 1.0
            or isinstance(most, bool) or not isinstance(most, int) or not 1 <= most <= 8):
        raise ValueError(f"threshold must be a cosine in (-1, 1], max_citations an integer in 1..8 (got {t!r}, "
                         f"{most!r})")
    return {"threshold": float(t), "max_citations": most}


class DeviceAttributor:
    """Attribution on the device for an engine with `encode_device` (engines.HipEngine).  A call makes ONE
    encode_device call over the distinct sentences of all units (sorted by length, so a packed batch wastes little; a
    string that occurs twice is encoded once), casts the rows to `dtype` (the collection's; float16 for an FP8 one)
    into one padded plane, uploads one pinned table, launches mmrag_attribute once and copies the result back once."""

    def __init__(self, engine, dtype=None):
        import torch

        self.engine = engine
        if dtype is None:
            dtype = settings.index_dtype()
        self.dtype = torch.float16 if dtype == torch.float8_e4m3fn else dtype

    # ---- the device part: sections of claims against evidence sets -> ranked sources per claim
    def rank(self, sections: Sequence[Tuple[Sequence[str], int]], evidence: Sequence[Tuple[Sequence[str], Sequence[int]]],
             n_sources: int, m: int) -> List[List[List[Tuple[int, int, float]]]]:
        """sections[u] = (1..MAX_CLAIMS claim sentences, the index of its evidence set); evidence[e] = (1..MAX_EVIDENCE
        sentences, the source ordinal of each).  Per section and claim the at most `m` best sources as (source, position
        in the evidence set, score), best first."""
        import numpy as np
        import torch

        from . import _native

        if not sections or any(not 1 <= len(c) <= _native.MAX_CLAIMS for c, _ in sections):
            raise ValueError(f"a section holds 1..{_native.MAX_CLAIMS} claims")
        if any(not 1 <= len(s) <= _native.MAX_EVIDENCE or len(s) != len(o) for s, o in evidence):
            raise ValueError(f"an evidence set holds 1..{_native.MAX_EVIDENCE} sentences, one source ordinal each")
        # the plane: every evidence set once, then every section's claims
        placed = [s for sents, _ in evidence for s in sents] + [s for claims, _ in sections for s in claims]
        ev_lens = [len(sents) for sents, _ in evidence]
        ev_starts = np.concatenate([[0], np.cumsum(ev_lens)]).astype(np.int64)
        n_ev = int(ev_starts[-1])
        claim_lens = [len(claims) for claims, _ in sections]
        claim_starts = n_ev + np.concatenate([[0], np.cumsum(claim_lens)[:-1]])
        distinct = sorted(set(placed), key=lambda s: (len(s), s))
        slot = {s: at for at, s in enumerate(distinct)}
        emb = self.engine.encode_device(distinct)            # [len(distinct), dim] float32, on the device
        dev, dim = emb.device, int(emb.shape[1])
        n_rows, n_units = len(placed), len(sections)
        source_of_row = [o for _, ords in evidence for o in ords] + [-1] * (n_rows - n_ev)
        parts = [claim_starts, claim_lens, [ev_starts[e] for _, e in sections], [ev_lens[e] for _, e in sections],
                 source_of_row, [slot[s] for s in placed]]
        table = _native._pinned_to_device(torch.from_numpy(np.concatenate(parts).astype(np.int32)), dev)
        at = [0, n_units, 2 * n_units, 3 * n_units, 4 * n_units, 4 * n_units + n_rows, 4 * n_units + 2 * n_rows]
        cs, cl, es, el, src_of, gather = (table[lo:hi] for lo, hi in zip(at, at[1:]))
        plane = torch.zeros((n_rows, _native.padded_dim(dim, self.dtype)), dtype=self.dtype, device=dev)
        plane[:, :dim] = emb.to(self.dtype).index_select(0, gather)
        most = max(claim_lens)
        src, ev, score, _ = _native.attribute(plane, dim, cs, cl, es, el, src_of, int(n_sources), int(m), most,
                                              want_support=False)
        back = torch.cat([src.reshape(-1), ev.reshape(-1), score.reshape(-1).view(torch.int32)]).cpu().numpy()
        size = n_units * most * int(m)                       # the one copy back
        src_h, ev_h = (back[i * size: (i + 1) * size].reshape(n_units, most, int(m)) for i in (0, 1))
        score_h = back[2 * size:].view(np.float32).reshape(n_units, most, int(m))
        if np.isnan(score_h[:, 0, 0]).any():
            raise RuntimeError("mmrag_attribute refused a unit the host built")
        return [[[(int(s), int(j), float(v)) for s, j, v in zip(src_h[u, i], ev_h[u, i], score_h[u, i]) if s >= 0]
                 for i in range(n)] for u, n in enumerate(claim_lens)]

    # ---- answers against passages
    def attribute(self, answers: Sequence[str], passages: Sequence[Sequence[str]],
                  owners: Optional[Sequence[Optional[Sequence[int]]]] = None, n_sources: Optional[int] = None,
                  max_citations: Optional[int] = None, threshold: Optional[float] = None) -> List[Dict[str, Any]]:
        """Per answer (with its own passages, in rank order; owners[a][i]: the source passage i of answer a belongs
        to, default i) {"citations": one entry per sentence of the answer, {"start", "end", "text", "score" (its best
        source's, None without evidence), "supported" (score >= threshold), "sources": the at most `max_citations`
        sources at or above the threshold, best first, {"source", "passage", "start", "end", "text", "score"}: the
        source's best-supporting sentence, in the passage's characters}, "groundedness": the share of the claims'
        characters whose claim is supported, "support": per source the share of the claims' characters whose claim is
        supported with that source as the best one (they add up to groundedness), "considered": {"claims",
        "evidence"}: the sentences that took part}.  An answer of more than MAX_CLAIMS sentences is cut into
        consecutive sections over the same evidence; evidence sentences past MAX_EVIDENCE are dropped.  An empty answer
        or no evidence: no citations, groundedness 0.0 -- and when that holds for every answer, no launch.
        `n_sources`: the length of every "support" list (default: an answer's highest owner + 1)."""
        from . import _native

        par = citation_parameters(threshold, max_citations)
        if len(passages) != len(answers) or (owners is not None and len(owners) != len(answers)):
            raise ValueError(f"{len(answers)} answers need as many passage lists (and owner lists)")
        most_sources = _native.MAX_ATTR_SOURCES
        if n_sources is not None and not 1 <= int(n_sources) <= most_sources:
            raise ValueError(f"n_sources must be in 1..{most_sources} (got {n_sources})")
        sections, evidence, plans = [], [], []
        for a, (answer, texts) in enumerate(zip(answers, passages)):
            answer, texts = answer or "", [t or "" for t in texts]
            own = list(range(len(texts))) if owners is None or owners[a] is None else [int(o) for o in owners[a]]
            if len(own) != len(texts):
                raise ValueError(f"{len(own)} owners for {len(texts)} passages")
            width = (max(own) + 1 if own else 1) if n_sources is None else int(n_sources)
            if own and (min(own) < 0 or max(own) >= width or width > most_sources):
                raise ValueError(f"a passage's owner must be a source ordinal in 0..{min(width, most_sources) - 1}: at "
                                 f"most {most_sources} sources take part (got {min(own)}..{max(own)})")
            claims = split_sentences(answer)
            where = [(p, lo, hi) for p, text in enumerate(texts) for lo, hi in split_sentences(text)]
            where = where[:_native.MAX_EVIDENCE]
            plan = {"answer": answer, "texts": texts, "own": own, "width": width, "claims": claims, "where": where,
                    "first": None}
            if claims and where:
                plan["first"] = len(sections)
                evidence.append(([texts[p][lo:hi] for p, lo, hi in where], [own[p] for p, _, _ in where]))
                for lo in range(0, len(claims), _native.MAX_CLAIMS):
                    sections.append(([answer[s:e] for s, e in claims[lo: lo + _native.MAX_CLAIMS]], len(evidence) - 1))
            plans.append(plan)
        found = []
        if sections:
            found = self.rank(sections, evidence, max(plan["width"] for plan in plans if plan["first"] is not None),
                              par["max_citations"])
        out = []
        for plan in plans:
            if plan["first"] is None:
                out.append({"citations": [], "groundedness": 0.0, "support": [0.0] * plan["width"],
                            "considered": {"claims": 0, "evidence": 0}})
                continue
            n_sections = -(-len(plan["claims"]) // _native.MAX_CLAIMS)
            ranked = [claim for sec in found[plan["first"]: plan["first"] + n_sections] for claim in sec]
            out.append(self._entry(plan, ranked, par["threshold"]))
        return out

    @staticmethod
    def _entry(plan, ranked, threshold: float) -> Dict[str, Any]:
        answer, texts, where = plan["answer"], plan["texts"], plan["where"]
        citations, chars, grounded, by_source = [], 0, 0, [0] * plan["width"]
        for (lo, hi), sources in zip(plan["claims"], ranked):
            best = sources[0][2] if sources else None
            supported = best is not None and best >= threshold
            cited = []
            for source, j, score in sources:
                if score >= threshold:
                    p, a, b = where[j]
                    cited.append({"source": source, "passage": p, "start": a, "end": b, "text": texts[p][a:b],
                                  "score": score})
            citations.append({"start": lo, "end": hi, "text": answer[lo:hi],
                              "score": None if best is None or not math.isfinite(best) else best,
                              "supported": supported, "sources": cited})
            chars += hi - lo
            if supported:
                grounded += hi - lo
                by_source[sources[0][0]] += hi - lo
        return {"citations": citations, "groundedness": grounded / chars, "support": [c / chars for c in by_source],
                "considered": {"claims": len(plan["claims"]), "evidence": len(where)}}
