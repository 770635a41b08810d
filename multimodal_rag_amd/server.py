"""FastAPI surface of the hot path: POST /upload and POST /query with the reference's request /
response schemas, status codes and messages (app/server/api.py:161-179, :244-413), plus the
maintenance routes that call into the embedder / retriever (:202-241, :416-508).

    uvicorn multimodal_rag_amd.server:app            # needs an MI355X

`create_app()` accepts replacement components so the out-of-scope stages (parser, summariser,
LLM) can be the reference's real ones; defaults are the minimal stand-ins in ingest.py.
"""
from __future__ import annotations

import functools
import logging
import time
import uuid
from contextlib import asynccontextmanager
from datetime import datetime
from typing import Annotated, Any, Dict, List, Literal, Optional, Tuple, Union

from fastapi import FastAPI, HTTPException, Request, status
from pydantic import BaseModel, Field, StrictBool

from .boost import parse_boost
from .config import settings
from .embedder import EmbeddingManager
from .index import DuplicateReportTruncated
from .ingest import ExtractiveAnswerer, PassthroughSummarizer, TextDocumentParser
from .retriever import MultiVectorRetriever
from .chunking import make_parser
from .summarize import make_summarizer

logger = logging.getLogger(__name__)

NO_DOCS_ANSWER = "Không tìm thấy tài liệu liên quan. Vui lòng upload tài liệu hoặc thử câu hỏi khác."  # api.py:342


# the examples of a recommend request: ids of stored items, texts of unwanted topics (16 examples in all at most)
ExampleIds = Annotated[List[Annotated[str, Field(min_length=1, max_length=200)]], Field(min_length=1, max_length=16)]
ExampleTexts = Annotated[List[Annotated[str, Field(min_length=1, max_length=2000)]], Field(min_length=1, max_length=16)]


class QueryRequest(BaseModel):  # api.py:161-164
    query: str = Field(..., min_length=1, max_length=2000)
    top_k: int = Field(5, ge=1, le=20)
    use_multimodal: bool = Field(False)
    # not in the reference: re-score max(top_k, MMRAG_RERANK_CANDIDATES) hits with the cross-encoder of
    # MMRAG_RERANKER_DIR and answer from the best top_k (each source then carries its `rerank_score`)
    rerank: bool = Field(False)
    # with `rerank`: which re-ranker (default MMRAG_RERANK_METHOD).  "cross" is the cross-encoder above; "late" is late
    # interaction with the bi-encoder itself (EmbeddingManager.late_rerank: token-level MaxSim), which needs no second
    # model.  `explain` (late only): each source also carries `matches`, one entry per query token -- the passage token
    # it matched, that token's position and the cosine
    rerank_method: Optional[Literal["cross", "late"]] = None
    explain: bool = Field(False)
    # not in the reference: candidates from dense + BM25 retrieval fused by reciprocal rank (EmbeddingManager
    # .hybrid_query); each source then carries its `hybrid_score`.  With `rerank`, max(top_k, MMRAG_RERANK_CANDIDATES)
    # hybrid hits are re-ranked
    hybrid: bool = Field(False)
    # with `hybrid`: the second leg, "lexical" (BM25, the default) or "sparse" (learned sparse retrieval: each source
    # then carries its `sparse_score` too)
    hybrid_leg: Optional[Literal["lexical", "sparse"]] = None
    # with `hybrid` and the lexical leg: typo tolerance -- true or "auto" (0 / 1 / 2 edits for terms of 1-2 / 3-5 / 6+
    # code points) or 0..2 edits for every term.  A query term no stored chunk holds is replaced by its closest
    # indexed term (csrc/fuzzy.hip) before BM25 scores; the response then carries `corrections`, a list of
    # {"term", "matched", "edits"}.  Unset: the MMRAG_LEXICAL_FUZZY setting
    fuzzy: Optional[Any] = None
    # with `hybrid` and the lexical leg: phrase queries -- a segment of the question between two '"' (or curly quotes)
    # is a phrase of 1..8 terms every returned chunk must hold (csrc/phrase.hip), its terms at most `slop` (0..16) other
    # tokens apart; the response then carries `phrases`, a list of {"text", "terms", "known", "rows"}.  Unset: the
    # MMRAG_LEXICAL_PHRASES / MMRAG_LEXICAL_SLOP settings
    phrases: Optional[bool] = None
    slop: Optional[int] = None
    # not in the reference: hits by learned sparse retrieval alone (EmbeddingManager.sparse_query: the question expanded
    # by the masked-LM of MMRAG_SPARSE_ENCODER_DIR, scored exactly against the stored sparse vectors); each source
    # carries its `sparse_score` and, with `explain`, `matched_terms`: the shared vocabulary strings with their
    # contribution, best first.  Takes `filter` and `doc_ids`; not combined with the other modes or `rerank` yet
    sparse: bool = Field(False)
    # not in the reference: diversified hits (EmbeddingManager.mmr_query: maximal marginal relevance over
    # MMRAG_MMR_CANDIDATES dense hits); each source then carries its `mmr_score`.  `mmr_lambda` (default
    # MMRAG_MMR_LAMBDA): 1 = plain relevance, 0 = pure diversity.  With `rerank`, max(top_k, MMRAG_RERANK_CANDIDATES)
    # diverse hits are re-ranked.  Not combined with `hybrid` yet
    mmr: bool = Field(False)
    mmr_lambda: Optional[float] = Field(None, ge=0.0, le=1.0)
    # not in the reference: hits grouped by document (EmbeddingManager.grouped_query over the `doc_id` metadata).
    # `top_k` then counts DOCUMENTS and `per_document` is the number of hits kept of each; every source carries its
    # `document` and 1-based `document_rank`, sources are in document order.  Not combined with `mmr`, `hybrid` or
    # `rerank` yet
    group_by_document: bool = Field(False)
    per_document: int = Field(1, ge=1, le=16)
    # not in the reference: multi-query retrieval (EmbeddingManager.multi_query).  `variants` are up to 15 further
    # phrasings or sub-questions searched together with `query`; the ranked lists are fused on the device (`fusion`:
    # "rrf" or "max", default MMRAG_FUSE_METHOD) and each source carries its `fused_score` and `matched_queries`
    # (the number of DISTINCT phrasings that returned it: one repeating `query` or an earlier one is searched once).
    # `query` is always list 0 and is the text the generator and the re-ranker see; `variant_weight` is the weight of
    # each further phrasing against 1.0 for `query`.  `expand` asks the application's query expander
    # (create_app(query_expander=...)) for that many phrasings more.  With `rerank`,
    # max(top_k, MMRAG_RERANK_CANDIDATES) fused hits are re-ranked against `query`.  Not combined with `mmr`, `hybrid`
    # or `group_by_document` yet
    variants: Optional[Annotated[List[Annotated[str, Field(min_length=1, max_length=2000)]],
                                 Field(max_length=15)]] = None
    variant_weight: Optional[float] = Field(None, ge=-1000.0, le=1000.0)
    fusion: Optional[Literal["rrf", "max"]] = None
    expand: int = Field(0, ge=0, le=15)
    # not in the reference: answer from these documents only (the `doc_id`s /upload returned; 1 to 64 of them).  A
    # plain or re-ranked query takes EmbeddingManager.scoped_query, where concurrent callers with different documents
    # share one search; `hybrid`, `mmr`, `group_by_document` and `variants` get the same restriction as their filter.
    # Ids no stored document has match nothing: the answer then has no sources
    doc_ids: Optional[Annotated[List[Annotated[str, Field(min_length=1, max_length=200)]],
                                Field(min_length=1, max_length=64)]] = None
    # not in the reference: boosted retrieval (EmbeddingManager.boosted_query): hits are ranked by cosine + a score
    # prior applied inside the scan.  {"recency": -10..10 (weight of 2 ** (-age / half life)), "half_life_days": > 0,
    # "values": {metadata key: {value: -10..10 added to the score}}}, at most 8 keys of 32 values; missing fields and
    # `true` take MMRAG_BOOST_RECENCY / MMRAG_BOOST_HALF_LIFE_DAYS.  Each source then carries its `boost` and final
    # `score`; `relevance_score` stays the cosine.  With `rerank`, max(top_k, MMRAG_RERANK_CANDIDATES) boosted hits are
    # re-ranked.  Not combined with `hybrid`, `mmr`, `group_by_document`, `variants` / `expand` or `doc_ids` yet
    boost: Optional[Union[StrictBool, Dict[str, Any]]] = None
    # not in the reference: recommend retrieval (EmbeddingManager.recommend), "about X, but not Y" and "more like these,
    # less like those".  `like` / `unlike`: ids of stored items (the `doc_id` of a source) used as positive / negative
    # examples next to the question; `not`: texts of unwanted topics, encoded with the question.  A hit scores
    # pos - w * max(neg, 0) inside one exact scan (w: `negative_weight`, default MMRAG_RECOMMEND_NEGATIVE_WEIGHT); each
    # source then carries its `score`, `penalty`, `matched` and `repelled_by`, and `relevance_score` stays the best
    # positive cosine.  At most 16 examples in all.  Not combined with `mmr`, `group_by_document`, `boost`, `variants`
    # / `expand`, `doc_ids` or `hybrid` yet
    like: Optional[ExampleIds] = None
    unlike: Optional[ExampleIds] = None
    not_: Optional[ExampleTexts] = Field(None, alias="not")
    negative_weight: Optional[float] = Field(None, ge=0.0, le=1000.0)
    # not in the reference: a metadata filter in the `where` grammar of the collection ({"type": "table"},
    # {"page": {"$gte": 10, "$lte": 40}}, "$and" / "$or" lists; at most 32 leaves, nested at most 8 deep).  A plain or
    # re-ranked query passes it on as its filter; every other mode gets it AND-ed into its restriction, next to
    # `doc_ids`.  The reserved key "$added_at" (UNIX seconds a row was added) needs device filters
    # (MMRAG_DEVICE_FILTERS)
    filter: Optional[Dict[str, Any]] = None
    # not in the reference: first-stage late-interaction retrieval (EmbeddingManager.late_query): the hits are the
    # stored items of highest MaxSim against the question's tokens, from one scan of the token store -- no pooled-vector
    # search before it.  Each source carries its `late_score` (the mean over the question's tokens of each token's
    # best cosine).  `relevance_score` stays the pooled cosine wherever a pooled search produced the hit; this mode
    # runs none, so here it is the late score too.  Needs the token store (MMRAG_LATE_STORE=1 or
    # EmbeddingManager.enable_late_store()); `doc_ids` and `filter` restrict it, `rerank` re-ranks its hits.  Not
    # combined with `hybrid`, `mmr`, `group_by_document`, `boost`, `variants` / `expand` or `like` / `unlike` / `not`
    # yet
    late: bool = Field(False)
    # not in the reference: answer passages (EmbeddingManager.extract_passages).  Each source also carries `passage`:
    # the part of the hit that answers the question -- the window of `passage_tokens` tokens (default
    # MMRAG_PASSAGE_TOKENS; whole blocks of 16, 16..512) with the highest MaxSim against the question, narrowed to the
    # blocks that hold a match -- as {text, char_start, char_end, score, share}; `share` is the part of the hit's
    # whole late-interaction score the window keeps.  Works with every mode: it reads the final hits.  With `rerank`
    # and the method "late" it comes out of the re-rank call itself.  The generator's context is unchanged
    passages: bool = Field(False)
    passage_tokens: Optional[int] = Field(None, ge=16, le=512)
    # not in the reference: an extractive answer (EmbeddingManager.extract_answer).  `answer` is then a handful of
    # sentences QUOTED from the hits' raw text passages -- central to them, close to the question, none repeating
    # another (sentence centrality with MMR selection, csrc/summarize.hip) -- instead of the generator's text, and every
    # source that was quoted carries `quotes`: [{start, end, text, score}] in the passage's characters.  Works with every
    # mode: it reads the final hits
    extractive_answer: bool = Field(False)
    # not in the reference: the extractive reader (EmbeddingManager.read_answers; needs MMRAG_READER_DIR, a local
    # BertForQuestionAnswering).  The response gains `answers` -- the best answer SPANS over the hits' raw text passages,
    # {text, score, probability, hit, passage, start, end} -- and `answerable` (best span score - lowest null score >
    # MMRAG_READER_NULL_THRESHOLD); every source carries its own `answer_spans`.  The generator call is unchanged.
    # `reader_answer` implies `reader`: `answer` is then the best span's text, or the "nothing found" wording when the
    # hits do not answer the question, and the generator is not called.  Works with the modes `passages` works with
    reader: bool = Field(False)
    reader_answer: bool = Field(False)
    # not in the reference: answer citations (EmbeddingManager.attribute_answer; csrc/attribute.hip).  The response gains
    # `citations` -- one entry per sentence of `answer`: {start, end, text, score, supported, sources: [{source, passage,
    # start, end, text, score}]}, `source` an index into `sources`, the span that source's best-supporting sentence in
    # its raw text passage -- and `groundedness`, the share of the answer's characters in supported sentences; every
    # source carries `cited_by` (the sentences that cite it) and `support`.  Similarity of sentence embeddings, not
    # entailment.  A sentence is supported at a cosine of at least `citation_threshold` (default
    # MMRAG_CITATION_THRESHOLD) and cites at most `max_citations` sources (default MMRAG_CITATION_MAX).  Works with
    # every mode and every way the answer is made.  Unset: the MMRAG_CITATIONS setting
    citations: bool = Field(default_factory=lambda: bool(settings.MMRAG_CITATIONS))
    citation_threshold: Optional[float] = Field(None, gt=-1.0, le=1.0)
    max_citations: Optional[int] = Field(None, ge=1, le=8)


FILTER_MAX_LEAVES, FILTER_MAX_DEPTH = 32, 8


def check_filter(where: Any, depth: int = 1) -> Tuple[int, bool]:
    """(leaves, whether "$added_at" is named) of a request's filter; ValueError for one that is not a dict, an operator
    match_where does not know (its message), more than FILTER_MAX_LEAVES leaves or nesting beyond FILTER_MAX_DEPTH"""
    from .index import _CMP

    if not isinstance(where, dict):
        raise ValueError("a filter must be an object")
    if depth > FILTER_MAX_DEPTH:
        raise ValueError(f"a filter nests at most {FILTER_MAX_DEPTH} deep")
    leaves, timed = 0, False
    for key, cond in where.items():
        if key in ("$and", "$or"):
            if not isinstance(cond, list):
                raise ValueError(f"{key} takes a list of filters")
            for sub in cond:
                n, t = check_filter(sub, depth + 1)
                leaves, timed = leaves + n, timed or t
            continue
        timed = timed or key == "$added_at"
        if isinstance(cond, dict):
            for op in cond:
                if op not in _CMP:
                    raise ValueError(f"unsupported where operator {op!r}")
            leaves += len(cond)
        else:
            leaves += 1
    if depth == 1 and leaves > FILTER_MAX_LEAVES:
        raise ValueError(f"a filter holds at most {FILTER_MAX_LEAVES} leaves (this one: {leaves})")
    return leaves, timed


class RecommendRequest(BaseModel):
    """POST /recommend, the "more like this" button: stored items as examples, no question and no generator call"""
    like: ExampleIds = Field(...)
    unlike: Optional[ExampleIds] = None
    not_: Optional[ExampleTexts] = Field(None, alias="not")
    top_k: int = Field(5, ge=1, le=20)
    filter: Optional[Dict[str, Any]] = None
    negative_weight: Optional[float] = Field(None, ge=0.0, le=1000.0)


class RelatedRequest(BaseModel):
    """POST /related: which stored documents cover these passages; no question and no generator call"""
    texts: List[str] = Field(..., min_length=1, max_length=8192)
    top_k: int = Field(5, ge=1, le=100)
    threshold: Optional[float] = Field(None, gt=0.0, le=1.0)
    filter: Optional[Dict[str, Any]] = None


class ExploreRequest(BaseModel):
    """POST /explore: everything at or above a score -- how many stored items, how they spread over metadata values,
    and the best of them; no generator call"""
    query: str = Field(..., min_length=1, max_length=2000)
    min_score: float = Field(..., gt=-1.0, le=1.0)      # a cosine
    limit: int = Field(20, ge=0, le=100)                 # hits returned; 0 = the numbers alone
    facets: List[Annotated[str, Field(min_length=1, max_length=200)]] = Field(default_factory=list, max_length=4)
    filter: Optional[Dict[str, Any]] = None
    doc_ids: Optional[Annotated[List[Annotated[str, Field(min_length=1, max_length=200)]],
                                Field(min_length=1, max_length=64)]] = None


class AttributeRequest(BaseModel):
    """POST /attribute: citations for an answer that was generated elsewhere, against `passages` (each its own source)
    or the raw text passages of stored `ids` (each id a source); no retrieval and no generator call"""
    answer: str = Field(..., max_length=100_000)
    passages: Optional[Annotated[List[Annotated[str, Field(max_length=1_000_000)]], Field(max_length=64)]] = None
    ids: Optional[Annotated[List[Annotated[str, Field(min_length=1, max_length=200)]],
                            Field(min_length=1, max_length=64)]] = None
    citation_threshold: Optional[float] = Field(None, gt=-1.0, le=1.0)
    max_citations: Optional[int] = Field(None, ge=1, le=8)


class ChunkRequest(BaseModel):
    """POST /chunk: how a text would be cut under MMRAG_CHUNKER=semantic; nothing is stored"""
    text: str = Field(..., max_length=4_000_000)
    chunk_size: Optional[int] = Field(None, ge=1, le=100_000)


# request flag -> what it needs of the embedder (method, `supports_*` check) and the 400 detail when that is missing;
# /query checks them in this order
MODE_NEEDS = (
    ("group_by_document", "grouped_query", "supports_grouping",
     "Grouping by document is not available with this embedder: it needs a single-GPU collection "
     "(EmbeddingManager.grouped_query)"),
    ("hybrid", "hybrid_query", "supports_hybrid",
     "Hybrid retrieval is not available with this embedder: it needs a single-GPU collection with lexical search "
     "(EmbeddingManager.hybrid_query); a float8_e4m3fn collection also needs its re-scoring plane "
     "(MMRAG_F8_RESCORE=float16)"),
    ("mmr", "mmr_query", "supports_mmr",
     "MMR retrieval is not available with this embedder: it needs a single-GPU collection "
     "(EmbeddingManager.mmr_query); a float8_e4m3fn collection also needs its re-scoring plane "
     "(MMRAG_F8_RESCORE=float16)"),
)


# learned sparse retrieval (`sparse`, `hybrid_leg`: "sparse"): the same
SPARSE_NEEDS = ("sparse_query", "supports_sparse",
                "Learned sparse retrieval is not available with this embedder: it needs a single-GPU collection, the "
                "fp16 BERT engine and a sparse encoder (MMRAG_SPARSE_ENCODER_DIR, EmbeddingManager.enable_sparse)")


# multi-query retrieval (`variants` / `expand`): the same
MULTI_NEEDS = ("multi_query", "supports_multi_query",
               "Multi-query retrieval is not available with this embedder: it needs a single-GPU collection "
               "(EmbeddingManager.multi_query)")


# boosted retrieval (`boost`): the same
BOOST_NEEDS = ("boosted_query", "supports_boost",
               "Boosted retrieval is not available with this embedder: it needs a single-GPU collection "
               "(EmbeddingManager.boosted_query); a float8_e4m3fn collection also needs its re-scoring plane "
               "(MMRAG_F8_RESCORE=float16)")


# recommend retrieval (`like` / `unlike` / `not`, POST /recommend): the same
RECOMMEND_NEEDS = ("recommend", "supports_recommend",
                   "Recommend retrieval is not available with this embedder: it needs a single-GPU collection "
                   "(EmbeddingManager.recommend); a float8_e4m3fn collection also needs its re-scoring plane "
                   "(MMRAG_F8_RESCORE=float16)")
RECOMMEND_COLUMNS = (("scores", "score"), ("penalties", "penalty"), ("matched", "matched"),
                     ("repelled_by", "repelled_by"))


# `rerank` with the method "late": the same
LATE_NEEDS = ("late_rerank", "has_late_reranker",
              "Late-interaction re-ranking is not available with this embedder: it needs a single BERT-family HIP "
              "engine in fp16 mode with a tokenizer (EmbeddingManager.late_rerank)")


# `passages`: the same
PASSAGES_NEEDS = ("extract_passages", "supports_passages",
                  "Answer passages are not available with this embedder: they need a single BERT-family HIP engine in "
                  "fp16 mode with a tokenizer and a collection that is not sharded (EmbeddingManager.extract_passages)")
PASSAGE_KEYS = ("text", "char_start", "char_end", "score", "share")


# `extractive_answer`: the same
EXTRACT_NEEDS = ("extract_answer", "supports_summaries",
                 "Extractive answers are not available with this embedder: they need an engine that leaves its "
                 "embeddings on the device (the single-GPU HIP engine; EmbeddingManager.extract_answer)")
QUOTE_KEYS = ("start", "end", "text", "score")


# `reader` / `reader_answer`: the answers a response lists, the keys of an answer and of a source's span, and the
# answer when the hits hold none
READER_ANSWERS = 3
ANSWER_KEYS = ("text", "score", "probability", "hit", "passage", "start", "end")
SPAN_KEYS = ("text", "passage", "start", "end", "score", "probability")
NO_ANSWER_FOUND = NO_DOCS_ANSWER


# first-stage late retrieval (`late`): the same
LATE_QUERY_NEEDS = ("late_query", "supports_late_query",
                    "Late retrieval is not available with this embedder: it needs a single BERT-family HIP engine in "
                    "fp16 mode, a single-GPU collection and the token store (MMRAG_LATE_STORE=1 or "
                    "EmbeddingManager.enable_late_store())")


# /duplicates: what it needs of the embedder and the 400 detail when that is missing (worded like MODE_NEEDS)
DEDUP_NEEDS = ("find_duplicates", "supports_dedup",
               "Near-duplicate detection is not available with this embedder: it needs a single-GPU collection "
               "(EmbeddingManager.find_duplicates); a float8_e4m3fn collection also needs its re-scoring plane "
               "(MMRAG_F8_RESCORE=float16)")


# /topics: the same for topic clustering
TOPICS_NEEDS = ("cluster_topics", "supports_clustering",
                "Topic clustering is not available with this embedder: it needs a single-GPU collection "
                "(EmbeddingManager.cluster_topics); a float8_e4m3fn collection also needs its re-scoring plane "
                "(MMRAG_F8_RESCORE=float16)")


# /topics?terms=n and /documents/{doc_id}/keywords: the same for significant terms
TERMS_NEEDS = ("document_keywords", "supports_terms",
               "Significant terms are not available with this embedder: they need a single-GPU collection with stored "
               "documents (EmbeddingManager.document_keywords)")
MAX_TOPIC_TERMS = 32  # the most terms a topic of /topics carries
LABEL_TERMS = 3       # the terms a topic's `label` joins
MAX_KEYWORDS = 100    # the most keywords /documents/{doc_id}/keywords returns


# /documents/{doc_id}/related and /related: the same for related-document retrieval
RELATED_NEEDS = ("related_documents", "supports_related",
                 "Related-document retrieval is not available with this embedder: it needs a single-GPU collection "
                 "(EmbeddingManager.related_documents); a float8_e4m3fn collection also needs its re-scoring plane "
                 "(MMRAG_F8_RESCORE=float16)")
RELATED_PAIRS = 5     # the best pairs of a related document that a response carries


# /explore: the same for range retrieval
RANGE_NEEDS = ("range_query", "supports_range",
               "Range retrieval is not available with this embedder: it needs a single-GPU collection "
               "(EmbeddingManager.range_query); a float8_e4m3fn collection also needs its re-scoring plane "
               "(MMRAG_F8_RESCORE=float16)")


# /chunk: the same for semantic chunking
CHUNK_NEEDS = ("chunk_texts", "supports_chunking",
               "Semantic chunking is not available with this embedder: it needs an engine that leaves its embeddings "
               "on the device (the single-GPU HIP engine; EmbeddingManager.chunk_texts)")


# `citations` and /attribute: the same for answer citations
CITATION_NEEDS = ("attribute_answer", "supports_citations",
                  "Answer citations are not available with this embedder: they need an engine that leaves its "
                  "embeddings on the device (the single-GPU HIP engine; EmbeddingManager.attribute_answer)")


class QueryResponse(BaseModel):  # api.py:167-170
    answer: str
    sources: List[dict]
    processing_time: float
    # `reader` only (the route leaves unset fields out of the response)
    answers: Optional[List[dict]] = None
    answerable: Optional[bool] = None
    # `fuzzy` only
    corrections: Optional[List[dict]] = None
    # `phrases` only
    phrases: Optional[List[dict]] = None
    # `citations` only
    citations: Optional[List[dict]] = None
    groundedness: Optional[float] = None


class UploadResponse(BaseModel):  # api.py:173-179
    doc_id: str
    filename: str
    doc_type: str
    chunks_processed: dict
    message: str
    processing_time: float


def parse_multipart_file(content_type: str, body: bytes, field: str = "file"):
    """Minimal multipart/form-data reader for the single `file` part /upload takes (api.py:245
    `file: UploadFile = File(...)`); python-multipart is not available in this image, so the
    stdlib MIME parser does the work.  Returns (filename, part content type, bytes) or None."""
    from email.parser import BytesParser
    from email.policy import HTTP

    if not content_type or "multipart/form-data" not in content_type.lower():
        return None
    msg = BytesParser(policy=HTTP).parsebytes(
        b"Content-Type: " + content_type.encode("latin-1") + b"\r\nMIME-Version: 1.0\r\n\r\n" + body)
    if not msg.is_multipart():
        return None
    for part in msg.iter_parts():
        if part.get_content_disposition() != "form-data":
            continue
        if part.get_param("name", header="content-disposition") != field:
            continue
        return part.get_filename(), part.get_content_type(), part.get_payload(decode=True) or b""
    return None


class Pipeline:
    """The stages behind the routes.  The stages this package does not own (parser, summariser, text / multimodal
    generators) are whatever the caller passes to `create_app`, else the stand-ins of ingest.py."""

    CONTEXT_KINDS = ("text_chunks", "table_chunks", "image_chunks")

    def __init__(self, parts: dict):
        self.parts = parts

    def __getattr__(self, name):          # pipeline.embedder, pipeline.retriever, ...
        try:
            return self.__dict__["parts"][name]
        except KeyError:
            raise AttributeError(name) from None

    async def start(self):
        p = self.parts
        # (MMRAG_CHUNKER=semantic: the parser finds the embedder, which is created below, at its first document)
        p["parser"] = p["parser"] or make_parser(lambda: p["embedder"]) or TextDocumentParser()
        p["llm"] = p["llm"] or ExtractiveAnswerer()
        p["mllm"] = p["mllm"] or p["llm"]
        await p["llm"].initialize()
        # (MMRAG_SUMMARIZER=extractive: the summariser finds the embedder, which is created below, at its first document)
        p["summarizer"] = p["summarizer"] or make_summarizer(lambda: p["embedder"]) or PassthroughSummarizer(p["mllm"])
        p["embedder"] = p["embedder"] or EmbeddingManager(batch_size=32, enable_cache=True)
        p["retriever"] = p["retriever"] or MultiVectorRetriever(enable_compression=True, enable_cache=True)
        for name in ("embedder", "retriever"):
            await p[name].initialize()

    async def stop(self):
        for name in ("llm", "embedder", "retriever"):
            try:
                await self.parts[name].cleanup()
            except Exception as e:  # pragma: no cover
                logger.error("Cleanup error: %s", e)

    async def ingest(self, filename: str, content_type: Optional[str], data: bytes) -> dict:
        """parse -> summarise -> embed + store vectors -> store raw items (api.py:262-300); returns the UploadResponse
        fields except the timing ones"""
        doc_id = "doc_" + uuid.uuid4().hex[:12]
        tree = await self.parser.parse_document(data, filename, content_type, doc_id=doc_id)
        items = await self.summarizer.summarize_parsed_document(tree, max_length=300, show_progress=True)
        if not items:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail="No content extracted")
        stored = await self.embedder.embed_and_store(items, doc_id)
        await self.retriever.store_raw_documents(doc_id, items, filename)
        return {"doc_id": doc_id, "filename": filename, "doc_type": tree.get("doc_type", "unknown"),
                "chunks_processed": stored}

    def _need(self, needs):
        """400 with the detail of `needs` unless the embedder has its method and says it supports it"""
        method, supports, detail = needs
        if not (hasattr(self.embedder, method) and getattr(self.embedder, supports, lambda: True)()):
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=detail)

    async def duplicates(self, threshold: Optional[float], doc_id: Optional[str], limit: int) -> dict:
        """the near-duplicate report (EmbeddingManager.find_duplicates) with `pairs` cut to `limit`"""
        self._need(DEDUP_NEEDS)
        try:
            report = await self.embedder.find_duplicates(threshold=threshold, doc_id=doc_id)
        except ValueError as e:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        return {"threshold": report["threshold"], "total_pairs": report["total_pairs"], "truncated": report["truncated"],
                "pairs": [{"a": a, "b": b, "cosine": c} for a, b, c in report["pairs"][:max(limit, 0)]],
                "groups": [{"keep": g[0], "duplicates": list(g[1:])} for g in report["groups"]]}

    async def topics(self, n_topics: Optional[int], doc_id: Optional[str], representatives: int, seed: int,
                     terms: Optional[int] = None) -> dict:
        """the topic report (EmbeddingManager.cluster_topics); `objective` is its last value.  `terms` (None: the
        MMRAG_TOPIC_TERMS setting) > 0: each topic also carries its significant `terms` and a `label`, the first
        LABEL_TERMS of them"""
        self._need(TOPICS_NEEDS)
        if not 1 <= representatives <= 10:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail="representatives must be in 1..10")
        terms = settings.topic_terms() if terms is None else terms
        if not 0 <= terms <= MAX_TOPIC_TERMS:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail=f"terms must be in 0..{MAX_TOPIC_TERMS}")
        more = {}
        if terms:
            self._need(TERMS_NEEDS)
            more["terms"] = terms
        try:
            report = await self.embedder.cluster_topics(n_topics=n_topics, doc_id=doc_id,
                                                        representatives=representatives, seed=seed, **more)
        except ValueError as e:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))

        def labelled(c: dict) -> dict:
            if not terms:
                return {}
            found = c.get("terms", [])
            return {"terms": found, "label": ", ".join(str(t["term"]) for t in found[:LABEL_TERMS])}

        return {"n_topics": report["n_clusters"], "iterations": report["iterations"], "converged": report["converged"],
                "objective": report["objective"][-1] if report["objective"] else None,
                "topics": [{"topic": c["cluster"], "size": c["size"], "cohesion": c["cohesion"],
                            "representatives": c["representatives"],
                            "documents": [{"doc_id": v, "count": n} for v, n in c["documents"]], **labelled(c)}
                           for c in report["clusters"]]}

    async def keywords(self, doc_id: str, top: int, min_count: int) -> dict:
        """a stored document's keywords (EmbeddingManager.document_keywords); 404 when no stored item has `doc_id`"""
        self._need(TERMS_NEEDS)
        if not 1 <= top <= MAX_KEYWORDS or min_count < 1:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail=f"top must be in 1..{MAX_KEYWORDS} and min_count at least 1")
        try:
            found = await self.embedder.document_keywords([doc_id], top=top, min_count=min_count)
        except ValueError as e:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        if not found or not found[0]["chunks"]:
            raise HTTPException(status_code=status.HTTP_404_NOT_FOUND, detail=f"no stored item has doc_id {doc_id!r}")
        return found[0]

    async def related(self, doc_id: Optional[str], texts: Optional[List[str]], top_k: int,
                      threshold: Optional[float], filter_dict: Optional[Dict] = None) -> dict:
        """the related documents of a stored document or of passages (EmbeddingManager.related_documents), each with
        its RELATED_PAIRS best pairs by score; 404 when no stored item has `doc_id`"""
        self._need(RELATED_NEEDS)
        try:
            out = await self.embedder.related_documents(doc_id=doc_id, texts=texts, n_results=top_k,
                                                        threshold=threshold, filter_dict=filter_dict)
        except LookupError as e:
            raise HTTPException(status_code=status.HTTP_404_NOT_FOUND, detail=str(e.args[0]) if e.args else str(e))
        except ValueError as e:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        related = [{**doc, "pairs": sorted(doc["pairs"], key=lambda p: -p["score"])[:RELATED_PAIRS]}
                   for doc in out["related"]]
        return {"chunks": out["chunks"], "threshold": out["threshold"], "related": related}

    async def remove_duplicates(self, threshold: Optional[float], doc_id: Optional[str]) -> dict:
        self._need(DEDUP_NEEDS)
        try:
            gone = await self.embedder.remove_duplicates(threshold=threshold, doc_id=doc_id)
        except DuplicateReportTruncated as e:
            raise HTTPException(status_code=status.HTTP_409_CONFLICT, detail=str(e))
        except ValueError as e:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        return {"deleted": len(gone), "ids": list(gone)}

    @staticmethod
    def _sources(hits: dict) -> List[dict]:
        """the `sources` of a response from one query's hits (api.py:390); the modes add their own columns"""
        return [{"rank": at, "doc_id": found, "relevance_score": round(float(1.0 - min(dist, 1.0)), 3),
                 "type": meta.get("type", "unknown")}
                for at, (found, dist, meta) in enumerate(zip(hits["ids"], hits["distances"], hits["metadatas"]), 1)]

    async def _generate(self, question: str, ids: List[str], multimodal: bool) -> str:
        """the generator's answer from the raw items of the hits (api.py:355-388)"""
        raw = await self.retriever.retrieve_raw_documents(ids)
        passages, tables, images = (raw[k] for k in self.CONTEXT_KINDS)
        body = "\n\n".join(passages) if passages else ""
        if multimodal and (images or tables):
            return await self.mllm.generate_multimodal(text=body, tables=tables, images=images, max_tokens=1000,
                                                       temperature=0.7)
        if tables:
            body += "\n\nBảng:\n" + "\n\n".join(tables)
        return await self.llm.generate_text(f"Context:\n{body}\n\nCâu hỏi: {question}\n\nTrả lời:", max_tokens=1000,
                                            temperature=0.7)

    async def answer(self, question: str, top_k: int, multimodal: bool, rerank: bool = False,
                     hybrid: bool = False, mmr: bool = False, mmr_lambda: Optional[float] = None,
                     group_by_document: bool = False, per_document: int = 1,
                     variants: Optional[List[str]] = None, variant_weight: Optional[float] = None,
                     fusion: Optional[str] = None, doc_ids: Optional[List[str]] = None,
                     rerank_method: Optional[str] = None, explain: bool = False, boost: Any = None,
                     recommend: Optional[Dict[str, Any]] = None,
                     filter_dict: Optional[Dict[str, Any]] = None, late: bool = False,
                     passage_tokens: Optional[int] = None, sparse: bool = False,
                     hybrid_leg: Optional[str] = None, extractive: bool = False,
                     reader: Optional[str] = None, fuzzy: Any = None, phrases: Optional[bool] = None,
                     slop: Optional[int] = None, citations: Optional[Dict[str, Any]] = None) -> Optional[dict]:
        """vector search -> raw items -> generator (api.py:338-400); None when nothing was retrieved.  `rerank`: search
        max(top_k, MMRAG_RERANK_CANDIDATES) hits, keep the re-ranker's best top_k (`rerank_method` "cross" or "late",
        default MMRAG_RERANK_METHOD; `explain`: late interaction's per-token matches on every source).  `hybrid`: from
        dense + BM25 retrieval fused by reciprocal rank.  `mmr`: the hits are a maximal-marginal-relevance selection of
        the dense candidates (`mmr_lambda`, default MMRAG_MMR_LAMBDA).  `group_by_document` (alone): the hits are the
        `per_document` best of each of the top_k best documents, flattened in document order.  `variants` (a list,
        possibly empty; alone or with `rerank`): the hits are the fusion of the ranked lists of `question` and these
        further phrasings (EmbeddingManager.multi_query; `variant_weight` for each of them against 1.0, `fusion`
        "rrf" or "max"); the generator and the re-ranker see `question` only.  `doc_ids`: hits from these documents
        only -- a plain (or re-ranked) query through EmbeddingManager.scoped_query, every other mode through its
        filter.  `boost` (a BoostSpec; alone or with `rerank`): the hits are ranked by cosine + the spec's score prior
        (EmbeddingManager.boosted_query).  `recommend` ({"like", "unlike", "unlike_texts", "negative_weight"}; alone or
        with `rerank`): the question is one positive example next to these (EmbeddingManager.recommend).
        `filter_dict`: a metadata filter every mode gets as (part of) its filter; a plain or re-ranked query with one
        goes through EmbeddingManager.query, `doc_ids` AND-ed into it.  `late` (alone or with `rerank`): the hits are
        the exact MaxSim top_k over the token store (EmbeddingManager.late_query).  `passage_tokens` (a window size;
        with any mode): every source carries its answer `passage` -- from the re-rank call when that is late
        interaction's, else from EmbeddingManager.extract_passages over the final hits.  The generator's context is
        built from the retriever's raw documents either way.  `sparse` (alone): the hits are the learned sparse top_k
        (EmbeddingManager.sparse_query; `explain`: every source carries its `matched_terms`).  `hybrid_leg` "sparse"
        (with `hybrid`): the dense hits are fused with the learned sparse leg instead of BM25.  `extractive` (with any
        mode): the answer is EmbeddingManager.extract_answer's over the hits' raw text passages, no generator call, and
        every quoted source carries its `quotes`.  `reader` ("spans" or "answer"; with any mode `passages` works with):
        EmbeddingManager.read_answers over the hits' raw text passages -- the result gains `answers` and `answerable`,
        every source its `answer_spans`; "answer": the answer is the best span's text (NO_ANSWER_FOUND when the hits do
        not answer the question), no generator call.  `fuzzy` (with `hybrid` and the lexical leg): the BM25 leg is
        typo-tolerant (EmbeddingManager.hybrid_query) and the result carries the `corrections` it made.  `phrases` /
        `slop` (with `hybrid` and the lexical leg): quoted segments of the question are phrases every hit must hold,
        and the result carries the `phrases` report.  `citations` ({"threshold", "max_citations"}, None where the
        settings decide; with any mode and any way the answer is made): EmbeddingManager.attribute_answer of the answer
        against the hits' raw text passages -- the result gains `citations` and `groundedness`, every source its
        `cited_by` and `support`"""
        multi = variants is not None
        sparse_leg = hybrid and hybrid_leg == "sparse"
        riding = passage_tokens is not None and rerank and rerank_method == "late"
        # the restriction as the filter the embedder's methods take (nothing is passed when there is none)
        docs_only = None if doc_ids is None else {"doc_id": {"$in": list(doc_ids)}}
        both = {"$and": [filter_dict, docs_only]} if filter_dict and docs_only else (filter_dict or docs_only)
        only = {} if both is None else {"filter_dict": both}
        if multi:
            weights = None if variant_weight is None else [1.0] + [float(variant_weight)] * len(variants)

            def search(text, n_results):
                return self.embedder.multi_query([text] + list(variants), n_results=n_results, weights=weights,
                                                 method=fusion, **only)
        elif boost is not None:
            search = functools.partial(self.embedder.boosted_query, boost=boost, **only)
        elif recommend is not None:
            search = functools.partial(self.embedder.recommend, **recommend, **only)
        elif mmr:
            search = functools.partial(self.embedder.mmr_query, lambda_mult=mmr_lambda, **only)
        elif sparse:
            search = functools.partial(self.embedder.sparse_query, explain=explain, **only)
        elif sparse_leg:
            search = functools.partial(self.embedder.hybrid_query, leg="sparse", **only)
        elif hybrid:
            search = functools.partial(self.embedder.hybrid_query, **only, **({} if fuzzy is None else {"fuzzy": fuzzy}),
                                       **({} if phrases is None else {"phrases": phrases}),
                                       **({} if slop is None else {"slop": slop}))
        elif late:
            search = functools.partial(self.embedder.late_query, **only)
        elif doc_ids is not None and not filter_dict and hasattr(self.embedder, "scoped_query"):
            search = functools.partial(self.embedder.scoped_query, doc_ids=list(doc_ids))
        else:
            search = functools.partial(self.embedder.query, **only)
        # per-hit columns re-ranking carries along
        extra = ("fused_scores", "matched_queries") if multi else ("mmr_scores",) if mmr else \
            ("hybrid_scores", "sparse_scores") if sparse_leg else \
            ("hybrid_scores",) if hybrid else ("late_scores",) if late else \
            ("scores", "boosts") if boost is not None else \
            tuple(column for column, _ in RECOMMEND_COLUMNS) if recommend is not None else ()
        if group_by_document:
            hits = await self.embedder.grouped_query(question, n_groups=top_k, group_size=per_document, **only)
        elif rerank:
            hits = await search(question, n_results=max(top_k, settings.MMRAG_RERANK_CANDIDATES))
            corrections, phrase_report = hits.get("corrections"), hits.get("phrases")
            if hits["ids"]:
                carried = {column: dict(zip(hits["ids"], hits[column])) for column in extra}
                # (the method is passed on only when one was chosen: an embedder without late interaction keeps its
                # two-argument rerank_results)
                chosen = {} if rerank_method is None and not explain else {"method": rerank_method, "explain": explain}
                if riding:
                    chosen["passages"] = passage_tokens
                hits = await self.embedder.rerank_results(question, hits, top_k=top_k, **chosen)
                for column, of_id in carried.items():
                    hits[column] = [of_id[found] for found in hits["ids"]]
                if corrections is not None:
                    hits["corrections"] = corrections
                if phrase_report is not None:
                    hits["phrases"] = phrase_report
        else:
            hits = await search(question, n_results=top_k)
        if not hits["ids"]:
            return None
        if passage_tokens is not None and "passages" not in hits:
            hits = await self.embedder.extract_passages(question, hits, window_tokens=passage_tokens)
        quoted = read = None
        if extractive or reader is not None or citations is not None:
            # hit by hit: which source a raw text passage belongs to (the buckets of one call do not say)
            texts, owner = [], []
            for at, found in enumerate(hits["ids"]):
                for passage in (await self.retriever.retrieve_raw_documents([found]))[self.CONTEXT_KINDS[0]]:
                    texts.append(passage)
                    owner.append(at)
        if reader is not None:
            read = await self.embedder.read_answers(question, hits, n_answers=READER_ANSWERS, texts=texts, owner=owner)
        if extractive:
            quoted = await self.embedder.extract_answer(question, texts)
            text = quoted["answer"]
        elif reader == "answer":
            text = read["answers"][0]["text"] if read["answerable"] else NO_ANSWER_FOUND
        else:
            text = await self._generate(question, hits["ids"], multimodal)
        cited = None
        if citations is not None:
            cited = await self.embedder.attribute_answer(text, texts, owner=owner, **citations)
        ranked = self._sources(hits)
        for on, column, key in ((rerank, "rerank_scores", "rerank_score"), (hybrid, "hybrid_scores", "hybrid_score"),
                                (mmr, "mmr_scores", "mmr_score"), (late, "late_scores", "late_score"),
                                (sparse or sparse_leg, "sparse_scores", "sparse_score"),
                                (sparse and explain, "matched_terms", "matched_terms"),
                                (multi, "fused_scores", "fused_score"),
                                (multi, "matched_queries", "matched_queries"), (boost is not None, "scores", "score"),
                                (boost is not None, "boosts", "boost"),
                                *((recommend is not None, column, key) for column, key in RECOMMEND_COLUMNS)):
            if on:
                for src, score in zip(ranked, hits[column]):
                    src[key] = score
        if rerank and "late_matches" in hits:
            for src, found in zip(ranked, hits["late_matches"]):
                src["matches"] = found
        if passage_tokens is not None:
            for src, found in zip(ranked, hits["passages"]):
                src["passage"] = {key: found[key] for key in PASSAGE_KEYS}
        if quoted is not None:
            for quote in quoted["quotes"]:
                ranked[owner[quote["passage"]]].setdefault("quotes", []).append({key: quote[key] for key in QUOTE_KEYS})
        if read is not None:
            for src, found in zip(ranked, read["answer_spans"]):
                src["answer_spans"] = [{key: span[key] for key in SPAN_KEYS} for span in found]
        if cited is not None:
            for at, src in enumerate(ranked):
                src["cited_by"] = [claim for claim, entry in enumerate(cited["citations"])
                                   if any(found["source"] == at for found in entry["sources"])]
                src["support"] = cited["support"][at] if at < len(cited["support"]) else 0.0
        if group_by_document:
            at = 0
            for document_rank, group in enumerate(hits["groups"], 1):
                for src in ranked[at: at + len(group["ids"])]:
                    src["document"] = group["key"]
                    src["document_rank"] = document_rank
                at += len(group["ids"])
        made = {key: hits[key] for key in ("corrections", "phrases") if key in hits}
        if cited is not None:
            made.update(citations=cited["citations"], groundedness=cited["groundedness"])
        if read is not None:
            return {"answer": text, "sources": ranked, "answerable": read["answerable"],
                    "answers": [{key: answer[key] for key in ANSWER_KEYS} for answer in read["answers"]], **made}
        return {"answer": text, "sources": ranked, **made}

    async def recommend(self, like: List[str], unlike: List[str], unlike_texts: List[str], top_k: int,
                        filter_dict: Optional[Dict], negative_weight: Optional[float]) -> dict:
        """POST /recommend: the sources of EmbeddingManager.recommend for stored items as examples; no generator call"""
        self._need(RECOMMEND_NEEDS)
        try:
            hits = await self.embedder.recommend(None, like=like, unlike=unlike, unlike_texts=unlike_texts,
                                                 n_results=top_k, filter_dict=filter_dict,
                                                 negative_weight=negative_weight)
        except ValueError as e:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        ranked = self._sources(hits)
        for column, key in RECOMMEND_COLUMNS:
            for src, value in zip(ranked, hits[column]):
                src[key] = value
        return {"sources": ranked}

    async def explore(self, question: str, min_score: float, limit: int, facets: List[str],
                      filter_dict: Optional[Dict], doc_ids: Optional[List[str]]) -> dict:
        """POST /explore: how many stored items clear `min_score` for the question, their spread over the `facets`
        keys, and the `limit` best as sources (EmbeddingManager.range_query); no generator call"""
        self._need(RANGE_NEEDS)
        docs_only = None if doc_ids is None else {"doc_id": {"$in": list(doc_ids)}}
        both = {"$and": [filter_dict, docs_only]} if filter_dict and docs_only else (filter_dict or docs_only)
        try:
            hits = await self.embedder.range_query(question, min_score, limit=limit, facets=list(facets),
                                                   filter_dict=both)
        except ValueError as e:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        return {"total": hits["total"], "truncated": hits["truncated"], "hits": self._sources(hits),
                "facets": hits["facets"]}

    async def attribute(self, answer: str, passages: Optional[List[str]], ids: Optional[List[str]],
                        threshold: Optional[float], max_citations: Optional[int]) -> dict:
        """POST /attribute: EmbeddingManager.attribute_answer of `answer` against `passages`, or against the raw text
        passages of the stored `ids` (source i is ids[i]); no retrieval and no generator call"""
        self._need(CITATION_NEEDS)
        owner = None
        if ids is not None:
            passages, owner = [], []
            for at, found in enumerate(ids):
                for passage in (await self.retriever.retrieve_raw_documents([found]))[self.CONTEXT_KINDS[0]]:
                    passages.append(passage)
                    owner.append(at)
        try:
            return await self.embedder.attribute_answer(answer, passages, owner=owner, threshold=threshold,
                                                        max_citations=max_citations)
        except ValueError as e:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))

    async def health(self) -> dict:
        parts = {"llm_adapter": await self.llm.health_check(),
                 "embedder": {"status": "healthy",
                              "documents": (await self.embedder.get_collection_stats()).get("count", 0)},
                 "retriever": await self.retriever.health_check()}
        fine = all(v.get("status") == "healthy" or v.get("healthy") is True for v in parts.values())
        return {"status": "healthy" if fine else "degraded", "components": parts,
                "timestamp": datetime.utcnow().isoformat(), "auth": "disabled"}

    async def report(self) -> dict:
        emb, ret, summ = [await self.parts[n].get_stats() for n in ("embedder", "retriever", "summarizer")]
        listing = await self.retriever.list_all_documents()
        per_kind = {kind: sum(doc.get("chunks", {}).get(kind, 0) for doc in listing) for kind in ("text", "table", "image")}
        return {"documents": {"total": len(listing), "total_chunks": emb.get("count", 0), "by_type": per_kind},
                "embedder": {"cache_hit_rate": emb.get("cache", {}).get("hit_rate", 0)},
                "retriever": {"compression_enabled": ret.get("features", {}).get("compression", False),
                              "compression_savings": ret.get("compression", {}).get("savings_percent", 0)},
                "summarizer": {"total_summaries": summ.get("total_summaries", 0),
                               "cache_hit_rate": summ.get("cache", {}).get("hit_rate", 0)},
                "auth": "disabled"}


def _as_http_500(fn):
    """route wrapper: anything but an HTTPException becomes a 500 with the message as detail (the reference's blanket
    `except Exception` around every route body)"""
    @functools.wraps(fn)
    async def wrapped(*a, **kw):
        try:
            return await fn(*a, **kw)
        except HTTPException:
            raise
        except Exception as e:
            logger.error("%s failed: %s", fn.__name__, e, exc_info=True)
            raise HTTPException(status_code=status.HTTP_500_INTERNAL_SERVER_ERROR, detail=str(e))

    return wrapped


def create_app(embedder: Optional[Any] = None, retriever: Optional[Any] = None, parser: Optional[Any] = None,
               summarizer: Optional[Any] = None, llm_adapter: Optional[Any] = None,
               mllm_adapter: Optional[Any] = None, query_expander: Optional[Any] = None) -> FastAPI:
    """`query_expander`: optional, any object with `async expand(question, n) -> List[str]` (ingest.LLMQueryExpander
    over a generator is one); /query's `expand` field asks it for further phrasings of the question"""
    pipe = Pipeline({"embedder": embedder, "retriever": retriever, "parser": parser, "summarizer": summarizer,
                     "llm": llm_adapter, "mllm": mllm_adapter, "expander": query_expander})

    @asynccontextmanager
    async def lifespan(app: FastAPI):  # api.py:65-128
        await pipe.start()
        yield
        await pipe.stop()

    app = FastAPI(title="Multi-modal RAG System (MI355X hot path)", version="2.0.0", lifespan=lifespan)
    app.state.components = pipe.parts

    @app.get("/health")
    async def health_check():  # api.py:202-241: never raises
        try:
            return await pipe.health()
        except Exception as e:
            return {"status": "unhealthy", "error": str(e)}

    @app.post("/upload", response_model=UploadResponse)
    @_as_http_500
    async def upload_document(request: Request):  # api.py:244-322
        t0 = time.time()
        form = parse_multipart_file(request.headers.get("content-type", ""), await request.body())
        if form is None:  # FastAPI's own answer to a missing File(...) field
            raise HTTPException(status_code=422, detail=[{"loc": ["body", "file"], "msg": "Field required",
                                                          "type": "missing"}])
        filename, content_type, data = form
        if not filename:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail="Filename is required")
        if len(data) > settings.MAX_UPLOAD_SIZE * 1024 * 1024:
            raise HTTPException(status_code=413, detail=f"File too large. Max: {settings.MAX_UPLOAD_SIZE}MB")
        out = await pipe.ingest(filename, content_type, data)
        took = time.time() - t0
        skipped = out["chunks_processed"].get("duplicates_skipped", 0)
        note = f", {skipped} duplicates skipped" if skipped > 0 else ""
        return {**out, "message": f"Processed in {took:.2f}s{note}", "processing_time": took}

    @app.post("/query", response_model=QueryResponse, response_model_exclude_unset=True)
    @_as_http_500
    async def query_documents(request: QueryRequest):  # api.py:325-413
        t0 = time.time()
        multi = request.variants is not None or request.expand > 0
        if multi and (request.mmr or request.hybrid or request.group_by_document):
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="Multi-query retrieval is not combined with MMR, hybrid retrieval or grouping "
                                       "by document yet: send `variants` / `expand` without `mmr`, `hybrid` and "
                                       "`group_by_document`")
        if request.group_by_document and (request.mmr or request.hybrid or request.rerank):
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="Grouping by document is not combined with MMR, hybrid retrieval or re-ranking "
                                       "yet: send `group_by_document` without `mmr`, `hybrid` and `rerank`")
        if request.hybrid_leg is not None and not request.hybrid:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="`hybrid_leg` belongs to hybrid retrieval: send it with `hybrid`")
        fuzzy = None
        if request.fuzzy is not None:
            from .lexical import parse_fuzzy

            if not request.hybrid:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="`fuzzy` belongs to hybrid retrieval's lexical leg: send it with `hybrid`")
            if request.hybrid_leg == "sparse":
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="`fuzzy` belongs to the lexical leg: send it without `hybrid_leg`: \"sparse\"")
            try:
                fuzzy = parse_fuzzy(request.fuzzy)
            except ValueError as e:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
            fuzzy = "" if fuzzy is None else fuzzy      # an explicit false overrides the setting
        if request.phrases is not None or request.slop is not None:
            from .lexical import parse_slop, query_phrases

            if not request.hybrid:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="`phrases` belongs to hybrid retrieval's lexical leg: send it with `hybrid`")
            if request.hybrid_leg == "sparse":
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="`phrases` belongs to the lexical leg: send it without `hybrid_leg`: \"sparse\"")
            try:
                if request.slop is not None:
                    parse_slop(request.slop)
                if request.phrases:
                    query_phrases(request.query)      # too long a phrase, too many of them
            except ValueError as e:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        if request.sparse:
            if (multi or request.mmr or request.hybrid or request.group_by_document or request.rerank or request.late
                    or (request.boost is not None and request.boost is not False) or request.like is not None
                    or request.unlike is not None or request.not_ is not None or request.passages or request.reader
                    or request.reader_answer):
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="Learned sparse retrieval is not combined with the other retrieval modes, "
                                           "re-ranking or answer passages yet: send `sparse` alone, with `filter`, "
                                           "`doc_ids` or `explain`")
        if request.sparse or request.hybrid_leg == "sparse":
            pipe._need(SPARSE_NEEDS)
            if not getattr(pipe.embedder, "has_sparse_encoder", lambda: False)():
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=SPARSE_NEEDS[2])
        if (request.rerank_method is not None or request.explain) and not request.rerank and not request.sparse:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="`rerank_method` and `explain` belong to re-ranking: send them with `rerank`")
        try:
            late = request.rerank and (request.rerank_method or settings.rerank_method()) == "late"
        except ValueError as e:      # a setting changed to neither method after start-up
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        if request.explain and not late and not request.sparse:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="`explain` needs late-interaction re-ranking: send `rerank_method`: \"late\"")
        if late:
            method, supports, detail = LATE_NEEDS
            if not (hasattr(pipe.embedder, method) and getattr(pipe.embedder, supports, lambda: False)()):
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=detail)
        elif request.rerank and not (hasattr(pipe.embedder, "has_reranker") and pipe.embedder.has_reranker()):
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="Re-ranking is not configured: set MMRAG_RERANKER_DIR to a local cross-encoder")
        if request.passage_tokens is not None and not request.passages:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="`passage_tokens` belongs to answer passages: send it with `passages`")
        window = None
        if request.passages:
            pipe._need(PASSAGES_NEEDS)
            try:
                window = request.passage_tokens if request.passage_tokens is not None else settings.passage_tokens()
            except ValueError as e:      # a setting changed out of range after start-up
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        if request.extractive_answer:
            pipe._need(EXTRACT_NEEDS)
        if request.reader or request.reader_answer:
            if not (hasattr(pipe.embedder, "read_answers") and getattr(pipe.embedder, "has_reader", lambda: False)()):
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="The extractive reader is not configured: set MMRAG_READER_DIR to a local "
                                           "BertForQuestionAnswering directory")
            if request.reader_answer and request.extractive_answer:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="`reader_answer` and `extractive_answer` both replace the generator's "
                                           "answer: send one of them")
        if (request.citation_threshold is not None or request.max_citations is not None) and not request.citations:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="`citation_threshold` and `max_citations` belong to answer citations: send them "
                                       "with `citations`")
        cite = None
        if request.citations:
            from .attribution import citation_parameters

            pipe._need(CITATION_NEEDS)
            try:      # a setting changed out of range after start-up
                cite = citation_parameters(request.citation_threshold, request.max_citations)
            except ValueError as e:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        if request.filter is not None:
            try:
                _, timed = check_filter(request.filter)
            except ValueError as e:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
            if timed and not (settings.MMRAG_DEVICE_FILTERS
                              and getattr(pipe.embedder, "supports_device_filters", lambda: False)()):
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail='A filter on "$added_at" needs device filters: set MMRAG_DEVICE_FILTERS=1 '
                                           "with a single-GPU collection (EmbeddingManager.supports_device_filters)")
        spec = None
        if request.boost is not None and request.boost is not False:
            if multi or request.mmr or request.hybrid or request.group_by_document or request.doc_ids is not None:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="Boosted retrieval is not combined with hybrid retrieval, MMR, grouping by "
                                           "document, multi-query retrieval or `doc_ids` yet: send `boost` without "
                                           "`hybrid`, `mmr`, `group_by_document`, `variants` / `expand` and `doc_ids`")
            try:
                spec = parse_boost(request.boost, settings.MMRAG_BOOST_RECENCY, settings.MMRAG_BOOST_HALF_LIFE_DAYS)
            except ValueError as e:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
            pipe._need(BOOST_NEEDS)
        recommend = None
        if request.like is not None or request.unlike is not None or request.not_ is not None:
            if (multi or request.mmr or request.hybrid or request.group_by_document or request.doc_ids is not None
                    or spec is not None):
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="Recommend retrieval is not combined with hybrid retrieval, MMR, grouping by "
                                           "document, boosted retrieval, multi-query retrieval or `doc_ids` yet: send "
                                           "`like` / `unlike` / `not` without `hybrid`, `mmr`, `group_by_document`, "
                                           "`boost`, `variants` / `expand` and `doc_ids`")
            recommend = {"like": request.like or [], "unlike": request.unlike or [],
                         "unlike_texts": request.not_ or [], "negative_weight": request.negative_weight}
            if 1 + sum(len(recommend[key]) for key in ("like", "unlike", "unlike_texts")) > 16:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="A recommend request takes at most 16 examples in all: the question, "
                                           "`like`, `unlike` and `not` together")
            pipe._need(RECOMMEND_NEEDS)
        elif request.negative_weight is not None:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="`negative_weight` belongs to recommend retrieval: send it with `like`, "
                                       "`unlike` or `not`")
        if request.mmr and request.hybrid:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="MMR and hybrid retrieval are not combined yet: send `mmr` or `hybrid`, not both")
        if request.late:
            if (multi or request.mmr or request.hybrid or request.group_by_document or spec is not None
                    or recommend is not None):
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="Late retrieval is not combined with hybrid retrieval, MMR, grouping by "
                                           "document, boosted retrieval, multi-query retrieval or recommend retrieval "
                                           "yet: send `late` without `hybrid`, `mmr`, `group_by_document`, `boost`, "
                                           "`variants` / `expand` and `like` / `unlike` / `not`")
            pipe._need(LATE_QUERY_NEEDS)
        for flag, method, supports, detail in MODE_NEEDS:
            if getattr(request, flag) and not (hasattr(pipe.embedder, method)
                                               and getattr(pipe.embedder, supports, lambda: True)()):
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=detail)
        variants = None
        if multi:
            pipe._need(MULTI_NEEDS)
            if request.expand > 0 and pipe.expander is None:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                    detail="Query expansion is not configured: pass a `query_expander` to create_app, "
                                           "or send the phrasings as `variants`")
            variants = list(request.variants or [])
            if request.expand > 0:
                variants += [str(v)[:2000] for v in await pipe.expander.expand(request.query, request.expand)]
            seen, kept = {request.query.strip()}, []
            for v in variants:                      # a phrasing searched twice would only count twice
                if v.strip() and v.strip() not in seen:
                    seen.add(v.strip())
                    kept.append(v)
            variants = kept[:15]
        # (combinations of modes were refused above: Pipeline.answer sees at most one of mmr / hybrid / grouping /
        # variants)
        try:
            out = await pipe.answer(request.query, request.top_k, request.use_multimodal, rerank=request.rerank,
                                    hybrid=request.hybrid, mmr=request.mmr, mmr_lambda=request.mmr_lambda,
                                    group_by_document=request.group_by_document, per_document=request.per_document,
                                    variants=variants, variant_weight=request.variant_weight, fusion=request.fusion,
                                    doc_ids=request.doc_ids,
                                    rerank_method="late" if late else request.rerank_method, explain=request.explain,
                                    **({} if spec is None else {"boost": spec}),
                                    **({} if recommend is None else {"recommend": recommend}),
                                    **({} if not request.filter else {"filter_dict": request.filter}),
                                    **({} if not request.late else {"late": True}),
                                    **({} if not request.sparse else {"sparse": True}),
                                    **({} if request.hybrid_leg is None else {"hybrid_leg": request.hybrid_leg}),
                                    **({} if fuzzy is None else {"fuzzy": fuzzy}),
                                    **({} if request.phrases is None else {"phrases": request.phrases}),
                                    **({} if request.slop is None else {"slop": request.slop}),
                                    **({} if window is None else {"passage_tokens": window}),
                                    **({} if not request.extractive_answer else {"extractive": True}),
                                    **({} if not (request.reader or request.reader_answer) else
                                       {"reader": "answer" if request.reader_answer else "spans"}),
                                    **({} if cite is None else {"citations": cite}))
        except ValueError as e:
            if recommend is None and cite is None:
                raise
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))   # an id no stored item has
        if out is None:
            out = {"answer": NO_DOCS_ANSWER, "sources": []}
        return {**out, "processing_time": time.time() - t0}

    @app.post("/recommend")
    @_as_http_500
    async def recommend_documents(request: RecommendRequest):
        t0 = time.time()
        if len(request.like) + len(request.unlike or []) + len(request.not_ or []) > 16:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="A recommend request takes at most 16 examples in all: `like`, `unlike` and "
                                       "`not` together")
        out = await pipe.recommend(request.like, request.unlike or [], request.not_ or [], request.top_k,
                                   request.filter, request.negative_weight)
        return {**out, "processing_time": time.time() - t0}

    @app.post("/related")
    @_as_http_500
    async def related_to_texts(request: RelatedRequest):
        t0 = time.time()
        out = await pipe.related(None, request.texts, request.top_k, request.threshold, request.filter)
        return {**out, "processing_time": time.time() - t0}

    @app.post("/chunk")
    @_as_http_500
    async def chunk_preview(request: ChunkRequest):
        t0 = time.time()
        pipe._need(CHUNK_NEEDS)
        try:
            chunks = (await pipe.embedder.chunk_texts([request.text], request.chunk_size))[0]
        except ValueError as e:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        return {"chunks": chunks, "chunker": "semantic", "processing_time": time.time() - t0}

    @app.post("/attribute")
    @_as_http_500
    async def attribute_answer(request: AttributeRequest):
        t0 = time.time()
        if (request.passages is None) == (request.ids is None):
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST,
                                detail="Send the evidence as `passages` or as stored `ids`, one of the two")
        out = await pipe.attribute(request.answer, request.passages, request.ids, request.citation_threshold,
                                   request.max_citations)
        return {**out, "processing_time": time.time() - t0}

    @app.post("/explore")
    @_as_http_500
    async def explore(request: ExploreRequest):
        t0 = time.time()
        if len(set(request.facets)) != len(request.facets):
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail="`facets` names a key twice")
        if request.filter is not None:
            try:
                check_filter(request.filter)
            except ValueError as e:
                raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail=str(e))
        out = await pipe.explore(request.query, request.min_score, request.limit, request.facets, request.filter,
                                 request.doc_ids)
        return {**out, "processing_time": time.time() - t0}

    @app.get("/documents/{doc_id}/related")
    @_as_http_500
    async def related_documents(doc_id: str, top_k: int = 5, threshold: Optional[float] = None):
        t0 = time.time()
        if not 1 <= top_k <= 100:
            raise HTTPException(status_code=status.HTTP_400_BAD_REQUEST, detail="top_k must be in 1..100")
        out = await pipe.related(doc_id, None, top_k, threshold)
        return {"doc_id": doc_id, **out, "processing_time": time.time() - t0}

    @app.get("/documents/{doc_id}/keywords")
    @_as_http_500
    async def document_keywords(doc_id: str, top: int = 10, min_count: int = 2):
        return await pipe.keywords(doc_id, top, min_count)

    @app.get("/documents")
    @_as_http_500
    async def list_documents():  # api.py:416-429
        listing = await pipe.retriever.list_all_documents()
        return {"total": len(listing), "documents": listing}

    @app.delete("/documents/{doc_id}")
    @_as_http_500
    async def delete_document(doc_id: str):  # api.py:432-445
        for store in (pipe.embedder, pipe.retriever):
            await store.delete_document(doc_id)
        return {"message": f"Document {doc_id} deleted"}

    @app.delete("/documents")
    @_as_http_500
    async def delete_all_documents():  # api.py:448-465
        n = len(await pipe.retriever.list_all_documents())
        for store in (pipe.embedder, pipe.retriever):
            await store.delete_all_documents()
        return {"message": f"Deleted {n} documents", "count": n}

    @app.get("/duplicates")
    @_as_http_500
    async def find_duplicates(threshold: Optional[float] = None, doc_id: Optional[str] = None, limit: int = 100):
        return await pipe.duplicates(threshold, doc_id, limit)

    @app.delete("/duplicates")
    @_as_http_500
    async def remove_duplicates(threshold: Optional[float] = None, doc_id: Optional[str] = None):
        return await pipe.remove_duplicates(threshold, doc_id)

    @app.get("/topics")
    @_as_http_500
    async def topics(n_topics: Optional[int] = None, doc_id: Optional[str] = None, representatives: int = 3,
                     seed: int = 0, terms: Optional[int] = None):
        return await pipe.topics(n_topics, doc_id, representatives, seed, terms)

    @app.get("/stats")
    @_as_http_500
    async def get_stats():  # api.py:468-508
        return await pipe.report()

    return app


app = create_app()
