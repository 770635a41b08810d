"""Settings for the hot path: the subset of the reference's `config.Settings`
(config.py:18-132) that the embed/retrieve path reads, with the same key names, defaults and
environment-variable overrides.  Extra keys (MMRAG_*) select the MI355X engine's options."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field


def _b(name: str, default: str) -> bool:
    return os.getenv(name, default).lower() == "true"


@dataclass
class Settings:
    # config.py:58-59
    CHROMA_PERSIST_DIR: str = field(default_factory=lambda: os.getenv("CHROMA_PERSIST_DIR", "./chroma_db"))
    CHROMA_COLLECTION_NAME: str = field(default_factory=lambda: os.getenv("CHROMA_COLLECTION_NAME", "multimodal_rag"))
    # config.py:64-66
    CHUNK_SIZE: int = field(default_factory=lambda: int(os.getenv("CHUNK_SIZE", "1000")))
    CHUNK_OVERLAP: int = field(default_factory=lambda: int(os.getenv("CHUNK_OVERLAP", "200")))
    TOP_K_RESULTS: int = field(default_factory=lambda: int(os.getenv("TOP_K_RESULTS", "5")))
    # config.py:79-81 (api.py:92-95 does not read them; kept for parity)
    EMBEDDER_BATCH_SIZE: int = field(default_factory=lambda: int(os.getenv("EMBEDDER_BATCH_SIZE", "32")))
    EMBEDDER_CACHE_SIZE: int = field(default_factory=lambda: int(os.getenv("EMBEDDER_CACHE_SIZE", "1000")))
    EMBEDDER_ENABLE_CACHE: bool = field(default_factory=lambda: _b("EMBEDDER_ENABLE_CACHE", "true"))
    # config.py:86-89
    RETRIEVER_ENABLE_COMPRESSION: bool = field(default_factory=lambda: _b("RETRIEVER_ENABLE_COMPRESSION", "true"))
    RETRIEVER_ENABLE_CACHE: bool = field(default_factory=lambda: _b("RETRIEVER_ENABLE_CACHE", "true"))
    RETRIEVER_CACHE_SIZE: int = field(default_factory=lambda: int(os.getenv("RETRIEVER_CACHE_SIZE", "100")))
    # config.py:102-106
    SENTENCE_TRANSFORMER_MODEL: str = field(
        default_factory=lambda: os.getenv("SENTENCE_TRANSFORMER_MODEL", "all-MiniLM-L6-v2"))
    CLIP_MODEL: str = field(default_factory=lambda: os.getenv("CLIP_MODEL", "ViT-B/32"))
    # config.py:117-119
    LOG_LEVEL: str = field(default_factory=lambda: os.getenv("LOG_LEVEL", "INFO"))
    ENABLE_CORS: bool = field(default_factory=lambda: _b("ENABLE_CORS", "true"))
    MAX_UPLOAD_SIZE: int = field(default_factory=lambda: int(os.getenv("MAX_UPLOAD_SIZE", "50")))  # MB

    # ---- engine options (not in the reference) ----
    # local Hugging Face style directory with config.json + model.safetensors + vocab.txt; when
    # empty the named architecture is random-initialised and a stand-in tokenizer is used
    MMRAG_MODEL_DIR: str = field(default_factory=lambda: os.getenv("MMRAG_MODEL_DIR", ""))
    # "float16" (default), "float32", "bfloat16", or "float8_e4m3fn": one-byte E4M3 codes scanned on the FP8 matrix
    # instruction (index.py VectorIndex).  MMRAG_F8_RESCORE: "float16" keeps a full-precision plane next to the FP8 one
    # and every search re-scores MMRAG_F8_OVERSAMPLE x n_results candidates (at least 20) exactly on it (1.5x the
    # memory of a float16 collection, faster scans); "none" is the capacity mode (0.5x; FP8 scores, no mmr / hybrid)
    MMRAG_INDEX_DTYPE: str = field(default_factory=lambda: os.getenv("MMRAG_INDEX_DTYPE", "float16"))
    MMRAG_F8_RESCORE: str = field(default_factory=lambda: os.getenv("MMRAG_F8_RESCORE", "float16"))
    MMRAG_F8_OVERSAMPLE: int = field(default_factory=lambda: int(os.getenv("MMRAG_F8_OVERSAMPLE", "4")))
    # float32 collections: batches of more than 64 queries are scored on the bf16 matrix pipe from a three-term split
    # of the float32 operands (|score error| <= 4e-5: approximate, and a query's score then depends on how many
    # requests the dispatcher batched it with).  "true" keeps the exact float32 matrix instruction for every batch
    # size (the batch is scanned 64 queries at a time: identical scores whatever the batch, ~2.5x the scan time)
    MMRAG_F32_EXACT_SEARCH: bool = field(default_factory=lambda: _b("MMRAG_F32_EXACT_SEARCH", "false"))
    # Row tables (ids, documents, metadata dicts) are millions of long-lived Python objects; every older-generation pass
    # of the cyclic collector walks them, and the lists a query batch builds trigger such passes: half of the 1 ms a
    # 256-query answer takes to build.  After this many rows have been added since the last time, the index calls
    # gc.freeze(): everything alive moves to the permanent generation (still freed by reference counting; no longer
    # scanned for cycles).  0 turns it off.
    MMRAG_GC_FREEZE_ROWS: int = field(default_factory=lambda: int(os.getenv("MMRAG_GC_FREEZE_ROWS", "100000")))
    MMRAG_WEIGHT_SEED: int = field(default_factory=lambda: int(os.getenv("MMRAG_WEIGHT_SEED", "0")))
    # "fp16" (throughput path) or "fp32": the reference's own arithmetic (SentenceTransformer.encode is float32,
    # embedder.py:397-403) -- scores within 1e-4 of the float32 model; pair it with MMRAG_INDEX_DTYPE=float32
    MMRAG_ENCODER_PRECISION: str = field(default_factory=lambda: os.getenv("MMRAG_ENCODER_PRECISION", "fp16"))
    # keep the collection across restarts: load it from CHROMA_PERSIST_DIR/mmrag_index in initialize(), save it there in
    # cleanup().  Off by default, as in the reference's current code: its chromadb.Client(Settings(persist_directory=...))
    # lacks is_persistent=True, i.e. the reference's collection is in-memory too
    MMRAG_PERSIST: bool = field(default_factory=lambda: _b("MMRAG_PERSIST", "false"))
    # cross-encoder re-ranking (rerank_results, POST /query with "rerank": true): a local BertForSequenceClassification
    # directory (config.json + model.safetensors + vocab.txt, e.g. cross-encoder/ms-marco-MiniLM-L-6-v2); empty = the
    # reference's placeholder (truncation only).  /query re-ranks max(top_k, MMRAG_RERANK_CANDIDATES) search hits
    MMRAG_RERANKER_DIR: str = field(default_factory=lambda: os.getenv("MMRAG_RERANKER_DIR", ""))
    MMRAG_RERANK_CANDIDATES: int = field(default_factory=lambda: int(os.getenv("MMRAG_RERANK_CANDIDATES", "20")))
    # extractive reader (EmbeddingManager.read_answers, POST /query with "reader": true; reader.py, csrc/span_head.hip):
    # a local BertForQuestionAnswering directory (config.json + model.safetensors + vocab.txt, e.g. a SQuAD2-trained
    # BERT); empty = the feature is off.  MMRAG_READER_MAX_ANSWER_TOKENS: the longest answer span, in tokens (1..64).
    # MMRAG_READER_NULL_THRESHOLD: the hits answer the question when best span score - lowest null score exceeds it.
    # MMRAG_READER_DOC_STRIDE: tokens two consecutive windows of a long passage share
    MMRAG_READER_DIR: str = field(default_factory=lambda: os.getenv("MMRAG_READER_DIR", ""))
    MMRAG_READER_MAX_ANSWER_TOKENS: int = field(
        default_factory=lambda: int(os.getenv("MMRAG_READER_MAX_ANSWER_TOKENS", "30")))
    MMRAG_READER_NULL_THRESHOLD: float = field(
        default_factory=lambda: float(os.getenv("MMRAG_READER_NULL_THRESHOLD", "0.0")))
    MMRAG_READER_DOC_STRIDE: int = field(default_factory=lambda: int(os.getenv("MMRAG_READER_DOC_STRIDE", "128")))
    # which re-ranker rerank_results uses when its caller names none: "cross" (the cross-encoder above; without one the
    # placeholder) or "late" (late interaction: token-level MaxSim with the bi-encoder itself, late.py -- needs no
    # second model).  MMRAG_LATE_MAX_DOC_TOKENS: passage tokens "late" scores (0 = the encoder's length; at most 512)
    MMRAG_RERANK_METHOD: str = field(default_factory=lambda: os.getenv("MMRAG_RERANK_METHOD", "cross"))
    MMRAG_LATE_MAX_DOC_TOKENS: int = field(default_factory=lambda: int(os.getenv("MMRAG_LATE_MAX_DOC_TOKENS", "0")))
    # answer passages (EmbeddingManager.extract_passages, csrc/maxsim_windows.hip): the window, in passage tokens, whose
    # MaxSim against the question picks the part of a hit that answers it -- a multiple of 16 in 16..512
    MMRAG_PASSAGE_TOKENS: int = field(default_factory=lambda: int(os.getenv("MMRAG_PASSAGE_TOKENS", "64")))
    # token store (late_store.py, csrc/maxsim_scan.hip): with MMRAG_LATE_STORE=1 an upload also keeps the token rows
    # of the stored texts on the device (768 bytes per MiniLM token), so a late re-rank encodes only the question and
    # late_query / POST /query {"late": true} retrieve by exact MaxSim over all of them.  MMRAG_LATE_STORE_MAX_BYTES
    # caps the plane (0 = no cap): past it new rows keep no tokens and are re-encoded by a re-rank
    MMRAG_LATE_STORE: bool = field(default_factory=lambda: os.getenv("MMRAG_LATE_STORE", "0") == "1")
    MMRAG_LATE_STORE_MAX_BYTES: int = field(
        default_factory=lambda: int(os.getenv("MMRAG_LATE_STORE_MAX_BYTES", "0")))
    # the plane's element type: "float16" (default) or "float8_e4m3fn" -- E4M3 codes, half the bytes per token (384 per
    # MiniLM token), scored by the FP8 MaxSim kernels; scores are then the quantised rows' own
    MMRAG_LATE_STORE_DTYPE: str = field(default_factory=lambda: os.getenv("MMRAG_LATE_STORE_DTYPE", "float16"))
    # BM25 lexical leg (VectorIndex.lexical_query / hybrid_query, csrc/lexical.hip): term-frequency saturation k1 and
    # length normalisation b of the score, the same for every query
    MMRAG_BM25_K1: float = field(default_factory=lambda: float(os.getenv("MMRAG_BM25_K1", "1.2")))
    MMRAG_BM25_B: float = field(default_factory=lambda: float(os.getenv("MMRAG_BM25_B", "0.75")))
    # typo tolerance of the lexical leg (csrc/fuzzy.hip): "" (off), "auto" (0 / 1 / 2 edits for terms of 1-2 / 3-5 / 6+
    # code points) or "0", "1", "2".  A query term no live row holds is replaced by its closest indexed term; what a
    # request says about `fuzzy` overrides it
    MMRAG_LEXICAL_FUZZY: str = field(default_factory=lambda: os.getenv("MMRAG_LEXICAL_FUZZY", ""))
    # phrase queries of the lexical leg (csrc/phrase.hip): with MMRAG_LEXICAL_PHRASES=1 a quoted segment of a hybrid
    # query is a phrase every returned chunk must hold; MMRAG_LEXICAL_SLOP (0..16) is how many other tokens may stand
    # between its terms.  What a request says about `phrases` / `slop` overrides them
    MMRAG_LEXICAL_PHRASES: bool = field(default_factory=lambda: os.getenv("MMRAG_LEXICAL_PHRASES", "0") == "1")
    MMRAG_LEXICAL_SLOP: int = field(default_factory=lambda: int(os.getenv("MMRAG_LEXICAL_SLOP", "0")))
    # hybrid retrieval: each leg returns max(n_results, MMRAG_HYBRID_CANDIDATES) hits (at most 4096), fused by
    # reciprocal rank with sum 1 / (MMRAG_HYBRID_RRF_K + rank)
    MMRAG_HYBRID_CANDIDATES: int = field(default_factory=lambda: int(os.getenv("MMRAG_HYBRID_CANDIDATES", "50")))
    MMRAG_HYBRID_RRF_K: int = field(default_factory=lambda: int(os.getenv("MMRAG_HYBRID_RRF_K", "60")))
    # learned sparse retrieval (sparse.py, csrc/sparse_expand.hip, csrc/sparse_score.hip): a LOCAL BertForMaskedLM
    # directory (config.json + model.safetensors + vocab.txt, e.g. a SPLADE checkpoint); empty = nothing is built,
    # stored or loaded.  Documents keep MMRAG_SPARSE_DOC_TERMS terms, questions MMRAG_SPARSE_QUERY_TERMS (at most 64);
    # impacts are min(255, rint(log1p(relu(logit)) * MMRAG_SPARSE_IMPACT_SCALE)).  MMRAG_SPARSE_QUERY_MODE: "expand"
    # (a forward pass on the question) or "tokens" (the question's own word pieces at impact scale: no model forward
    # on the query path)
    MMRAG_SPARSE_ENCODER_DIR: str = field(default_factory=lambda: os.getenv("MMRAG_SPARSE_ENCODER_DIR", ""))
    MMRAG_SPARSE_DOC_TERMS: int = field(default_factory=lambda: int(os.getenv("MMRAG_SPARSE_DOC_TERMS", "128")))
    MMRAG_SPARSE_QUERY_TERMS: int = field(default_factory=lambda: int(os.getenv("MMRAG_SPARSE_QUERY_TERMS", "32")))
    MMRAG_SPARSE_IMPACT_SCALE: float = field(default_factory=lambda: float(os.getenv("MMRAG_SPARSE_IMPACT_SCALE", "64")))
    MMRAG_SPARSE_QUERY_MODE: str = field(default_factory=lambda: os.getenv("MMRAG_SPARSE_QUERY_MODE", "expand"))
    # diversified retrieval (VectorIndex.mmr_query, csrc/mmr.hip): maximal marginal relevance picks n_results of
    # max(n_results, MMRAG_MMR_CANDIDATES) dense hits (at most 1024) with v = lambda rel - (1 - lambda) max sim to the
    # picks so far; lambda = 1 is the plain dense order, 0 pure diversity
    MMRAG_MMR_CANDIDATES: int = field(default_factory=lambda: int(os.getenv("MMRAG_MMR_CANDIDATES", "50")))
    MMRAG_MMR_LAMBDA: float = field(default_factory=lambda: float(os.getenv("MMRAG_MMR_LAMBDA", "0.5")))
    # grouping hits by document (VectorIndex.grouped_query, csrc/group.hip): the first pass groups
    # min(max(MMRAG_GROUP_CANDIDATES, 4 * n_groups * group_size), 4096) dense hits; queries that neither found
    # n_groups groups nor exhausted their list are searched again 4 x deeper, up to 4096
    MMRAG_GROUP_CANDIDATES: int = field(default_factory=lambda: int(os.getenv("MMRAG_GROUP_CANDIDATES", "64")))
    # metadata filters on the device (multimodal_rag_amd/filters.py, csrc/filtered.hip).  "true": a `where` the compiler
    # covers becomes its row bitmap with one kernel launch over typed metadata columns instead of on the host (the words
    # are identical, so every retrieval mode returns what it returned), and the dispatcher batches requests with
    # different filters into one filtered_query.  VectorIndex.filtered_search evaluates at most
    # MMRAG_FILTER_BITMAP_BYTES of bitmaps (distinct filters x 4 * ceil(n / 128) words) per launch; more are served in
    # slices
    MMRAG_DEVICE_FILTERS: bool = field(default_factory=lambda: _b("MMRAG_DEVICE_FILTERS", "false"))
    MMRAG_FILTER_BITMAP_BYTES: int = field(default_factory=lambda: int(os.getenv("MMRAG_FILTER_BITMAP_BYTES",
                                                                                 str(256 << 20))))
    # multi-query retrieval (VectorIndex.fused_query, csrc/fuse.hip): every phrasing of a question returns
    # max(n_results, MMRAG_FUSE_CANDIDATES) hits (at most 256); the lists are fused by MMRAG_FUSE_METHOD: "rrf" = sum of
    # weight / (MMRAG_FUSE_RRF_K + rank), "max" = largest weight * cosine
    MMRAG_FUSE_CANDIDATES: int = field(default_factory=lambda: int(os.getenv("MMRAG_FUSE_CANDIDATES", "50")))
    MMRAG_FUSE_METHOD: str = field(default_factory=lambda: os.getenv("MMRAG_FUSE_METHOD", "rrf"))
    MMRAG_FUSE_RRF_K: int = field(default_factory=lambda: int(os.getenv("MMRAG_FUSE_RRF_K", "60")))
    # near-duplicate detection (VectorIndex.near_duplicates / add(dedup_threshold=...), csrc/simjoin.hip).
    # MMRAG_DEDUP_THRESHOLD: 0 = off (default); above 0 (at most 1) embed_and_store skips a chunk whose cosine to a stored
    # chunk, or to an earlier kept chunk of the same upload, is at least this.  MMRAG_DEDUP_REPORT_THRESHOLD: the default
    # threshold of near_duplicates / drop_duplicates and of the /duplicates routes
    MMRAG_DEDUP_THRESHOLD: float = field(default_factory=lambda: float(os.getenv("MMRAG_DEDUP_THRESHOLD", "0")))
    MMRAG_DEDUP_REPORT_THRESHOLD: float = field(
        default_factory=lambda: float(os.getenv("MMRAG_DEDUP_REPORT_THRESHOLD", "0.98")))
    # boosted retrieval (VectorIndex.boosted_query, csrc/boosted.hip): the defaults of a request's "boost" object.
    # MMRAG_BOOST_RECENCY: the weight of the recency term (0 = none); a non-zero default applies only to a request that
    # asks with "boost": true -- plain requests never change.  MMRAG_BOOST_HALF_LIFE_DAYS: the age at which the recency
    # term has halved.  MMRAG_BOOST_REFRESH_S: a spec's prior column is rebuilt when the clock passes a multiple of this.
    # MMRAG_BOOST_TIME_KEY: a key of an uploaded item that holds its UNIX time ("" = the time of the upload call)
    MMRAG_BOOST_RECENCY: float = field(default_factory=lambda: float(os.getenv("MMRAG_BOOST_RECENCY", "0.0")))
    MMRAG_BOOST_HALF_LIFE_DAYS: float = field(
        default_factory=lambda: float(os.getenv("MMRAG_BOOST_HALF_LIFE_DAYS", "30")))
    MMRAG_BOOST_REFRESH_S: float = field(default_factory=lambda: float(os.getenv("MMRAG_BOOST_REFRESH_S", "3600")))
    MMRAG_BOOST_TIME_KEY: str = field(default_factory=lambda: os.getenv("MMRAG_BOOST_TIME_KEY", ""))
    # recommend retrieval (VectorIndex.recommend_query, csrc/recommend.hip): the default weight w >= 0 of the penalty in
    # final = pos - w * max(neg, 0) when a request names negatives and gives none
    MMRAG_RECOMMEND_NEGATIVE_WEIGHT: float = field(
        default_factory=lambda: float(os.getenv("MMRAG_RECOMMEND_NEGATIVE_WEIGHT", "1.0")))
    # related-document retrieval (VectorIndex.related_query, csrc/related.hip): the scan keeps one 8-byte key per
    # (vector of the sets, stored document); a call whose table would exceed this many bytes is split by whole sets
    # (exact: sets are independent), a single set that exceeds it alone is refused.  A memory budget, not a measurement
    MMRAG_RELATED_TABLE_BYTES: int = field(
        default_factory=lambda: int(os.getenv("MMRAG_RELATED_TABLE_BYTES", str(1 << 30))))
    # range retrieval (VectorIndex.range_query, csrc/range.hip): the scan adds into one 4-byte counter per (query, facet
    # slot: a key's distinct values + 1); a batch whose tables would exceed this many bytes is split by queries (exact:
    # queries are independent), a single query that exceeds it alone is refused.  A memory budget, not a measurement
    MMRAG_RANGE_TABLE_BYTES: int = field(
        default_factory=lambda: int(os.getenv("MMRAG_RANGE_TABLE_BYTES", str(256 << 20))))
    # topic clustering (VectorIndex.cluster, csrc/kmeans.hip): the default number of topics of cluster() / GET /topics;
    # 0 (default) = automatic, auto_topics(live rows); else 1 .. 4096
    MMRAG_TOPICS: int = field(default_factory=lambda: int(os.getenv("MMRAG_TOPICS", "0")))
    # significant terms (VectorIndex.significant_terms, csrc/terms.hip).  MMRAG_TOPIC_TERMS (0..32): the terms each topic
    # of GET /topics carries when the request does not say; 0 (default) = none, and the response is what it was.
    # MMRAG_KEYWORD_MIN_LENGTH (>= 1): the fewest code points of a term that may stand in a topic's terms or a
    # document's keywords
    MMRAG_TOPIC_TERMS: int = field(default_factory=lambda: int(os.getenv("MMRAG_TOPIC_TERMS", "0")))
    MMRAG_KEYWORD_MIN_LENGTH: int = field(default_factory=lambda: int(os.getenv("MMRAG_KEYWORD_MIN_LENGTH", "3")))
    # the summary an upload embeds (summarize.py, csrc/summarize.hip).  MMRAG_SUMMARIZER: "fallback" (default: the
    # chunk's first 300 characters) or "extractive": the chunk's most central sentences -- LexRank centrality over the
    # sentence embeddings, a non-redundant set under the length budget by MMR.  An edge of the sentence graph needs a
    # cosine of at least MMRAG_SUMMARY_EDGE_THRESHOLD; MMRAG_SUMMARY_ALPHA in (0, 1] is the weight of the prior in each
    # of the MMRAG_SUMMARY_ITERATIONS (0..64) steps; MMRAG_SUMMARY_LAMBDA in [0, 1] trades centrality (1) against
    # redundancy (0).  The same settings serve EmbeddingManager.extract_answer (POST /query "extractive_answer")
    MMRAG_SUMMARIZER: str = field(default_factory=lambda: os.getenv("MMRAG_SUMMARIZER", "fallback"))
    MMRAG_SUMMARY_EDGE_THRESHOLD: float = field(
        default_factory=lambda: float(os.getenv("MMRAG_SUMMARY_EDGE_THRESHOLD", "0.1")))
    MMRAG_SUMMARY_ALPHA: float = field(default_factory=lambda: float(os.getenv("MMRAG_SUMMARY_ALPHA", "0.15")))
    MMRAG_SUMMARY_ITERATIONS: int = field(default_factory=lambda: int(os.getenv("MMRAG_SUMMARY_ITERATIONS", "32")))
    MMRAG_SUMMARY_LAMBDA: float = field(default_factory=lambda: float(os.getenv("MMRAG_SUMMARY_LAMBDA", "0.7")))
    # how an upload's text is cut into chunks (chunking.py, csrc/chunk.hip).  MMRAG_CHUNKER: "basic" (default: the
    # sliding CHUNK_SIZE-character window of ingest.basic_chunk_text) or "semantic": sentences are embedded and the
    # text is cut where the topic changes -- the partition of greatest total within-chunk similarity above tau, chunks
    # of at most CHUNK_SIZE characters and MMRAG_CHUNK_MAX_SENTENCES (1..64) sentences.  MMRAG_CHUNK_THRESHOLD: "" (default)
    # = tau is MMRAG_CHUNK_AUTO_SCALE (> 0) times the document's mean adjacent-sentence similarity; a float fixes tau.
    # MMRAG_CHUNK_PENALTY >= 0 is a price per chunk, against slivers.  MMRAG_CHUNK_SEMANTIC_OVERLAP: 1 = each chunk is
    # prefixed with the trailing whole sentences of its predecessor that fit in CHUNK_OVERLAP characters (default 0:
    # none).  The defaults 0.5 and 0.0 are untuned starting points
    MMRAG_CHUNKER: str = field(default_factory=lambda: os.getenv("MMRAG_CHUNKER", "basic"))
    MMRAG_CHUNK_THRESHOLD: str = field(default_factory=lambda: os.getenv("MMRAG_CHUNK_THRESHOLD", ""))
    MMRAG_CHUNK_AUTO_SCALE: float = field(default_factory=lambda: float(os.getenv("MMRAG_CHUNK_AUTO_SCALE", "0.5")))
    MMRAG_CHUNK_PENALTY: float = field(default_factory=lambda: float(os.getenv("MMRAG_CHUNK_PENALTY", "0.0")))
    MMRAG_CHUNK_MAX_SENTENCES: int = field(default_factory=lambda: int(os.getenv("MMRAG_CHUNK_MAX_SENTENCES", "64")))
    MMRAG_CHUNK_SEMANTIC_OVERLAP: int = field(
        default_factory=lambda: int(os.getenv("MMRAG_CHUNK_SEMANTIC_OVERLAP", "0")))
    # answer citations (attribution.py, csrc/attribute.hip): which source stands behind which sentence of an answer, by
    # the bi-encoder's sentence similarity (not entailment).  MMRAG_CITATIONS: the default of POST /query's `citations`
    # flag (0: off).  A sentence is supported, and a source cited, at a cosine of at least MMRAG_CITATION_THRESHOLD, in
    # (-1, 1]; a sentence cites at most MMRAG_CITATION_MAX (1..8) sources.  The default 0.6 is an untuned starting
    # point: it presumes a trained sentence encoder, and with seeded random weights it means nothing
    MMRAG_CITATIONS: int = field(default_factory=lambda: int(os.getenv("MMRAG_CITATIONS", "0")))
    MMRAG_CITATION_THRESHOLD: float = field(
        default_factory=lambda: float(os.getenv("MMRAG_CITATION_THRESHOLD", "0.6")))
    MMRAG_CITATION_MAX: int = field(default_factory=lambda: int(os.getenv("MMRAG_CITATION_MAX", "3")))
    # CLIP engines only: embed image items from their pixels (vision tower) instead of their summary text
    MMRAG_EMBED_IMAGE_PIXELS: bool = field(default_factory=lambda: _b("MMRAG_EMBED_IMAGE_PIXELS", "true"))

    def __post_init__(self):
        self.dedup_threshold()
        self.topics()
        self.rerank_method()
        self.late_store_dtype()
        self.passage_tokens()
        self.summarizer()
        self.lexical_fuzzy()
        self.lexical_slop()
        self.chunker()
        self.topic_terms()
        self.keyword_min_length()
        self.citation_parameters()

    def citation_parameters(self) -> dict:
        """the MMRAG_CITATION* settings as attribution's parameters, checked (the C entry refuses a count out of range
        too, with less to go on); "default": what a request without the `citations` flag gets"""
        on, t, most = self.MMRAG_CITATIONS, self.MMRAG_CITATION_THRESHOLD, self.MMRAG_CITATION_MAX
        if (on not in (0, 1) or isinstance(t, bool) or not isinstance(t, (int, float)) or not -1.0 < float(t) <= 1.0
                or isinstance(most, bool) or not isinstance(most, int) or not 1 <= most <= 8):
            raise ValueError("MMRAG_CITATIONS must be 0 or 1, MMRAG_CITATION_THRESHOLD a cosine in (-1, 1], "
                             f"MMRAG_CITATION_MAX an integer in 1..8 (got {on!r}, {t!r}, {most!r})")
        return {"default": bool(on), "threshold": float(t), "max_citations": most}

    def topic_terms(self) -> int:
        """MMRAG_TOPIC_TERMS checked: an integer in 0..32"""
        t = self.MMRAG_TOPIC_TERMS
        if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t <= 32:
            raise ValueError(f"MMRAG_TOPIC_TERMS must be an integer in 0..32 (got {t!r})")
        return t

    def keyword_min_length(self) -> int:
        """MMRAG_KEYWORD_MIN_LENGTH checked: an integer >= 1"""
        m = self.MMRAG_KEYWORD_MIN_LENGTH
        if isinstance(m, bool) or not isinstance(m, int) or m < 1:
            raise ValueError(f"MMRAG_KEYWORD_MIN_LENGTH must be an integer >= 1 (got {m!r})")
        return m

    def chunker(self) -> str:
        """MMRAG_CHUNKER checked: 'basic' or 'semantic' (tests set the attribute after start-up, so users call this);
        under 'semantic' the MMRAG_CHUNK_* parameters are checked with it"""
        if self.MMRAG_CHUNKER not in ("basic", "semantic"):
            raise ValueError(f"MMRAG_CHUNKER must be 'basic' or 'semantic' (got {self.MMRAG_CHUNKER!r})")
        if self.MMRAG_CHUNKER == "semantic":
            self.chunk_parameters()
        return self.MMRAG_CHUNKER

    def chunk_parameters(self) -> dict:
        """the MMRAG_CHUNK_* settings as the segmentation's parameters, checked (the C entry refuses them too, with
        less to go on): threshold None = tau by auto_scale"""
        text = str(self.MMRAG_CHUNK_THRESHOLD).strip()
        try:
            threshold = float(text) if text else None
        except ValueError:
            threshold = math.nan
        scale, penalty = float(self.MMRAG_CHUNK_AUTO_SCALE), float(self.MMRAG_CHUNK_PENALTY)
        most, overlap = int(self.MMRAG_CHUNK_MAX_SENTENCES), int(self.MMRAG_CHUNK_SEMANTIC_OVERLAP)
        if ((threshold is not None and not math.isfinite(threshold)) or not 0.0 < scale < math.inf
                or not 0.0 <= penalty < math.inf or not 1 <= most <= 64 or overlap not in (0, 1)):
            raise ValueError("MMRAG_CHUNK_THRESHOLD must be empty (auto) or a finite float, MMRAG_CHUNK_AUTO_SCALE "
                             "finite and > 0, MMRAG_CHUNK_PENALTY finite and >= 0, MMRAG_CHUNK_MAX_SENTENCES in 1..64, "
                             f"MMRAG_CHUNK_SEMANTIC_OVERLAP 0 or 1 (got {self.MMRAG_CHUNK_THRESHOLD!r}, {scale}, "
                             f"{penalty}, {most}, {overlap})")
        return {"threshold": threshold, "auto_scale": scale, "penalty": penalty, "max_sentences": most,
                "overlap": self.CHUNK_OVERLAP if overlap else 0}

    def lexical_fuzzy(self) -> str:
        """MMRAG_LEXICAL_FUZZY checked: '', 'auto', '0', '1' or '2'"""
        if self.MMRAG_LEXICAL_FUZZY not in ("", "auto", "0", "1", "2"):
            raise ValueError(f"MMRAG_LEXICAL_FUZZY must be '' (off), 'auto', '0', '1' or '2' "
                             f"(got {self.MMRAG_LEXICAL_FUZZY!r})")
        return self.MMRAG_LEXICAL_FUZZY

    def lexical_slop(self) -> int:
        """MMRAG_LEXICAL_SLOP checked: an integer in 0..16 (MMRAG_MAX_PHRASE_SLOP)"""
        slop = self.MMRAG_LEXICAL_SLOP
        if isinstance(slop, bool) or not isinstance(slop, int) or not 0 <= slop <= 16:
            raise ValueError(f"MMRAG_LEXICAL_SLOP must be an integer in 0..16 (got {slop!r})")
        return slop

    def summarizer(self) -> str:
        """MMRAG_SUMMARIZER checked: 'fallback' or 'extractive' (tests set the attribute after start-up, so users call
        this)"""
        if self.MMRAG_SUMMARIZER not in ("fallback", "extractive"):
            raise ValueError(f"MMRAG_SUMMARIZER must be 'fallback' or 'extractive' (got {self.MMRAG_SUMMARIZER!r})")
        return self.MMRAG_SUMMARIZER

    def dedup_threshold(self) -> float:
        """MMRAG_DEDUP_THRESHOLD checked: 0 (off) or a cosine in (0, 1]"""
        t = float(self.MMRAG_DEDUP_THRESHOLD)
        if not 0.0 <= t <= 1.0:     # false for NaN too
            raise ValueError(f"MMRAG_DEDUP_THRESHOLD must be 0 (off) or a cosine in (0, 1] (got {self.MMRAG_DEDUP_THRESHOLD!r})")
        return t

    def rerank_method(self) -> str:
        """MMRAG_RERANK_METHOD checked: 'cross' or 'late' (tests set the attribute after start-up, so users call this)"""
        if self.MMRAG_RERANK_METHOD not in ("cross", "late"):
            raise ValueError(f"MMRAG_RERANK_METHOD must be 'cross' or 'late' (got {self.MMRAG_RERANK_METHOD!r})")
        return self.MMRAG_RERANK_METHOD

    def passage_tokens(self) -> int:
        """MMRAG_PASSAGE_TOKENS checked: a multiple of 16 in 16..512"""
        n = int(self.MMRAG_PASSAGE_TOKENS)
        if not 16 <= n <= 512 or n % 16:
            raise ValueError(f"MMRAG_PASSAGE_TOKENS must be a multiple of 16 in 16..512 (got {n})")
        return n

    def late_store_dtype(self) -> str:
        """MMRAG_LATE_STORE_DTYPE checked: 'float16' or 'float8_e4m3fn'"""
        if self.MMRAG_LATE_STORE_DTYPE not in ("float16", "float8_e4m3fn"):
            raise ValueError("MMRAG_LATE_STORE_DTYPE must be 'float16' or 'float8_e4m3fn' "
                             f"(got {self.MMRAG_LATE_STORE_DTYPE!r})")
        return self.MMRAG_LATE_STORE_DTYPE

    def topics(self) -> int:
        """MMRAG_TOPICS checked: 0 (automatic) or a cluster count in 1 .. 4096"""
        k = int(self.MMRAG_TOPICS)
        if not 0 <= k <= 4096:
            raise ValueError(f"MMRAG_TOPICS must be 0 (automatic) or in 1..4096 (got {self.MMRAG_TOPICS!r})")
        return k

    def index_dtype(self):
        """MMRAG_INDEX_DTYPE as a torch dtype"""
        import torch

        names = {"float16": torch.float16, "float32": torch.float32, "bfloat16": torch.bfloat16,
                 "float8_e4m3fn": torch.float8_e4m3fn}
        if self.MMRAG_INDEX_DTYPE not in names:
            raise ValueError(f"MMRAG_INDEX_DTYPE must be one of {sorted(names)} (got {self.MMRAG_INDEX_DTYPE!r})")
        return names[self.MMRAG_INDEX_DTYPE]

    def f8_rescore_dtype(self):
        """MMRAG_F8_RESCORE as a torch dtype, None for "none" (capacity mode)"""
        import torch

        names = {"float16": torch.float16, "float32": torch.float32, "bfloat16": torch.bfloat16, "none": None}
        key = self.MMRAG_F8_RESCORE.lower()
        if key not in names:
            raise ValueError(f"MMRAG_F8_RESCORE must be one of {sorted(names)} (got {self.MMRAG_F8_RESCORE!r})")
        return names[key]


def auto_topics(live: int) -> int:
    """the automatic number of topics of `live` rows (MMRAG_TOPICS=0): min(256, max(2, round(sqrt(live / 2)))), halves up"""
    return min(256, max(2, int(math.floor(math.sqrt(max(int(live), 0) / 2.0) + 0.5))))


settings = Settings()
