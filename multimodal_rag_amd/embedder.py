"""`EmbeddingManager`: the reference's app/utils/embedder.py surface over the MI355X engines.

Class names, constructor and method signatures, return shapes, statistics keys, messages and the retry / error
conventions are the reference's (each method names the lines it answers to).  The bodies are this package's own:
vectors travel as numpy matrices between the encoder and the collection (Python float lists exist only where a
signature returns them), every engine call goes through one retry helper, and both caches are one LRU class.

    reference                               here
    SentenceTransformer(...).encode    ->   DeviceEncoder (HIP kernels, libmmrag.so)            engines.HipEngine
    chromadb collection (HNSW, CPU)    ->   VectorIndex  (fused MFMA GEMM + exact top-k, HBM)   index.VectorIndex

Deliberate differences:
  * no "CUDA OOM -> fall back to CPU" path (embedder.py:231-243, :407-426): there is no second backend, an
    out-of-memory error propagates;
  * `batch_query` embeds the whole list in one pass and runs ONE [B, d] x [N, d]^T search instead of N concurrent
    single queries (embedder.py:808-815); same result list, per-query failures still become dicts carrying 'error';
  * distances are cosine distances (1 - cos), the space of the collection the reference committed;
  * `get_stats()` exists because api.py:472 calls it.
"""
from __future__ import annotations

import asyncio
import copy
import hashlib
import logging
import math
import threading
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import tracing
from ._native import MAX_RECOMMEND_EXAMPLES, MAX_RELATED_ROWS
from .config import settings
from .engines import CLIP_MODEL_NAMES, ClipEngine, HipEngine, _is_clip_dir, load_item_image  # noqa: F401 (re-exported)
from .hostutil import CountingLRU, call_with_retry, load_hostrows

logger = logging.getLogger(__name__)

ITEM_KINDS = ("text", "table", "image")           # the kinds embed_and_store counts (embedder.py:477-479)
RESULT_KEYS = ("ids", "distances", "metadatas", "documents")
CHUNK_SPAN_KEYS = ("char_start", "char_end", "sentence_count", "chunker")   # a semantic chunk's stored metadata
HYBRID_KEYS = RESULT_KEYS + ("hybrid_scores", "lexical_scores")
MMR_KEYS = RESULT_KEYS + ("mmr_scores",)
LATE_KEYS = RESULT_KEYS + ("late_scores",)
SPARSE_KEYS = RESULT_KEYS + ("sparse_scores",)
SPARSE_HYBRID_KEYS = RESULT_KEYS + ("hybrid_scores", "sparse_scores")
FUSED_KEYS = RESULT_KEYS + ("fused_scores", "matched_queries", "best_query")
BOOST_KEYS = RESULT_KEYS + ("scores", "boosts")
RECOMMEND_KEYS = RESULT_KEYS + ("scores", "penalties", "matched", "repelled_by")
RANGE_KEYS = RESULT_KEYS + ("total", "truncated", "facets")
_HOSTROWS = load_hostrows()
_COLLECTION_NOTE = {"description": "Multi-modal RAG embeddings"}
# what a retrieval mode needs of the collection: (method, the error of a collection that lacks it)
_NEEDS_HYBRID = ("hybrid_query", "hybrid retrieval needs a single-GPU collection (VectorIndex)")
_NEEDS_MMR = ("mmr_query", "MMR retrieval needs a single-GPU collection (VectorIndex)")
_NEEDS_MULTI = ("fused_query", "multi-query retrieval needs a single-GPU collection (VectorIndex)")
_NEEDS_GROUPING = ("grouped_query", "grouped retrieval needs a single-GPU collection (VectorIndex)")
_NEEDS_DEDUP = ("near_duplicates", "near-duplicate detection needs a single-GPU collection (VectorIndex) with "
                                   "full-precision rows")
_NEEDS_CLUSTERING = ("cluster", "topic clustering needs a single-GPU collection (VectorIndex) with full-precision rows")
_NEEDS_TERMS = ("significant_terms", "significant terms need a single-GPU collection (VectorIndex) with stored documents")
_NEEDS_BOOST = ("boosted_query", "boosted retrieval needs a single-GPU collection (VectorIndex) with full-precision "
                                 "rows")
_NEEDS_RECOMMEND = ("recommend_query", "recommend retrieval needs a single-GPU collection (VectorIndex) with "
                                        "full-precision rows")
_NEEDS_RELATED = ("related_query", "related-document retrieval needs a single-GPU collection (VectorIndex) with "
                                   "full-precision rows")
_NEEDS_RANGE = ("range_query", "range retrieval needs a single-GPU collection (VectorIndex) with full-precision rows")
_NEEDS_SPARSE = ("sparse_query", "learned sparse retrieval needs a single-GPU collection (VectorIndex) and a sparse "
                                  "encoder (MMRAG_SPARSE_ENCODER_DIR, or EmbeddingManager.enable_sparse)")
_sparse_warned = False   # "MMRAG_SPARSE_ENCODER_DIR is set but this collection cannot keep sparse vectors": once per process
_NEEDS_LATE = ("late_query", "late retrieval needs a single-GPU collection (VectorIndex) with a token store")
_late_store_warned = False   # "MMRAG_LATE_STORE is set but this embedder cannot keep token rows": once per process
_boost_warned = False   # "this collection cannot boost": once per process
_dedup_warned = False    # "MMRAG_DEDUP_THRESHOLD is set but this collection cannot de-duplicate": once per process
# the answer of a batch's query that could not be answered, before its 'error' (copied for every such query)
_EMPTY = {key: [] for key in RESULT_KEYS}
_EMPTY_MMR = {key: [] for key in MMR_KEYS}
_EMPTY_LATE = {key: [] for key in LATE_KEYS}
_EMPTY_SPARSE = {key: [] for key in SPARSE_KEYS}
_EMPTY_FUSED = {key: [] for key in FUSED_KEYS}
_EMPTY_BOOST = {key: [] for key in BOOST_KEYS}
_EMPTY_RECOMMEND = {key: [] for key in RECOMMEND_KEYS}
_EMPTY_RANGE = {**_EMPTY, "total": 0, "truncated": False, "facets": {}}
_EMPTY_GROUPED = {**_EMPTY, "groups": [], "exhaustive": False, "fetch_k": 0}


class LRUCache(CountingLRU):
    """text -> embedding cache (embedder.py:26-80: maxsize 1000, hit/miss counters, hit rate rounded to 3 places)"""

    def __init__(self, maxsize: int = 1000):
        super().__init__(maxsize)


class EmbeddingManager:
    """embedder.py:83-930."""

    def __init__(self, batch_size: int = 32, enable_cache: bool = True, cache_size: int = 1000,
                 device: Optional[str] = None, max_retries: int = 3, enable_progress_logging: bool = True,
                 *, engine: Any = None):
        self.batch_size = batch_size
        self.enable_cache = enable_cache
        self.max_retries = max_retries
        self.enable_progress_logging = enable_progress_logging
        self.device = device
        self.client = None
        self.collection = None
        self.text_model = None
        self.is_initialized = False
        self.cache = LRUCache(maxsize=cache_size) if enable_cache else None
        self.stats = dict.fromkeys(("total_embeddings_created", "total_items_stored", "total_queries", "cache_hits",
                                    "cache_misses"), 0)
        self._engine = engine
        self._dispatcher = None
        self._encode_lock = asyncio.Lock()       # one encoder pass at a time from this event loop
        self._sleep = asyncio.sleep              # (tests swap the back-off sleep out)
        self._reranker = None                    # cross-encoder (MMRAG_RERANKER_DIR), loaded on first use
        self._reranker_lock = threading.Lock()
        self._reader = None                      # extractive reader (MMRAG_READER_DIR), loaded on first use
        self._late = None                        # late.LateInteractionScorer over the engine's own encoder, on first use
        self._sparse = None                      # sparse.DeviceSparseEncoder (MMRAG_SPARSE_ENCODER_DIR), on first use
        self._sparse_lock = threading.Lock()

    # ------------------------------------------------------------------ lifecycle -----------
    async def initialize(self):
        """embedder.py:152-248: bring up the model and the collection (idempotent)."""
        if self.is_initialized:
            return
        try:
            if self._engine is None:
                name = settings.SENTENCE_TRANSFORMER_MODEL
                joint = name in CLIP_MODEL_NAMES or _is_clip_dir(settings.MMRAG_MODEL_DIR)
                self._engine = await asyncio.to_thread(ClipEngine if joint else HipEngine, name, self.device)
            self.text_model = self.client = self._engine
            self.device = getattr(self._engine, "device_name", self.device or "cuda")
            self.collection = self._engine.new_collection(settings.CHROMA_COLLECTION_NAME, dict(_COLLECTION_NOTE))
            if settings.MMRAG_PERSIST:
                self._restore_collection()
            self.is_initialized = True
            logger.info("EmbeddingManager initialized (device=%s, dim=%d)", self.device, self.get_embedding_dimension())
        except Exception as e:
            logger.error("Failed to initialize EmbeddingManager: %s", e, exc_info=True)
            raise

    async def _ready(self):
        if not self.is_initialized:
            await self.initialize()

    def _persist_dir(self) -> str:
        import os

        return os.path.join(settings.CHROMA_PERSIST_DIR, "mmrag_index")

    def _restore_collection(self):
        """MMRAG_PERSIST: pick up what the last cleanup() saved (a collection with load(), or a VectorIndex directory)"""
        import os

        where = self._persist_dir()
        if not os.path.isdir(where):
            return
        if hasattr(self.collection, "load"):                 # serving.ShardedCollection
            self.collection.load(where)
        elif os.path.exists(os.path.join(where, "tables.json")):
            from .persistence import load_index

            self.collection = load_index(where, device=str(getattr(self.collection, "device", "cuda:0")))
        logger.info("Restored %d rows from %s", self.collection.count(), where)

    def _save_collection(self):
        import os

        where = self._persist_dir()
        os.makedirs(where, exist_ok=True)
        if hasattr(self.collection, "save"):
            self.collection.save(where)
        elif hasattr(self.collection, "matrix"):
            from .persistence import save_index

            save_index(self.collection, where)

    async def cleanup(self):
        """embedder.py:250-264."""
        if settings.MMRAG_PERSIST and self.collection is not None:
            try:
                await asyncio.to_thread(self._save_collection)
            except Exception as e:   # noqa: BLE001 -- shutting down: report, do not mask the shutdown
                logger.error("Could not save the collection: %s", e)
        if self._dispatcher is not None:
            await self._dispatcher.stop()
            self._dispatcher = None
        release = getattr(self._engine, "release", None)
        if release is not None:
            release()
        self.client = self.collection = self.text_model = None
        self.is_initialized = False
        if self.cache:
            self.cache.clear()

    def _engine_call(self, what: str, fn, *args, **kwargs):
        return call_with_retry(what, fn, *args, attempts=self.max_retries, sleep=self._sleep, log=logger, **kwargs)

    # ------------------------------------------------------------------ embed ---------------
    def _get_cache_key(self, text: str) -> str:
        """embedder.py:736-742."""
        return hashlib.md5(text.encode("utf-8")).hexdigest()

    def _lookup(self, texts: Sequence[str]):
        """cache pass over `texts`: (rows with the hits filled in, positions still to encode, their cache keys).
        A cached value of length 0 counts as a miss, as the reference's truthiness test does (embedder.py:306)."""
        rows: List[Optional[np.ndarray]] = [None] * len(texts)
        todo: List[int] = []
        keys: Dict[int, str] = {}
        for at, text in enumerate(texts):
            if self.cache:
                keys[at] = self._get_cache_key(text)
                seen = self.cache.get(keys[at])
                if seen is not None and len(seen):
                    rows[at] = np.asarray(seen, dtype=np.float32)
                    continue
            todo.append(at)
        return rows, todo, keys

    def _encode_into(self, texts: Sequence[str], rows, part: List[int], keys: Dict[int, str]):
        """one encoder pass (blocking): the texts at positions `part` -> their rows, and into the cache"""
        fresh = np.asarray(self.text_model.encode([texts[at] for at in part]), dtype=np.float32)
        for at, row in zip(part, fresh):
            rows[at] = row
            if self.cache:
                self.cache.put(keys[at], row)

    def _stack(self, rows, n_new: int) -> np.ndarray:
        self.stats["total_embeddings_created"] += n_new
        if self.cache:
            self.stats["cache_hits"], self.stats["cache_misses"] = self.cache.hits, self.cache.misses
        if not rows:
            return np.zeros((0, self.get_embedding_dimension()), dtype=np.float32)
        return np.stack(rows)

    async def _embed_matrix(self, texts: Sequence[str], rows_per_pass: int) -> np.ndarray:
        """[len(texts), dim] float32: cached rows reused, the rest encoded `rows_per_pass` texts at a time (each pass
        in a worker thread), every row at its text's position (embedder.py:301-332 partitions, encodes the misses,
        caches them, restores the order)."""
        rows, todo, keys = self._lookup(texts)
        step = max(1, rows_per_pass)
        for lo in range(0, len(todo), step):
            async with self._encode_lock:
                await asyncio.to_thread(self._encode_into, texts, rows, todo[lo: lo + step], keys)
        return self._stack(rows, len(todo))

    async def embed_texts_batch(self, texts: List[str], show_progress: bool = None) -> List[List[float]]:
        """embedder.py:266-383: lists of Python floats, input order, misses encoded in slices of `batch_size`."""
        await self._ready()
        if not texts:
            return []
        loud = (len(texts) > 100 and self.enable_progress_logging) if show_progress is None else show_progress
        if loud:
            logger.info("Creating embeddings for %d texts...", len(texts))
        before = self.stats["total_embeddings_created"]
        matrix = await self._embed_matrix(texts, self.batch_size)
        if loud:
            made = self.stats["total_embeddings_created"] - before
            logger.info("Created %d new embeddings, %d from cache", made, len(texts) - made)
        return matrix.tolist()

    # ------------------------------------------------------------------ store ---------------
    async def embed_and_store(self, summaries: List[Dict[str, Any]], doc_id: str) -> Dict[str, int]:
        """embedder.py:428-500: embed every item's `summary`, store it under f"{doc_id}_{item id}"."""
        await self._ready()
        counts = dict.fromkeys(ITEM_KINDS, 0)
        if not summaries:
            logger.warning("No summaries provided for embedding")
            return counts
        t0 = time.time()
        texts = [item["summary"] for item in summaries]
        ids = [f"{doc_id}_{item['id']}" for item in summaries]
        metas = [{"doc_id": doc_id, "item_id": item["id"], "type": item["type"]} for item in summaries]
        for item, meta in zip(summaries, metas):
            if item["type"] in counts:           # other kinds are stored but not counted (:477-479)
                counts[item["type"]] += 1
            found = item.get("metadata") or {}
            if found.get("chunker"):             # a semantic chunk (chunking.py) is stored with where it lies in its text
                meta.update({key: found[key] for key in CHUNK_SPAN_KEYS if key in found})
        joint = hasattr(self._engine, "encode_images")
        # when the rows were added (what a recency boost reads): the time of this call, or each item's own UNIX time
        # under MMRAG_BOOST_TIME_KEY; kept beside the rows, never in their metadata
        extra = {}
        if hasattr(self.collection, "boosted_query"):
            extra["timestamps"] = self._item_times(summaries, t0)
        dedup = settings.dedup_threshold()
        if dedup > 0 and not self.supports_dedup():
            global _dedup_warned
            if not _dedup_warned:
                _dedup_warned = True
                logger.warning("MMRAG_DEDUP_THRESHOLD=%s is ignored: %s", dedup, _NEEDS_DEDUP[1])
            dedup = 0.0
        skipped = None
        if getattr(self.collection, "encode_fn", None) is not None and not joint:
            # multi-GPU serving loop with an encoder on every rank: ship the strings, each rank embeds and stores the
            # items it owns (serving.ShardedCollection.add_texts) -- no vector leaves its GPU
            await asyncio.to_thread(self.collection.add_texts, texts, documents=texts, metadatas=metas, ids=ids)
        else:
            matrix = await self._embed_matrix(texts, self.batch_size)
            if joint and settings.MMRAG_EMBED_IMAGE_PIXELS:
                # joint-space engines (CLIP, BASELINE config 4): image items are embedded from their pixels
                pixels = {at: load_item_image(item) for at, item in enumerate(summaries) if item.get("type") == "image"}
                pixels = {at: px for at, px in pixels.items() if px is not None}
                if pixels:
                    async with self._encode_lock:
                        vecs = await asyncio.to_thread(self._engine.encode_images, list(pixels.values()))
                    matrix[list(pixels)] = np.asarray(vecs, dtype=np.float32)
            if dedup > 0:
                done = await self._engine_call("Store", self.collection.add, embeddings=matrix, documents=texts,
                                               metadatas=metas, ids=ids, dedup_threshold=dedup, **extra)
                skipped = len(done["skipped"])
                counts["duplicates_skipped"] = skipped     # the per-kind counts keep counting items processed
            else:
                await self._store_with_retry(embeddings=matrix, documents=texts, metadatas=metas, ids=ids, **extra)
        if settings.MMRAG_LATE_STORE:
            if self.supports_late_store():
                await asyncio.to_thread(self._store_tokens, ids, texts)
            else:
                global _late_store_warned
                if not _late_store_warned:
                    _late_store_warned = True
                    logger.warning("MMRAG_LATE_STORE=1 is ignored: the token store needs a single BERT-family fp16 HIP "
                                   "engine with a tokenizer and a single-GPU collection")
        if self.has_sparse_encoder():
            if self.supports_sparse():
                await asyncio.to_thread(self._store_sparse, ids, texts)
            else:
                global _sparse_warned
                if not _sparse_warned:
                    _sparse_warned = True
                    logger.warning("MMRAG_SPARSE_ENCODER_DIR is ignored: %s", _NEEDS_SPARSE[1])
        if skipped:
            logger.info("Skipped %d near-duplicate items of doc %s (cosine >= %s)", skipped, doc_id, dedup)
        self.stats["total_items_stored"] += len(summaries)
        logger.info("Stored %d embeddings for doc %s (text: %d, table: %d, image: %d) in %.2fs", len(summaries), doc_id,
                    counts["text"], counts["table"], counts["image"], time.time() - t0)
        return counts

    async def _store_with_retry(self, embeddings, documents, metadatas, ids, **extra):
        """embedder.py:502-537."""
        await self._engine_call("Store", self.collection.add, embeddings=embeddings, documents=documents,
                                metadatas=metadatas, ids=ids, **extra)

    @staticmethod
    def _item_times(summaries: List[Dict[str, Any]], call_time: float) -> List[float]:
        """each item's add time: its own finite UNIX time under MMRAG_BOOST_TIME_KEY when that is set, else call_time"""
        key = settings.MMRAG_BOOST_TIME_KEY
        times = []
        for item in summaries:
            t = item.get(key) if key else None
            if t is None and key and isinstance(item.get("metadata"), dict):
                t = item["metadata"].get(key)
            ok = isinstance(t, (int, float)) and not isinstance(t, bool) and math.isfinite(t)
            times.append(float(t) if ok else call_time)
        return times

    # ------------------------------------------------------------------ query ---------------
    def enable_dynamic_batching(self, max_batch: int = 256, max_wait_ms: float = 2.0):
        """Route query() through a micro-batching dispatcher (not in the reference): concurrent single
        queries are served by one batched encode + one batched search."""
        from .dispatcher import QueryDispatcher

        def scoped(texts, n_results, doc_ids_per_query):      # the dispatcher's (texts, k, documents) order
            return self.batch_scoped_query(texts, doc_ids_per_query, n_results=n_results)

        def filtered(texts, n_results, filters):              # the dispatcher's (texts, k, filters) order
            return self.batch_filtered_query(texts, filters, n_results=n_results)

        def boosted(texts, n_results, filter_dict, spec):
            return self.batch_boosted_query(texts, n_results=n_results, filter_dict=filter_dict, boost=spec)

        def sparse(texts, n_results, filter_dict):
            return self.batch_sparse_query(texts, n_results=n_results, filter_dict=filter_dict)

        def recommend(requests, n_results, filter_dict):      # a failing engine raises: only a request's own fault
            return self.batch_recommend(requests, n_results=n_results, filter_dict=filter_dict,     # is an 'error'
                                        raise_engine_errors=True)

        self._dispatcher = QueryDispatcher(self.batch_query, max_batch=max_batch, max_wait_ms=max_wait_ms,
                                           scoped_fn=scoped if self.supports_scoped() else None,
                                           boosted_fn=boosted if self.supports_boost() else None,
                                           recommend_fn=recommend if self.supports_recommend() else None,
                                           sparse_fn=sparse if self.has_sparse_encoder() and self.supports_sparse()
                                           else None,
                                           filtered_fn=filtered if (settings.MMRAG_DEVICE_FILTERS
                                                                    and self.supports_device_filters()) else None)
        return self._dispatcher

    _INCLUDE = ["metadatas", "documents", "distances"]

    @staticmethod
    def _split(res: Dict[str, Any], n: int) -> List[Dict[str, Any]]:
        """collection.query's lists of lists -> one dict per query (embedder.py:604-609)"""
        cols = [res[key] if res.get(key) else [[] for _ in range(n)] for key in RESULT_KEYS]
        if _HOSTROWS is not None and all(type(col) is list and len(col) == n for col in cols):
            return _HOSTROWS.split(RESULT_KEYS, tuple(cols))
        return [dict(zip(RESULT_KEYS, per_query)) for per_query in zip(*(col[:n] for col in cols))]

    def _embed(self, texts: Sequence[str], looked=None) -> np.ndarray:
        """blocking: [len(texts), dim] float32, cached rows reused and ONE encoder pass for the misses (`looked`: the
        _lookup(texts) the caller already made)"""
        rows, todo, keys = looked or self._lookup(texts)
        if todo:
            self._encode_into(texts, rows, todo, keys)
        return self._stack(rows, len(todo))

    def _answer(self, texts: Sequence[str], n_results: int, filter_dict: Optional[Dict]) -> List[Dict[str, Any]]:
        """Blocking, runs in ONE worker thread: cache lookups, ONE encoder pass for the misses, ONE collection.query
        for all of them (embedder.py:566 + :595-601).  One thread hop per request instead of one per stage."""
        rows, todo, keys = looked = self._lookup(texts)
        if (len(todo) == len(texts) and texts and hasattr(self.text_model, "encode_device")
                and getattr(self.collection, "accepts_device_queries", False)):
            # nothing cached: the embeddings go from the encoder to the search kernel on the device; the host does not
            # wait in between and reads them back (for the cache) only after the answer is there
            dev = self.text_model.encode_device(list(texts))
            res = self.collection.query(query_embeddings=dev, n_results=n_results, where=filter_dict,
                                        include=self._INCLUDE, check_norm=False)
            if self.cache:
                for at, row in zip(todo, dev.cpu().numpy()):
                    self.cache.put(keys[at], row)
            self._stack([], len(todo))
            with tracing.stage("split"):
                return self._split(res, len(texts))
        res = self.collection.query(query_embeddings=self._embed(texts, looked), n_results=n_results,
                                    where=filter_dict, include=self._INCLUDE)
        return self._split(res, len(texts))

    async def _query_with_retry(self, query_embedding: List[float], n_results: int,
                                filter_dict: Optional[Dict]) -> Dict[str, Any]:
        """embedder.py:585-617: search for one ready-made vector."""
        matrix = np.asarray([query_embedding], dtype=np.float32)
        res = await self._engine_call("Query", self.collection.query, query_embeddings=matrix, n_results=n_results,
                                      where=filter_dict, include=self._INCLUDE)
        return self._split(res, 1)[0]

    async def _single(self, label: str, needs, answer, query_text: str, *args, dispatched: bool = False):
        """One query of any mode: the checks in the reference's order (embedder.py:539-583), then `answer([query_text],
        *args)[0]` through the retry helper.  `needs`: None or (collection method, message when it is missing);
        `dispatched`: hand the query to the dynamic-batching dispatcher when there is one."""
        await self._ready()
        if not query_text or not query_text.strip():
            raise ValueError("Query text cannot be empty")
        if needs and not hasattr(self.collection, needs[0]):
            raise ValueError(needs[1])
        if dispatched and self._dispatcher is not None:
            return await self._dispatcher.submit(query_text, *args)
        try:
            hit = (await self._engine_call(label, answer, [query_text], *args))[0]
        except Exception as e:
            logger.error(label + " failed: %s", e, exc_info=True)
            raise
        self.stats["total_queries"] += 1
        return hit

    async def _batch(self, label: str, needs, empty: Dict[str, Any], answer, queries: List[str],
                     *args) -> List[Dict[str, Any]]:
        """A list of queries of any mode (embedder.py:784-832): ONE `answer(live queries, *args)` call; a query that
        cannot be answered -- empty, or all of them when the call or a capability (`needs`, as in _single) fails --
        gets a copy of `empty` with the reason under 'error' instead of an exception (:817-830)."""
        await self._ready()

        def failed(why: str) -> Dict[str, Any]:
            return {**copy.deepcopy(empty), "error": why}

        answers: List[Optional[Dict[str, Any]]] = [None] * len(queries)
        live = [at for at, q in enumerate(queries) if q and q.strip()]
        for at in set(range(len(queries))) - set(live):
            answers[at] = failed("Query text cannot be empty")
        if live:
            try:
                if needs and not hasattr(self.collection, needs[0]):
                    raise ValueError(needs[1])
                hits = await self._engine_call(label, answer, [queries[at] for at in live], *args)
                for at, hit in zip(live, hits):
                    answers[at] = hit
                self.stats["total_queries"] += len(live)
            except Exception as e:
                logger.error(label + " failed: %s", e)
                for at in live:
                    answers[at] = failed(str(e))
        return answers  # type: ignore[return-value]

    async def query(self, query_text: str, n_results: int = 5, filter_dict: Optional[Dict] = None) -> Dict[str, Any]:
        """embedder.py:539-583."""
        return await self._single("Query", None, self._answer, query_text, n_results, filter_dict, dispatched=True)

    def supports_scoped(self) -> bool:
        """True when ONE search serves a batch whose queries each name their own documents (VectorIndex.scoped_query; a
        float8_e4m3fn collection needs its re-scoring plane).  Any other collection still answers scoped_query, by one
        filtered search per distinct set of documents."""
        return self.collection is None or (hasattr(self.collection, "scoped_query") and self._has_full_rows())

    def _answer_scoped(self, texts: Sequence[str], n_results: int,
                       doc_ids_per_query: Sequence[Sequence[str]]) -> List[Dict[str, Any]]:
        """blocking, one worker thread: cached or fresh embeddings (ONE encoder pass for the misses), then ONE
        collection.scoped_query for all of them; a collection without it (sharded) is asked once per distinct scope
        with the scope as a `where` filter"""
        emb = self._embed(texts)
        if hasattr(self.collection, "scoped_query") and self._has_full_rows():
            res = self.collection.scoped_query(emb, n_results=n_results, scopes=[list(ids) for ids in doc_ids_per_query],
                                               include=self._INCLUDE)
            return self._split(res, len(texts))
        by_scope: Dict[Tuple[str, ...], List[int]] = {}
        for at, ids in enumerate(doc_ids_per_query):
            by_scope.setdefault(tuple(ids), []).append(at)
        out: List[Optional[Dict[str, Any]]] = [None] * len(texts)
        for ids, mine in by_scope.items():
            res = self.collection.query(query_embeddings=emb[mine], n_results=n_results,
                                        where={"doc_id": {"$in": list(ids)}}, include=self._INCLUDE)
            for at, hit in zip(mine, self._split(res, len(mine))):
                out[at] = hit
        return out  # type: ignore[return-value]

    async def scoped_query(self, query_text: str, doc_ids: Sequence[str], n_results: int = 5) -> Dict[str, Any]:
        """query() answered from the documents `doc_ids` only: the result dict of query().  Unknown ids match nothing
        (empty lists).  Same empty-query error, embedding cache and query count as query(); with dynamic batching on,
        concurrent callers share one encode and one scoped search whatever their documents."""
        if self._dispatcher is not None:
            await self._ready()
            if not query_text or not query_text.strip():
                raise ValueError("Query text cannot be empty")
            return await self._dispatcher.submit(query_text, n_results, None, list(doc_ids))
        return await self._single("Scoped query", None, self._answer_scoped, query_text, n_results, [list(doc_ids)])

    async def batch_scoped_query(self, queries: List[str], doc_ids_per_query: Sequence[Sequence[str]],
                                 n_results: int = 5) -> List[Dict[str, Any]]:
        """batch_query's twin for scoped_query: query i is answered from the documents doc_ids_per_query[i]; one batched
        encode and one search for all of them; a query that cannot be answered gets a dict with empty lists and an
        'error' message."""
        if len(doc_ids_per_query) != len(queries):
            raise ValueError(f"{len(doc_ids_per_query)} document lists for {len(queries)} queries")
        live = [list(ids) for q, ids in zip(queries, doc_ids_per_query) if q and q.strip()]    # as _batch picks them
        return await self._batch("Batch scoped query", None, _EMPTY, self._answer_scoped, queries, n_results, live)

    def supports_device_filters(self) -> bool:
        """True when ONE search serves a batch whose queries each carry their own metadata filter, evaluated on the
        device (VectorIndex.filtered_query; a float8_e4m3fn collection needs its re-scoring plane).  Any other
        collection still answers batch_filtered_query, by one filtered search per distinct filter."""
        return self.collection is None or (hasattr(self.collection, "filtered_query") and self._has_full_rows())

    def _answer_filtered(self, texts: Sequence[str], n_results: int,
                         filters: Sequence[Optional[Dict]]) -> List[Dict[str, Any]]:
        """blocking, one worker thread: cached or fresh embeddings (ONE encoder pass for the misses), then ONE
        collection.filtered_query for all of them; a collection without it is asked once per distinct filter"""
        emb = self._embed(texts)
        if hasattr(self.collection, "filtered_query") and self._has_full_rows():
            res = self.collection.filtered_query(emb, n_results=n_results, wheres=list(filters), include=self._INCLUDE)
            return self._split(res, len(texts))
        by_filter: Dict[str, List[int]] = {}
        for at, flt in enumerate(filters):
            by_filter.setdefault(repr(flt), []).append(at)
        out: List[Optional[Dict[str, Any]]] = [None] * len(texts)
        for mine in by_filter.values():
            res = self.collection.query(query_embeddings=emb[mine], n_results=n_results, where=filters[mine[0]],
                                        include=self._INCLUDE)
            for at, hit in zip(mine, self._split(res, len(mine))):
                out[at] = hit
        return out  # type: ignore[return-value]

    async def batch_filtered_query(self, queries: List[str], filters: Sequence[Optional[Dict]],
                                   n_results: int = 5) -> List[Dict[str, Any]]:
        """batch_scoped_query's twin for metadata filters: query i is answered from the rows that match filters[i] (None
        = every row); one batched encode and one search for all of them whatever the filters; a query that cannot be
        answered gets a dict with empty lists and an 'error' message."""
        if len(filters) != len(queries):
            raise ValueError(f"{len(filters)} filters for {len(queries)} queries")
        live = [flt for q, flt in zip(queries, filters) if q and q.strip()]    # as _batch picks them
        return await self._batch("Batch filtered query", None, _EMPTY, self._answer_filtered, queries, n_results, live)

    def supports_boost(self) -> bool:
        """True when the collection can rank with a score prior (a single-GPU VectorIndex with full-precision rows; not
        the sharded serving path, which does not carry the request: one warning says so)"""
        ok = self.collection is None or (hasattr(self.collection, "boosted_query") and self._has_full_rows())
        if not ok:
            global _boost_warned
            if not _boost_warned:
                _boost_warned = True
                logger.warning("Boosted retrieval is not available: %s", _NEEDS_BOOST[1])
        return ok

    @staticmethod
    def _boost_spec(boost):
        """a request's `boost` (None / True: the configured defaults; a dict {"recency", "half_life_days", "values"};
        or a ready BoostSpec) as a BoostSpec; ValueError for a malformed one and for False, which means "no boost" to
        POST /query: such a request belongs to query()"""
        from .boost import BoostSpec, parse_boost

        if isinstance(boost, BoostSpec):
            return boost
        if boost is False:
            raise ValueError("'boost' is false: a query without a boost is query(), not boosted_query()")
        return parse_boost(True if boost is None else boost, settings.MMRAG_BOOST_RECENCY,
                           settings.MMRAG_BOOST_HALF_LIFE_DAYS)

    def _answer_boosted(self, texts: Sequence[str], n_results: int, filter_dict: Optional[Dict],
                        spec) -> List[Dict[str, Any]]:
        """blocking, one worker thread: cached or fresh embeddings (ONE encoder pass for the misses), then ONE
        collection.boosted_query for all of them (one scan with the spec's prior column)"""
        if not self._has_full_rows():
            raise ValueError(_NEEDS_BOOST[1])
        res = self.collection.boosted_query(self._embed(texts), n_results=n_results, prior=spec, weight=1.0,
                                            where=filter_dict, include=self._INCLUDE)
        return [{key: res[key][at] for key in BOOST_KEYS} for at in range(len(texts))]

    async def boosted_query(self, query_text: str, n_results: int = 5, filter_dict: Optional[Dict] = None,
                            boost=None) -> Dict[str, Any]:
        """query() ranked by cosine + a score prior (VectorIndex.boosted_query): `boost` is {"recency": weight of the
        recency term, "half_life_days": the age at which it has halved, "values": {metadata key: {value: added
        score}}}, missing fields from MMRAG_BOOST_RECENCY / MMRAG_BOOST_HALF_LIFE_DAYS.  One result dict with the keys of
        query() plus `scores` (final, descending) and `boosts`; `distances` stay 1 - cosine and are not ascending.  Same
        empty-query error, embedding cache and query count as query(); with dynamic batching on, concurrent callers of
        one n_results and one boost share one encode and one search."""
        spec = self._boost_spec(boost)
        if self._dispatcher is not None and self._dispatcher.boosted_fn is not None:
            await self._ready()
            if not query_text or not query_text.strip():
                raise ValueError("Query text cannot be empty")
            return await self._dispatcher.submit(query_text, n_results, filter_dict, None, boost=spec)
        return await self._single("Boosted query", _NEEDS_BOOST, self._answer_boosted, query_text, n_results,
                                  filter_dict, spec)

    async def batch_boosted_query(self, queries: List[str], n_results: int = 5, filter_dict: Optional[Dict] = None,
                                  boost=None) -> List[Dict[str, Any]]:
        """batch_query's twin for boosted_query: one batched encode and one boosted search for all the queries; a query
        that cannot be answered gets a dict with empty lists and an 'error' message."""
        return await self._batch("Batch boosted query", _NEEDS_BOOST, _EMPTY_BOOST, self._answer_boosted, queries,
                                 n_results, filter_dict, self._boost_spec(boost))

    # ---- recommend retrieval: positive and negative examples (VectorIndex.recommend_query, csrc/recommend.hip) ----
    def supports_recommend(self) -> bool:
        """True when the collection can search by examples (a single-GPU VectorIndex with full-precision rows; not a
        sharded engine or one without the method: recommend() raises ValueError there)"""
        return self.collection is None or (hasattr(self.collection, "recommend_query") and self._has_full_rows())

    @staticmethod
    def _recommend_request(query_text=None, like=(), unlike=(), unlike_texts=(), negative_weight=None) -> Dict[str, Any]:
        """one request of recommend(), checked: the question (if given) is one positive, `like` / `unlike` are stored
        ids, `unlike_texts` are encoded; at least one of query_text and like, at most 16 examples in all"""
        if isinstance(like, str) or isinstance(unlike, str) or isinstance(unlike_texts, str):
            raise ValueError("like, unlike and unlike_texts are lists")
        text = query_text if query_text and query_text.strip() else None
        req = {"query_text": text, "like": list(like or ()), "unlike": list(unlike or ()),
               "unlike_texts": list(unlike_texts or ()), "negative_weight": negative_weight}
        if query_text is not None and text is None:
            raise ValueError("Query text cannot be empty")
        if text is None and not req["like"]:
            raise ValueError("recommend needs a question or at least one `like` id")
        if not all(isinstance(x, str) and x for x in req["like"] + req["unlike"]):
            raise ValueError("like and unlike hold the ids of stored items")
        if not all(isinstance(x, str) and x.strip() for x in req["unlike_texts"]):
            raise ValueError("unlike_texts holds non-empty texts")
        total = (text is not None) + len(req["like"]) + len(req["unlike"]) + len(req["unlike_texts"])
        if total > MAX_RECOMMEND_EXAMPLES:
            raise ValueError(f"a recommend request takes at most {MAX_RECOMMEND_EXAMPLES} examples in all (got {total})")
        if negative_weight is not None:
            w = float(negative_weight)
            if not (math.isfinite(w) and w >= 0.0):
                raise ValueError("negative_weight must be finite and >= 0")
        return req

    def _answer_recommend(self, requests: Sequence[Dict[str, Any]], n_results: int,
                          filter_dict: Optional[Dict]) -> List[Dict[str, Any]]:
        """blocking, one worker thread: the questions and the unwanted texts of ALL requests in ONE encoder batch, then
        ONE collection.recommend_query (one scan).  A request that names an id no stored item has gets an 'error'
        dict; the others are answered."""
        if not (hasattr(self.collection, "recommend_query") and self._has_full_rows()):
            raise ValueError(_NEEDS_RECOMMEND[1])
        named = sorted({i for r in requests for i in r["like"] + r["unlike"]})
        known = set(self.collection.get(ids=named, include=[])["ids"]) if named else set()
        out: List[Optional[Dict[str, Any]]] = [None] * len(requests)
        live = []
        for at, r in enumerate(requests):
            missing = [i for i in r["like"] + r["unlike"] if i not in known]
            if missing:
                out[at] = {**copy.deepcopy(_EMPTY_RECOMMEND), "error": f"Item not found: {missing[0]}"}
            else:
                live.append(at)
        if not live:
            return out  # type: ignore[return-value]
        texts: List[str] = []
        for at in live:
            r = requests[at]
            texts.extend(([r["query_text"]] if r["query_text"] is not None else []) + r["unlike_texts"])
        emb = self._embed(texts) if texts else np.zeros((0, 0), np.float32)
        pos, neg, weights, at_text = [], [], [], 0
        default_w = settings.MMRAG_RECOMMEND_NEGATIVE_WEIGHT
        for at in live:
            r = requests[at]
            mine_pos: List[Any] = []
            if r["query_text"] is not None:
                mine_pos.append(emb[at_text])
                at_text += 1
            pos.append(mine_pos + r["like"])
            neg.append(r["unlike"] + [emb[at_text + j] for j in range(len(r["unlike_texts"]))])
            at_text += len(r["unlike_texts"])
            weights.append(float(default_w if r["negative_weight"] is None else r["negative_weight"]))
        res = self.collection.recommend_query(pos, neg, n_results=n_results, negative_weight=weights,
                                              where=filter_dict, include=self._INCLUDE)
        for j, at in enumerate(live):
            r = requests[at]
            hit = {key: res[key][j] for key in RECOMMEND_KEYS}
            # an example that is a vector is named by what it was: the question, or the unwanted text
            has_q = r["query_text"] is not None
            hit["matched"] = ["query" if has_q and m == "vector:0" else m for m in hit["matched"]]
            n_ids = len(r["unlike"])
            hit["repelled_by"] = [r["unlike_texts"][int(m[7:]) - n_ids] if isinstance(m, str) and m.startswith("vector:")
                                  and int(m[7:]) >= n_ids else m for m in hit["repelled_by"]]
            out[at] = hit
        return out  # type: ignore[return-value]

    async def recommend(self, query_text: Optional[str] = None, like: Sequence[str] = (), unlike: Sequence[str] = (),
                        unlike_texts: Sequence[str] = (), n_results: int = 5, filter_dict: Optional[Dict] = None,
                        negative_weight: Optional[float] = None) -> Dict[str, Any]:
        """"More like these, less like those" (VectorIndex.recommend_query): the question, if given, is one positive
        example, `like` / `unlike` are ids of stored items, `unlike_texts` ("jaguar, NOT the car") are encoded in the
        same encoder batch as the question.  At least one of query_text and like; at most 16 examples in all.  A hit x
        scores pos - w * max(neg, 0) (pos / neg: its best cosine to a positive / negative example; w: negative_weight,
        default MMRAG_RECOMMEND_NEGATIVE_WEIGHT), formed inside one exact scan.  One result dict with the keys of
        query() plus `scores` (descending), `penalties`, `matched` ("query" or the id of the positive that scored best)
        and `repelled_by` (the id or the text of the negative that fired, else None); `distances` are 1 - pos and not
        ascending; the stored items named are not returned.  ValueError for a malformed request, an unknown id and a
        collection that cannot (supports_recommend).  With dynamic batching on, concurrent callers of one n_results
        and filter share one encode and one search whatever their examples."""
        req = self._recommend_request(query_text, like, unlike, unlike_texts, negative_weight)
        await self._ready()
        if not self.supports_recommend():
            raise ValueError(_NEEDS_RECOMMEND[1])
        if self._dispatcher is not None and self._dispatcher.recommend_fn is not None:
            return await self._dispatcher.submit("", n_results, filter_dict, None, recommend=req)
        try:
            hit = (await self._engine_call("Recommend", self._answer_recommend, [req], n_results, filter_dict))[0]
        except Exception as e:
            logger.error("Recommend failed: %s", e, exc_info=True)
            raise
        if "error" in hit:
            raise ValueError(hit["error"])
        self.stats["total_queries"] += 1
        return hit

    async def batch_recommend(self, requests: Sequence[Dict[str, Any]], n_results: int = 5,
                              filter_dict: Optional[Dict] = None, raise_engine_errors: bool = False) -> List[Dict[str, Any]]:
        """recommend() for a list of requests (dicts with recommend()'s keys query_text, like, unlike, unlike_texts,
        negative_weight): ONE encoder batch and ONE search for all of them; a request that cannot be answered gets a
        dict with empty lists and an 'error' message.  `raise_engine_errors` (the dispatcher): only a request's own
        fault -- a broken rule, an id no stored item has -- becomes such a dict; a failure of the encoder or the search
        is raised, so that it is not mistaken for a bad request."""
        await self._ready()
        answers: List[Optional[Dict[str, Any]]] = [None] * len(requests)
        checked, live = [], []
        for at, r in enumerate(requests):
            try:
                checked.append(self._recommend_request(**{k: r.get(k) for k in ("query_text", "like", "unlike",
                                                                                 "unlike_texts", "negative_weight")
                                                          if r.get(k) is not None}))
                live.append(at)
            except (ValueError, TypeError) as e:
                answers[at] = {**copy.deepcopy(_EMPTY_RECOMMEND), "error": str(e)}
        if live:
            try:
                hits = await self._engine_call("Batch recommend", self._answer_recommend, checked, n_results, filter_dict)
                for at, hit in zip(live, hits):
                    answers[at] = hit
                self.stats["total_queries"] += sum("error" not in h for h in hits)
            except Exception as e:
                logger.error("Batch recommend failed: %s", e)
                if raise_engine_errors:
                    raise
                for at in live:
                    answers[at] = {**copy.deepcopy(_EMPTY_RECOMMEND), "error": str(e)}
        return answers  # type: ignore[return-value]

    def supports_hybrid(self) -> bool:
        """True when the collection can answer hybrid_query (a single-GPU VectorIndex; not the sharded serving path)"""
        return self.collection is None or (hasattr(self.collection, "hybrid_query") and self._has_full_rows())

    def _has_full_rows(self) -> bool:
        """False for a float8_e4m3fn collection without a re-scoring plane (MMRAG_F8_RESCORE=none): mmr and hybrid
        queries read full-precision rows"""
        c = self.collection
        return not (getattr(c, "is_f8", False) and getattr(c, "plane", None) is None)

    def _answer_hybrid(self, texts: Sequence[str], n_results: int, filter_dict: Optional[Dict],
                       fuzzy=None, slop: Optional[int] = None) -> List[Dict[str, Any]]:
        """blocking, one worker thread: cached or fresh embeddings, then ONE collection.hybrid_query.  `slop` not None:
        phrase queries with that slop (the dict then carries `phrases`)"""
        more = {} if fuzzy is None else {"fuzzy": fuzzy}
        if slop is not None:
            more.update(phrases=True, slop=slop)
        res = self.collection.hybrid_query(self._embed(texts), list(texts), n_results=n_results, where=filter_dict,
                                           include=self._INCLUDE, **more)
        keys = HYBRID_KEYS + tuple(key for key in ("corrections", "phrases") if key in res)
        return [{key: res[key][at] for key in keys} for at in range(len(texts))]

    async def suggest_terms(self, words: Sequence[str], fuzzy="auto", limit: int = 5) -> List[List[Dict[str, Any]]]:
        """"Did you mean" (VectorIndex.suggest_terms): per word up to `limit` indexed terms within the allowed edits, as
        {"term", "edits", "df"}, best first"""
        await self._ready()
        if not hasattr(self.collection, "suggest_terms"):
            raise ValueError(_NEEDS_HYBRID[1])
        return await asyncio.to_thread(self.collection.suggest_terms, list(words), fuzzy, limit)

    async def hybrid_query(self, query_text: str, n_results: int = 5,
                           filter_dict: Optional[Dict] = None, leg: str = "lexical", fuzzy=None,
                           phrases: Optional[bool] = None, slop: Optional[int] = None) -> Dict[str, Any]:
        """Dense + BM25 retrieval fused by reciprocal rank (VectorIndex.hybrid_query): one result dict with `ids`,
        `distances`, `metadatas`, `documents`, `hybrid_scores` and `lexical_scores`, in hybrid-score order (distances
        are therefore not ascending).  Same empty-query error, embedding cache and query count as query(); it calls
        the collection directly (no dynamic batching).  `leg` = "sparse": the second leg is learned sparse retrieval
        instead of BM25 (VectorIndex.sparse_hybrid_query) and the dict carries `sparse_scores` in place of
        `lexical_scores`.  `fuzzy` ("auto", True or 0..2 edits; None: the MMRAG_LEXICAL_FUZZY setting) makes the BM25 leg
        typo-tolerant (VectorIndex.lexical_query) and the dict then carries `corrections`; it does not go with the
        sparse leg.  `phrases` (None: the MMRAG_LEXICAL_PHRASES setting): a quoted segment of the question is a phrase
        every hit must hold (VectorIndex.hybrid_query, phrase_mode "require"), its terms at most `slop` (0..16; None:
        MMRAG_LEXICAL_SLOP) other tokens apart; the dict then carries `phrases`.  Not with the sparse leg either."""
        from .lexical import parse_fuzzy, parse_slop

        if leg == "sparse" and parse_fuzzy(fuzzy) is not None:
            raise ValueError("fuzzy matching belongs to the lexical leg, not the learned sparse one")
        if leg == "sparse" and phrases:
            raise ValueError("phrase queries belong to the lexical leg, not the learned sparse one")
        if leg == "sparse":
            await self._ready()
            if not (self.has_sparse_encoder() and self.supports_sparse()):
                raise ValueError(_NEEDS_SPARSE[1])
            return await self._single("Sparse hybrid query", _NEEDS_SPARSE, self._answer_sparse_hybrid, query_text,
                                      n_results, filter_dict)
        if leg != "lexical":
            raise ValueError(f"hybrid leg must be 'lexical' or 'sparse', not {leg!r}")
        fuzzy = parse_fuzzy(settings.MMRAG_LEXICAL_FUZZY if fuzzy is None else fuzzy)
        if settings.MMRAG_LEXICAL_PHRASES if phrases is None else phrases:
            slop = parse_slop(settings.lexical_slop() if slop is None else slop)
            return await self._single("Hybrid query", _NEEDS_HYBRID, self._answer_hybrid, query_text, n_results,
                                      filter_dict, fuzzy, slop)
        return await self._single("Hybrid query", _NEEDS_HYBRID, self._answer_hybrid, query_text, n_results, filter_dict,
                                  *(() if fuzzy is None else (fuzzy,)))

    # ------------------------------------------------------------------ learned sparse ------
    def has_sparse_encoder(self) -> bool:
        """True when a sparse encoder is configured (MMRAG_SPARSE_ENCODER_DIR) or was attached (enable_sparse)"""
        return self._sparse is not None or bool(settings.MMRAG_SPARSE_ENCODER_DIR)

    def supports_sparse(self) -> bool:
        """True when the collection can keep and search learned sparse vectors: a single-GPU VectorIndex (not the
        sharded serving path) behind a BERT-family fp16 HIP engine (not the CLIP engine, not the fp32 encoder mode)"""
        if self.collection is not None and not hasattr(self.collection, "sparse_query"):
            return False
        eng = self._engine
        if eng is None:
            return True
        return not hasattr(eng, "encode_images") and getattr(getattr(eng, "encoder", None), "_f32", False) is False

    def _get_sparse(self):
        """the sparse encoder of MMRAG_SPARSE_ENCODER_DIR, loaded once on the embedder's device"""
        with self._sparse_lock:
            if self._sparse is None:
                from .sparse import DeviceSparseEncoder

                if not settings.MMRAG_SPARSE_ENCODER_DIR:
                    raise ValueError(_NEEDS_SPARSE[1])
                device = str(getattr(self.collection, "device", None) or "cuda:0")
                self._sparse = DeviceSparseEncoder.from_local_dir(settings.MMRAG_SPARSE_ENCODER_DIR, device)
            return self._sparse

    def _doc_terms(self) -> int:
        return max(1, min(int(settings.MMRAG_SPARSE_DOC_TERMS), 256))

    def _query_terms(self) -> int:
        return max(1, min(int(settings.MMRAG_SPARSE_QUERY_TERMS), 64))

    def _store_sparse(self, ids: Sequence[str], texts: Sequence[Optional[str]], batch: int = 256):
        """blocking: expand the texts and give the stored rows their sparse vectors (rows that were skipped as
        duplicates have no row and are passed over)"""
        enc = self._get_sparse()
        self.collection.enable_sparse(enc.cfg.vocab)
        rows = self.collection.rows_of_ids(list(ids))
        have = [at for at, r in enumerate(rows) if r >= 0]
        for s in range(0, len(have), batch):
            part = have[s: s + batch]
            off, terms, imps = enc.expand_texts([texts[at] or "" for at in part], self._doc_terms())
            self.collection.set_sparse([rows[at] for at in part], off, terms, imps)

    def _enable_sparse_sync(self, encoder) -> Dict[str, Any]:
        if encoder is not None:
            self._sparse = encoder
        if not self.supports_sparse():
            raise ValueError(_NEEDS_SPARSE[1])
        enc = self._get_sparse()
        c = self.collection
        c.enable_sparse(enc.cfg.vocab)
        got = c.get(include=["documents"])
        self._store_sparse(got["ids"], got["documents"])
        return {"items": len(got["ids"]), "vocab": enc.cfg.vocab}

    async def enable_sparse(self, encoder=None) -> Dict[str, Any]:
        """Attach a sparse encoder (`encoder`: a DeviceSparseEncoder; None: the one of MMRAG_SPARSE_ENCODER_DIR) and
        expand the documents already stored, in batches -- the sparse state is not persisted, so this is also what
        brings it back after a restore.  From then on embed_and_store expands what it stores."""
        await self._ready()
        return await asyncio.to_thread(self._enable_sparse_sync, encoder)

    def _sparse_queries(self, texts: Sequence[str]):
        enc = self._get_sparse()
        if settings.MMRAG_SPARSE_QUERY_MODE == "tokens":
            return enc.token_terms(list(texts), self._query_terms())
        return enc.expand_texts(list(texts), self._query_terms())

    @staticmethod
    def _sparse_distances(res: Dict[str, Any]) -> List[List[float]]:
        # there is no cosine: a source's relevance reads the sparse score itself, cut to 0..1
        return [[max(0.0, 1.0 - s) for s in row] for row in res["sparse_scores"]]

    def _answer_sparse(self, texts: Sequence[str], n_results: int, filter_dict: Optional[Dict],
                       explain: bool = False) -> List[Dict[str, Any]]:
        """blocking, one worker thread: ONE expansion of the questions (or their word pieces), ONE impact search"""
        queries = self._sparse_queries(texts)
        enc = self._get_sparse()
        self.collection.enable_sparse(enc.cfg.vocab)
        scales = (enc.scale, enc.scale)
        res = self.collection.sparse_query(queries, n_results=n_results, where=filter_dict,
                                           include=("metadatas", "documents"), scales=scales)
        res["distances"] = self._sparse_distances(res)
        out = [{key: res[key][at] for key in SPARSE_KEYS} for at in range(len(texts))]
        if explain:
            off, terms, imps = queries
            for at, hit in enumerate(out):
                qt, qi = terms[off[at]: off[at + 1]], imps[off[at]: off[at + 1]]
                hit["matched_terms"] = []
                for row in res["rows"][at]:
                    pairs = self.collection.sparse_explain(qt, qi, row, scales)
                    names = enc.terms_to_strings([t for t, _ in pairs])
                    hit["matched_terms"].append([{"term": n, "score": c} for n, (_, c) in zip(names, pairs)])
        return out

    def _answer_sparse_hybrid(self, texts: Sequence[str], n_results: int,
                              filter_dict: Optional[Dict]) -> List[Dict[str, Any]]:
        enc = self._get_sparse()
        self.collection.enable_sparse(enc.cfg.vocab)
        res = self.collection.sparse_hybrid_query(self._embed(texts), self._sparse_queries(texts), n_results=n_results,
                                                  where=filter_dict, include=self._INCLUDE,
                                                  scales=(enc.scale, enc.scale))
        return [{key: res[key][at] for key in SPARSE_HYBRID_KEYS} for at in range(len(texts))]

    async def sparse_query(self, query_text: str, n_results: int = 5, filter_dict: Optional[Dict] = None,
                           explain: bool = False) -> Dict[str, Any]:
        """Learned sparse retrieval (VectorIndex.sparse_query): the question is expanded by the sparse encoder
        (MMRAG_SPARSE_QUERY_MODE=tokens: its own word pieces, no forward pass) and scored exactly against the stored
        sparse vectors.  One result dict with `ids`, `metadatas`, `documents`, `sparse_scores` (descending) and
        `distances` = max(0, 1 - sparse score) (there is no cosine).  `explain`: `matched_terms`, per hit the shared
        vocabulary strings with their contribution to the score, best first.  Same empty-query error and query
        count as query(); with dynamic batching on, concurrent callers of one n_results and filter share one batch."""
        if not self.has_sparse_encoder():
            raise ValueError(_NEEDS_SPARSE[1])
        if explain or self._dispatcher is None or getattr(self._dispatcher, "sparse_fn", None) is None:
            return await self._single("Sparse query", _NEEDS_SPARSE, self._answer_sparse, query_text, n_results,
                                      filter_dict, explain)
        await self._ready()
        if not query_text or not query_text.strip():
            raise ValueError("Query text cannot be empty")
        return await self._dispatcher.submit(query_text, n_results, filter_dict, sparse=True)

    async def batch_sparse_query(self, queries: List[str], n_results: int = 5,
                                 filter_dict: Optional[Dict] = None) -> List[Dict[str, Any]]:
        """batch_query's twin for sparse_query: one expansion forward and one impact search for all the queries; a
        query that cannot be answered gets a dict with empty lists and an 'error' message."""
        return await self._batch("Batch sparse query", _NEEDS_SPARSE, _EMPTY_SPARSE, self._answer_sparse, queries,
                                 n_results, filter_dict)

    def supports_mmr(self) -> bool:
        """True when the collection can answer mmr_query (a single-GPU VectorIndex; not the sharded serving path, whose
        candidates' rows live on different GPUs)"""
        return self.collection is None or (hasattr(self.collection, "mmr_query") and self._has_full_rows())

    def _answer_mmr(self, texts: Sequence[str], n_results: int, filter_dict: Optional[Dict], fetch_k: Optional[int],
                    lambda_mult: Optional[float]) -> List[Dict[str, Any]]:
        """blocking, one worker thread: cached or fresh embeddings (ONE encoder pass for the misses), then ONE
        collection.mmr_query for all of them (one search, one selection launch)"""
        res = self.collection.mmr_query(self._embed(texts), n_results=n_results, fetch_k=fetch_k,
                                        lambda_mult=lambda_mult, where=filter_dict, include=self._INCLUDE)
        return [{key: res[key][at] for key in MMR_KEYS} for at in range(len(texts))]

    async def mmr_query(self, query_text: str, n_results: int = 5, filter_dict: Optional[Dict] = None,
                        fetch_k: Optional[int] = None, lambda_mult: Optional[float] = None) -> Dict[str, Any]:
        """Diversified retrieval (VectorIndex.mmr_query): maximal-marginal-relevance selection of n_results of the
        fetch_k best dense hits.  One result dict with the keys of query() plus `mmr_scores`, in pick order (distances
        are therefore not ascending).  Same empty-query error, embedding cache and query count as query(); it calls
        the collection directly (no dynamic batching)."""
        return await self._single("MMR query", _NEEDS_MMR, self._answer_mmr, query_text, n_results, filter_dict,
                                  fetch_k, lambda_mult)

    async def batch_mmr_query(self, queries: List[str], n_results: int = 5, filter_dict: Optional[Dict] = None,
                              fetch_k: Optional[int] = None,
                              lambda_mult: Optional[float] = None) -> List[Dict[str, Any]]:
        """batch_query's twin for mmr_query: one batched encode, one search and one selection launch for all the
        queries; a query that cannot be answered gets a dict with empty lists and an 'error' message."""
        return await self._batch("Batch MMR query", _NEEDS_MMR, _EMPTY_MMR, self._answer_mmr, queries,
                                 n_results, filter_dict, fetch_k, lambda_mult)

    def supports_dedup(self) -> bool:
        """True when the collection can find near-duplicates (a single-GPU VectorIndex with full-precision rows; not the
        sharded serving path, whose rows live on different GPUs, nor a float8_e4m3fn collection without its re-scoring
        plane)"""
        return self.collection is None or (hasattr(self.collection, "near_duplicates") and self._has_full_rows())

    async def _dedup_call(self, label: str, method: str, threshold: Optional[float], doc_id: Optional[str],
                          max_pairs: int):
        await self._ready()
        if not self.supports_dedup():
            raise ValueError(_NEEDS_DEDUP[1])
        return await self._refusing_call(label, getattr(self.collection, method), threshold=threshold,
                                         where={"doc_id": doc_id} if doc_id else None, max_pairs=max_pairs)

    async def _refusing_call(self, label: str, fn, **kw):
        """fn(**kw) through _engine_call; a ValueError of fn's (a bad threshold, a truncated report, a bad cluster count)
        is the caller's answer, not worth a retry: raised as it is"""
        def run(**kw):
            try:
                return fn(**kw)
            except ValueError as refusal:
                return refusal

        out = await self._engine_call(label, run, **kw)
        if isinstance(out, ValueError):
            raise out
        return out

    async def find_duplicates(self, threshold: Optional[float] = None, doc_id: Optional[str] = None,
                              max_pairs: int = 1 << 20) -> Dict[str, Any]:
        """The near-duplicate report of the collection (VectorIndex.near_duplicates), of one document's chunks with
        `doc_id`: pairs at or above the cosine `threshold` (default MMRAG_DEDUP_REPORT_THRESHOLD) and their groups."""
        return await self._dedup_call("Find duplicates", "near_duplicates", threshold, doc_id, max_pairs)

    async def remove_duplicates(self, threshold: Optional[float] = None, doc_id: Optional[str] = None,
                                max_pairs: int = 1 << 20) -> List[str]:
        """Delete all but the earliest stored member of every near-duplicate group (VectorIndex.drop_duplicates);
        returns the deleted ids.  ValueError, and nothing deleted, when the groups would come from a truncated report."""
        return await self._dedup_call("Remove duplicates", "drop_duplicates", threshold, doc_id, max_pairs)

    def supports_clustering(self) -> bool:
        """True when the collection can report its topics (where supports_dedup() is: a single-GPU VectorIndex with
        full-precision rows; not the sharded serving path)"""
        return self.collection is None or (hasattr(self.collection, "cluster") and self._has_full_rows())

    def supports_terms(self) -> bool:
        """True when the collection can report significant terms (a single-GPU VectorIndex, whose lexical leg holds
        the stored chunks' terms; not the sharded serving path)"""
        return self.collection is None or hasattr(self.collection, "significant_terms")

    async def document_keywords(self, doc_ids: Sequence[str], top: int = 10, min_count: int = 2) -> List[Dict[str, Any]]:
        """The keywords of stored documents (VectorIndex.significant_terms over key "doc_id"): per doc_id, in order,
        {"doc_id", "chunks": its live chunks, "keywords": [{"term", "score", "count", "background"}]} -- the terms of
        at least MMRAG_KEYWORD_MIN_LENGTH code points that at least `min_count` of its chunks hold and that are more
        frequent in it than in the collection, best first.  A doc_id nothing is stored under has 0 chunks and no
        keywords.  ValueError for arguments the collection refuses."""
        await self._ready()
        if not self.supports_terms():
            raise ValueError(_NEEDS_TERMS[1])
        doc_ids = list(doc_ids)
        if not doc_ids:
            return []
        found = await self._refusing_call("Document keywords", self.collection.significant_terms, key="doc_id",
                                          values=doc_ids, top=top, min_count=min_count,
                                          min_length=settings.keyword_min_length())
        return [{"doc_id": g["group"], "chunks": g["size"], "keywords": g["terms"]} for g in found]

    async def cluster_topics(self, n_topics: Optional[int] = None, doc_id: Optional[str] = None,
                             representatives: int = 3, seed: int = 0, terms: int = 0) -> Dict[str, Any]:
        """The topics of the collection, of one document's chunks with `doc_id` (VectorIndex.cluster): its report
        without the centroid tensor, every representative expanded to {"id", "score", "document", "metadata"}.
        n_topics None: MMRAG_TOPICS.  `terms` > 0: every cluster carries its `terms` significant terms (ValueError where
        supports_terms() is false).  ValueError for a cluster count the collection refuses."""
        await self._ready()
        if not self.supports_clustering():
            raise ValueError(_NEEDS_CLUSTERING[1])
        more = {}
        if terms:
            if not self.supports_terms():
                raise ValueError(_NEEDS_TERMS[1])
            more["terms"] = int(terms)
        report = await self._refusing_call("Cluster topics", self.collection.cluster, n_clusters=n_topics,
                                           where={"doc_id": doc_id} if doc_id else None,
                                           representatives=representatives, seed=seed, **more)
        report = {key: val for key, val in report.items() if key != "centroids"}
        wanted = [i for c in report["clusters"] for i, _ in c["representatives"]]
        got = self.collection.get(ids=wanted, include=["metadatas", "documents"]) if wanted else {"ids": []}
        row = {i: at for at, i in enumerate(got["ids"])}
        for c in report["clusters"]:
            c["representatives"] = [{"id": i, "score": s, "document": got["documents"][row[i]] if i in row else None,
                                     "metadata": got["metadatas"][row[i]] if i in row else {}}
                                    for i, s in c["representatives"]]
        return report

    def supports_related(self) -> bool:
        """True when the collection can rank documents against a set of vectors (where supports_dedup() is: a
        single-GPU VectorIndex with full-precision rows; not the sharded serving path)"""
        return self.collection is None or (hasattr(self.collection, "related_query") and self._has_full_rows())

    async def related_documents(self, doc_id: Optional[str] = None, texts: Optional[Sequence[str]] = None,
                                n_results: int = 5, threshold: Optional[float] = None,
                                filter_dict: Optional[Dict] = None) -> Dict[str, Any]:
        """The stored documents most like ONE set of passages (VectorIndex.related_query): the chunks stored under
        `doc_id` (that document itself is no candidate) or the given `texts`, encoded in one batched call -- exactly one
        of the two.  Returns {"chunks": m, "threshold": t, "related": [{"key": doc_id, "similarity", "coverage",
        "matched", "rows_in_group", "pairs": [...]}, ...]} in rank order; `threshold` (default
        MMRAG_DEDUP_REPORT_THRESHOLD) is the cosine from which a chunk counts as contained.  LookupError when no stored
        item has `doc_id`; ValueError for arguments the collection refuses."""
        if (doc_id is None) == (texts is None):
            raise ValueError("related_documents takes exactly one of doc_id and texts")
        await self._ready()
        if not self.supports_related():
            raise ValueError(_NEEDS_RELATED[1])
        if texts is not None:
            texts = list(texts)
            if not texts or not all(isinstance(t, str) and t.strip() for t in texts):
                raise ValueError("texts must be a non-empty list of non-empty strings")
            if len(texts) > MAX_RELATED_ROWS:
                raise ValueError(f"texts holds {len(texts)} passages, at most {MAX_RELATED_ROWS}")
            entry, m = await self._embed_matrix(texts, self.batch_size), len(texts)
        else:
            m = len(self.collection.get(where={"doc_id": doc_id}, include=())["ids"])
            if not m:
                raise LookupError(f"no stored item has doc_id {doc_id!r}")
            entry = {"value": doc_id}
        t = settings.MMRAG_DEDUP_REPORT_THRESHOLD if threshold is None else threshold
        found = await self._refusing_call("Related documents", self.collection.related_query, sets=[entry],
                                          n_results=n_results, threshold=t, where=filter_dict)
        return {"chunks": m, "threshold": float(t), "related": found[0]}

    # ---- range retrieval: everything above a score, counted and faceted (VectorIndex.range_query, csrc/range.hip) ----
    def supports_range(self) -> bool:
        """True when the collection can answer range_query (a single-GPU VectorIndex with full-precision rows; not the
        sharded serving path, whose counts would have to be added across GPUs)"""
        return self.collection is None or (hasattr(self.collection, "range_query") and self._has_full_rows())

    def _answer_range(self, texts: Sequence[str], min_scores: Sequence[float], limit: int, facets: Sequence[str],
                      filter_dict: Optional[Dict]) -> List[Dict[str, Any]]:
        """blocking, one worker thread: cached or fresh embeddings (ONE encoder pass for the misses), then ONE
        collection.range_query for all of them (one scan that counts, facets and keeps the best `limit`)"""
        if not self._has_full_rows():
            raise ValueError(_NEEDS_RANGE[1])
        res = self.collection.range_query(self._embed(texts), threshold=list(min_scores), limit=limit, wheres=filter_dict,
                                          facets=list(facets), include=self._INCLUDE)
        hits = self._split(res, len(texts))
        for at, hit in enumerate(hits):
            hit.update(total=res["total"][at], truncated=res["truncated"][at], facets=res["facets"][at])
        return hits

    async def range_query(self, query_text: str, min_score: float, limit: int = 20, facets: Sequence[str] = (),
                          filter_dict: Optional[Dict] = None) -> Dict[str, Any]:
        """Everything relevant, and how much of it there is (VectorIndex.range_query): the `limit` best stored items
        whose cosine with the query is at least `min_score`, as the result dict of query(), plus `total` (how many
        items clear the score), `truncated` (total > limit) and `facets` ({metadata key: [{"value", "count"}, ...]}
        over ALL of them, for each key in `facets`).  limit 0 = the numbers alone.  Same empty-query error, embedding
        cache and query count as query(); it calls the collection directly (no dynamic batching)."""
        return await self._single("Range query", _NEEDS_RANGE, self._answer_range, query_text, [float(min_score)],
                                  int(limit), list(facets), filter_dict)

    async def batch_range_query(self, queries: List[str], min_score, limit: int = 20, facets: Sequence[str] = (),
                                filter_dict: Optional[Dict] = None) -> List[Dict[str, Any]]:
        """batch_query's twin for range_query: one batched encode and one scan for all the queries; `min_score` is one
        float or one per query; a query that cannot be answered gets a dict with empty lists, zero totals and an
        'error' message."""
        scores = [float(min_score)] * len(queries) if isinstance(min_score, (int, float)) else [float(x) for x in min_score]
        if len(scores) != len(queries):
            raise ValueError(f"{len(scores)} scores for {len(queries)} queries")
        live = [t for q, t in zip(queries, scores) if q and q.strip()]    # as _batch picks them
        return await self._batch("Batch range query", _NEEDS_RANGE, _EMPTY_RANGE, self._answer_range, queries, live,
                                 int(limit), list(facets), filter_dict)

    def supports_grouping(self) -> bool:
        """True when the collection can answer grouped_query (a single-GPU VectorIndex; not the sharded serving path,
        whose rows' group ordinals live with their shards)"""
        return self.collection is None or hasattr(self.collection, "grouped_query")

    def _answer_grouped(self, texts: Sequence[str], n_groups: int, group_size: int, filter_dict: Optional[Dict],
                        group_by: str, fetch_k: Optional[int]) -> List[Dict[str, Any]]:
        """blocking, one worker thread: cached or fresh embeddings (ONE encoder pass for the misses), then ONE
        collection.grouped_query for all of them (one batched search and one grouping launch per rung of its ladder)"""
        res = self.collection.grouped_query(self._embed(texts), n_groups=n_groups, group_size=group_size,
                                            group_by=group_by, fetch_k=fetch_k, where=filter_dict,
                                            include=self._INCLUDE)
        out = []
        for groups, whole, depth in zip(res["groups"], res["exhaustive"], res["fetch_k"]):
            hit: Dict[str, Any] = {key: [x for g in groups for x in g[key]] for key in RESULT_KEYS}   # in group order
            hit.update(groups=groups, exhaustive=whole, fetch_k=depth)
            out.append(hit)
        return out

    async def grouped_query(self, query_text: str, n_groups: int = 5, group_size: int = 1,
                            filter_dict: Optional[Dict] = None, group_by: str = "doc_id",
                            fetch_k: Optional[int] = None) -> Dict[str, Any]:
        """Retrieval grouped by document (VectorIndex.grouped_query): the n_groups best values of the metadata key
        `group_by` and the group_size best hits of each.  One result dict with `groups` (group-rank order; each
        {"key", "ids", "distances", "metadatas", "documents"}), `exhaustive` and `fetch_k`, plus the keys of query()
        holding the same hits flattened in group order (so `distances` are not ascending, and
        MultiVectorRetriever.retrieve_raw_documents(ids) works as it is).  Same empty-query error, embedding cache and
        query count as query(); it calls the collection directly (no dynamic batching)."""
        return await self._single("Grouped query", _NEEDS_GROUPING, self._answer_grouped, query_text, n_groups,
                                  group_size, filter_dict, group_by, fetch_k)

    async def batch_grouped_query(self, queries: List[str], n_groups: int = 5, group_size: int = 1,
                                  filter_dict: Optional[Dict] = None, group_by: str = "doc_id",
                                  fetch_k: Optional[int] = None) -> List[Dict[str, Any]]:
        """batch_query's twin for grouped_query: one batched encode and one batched grouped search for all the queries;
        a query that cannot be answered gets a dict with empty lists and an 'error' message."""
        return await self._batch("Batch grouped query", _NEEDS_GROUPING, _EMPTY_GROUPED, self._answer_grouped, queries,
                                 n_groups, group_size, filter_dict, group_by, fetch_k)

    def supports_multi_query(self) -> bool:
        """True when the collection can answer fused_query (a single-GPU VectorIndex; not the sharded serving path,
        whose per-variant lists would have to be merged across the shards before they are fused)"""
        return self.collection is None or hasattr(self.collection, "fused_query")

    def _answer_fused(self, questions: Sequence[Sequence[str]], n_results: int, filter_dict: Optional[Dict],
                      weights: Optional[Sequence[Optional[Sequence[float]]]],
                      method: Optional[str]) -> List[Dict[str, Any]]:
        """blocking, one worker thread: every variant of every question through the cache and ONE encoder pass for the
        misses, then ONE collection.fused_query (one search over all of them, one fusion launch)"""
        flat = [text for variants in questions for text in variants]
        list_off = [0]
        for variants in questions:
            list_off.append(list_off[-1] + len(variants))
        flat_w = None
        if weights is not None and any(w is not None for w in weights):
            flat_w = []
            for variants, w in zip(questions, weights):
                w = [1.0] * len(variants) if w is None else [float(x) for x in w]
                if len(w) != len(variants):
                    raise ValueError(f"{len(w)} weights for {len(variants)} query variants")
                flat_w.extend(w)
        res = self.collection.fused_query(self._embed(flat), list_off, n_results=n_results, weights=flat_w,
                                          method=method, where=filter_dict, include=self._INCLUDE)
        return [{key: res[key][at] for key in FUSED_KEYS} for at in range(len(questions))]

    @staticmethod
    def _variants_problem(variants) -> Optional[str]:
        """why these variants cannot be searched (query()'s own message for an empty text), or None"""
        if isinstance(variants, str) or not variants or any(not isinstance(v, str) or not v.strip() for v in variants):
            return "Query text cannot be empty"
        if len(variants) > 16:
            return "at most 16 query variants are fused per question"
        return None

    async def multi_query(self, queries: List[str], n_results: int = 5, filter_dict: Optional[Dict] = None,
                          weights: Optional[List[float]] = None, method: Optional[str] = None) -> Dict[str, Any]:
        """Multi-query retrieval (VectorIndex.fused_query): `queries` are phrasings or sub-questions of ONE question
        (at most 16); each is searched and the ranked lists are fused on the device, so a hit several phrasings agree
        on outranks a hit only one of them likes.  One result dict with the keys of query() plus `fused_scores`,
        `matched_queries` (how many phrasings returned the hit) and `best_query` (the index of the phrasing that
        scored it best), in fused order; `distances` are 1 - the best cosine over the phrasings, so they are not
        ascending.  weights: one per phrasing (default 1.0); method: "rrf" or "max" (default MMRAG_FUSE_METHOD).  An
        empty list or an empty phrasing raises query()'s empty-query error; same embedding cache; counts as one query;
        it calls the collection directly (no dynamic batching)."""
        await self._ready()
        why = self._variants_problem(queries)
        if why:
            raise ValueError(why)
        if not hasattr(self.collection, _NEEDS_MULTI[0]):
            raise ValueError(_NEEDS_MULTI[1])
        try:
            hit = (await self._engine_call("Multi-query", self._answer_fused, [list(queries)], n_results, filter_dict,
                                           [weights], method))[0]
        except Exception as e:
            logger.error("Multi-query failed: %s", e, exc_info=True)
            raise
        self.stats["total_queries"] += 1
        return hit

    async def batch_multi_query(self, question_variants: List[List[str]], n_results: int = 5,
                                filter_dict: Optional[Dict] = None,
                                weights: Optional[List[Optional[List[float]]]] = None,
                                method: Optional[str] = None) -> List[Dict[str, Any]]:
        """batch_query's twin for multi_query: every phrasing of every question in one batched encode, one search and
        one fusion launch; `weights` is one list per question (or None).  A question that cannot be answered -- no
        phrasings, an empty one, or all of them when the call fails -- gets a dict with empty lists and an 'error'
        message."""
        await self._ready()

        def failed(why: str) -> Dict[str, Any]:
            return {**copy.deepcopy(_EMPTY_FUSED), "error": why}

        answers: List[Optional[Dict[str, Any]]] = [None] * len(question_variants)
        live = []
        for at, variants in enumerate(question_variants):
            why = self._variants_problem(variants)
            if why:
                answers[at] = failed(why)
            else:
                live.append(at)
        if live:
            try:
                if not hasattr(self.collection, _NEEDS_MULTI[0]):
                    raise ValueError(_NEEDS_MULTI[1])
                if weights is not None and len(weights) != len(question_variants):
                    raise ValueError(f"{len(weights)} weight lists for {len(question_variants)} questions")
                hits = await self._engine_call("Batch multi-query", self._answer_fused,
                                               [list(question_variants[at]) for at in live], n_results, filter_dict,
                                               [weights[at] for at in live] if weights is not None else None, method)
                for at, hit in zip(live, hits):
                    answers[at] = hit
                self.stats["total_queries"] += len(live)
            except Exception as e:
                logger.error("Batch multi-query failed: %s", e)
                for at in live:
                    answers[at] = failed(str(e))
        return answers  # type: ignore[return-value]

    async def batch_query(self, queries: List[str], n_results: int = 5,
                          filter_dict: Optional[Dict] = None) -> List[Dict[str, Any]]:
        """embedder.py:784-832: one result dict per query, input order; a query that cannot be answered gets a dict
        with empty lists and an 'error' message instead of an exception (:817-830)."""
        return await self._batch("Batch query", None, _EMPTY, self._answer, queries, n_results,
                                 filter_dict)

    async def get_similar_documents(self, doc_id: str, item_id: str, n_results: int = 5) -> Dict[str, Any]:
        """embedder.py:861-930: the stored vector of one item searched for its n nearest OTHER items."""
        await self._ready()
        try:
            me = f"{doc_id}_{item_id}"
            stored = await asyncio.to_thread(self.collection.get, ids=[me], include=["embeddings", "documents"])
            if not stored["ids"]:
                raise ValueError(f"Item not found: {me}")
            near = await asyncio.to_thread(self.collection.query, query_embeddings=[stored["embeddings"][0]],
                                           n_results=n_results + 1, include=["metadatas", "documents", "distances"])
            others = [j for j, found in enumerate(near["ids"][0]) if found != me][:n_results]
            return {key: [near[key][0][j] for j in others] for key in RESULT_KEYS}
        except Exception as e:
            logger.error("Failed to find similar documents: %s", e)
            raise

    def has_reranker(self) -> bool:
        """True when rerank_results re-scores (a cross-encoder is configured: MMRAG_RERANKER_DIR, or one was set)"""
        return self._reranker is not None or bool(settings.MMRAG_RERANKER_DIR)

    def _get_reranker(self):
        """the cross-encoder of MMRAG_RERANKER_DIR, loaded once on the embedder's device"""
        with self._reranker_lock:
            if self._reranker is None:
                from .reranker import DeviceCrossEncoder

                device = getattr(self._engine, "device", None) or "cuda:0"
                self._reranker = DeviceCrossEncoder.from_local_dir(settings.MMRAG_RERANKER_DIR, device)
            return self._reranker

    # ---- extractive reader: answer spans from a BertForQuestionAnswering (reader.py, csrc/span_head.hip) ----
    def has_reader(self) -> bool:
        """True when read_answers can run (a reader is configured: MMRAG_READER_DIR, or one was set)"""
        return self._reader is not None or bool(settings.MMRAG_READER_DIR)

    def _get_reader(self):
        """the reader of MMRAG_READER_DIR, loaded once on the embedder's device"""
        with self._reranker_lock:
            if self._reader is None:
                if not settings.MMRAG_READER_DIR:
                    raise ValueError("The extractive reader is not configured: set MMRAG_READER_DIR to a local "
                                     "BertForQuestionAnswering directory")
                from .reader import DeviceReader

                device = getattr(self._engine, "device", None) or "cuda:0"
                self._reader = DeviceReader.from_local_dir(settings.MMRAG_READER_DIR, device)
            return self._reader

    async def batch_read_answers(self, queries: List[str], results_list: List[Dict[str, Any]], n_answers: int = 3,
                                 texts_list: Optional[Sequence[Optional[Sequence[str]]]] = None,
                                 owners_list: Optional[Sequence[Optional[Sequence[int]]]] = None,
                                 max_answer_tokens: Optional[int] = None, doc_stride: Optional[int] = None,
                                 null_threshold: Optional[float] = None) -> List[Dict[str, Any]]:
        """read_answers of results_list[i] against queries[i], ONE reader call (one forward per token budget) for all
        questions' hits"""
        if len(queries) != len(results_list):
            raise ValueError(f"{len(results_list)} result dicts for {len(queries)} queries")
        from .reader import best_answers

        reader = self._reader if self._reader is not None else await asyncio.to_thread(self._get_reader)
        max_answer_tokens = settings.MMRAG_READER_MAX_ANSWER_TOKENS if max_answer_tokens is None else max_answer_tokens
        doc_stride = settings.MMRAG_READER_DOC_STRIDE if doc_stride is None else doc_stride
        null_threshold = settings.MMRAG_READER_NULL_THRESHOLD if null_threshold is None else null_threshold
        n_best = max(1, min(int(n_answers), 8))
        questions, passages, owners = [], [], []
        for at, (query, results) in enumerate(zip(queries, results_list)):
            texts = texts_list[at] if texts_list is not None and texts_list[at] is not None else None
            if texts is None:      # the hits' own stored texts, one per hit
                texts = [d if d is not None else "" for d in results["documents"]]
                owner = list(range(len(texts)))
            else:
                owner = list(owners_list[at]) if owners_list is not None and owners_list[at] is not None \
                    else list(range(len(texts)))
                if len(owner) != len(texts):
                    raise ValueError(f"{len(owner)} owners for {len(texts)} texts")
            questions += [query] * len(texts)
            passages += list(texts)
            owners.append(owner)
        found = await asyncio.to_thread(reader.read, questions, passages, n_best, max_answer_tokens,
                                        doc_stride) if passages else []
        out, at = [], 0
        for results, owner in zip(results_list, owners):
            mine = found[at: at + len(owner)]
            at += len(owner)
            spans: List[List[Dict[str, Any]]] = [[] for _ in results["ids"]]
            for at_text, (hit, f) in enumerate(zip(owner, mine)):
                spans[hit].extend({**s, "passage": at_text} for s in f["spans"])
            out.append({**results, **best_answers(mine, owner, n_answers, float(null_threshold)),
                        "answer_spans": spans})
        return out

    async def read_answers(self, query_text: str, results: Dict[str, Any], n_answers: int = 3,
                           texts: Optional[Sequence[str]] = None, owner: Optional[Sequence[int]] = None,
                           max_answer_tokens: Optional[int] = None, doc_stride: Optional[int] = None,
                           null_threshold: Optional[float] = None) -> Dict[str, Any]:
        """Answer spans of `query_text` in the hits of `results` (any retrieval mode's answer).  Returns `results` plus
        `answers`: the best `n_answers` spans over all hits, {"text", "score", "probability", "hit" (index into the
        hits), "passage" (index into the texts read), "start", "end"}, character-identical texts from different hits
        merged (the best stays); `answerable`:
        best span score - the lowest null score over the hits > `null_threshold` (default
        MMRAG_READER_NULL_THRESHOLD); `null_score`; and `answer_spans`, per hit its own spans.  The texts read are the
        hits' `documents`, or `texts` (e.g. the retriever's raw passages) with `owner[i]` the hit texts[i] belongs to;
        start / end are characters of that text.  One reader.DeviceReader.read call."""
        return (await self.batch_read_answers([query_text], [results], n_answers,
                                              None if texts is None else [texts], None if owner is None else [owner],
                                              max_answer_tokens, doc_stride, null_threshold))[0]

    # ---- late interaction: re-ranking with the bi-encoder alone (late.py, csrc/maxsim.hip) ----
    def has_late_reranker(self) -> bool:
        """True when late_rerank can run: ONE BERT-family HIP engine in fp16 mode with a tokenizer (not the CLIP
        towers, not the fp32 encoder mode, not a sharded engine)"""
        enc = getattr(self._engine, "encoder", None)
        return (enc is not None and hasattr(enc, "encode_tokens") and getattr(enc, "precision", None) == "fp16"
                and getattr(self._engine, "tokenizer", None) is not None)

    def _get_late(self):
        with self._reranker_lock:
            if self._late is None:
                if not self.has_late_reranker():
                    raise ValueError("late-interaction re-ranking needs a single BERT-family fp16 HIP engine with a "
                                     "tokenizer")
                from .late import LateInteractionScorer

                self._late = LateInteractionScorer(self._engine.encoder, self._engine.tokenizer)
            return self._late

    # ---- the token store (late_store.py, csrc/maxsim_scan.hip): stored token rows, late retrieval ----
    def supports_late_store(self) -> bool:
        """True when the collection can keep token rows: has_late_reranker's rules (not the CLIP engine, not the fp32
        encoder mode) and a single-GPU VectorIndex (not a sharded collection)"""
        return self.has_late_reranker() and (self.collection is None or hasattr(self.collection, "enable_token_store"))

    def late_store_enabled(self) -> bool:
        return getattr(self.collection, "token_store", None) is not None

    def supports_late_query(self) -> bool:
        """True when late_query can run: a token store is attached (MMRAG_LATE_STORE=1 or enable_late_store())"""
        return self.supports_late_store() and self.late_store_enabled()

    def _token_store(self):
        """the collection's token store, attached on first use with the scorer's dim and passage length"""
        scorer = self._get_late()
        dim = int(scorer.projection.shape[0]) if scorer.projection is not None else int(scorer.encoder.cfg.hidden)
        return self.collection.enable_token_store(dim, scorer.max_doc_tokens)

    def _store_tokens(self, ids: Sequence[str], texts: Sequence[Optional[str]], batch: int = 64):
        """blocking: encode_tokens over `texts` in batches and keep the trimmed rows under the rows of `ids`.  Only ids
        whose live row keeps no tokens yet are encoded (an id add() ignored because it exists keeps the tokens of the
        document stored under it; a skipped duplicate has no row), and each batch is written by id under the index's
        lock (VectorIndex.set_tokens_for_ids): a delete, compaction or reset while the forward ran cannot misplace it."""
        self._token_store()
        scorer = self._get_late()
        text_of = dict(zip(ids, texts))
        todo = self.collection.ids_without_tokens(list(ids))
        for lo in range(0, len(todo), batch):
            part = todo[lo: lo + batch]
            tok, lens, tok_ids = scorer.encode_documents([text_of[i] for i in part], batch)
            self.collection.set_tokens_for_ids(part, tok, lens, tok_ids)

    def _enable_late_store_sync(self) -> Dict[str, Any]:
        if not self.supports_late_store():
            raise ValueError("the token store needs a single BERT-family fp16 HIP engine with a tokenizer and a "
                             "single-GPU collection (VectorIndex)")
        store = self._token_store()
        got = self.collection.get(include=("documents",))
        todo = set(self.collection.ids_without_tokens(got["ids"]))      # get() lists the live rows in row order
        ids = [i for i in got["ids"] if i in todo]
        text_of = dict(zip(got["ids"], got["documents"]))
        # Rows behind the last one that keeps tokens are appended batch by batch.  Rows before it are holes (the cap, or
        # uploads while the store was off): a fill rebuilds the plane, so all of them are encoded first and written in
        # ONE rebuild.  What that holds at once is the holes' token rows, not the plane's.
        rows = self.collection.rows_of_ids(ids)
        frontier = store.frontier()
        holes = [i for i, r in zip(ids, rows) if 0 <= r < frontier]
        self._store_tokens([i for i, r in zip(ids, rows) if r >= frontier], [text_of[i] for i, r in zip(ids, rows)
                                                                              if r >= frontier])
        if holes:
            import torch

            scorer, parts, lens, tok_ids = self._get_late(), [], [], []
            for lo in range(0, len(holes), 64):
                tok, n, t_ids = scorer.encode_documents([text_of[i] for i in holes[lo: lo + 64]], 64)
                parts.append(tok)
                lens.extend(int(x) for x in n)
                tok_ids.extend(t_ids)
            self.collection.set_tokens_for_ids(holes, torch.cat(parts), lens, tok_ids)
        return self.collection.token_stats()

    async def enable_late_store(self) -> Dict[str, Any]:
        """Attach the token store and fill it from the stored documents, in batches (the pattern of enable_lexical);
        rows that already keep tokens are left alone.  From then on late_rerank scores stored passages from the plane
        and late_query is available; uploads keep filling it only with MMRAG_LATE_STORE=1.  The plane is not persisted:
        after a restore, call this again.  Returns the store's statistics."""
        await self._ready()
        return await asyncio.to_thread(self._enable_late_store_sync)

    def _stored_spans(self, scorer, results_list: List[Dict[str, Any]], with_ids: bool):
        """(spans, plane) for _late_rerank_sync: per hit, in order, (first plane row, length, token ids) of the rows the
        token store keeps under the hit's id, or None -- no store, a store built for another passage length, an id the
        collection does not have, or a row that keeps no tokens.  One snapshot under the index's lock
        (VectorIndex.token_spans).  The token ids are read only `with_ids` (explain)"""
        if not hasattr(self.collection, "token_spans"):
            return None, None
        spans, plane, max_doc = self.collection.token_spans([r["ids"] for r in results_list], with_ids)
        if spans is None or max_doc != scorer.max_doc_tokens:
            return None, None
        return spans, plane

    def _answer_late(self, texts: Sequence[str], n_results: int, filter_dict: Optional[Dict]) -> List[Dict[str, Any]]:
        """blocking, one worker thread: ONE forward over the questions (token rows, not pooled), ONE scan of the token
        plane for all of them"""
        scorer = self._get_late()
        tokens, q_start, q_len, _ = scorer.encode_questions(list(texts))
        res = self.collection.late_query(tokens, q_start, q_len, n_results=n_results, where=filter_dict,
                                         include=self._INCLUDE)
        return [{key: res[key][at] for key in LATE_KEYS} for at in range(len(texts))]

    def _late_query_problem(self) -> Optional[str]:
        """why late_query cannot run on a collection that has the method, or None (checked before the engine call: a
        missing store is the caller's to fix, not a failure to retry)"""
        if hasattr(self.collection, "late_query") and not self.supports_late_query():
            return ("Late retrieval needs the token store: set MMRAG_LATE_STORE=1 before uploading, or call "
                    "EmbeddingManager.enable_late_store()")
        return None

    async def late_query(self, query_text: str, n_results: int = 5, filter_dict: Optional[Dict] = None) -> Dict[str, Any]:
        """First-stage late-interaction retrieval (VectorIndex.late_query, csrc/maxsim_scan.hip): the n_results stored
        items of highest MaxSim against the question's tokens, over ALL stored items that keep token rows -- a passage
        whose pooled cosine is middling but three of whose tokens answer the question is found.  One result dict with
        the keys of query() plus `late_scores` (the mean over the question's tokens of each token's best cosine;
        `distances` is 1 - that).  Needs the token store."""
        await self._ready()
        problem = self._late_query_problem()
        if problem:
            raise ValueError(problem)
        return await self._single("Late query", _NEEDS_LATE, self._answer_late, query_text, n_results, filter_dict)

    async def batch_late_query(self, queries: List[str], n_results: int = 5,
                               filter_dict: Optional[Dict] = None) -> List[Dict[str, Any]]:
        """batch_query's twin for late_query: one question forward and one scan for all the queries; a query that cannot
        be answered gets a dict with empty lists and an 'error' message."""
        await self._ready()
        problem = self._late_query_problem()
        if problem:
            return [{**copy.deepcopy(_EMPTY_LATE), "error": problem} for _ in queries]
        return await self._batch("Batch late query", _NEEDS_LATE, _EMPTY_LATE, self._answer_late, queries, n_results,
                                 filter_dict)

    def _late_score_sync(self, queries: List[str], results_list: List[Dict[str, Any]], explain: bool,
                         passages: Optional[int] = None):
        """ONE scoring call for every (queries[i], document of results_list[i]) pair, flat in that order: (scores,
        explain records | [], passages entries | []).  `passages` (a window size in tokens): the windows launch in place
        of the scores launch -- its out_sum is the score, so a re-rank orders as it does without; with `explain` as
        well, best_idx comes from a second launch."""
        scorer = self._get_late()
        docs: List[str] = []
        pairs: List[Tuple[int, int]] = []
        for at, results in enumerate(results_list):
            for d in results["documents"]:
                pairs.append((at, len(docs)))
                docs.append(d if d is not None else "")
        scores: Any = []
        records: List[Any] = []
        found: List[Any] = []
        if pairs:
            # hits whose token rows the store keeps are scored from the plane; the rest are encoded as before
            # (without a store, or when it keeps none of them, the scorer is called exactly as before).  An FP8 store's
            # plane is passed even when it keeps none of the hits: the scorer then quantises what it encodes, so a
            # passage scores the same whether or not its tokens are stored.  (Passages read the stored token ids too:
            # a passage's text is given only for the ids that were scored.)
            spans, plane = self._stored_spans(scorer, results_list, explain or passages is not None)
            store = getattr(self.collection, "token_store", None)
            plane_f8 = bool(spans) and store is not None and store.f8
            stored = {}
            if spans and (plane_f8 or any(s is not None for s in spans)):
                stored = {"spans": spans, "plane": plane}
                if plane_f8:
                    stored["plane_f8"] = True
            if explain:
                scores, records = scorer.explain_pairs(list(queries), docs, pairs, **stored)
            if passages is not None:
                windows = scorer.best_passages(list(queries), docs, pairs, int(passages), **stored)
                scores = [w["score"] for w in windows]
                given = [d for results in results_list for d in results["documents"]]
                found = [self._passage_of(scorer, d, w) for d, w in zip(given, windows)]
            elif not explain:
                scores = scorer.score_pairs(list(queries), docs, pairs, **stored)
        return scores, records, found

    def _late_rerank_sync(self, queries: List[str], results_list: List[Dict[str, Any]], top_k: Optional[int],
                          explain: bool, passages: Optional[int] = None) -> List[Dict[str, Any]]:
        scores, records, found = self._late_score_sync(queries, results_list, explain, passages)
        out, lo = [], 0
        for results in results_list:
            n = len(results["documents"])
            mine = [float(x) for x in scores[lo: lo + n]]
            order = sorted(range(n), key=lambda i: -mine[i])
            if top_k:
                order = order[:top_k]
            hit = {key: [results[key][i] for i in order] for key in RESULT_KEYS}
            hit["rerank_scores"] = [mine[i] for i in order]
            if explain:
                hit["late_matches"] = [records[lo + i] for i in order]
            if passages is not None:
                hit["passages"] = [found[lo + i] for i in order]
            out.append(hit)
            lo += n
        return out

    # ---- answer passages: the best window of each hit by windowed MaxSim (late.py, csrc/maxsim_windows.hip) ----
    def supports_passages(self) -> bool:
        """True when extract_passages can run: where late_rerank works (has_late_reranker: ONE BERT-family HIP engine in
        fp16 mode with a tokenizer -- not the CLIP towers, not the fp32 encoder mode) and the collection is not sharded"""
        return self.has_late_reranker() and not hasattr(self.collection, "load")     # serving.ShardedCollection

    @staticmethod
    def _passage_of(scorer, document: Optional[str], window: Dict[str, Any]) -> Dict[str, Any]:
        """One hit's `passages` entry from best_passages' record: where the tight span lies in the document's
        characters.  The document is tokenised again with character spans; the text is given only when that yields the
        very ids that were scored (for a stored passage: the ids the store keeps) -- a document that changed since it
        was stored, or a tokenizer without encode_with_spans, gives text None, as does a None document."""
        share = window["window_sum"] / window["sum"] if window["sum"] > 0 else None
        entry = {"text": None, "char_start": None, "char_end": None, "token_start": window["token_start"],
                 "token_end": window["token_end"], "score": window["window_score"], "share": share}
        encode = getattr(scorer.tokenizer, "encode_with_spans", None)
        if document is None or encode is None:
            return entry
        ids, spans = encode(document, scorer.max_doc_tokens + 2)
        first, count = (int(v[0]) for v in scorer.trimmed(np.array([len(ids)])))
        if [int(i) for i in ids[first: first + count]] != [int(i) for i in window["doc_ids"]]:
            return entry
        inside = spans[first + window["token_start"]: first + window["token_end"]]
        if not inside or first == 0:        # (a text without a single token: its [CLS] row stood in)
            return entry
        lo, hi = inside[0][0], max(e for _, e in inside)
        entry.update(text=document[lo:hi], char_start=lo, char_end=hi)
        return entry

    def _extract_passages_sync(self, queries: List[str], results_list: List[Dict[str, Any]],
                               window_tokens: Optional[int]) -> List[Dict[str, Any]]:
        if not self.supports_passages():
            raise ValueError("answer passages need a single BERT-family fp16 HIP engine with a tokenizer and a "
                             "collection that is not sharded")
        window = settings.passage_tokens() if window_tokens is None else int(window_tokens)
        _, _, found = self._late_score_sync(queries, results_list, False, passages=window)
        out, lo = [], 0
        for results in results_list:
            n = len(results["documents"])
            out.append({**results, "passages": found[lo: lo + n]})
            lo += n
        return out

    async def extract_passages(self, query_text: str, results: Dict[str, Any],
                               window_tokens: Optional[int] = None) -> Dict[str, Any]:
        """The answer passage of every hit of `results` (any retrieval mode's answer: only its `documents` and `ids` are
        read): the window of `window_tokens` tokens (default MMRAG_PASSAGE_TOKENS; whole blocks of 16) of the document
        that keeps the most of its MaxSim against `query_text`, narrowed to the blocks that hold some query token's best
        match (mmrag_maxsim_windows).  Returns `results` plus `passages`, one entry per hit, in the hits' order:
          text                     the document's characters from the first token's start to the last token's end; None
                                   for a None document and when tokenising the document does not give the ids that
                                   were scored (a stored passage: the ids the token store keeps)
          char_start, char_end     where that text lies in the document (None with it)
          token_start, token_end   the same span in scored tokens
          score                    the window's MaxSim mean, to be read next to a late re-rank score
          share                    window sum / whole passage's sum, None when the latter is not positive
        Hits whose token rows the store keeps are scored from the plane.  One encoder forward, one launch."""
        await self._ready()
        return (await asyncio.to_thread(self._extract_passages_sync, [query_text], [results], window_tokens))[0]

    async def batch_extract_passages(self, queries: List[str], results_list: List[Dict[str, Any]],
                                     window_tokens: Optional[int] = None) -> List[Dict[str, Any]]:
        """extract_passages of results_list[i] against queries[i], ONE scoring call for all"""
        if len(queries) != len(results_list):
            raise ValueError(f"{len(results_list)} result dicts for {len(queries)} queries")
        await self._ready()
        return await asyncio.to_thread(self._extract_passages_sync, list(queries), list(results_list), window_tokens)

    # ---- extractive summaries and answers: sentence centrality + MMR (summarize.py, csrc/summarize.hip) ----
    def supports_summaries(self) -> bool:
        """True when summarize_texts / extract_answer can run: the engine leaves its embeddings on the device
        (encode_device: the HIP engine; not the CLIP towers, not a sharded engine without it)"""
        return hasattr(self._engine, "encode_device")

    def _summarizer(self):
        from .summarize import DeviceSummarizer

        if not self.supports_summaries():
            raise ValueError("extractive summaries need an engine with encode_device (the single-GPU HIP engine)")
        dtype = getattr(self.collection, "dtype", None)
        return DeviceSummarizer(self._engine, dtype if dtype is not None else settings.index_dtype())

    async def summarize_texts(self, texts: List[str], max_length: int = 300, by_lines: bool = False,
                              questions: Optional[Sequence[Optional[str]]] = None) -> List[Dict[str, Any]]:
        """An extractive summary of every text, at most `max_length` characters: its most central sentences
        (`by_lines`: lines, for tables) in document order -- summarize.DeviceSummarizer.summarize.  One encoder call
        over all sentences of all texts, one mmrag_summary_select launch, one copy back.  Per text {"summary", "spans",
        "scores"}; `questions` (one per text, None allowed) bias a text's selection toward a question."""
        await self._ready()
        worker = self._summarizer()
        async with self._encode_lock:
            return await asyncio.to_thread(worker.summarize, list(texts), max_length, questions, by_lines)

    async def extract_answer(self, question: str, passages: Sequence[str], max_chars: int = 600,
                             top_sentences: int = 8) -> Dict[str, Any]:
        """A query-focused extract of `passages` (the hits' raw texts, in rank order): at most `top_sentences` of their
        sentences, `max_chars` characters in all, central to the passages AND close to `question`, none repeating
        another (summarize.DeviceSummarizer.answer).  {"answer", "quotes": [{"passage", "start", "end", "text",
        "score"} ...] ordered by (passage, start), "considered": the number of sentences that took part (at most
        128)}."""
        await self._ready()
        worker = self._summarizer()
        async with self._encode_lock:
            return await asyncio.to_thread(worker.answer, question, list(passages), max_chars, top_sentences)

    # ---- answer citations: sentence-to-source attribution (attribution.py, csrc/attribute.hip) ----
    def supports_citations(self) -> bool:
        """True when attribute_answer can run: supports_summaries' requirement (an engine with encode_device)"""
        return self.supports_summaries()

    def _attributor(self):
        from .attribution import DeviceAttributor

        if not self.supports_citations():
            raise ValueError("answer citations need an engine with encode_device (the single-GPU HIP engine)")
        dtype = getattr(self.collection, "dtype", None)
        return DeviceAttributor(self._engine, dtype if dtype is not None else settings.index_dtype())

    async def attribute_answer(self, answer: str, passages: Sequence[str], owner: Optional[Sequence[int]] = None,
                               threshold: Optional[float] = None, max_citations: Optional[int] = None) -> Dict[str, Any]:
        """Which source stands behind which sentence of `answer`: `passages` are the sources' raw texts in rank order,
        owner[i] the source passage i belongs to (default i).  Similarity of sentence embeddings, not entailment
        (attribution.DeviceAttributor.attribute).  {"citations": per sentence {"start", "end", "text", "score",
        "supported", "sources": [{"source", "passage", "start", "end", "text", "score"} ...]}, "groundedness",
        "support": per source, "considered": {"claims", "evidence"}}.  `threshold` (default
        MMRAG_CITATION_THRESHOLD) is the cosine at which a sentence counts as supported and a source as cited,
        `max_citations` (default MMRAG_CITATION_MAX, 1..8) the most sources a sentence cites."""
        return (await self.batch_attribute_answers([answer], [passages], None if owner is None else [owner],
                                                   threshold, max_citations))[0]

    async def batch_attribute_answers(self, answers: Sequence[str], passages_list: Sequence[Sequence[str]],
                                      owners: Optional[Sequence[Optional[Sequence[int]]]] = None,
                                      threshold: Optional[float] = None,
                                      max_citations: Optional[int] = None) -> List[Dict[str, Any]]:
        """attribute_answer of answers[i] against passages_list[i]: ONE encoder call and ONE mmrag_attribute launch
        for all of them"""
        await self._ready()
        worker = self._attributor()
        async with self._encode_lock:
            return await asyncio.to_thread(worker.attribute, list(answers), [list(p) for p in passages_list], owners,
                                           None, max_citations, threshold)

    # ---- semantic chunking: topic-boundary segmentation (chunking.py, csrc/chunk.hip) ----
    def supports_chunking(self) -> bool:
        """True when chunk_texts can run: supports_summaries' requirement (an engine with encode_device)"""
        return self.supports_summaries()

    async def chunk_texts(self, texts: List[str], chunk_size: Optional[int] = None) -> List[List[Dict[str, Any]]]:
        """The semantic chunks of every text, none longer than `chunk_size` (default CHUNK_SIZE) characters: the text
        cut where its topic changes -- chunking.DeviceChunker.chunk_texts.  One encoder call over all sentences of all
        texts, one mmrag_chunk_boundaries launch, one copy back.  Per text a list of {"content", "start", "end",
        "sentences", "gain"} in order."""
        from .chunking import DeviceChunker

        await self._ready()
        if not self.supports_chunking():
            raise ValueError("semantic chunking needs an engine with encode_device (the single-GPU HIP engine)")
        dtype = getattr(self.collection, "dtype", None)
        worker = DeviceChunker(self._engine, dtype if dtype is not None else settings.index_dtype())
        async with self._encode_lock:
            return await asyncio.to_thread(worker.chunk_texts, list(texts), chunk_size)

    async def late_rerank(self, query_text: str, results: Dict[str, Any], top_k: Optional[int] = None,
                          explain: bool = False, passages: Optional[int] = None) -> Dict[str, Any]:
        """Re-rank `results` (any retrieval mode's answer: only its `documents` are read) by late interaction with the
        bi-encoder itself: every (query_text, document) pair scores the mean over the query's tokens of each token's
        best cosine against the document's tokens.  Output as the cross-encoder path's: reordered by descending score
        (stable), truncated to top_k, with `rerank_scores`; `explain` adds `late_matches`, per hit one dict per query
        token (query_token, doc_token, doc_index, similarity).  One encoder forward and one MaxSim launch.
        `passages` (a window size in tokens): the hits also carry `passages`, extract_passages' entries in the new
        order, from the same call -- the windows launch stands in for the scores launch and its sum is the score."""
        await self._ready()
        return (await asyncio.to_thread(self._late_rerank_sync, [query_text], [results], top_k, explain, passages))[0]

    async def batch_late_rerank(self, queries: List[str], results_list: List[Dict[str, Any]],
                                top_k: Optional[int] = None, passages: Optional[int] = None) -> List[Dict[str, Any]]:
        """late_rerank of results_list[i] against queries[i], ONE scoring call (one forward, one launch) for all"""
        if len(queries) != len(results_list):
            raise ValueError(f"{len(results_list)} result dicts for {len(queries)} queries")
        await self._ready()
        return await asyncio.to_thread(self._late_rerank_sync, list(queries), list(results_list), top_k, False,
                                       passages)

    async def rerank_results(self, query_text: str, results: Dict[str, Any],
                             top_k: Optional[int] = None, method: Optional[str] = None,
                             explain: bool = False, passages: Optional[int] = None) -> Dict[str, Any]:
        """embedder.py:834-859.  `method`: "cross" or "late" (default MMRAG_RERANK_METHOD, whose default is "cross").
        "late": late_rerank (the bi-encoder's token rows; `explain` adds `late_matches`, `passages` -- a window size in
        tokens, late only -- adds `passages`).  "cross", without a
        cross-encoder (MMRAG_RERANKER_DIR empty): the reference's placeholder -- no
        re-ranking, only truncation to top_k.  With one: every (query_text, document) pair is scored (a None document
        as ""), the results are reordered by descending score (stable: ties keep the search order), truncated to top_k
        and carry their scores in `rerank_scores` (a multi-label model's first logit column is the score)."""
        method = method or settings.rerank_method()
        if method not in ("cross", "late"):
            raise ValueError(f"rerank method must be 'cross' or 'late', not {method!r}")
        if passages is not None and method != "late":
            raise ValueError("`passages` rides on late-interaction re-ranking: use method 'late', or extract_passages "
                             "on the re-ranked hits")
        if method == "late":
            more = {} if passages is None else {"passages": passages}
            return await self.late_rerank(query_text, results, top_k=top_k, explain=explain, **more)
        if not self.has_reranker():
            logger.warning("Re-ranking not implemented yet")
            if top_k and top_k < len(results["ids"]):
                return {key: results[key][:top_k] for key in RESULT_KEYS}
            return results
        reranker = self._reranker if self._reranker is not None else await asyncio.to_thread(self._get_reranker)
        docs = [d if d is not None else "" for d in results["documents"]]
        scores = await asyncio.to_thread(reranker.predict, [(query_text, d) for d in docs]) if docs else []
        scores = [float(x) for x in np.asarray(scores, np.float64).reshape(len(docs), -1)[:, 0]] if docs else []
        order = sorted(range(len(docs)), key=lambda i: -scores[i])
        if top_k:
            order = order[:top_k]
        out = {key: [results[key][i] for i in order] for key in RESULT_KEYS}
        out["rerank_scores"] = [scores[i] for i in order]
        return out

    # ------------------------------------------------------------------ maintenance ---------
    async def delete_document(self, doc_id: str):
        """embedder.py:619-656: drop every row whose metadata carries this doc_id."""
        await self._ready()
        gone = await self._engine_call(f"Delete of document {doc_id}", self.collection.delete, where={"doc_id": doc_id})
        if gone:
            logger.info("Deleted %d embeddings for doc %s", len(gone), doc_id)
        else:
            logger.warning("No embeddings found for doc %s", doc_id)

    async def delete_all_documents(self):
        """embedder.py:658-688: a fresh collection under the same name, and an empty cache."""
        await self._ready()
        try:
            self.collection = await asyncio.to_thread(self._engine.new_collection, settings.CHROMA_COLLECTION_NAME,
                                                      dict(_COLLECTION_NOTE))
        except Exception as e:
            logger.error("Failed to delete all documents: %s", e)
            raise
        if self.cache:
            self.cache.clear()

    async def get_collection_stats(self) -> Dict[str, Any]:
        """embedder.py:690-728 (same keys; an engine failure is reported in the dict, not raised)."""
        await self._ready()
        try:
            report = {
                "name": settings.CHROMA_COLLECTION_NAME,
                "count": await asyncio.to_thread(self.collection.count),
                "model": settings.SENTENCE_TRANSFORMER_MODEL,
                "device": self.device,
                "embedding_dim": self.get_embedding_dimension(),
                "batch_size": self.batch_size,
                "stats": {key: self.stats[key] for key in ("total_embeddings_created", "total_items_stored",
                                                           "total_queries")},
            }
        except Exception as e:
            logger.error("Failed to get collection stats: %s", e)
            return {"name": settings.CHROMA_COLLECTION_NAME, "count": 0, "error": str(e)}
        if hasattr(self.collection, "bytes_per_row"):   # a VectorIndex: how its rows are stored
            report["index_dtype"] = str(self.collection.dtype).split(".")[-1]
            report["bytes_per_row"] = self.collection.bytes_per_row()
        if getattr(self.collection, "token_store", None) is not None:     # tokens and bytes of the late store
            report["late_store"] = self.collection.token_stats()
        if getattr(self.collection, "positions_enabled", False):          # the positions plane, once a phrase query built it
            report["lexical_positions_bytes"] = self.collection.positions_bytes()
        if self.cache:
            report["cache"] = self.cache.get_stats()
        return report

    def get_stage_timers(self) -> Dict[str, Dict[str, float]]:
        """Not in the reference (it only logs time.time() deltas): wall clock per stage of this process' requests --
        tokenize / encode / search / collect, shard.* in the sharded service -- see tracing.py."""
        return tracing.snapshot()

    async def get_stats(self) -> Dict[str, Any]:
        """api.py:472 calls this name; the reference class only defines get_collection_stats."""
        return await self.get_collection_stats()

    def get_embedding_dimension(self) -> int:
        """embedder.py:730-734 (384 while no model is loaded)."""
        return int(self.text_model.dim) if self.text_model else 384

    async def warmup_cache(self, common_queries: List[str]):
        """embedder.py:744-762."""
        if not self.cache:
            logger.warning("Cache not enabled, skipping warmup")
            return
        await self.embed_texts_batch(common_queries, show_progress=False)

    async def get_cache_stats(self) -> Dict[str, Any]:
        """embedder.py:764-772."""
        return {"enabled": True, **self.cache.get_stats()} if self.cache else {"enabled": False}

    async def clear_cache(self):
        """embedder.py:774-780."""
        if self.cache:
            self.cache.clear()
        else:
            logger.warning("Cache not enabled")
