"""Dynamic batching in front of `EmbeddingManager.query`.

The service issues batch-of-1 queries (api.py:338).  The dispatcher collects concurrent requests
for up to `max_wait_ms` (or `max_batch` requests), runs ONE batched encode + ONE
[B, d] x [N, d]^T search for them, and resolves each caller's future -- this is what converts the
kernel's batched throughput into served queries/s, and it also serialises device work (and, in a
multi-GPU deployment, the RCCL collectives) through a single task.
"""
from __future__ import annotations

import asyncio
import time
from typing import Any, Awaitable, Callable, Dict, List, Optional, Tuple

BatchFn = Callable[[List[str], int, Optional[Dict]], Awaitable[List[Dict[str, Any]]]]
# (texts, k, each text's doc_ids): ONE batched encode and ONE scoped search whatever the scopes (csrc/scoped.hip)
ScopedFn = Callable[[List[str], int, List[List[str]]], Awaitable[List[Dict[str, Any]]]]
# (texts, k, filter, the batch's boost spec): ONE batched encode and ONE boosted search (csrc/boosted.hip)
BoostedFn = Callable[[List[str], int, Optional[Dict], Any], Awaitable[List[Dict[str, Any]]]]
# (requests, k, filter): ONE encode of every request's texts and ONE recommend search (csrc/recommend.hip).  An 'error'
# dict it returns is the request's own fault (a ValueError for its caller); anything else it raises
# (texts, k, each text's filter or None): ONE batched encode and ONE filtered search whatever the filters
# (csrc/filtered.hip)
FilteredFn = Callable[[List[str], int, List[Optional[Dict]]], Awaitable[List[Dict[str, Any]]]]
RecommendFn = Callable[[List[Dict[str, Any]], int, Optional[Dict]], Awaitable[List[Dict[str, Any]]]]
# (texts, k, filter): ONE expansion of the questions and ONE impact search (csrc/sparse_expand.hip, csrc/sparse_score.hip)
SparseFn = Callable[[List[str], int, Optional[Dict]], Awaitable[List[Dict[str, Any]]]]


class QueryDispatcher:
    def __init__(self, batch_fn: BatchFn, max_batch: int = 256, max_wait_ms: float = 2.0, idle_ms: float = 0.25,
                 scoped_fn: Optional[ScopedFn] = None, boosted_fn: Optional[BoostedFn] = None,
                 recommend_fn: Optional[RecommendFn] = None, filtered_fn: Optional[FilteredFn] = None,
                 sparse_fn: Optional[SparseFn] = None):
        self.batch_fn = batch_fn
        self.sparse_fn = sparse_fn
        self.filtered_fn = filtered_fn
        self.scoped_fn = scoped_fn
        self.boosted_fn = boosted_fn
        self.recommend_fn = recommend_fn
        self.max_batch = max_batch
        self.max_wait = max_wait_ms / 1e3
        # a batch also closes when nothing new has arrived for `idle_ms`: with a fixed set of callers that all come back
        # right after their answers, waiting out the whole window for requests that cannot exist is a quarter of the cycle
        self.idle = idle_ms / 1e3
        # (text, k, filter, the caller's future, doc_ids, boost spec, recommend request, learned sparse?)
        self._queue: "asyncio.Queue[Tuple[str, int, Optional[Dict], asyncio.Future, Optional[List[str]], Any, Any, bool]]" = \
            asyncio.Queue()
        self._task: Optional[asyncio.Task] = None
        self.stats = {"requests": 0, "batches": 0, "max_batch_seen": 0}

    def start(self):
        if self._task is None or self._task.done():
            self._task = asyncio.get_running_loop().create_task(self._run())

    async def stop(self):
        if self._task is not None:
            self._task.cancel()
            try:
                await self._task
            except asyncio.CancelledError:
                pass
            self._task = None

    async def submit(self, text: str, n_results: int = 5, filter_dict: Optional[Dict] = None,
                     doc_ids: Optional[List[str]] = None, boost: Any = None,
                     recommend: Optional[Dict[str, Any]] = None, sparse: bool = False) -> Dict[str, Any]:
        """`sparse`: answer by learned sparse retrieval (needs a `sparse_fn`; takes no doc_ids, boost or recommend
        request): requests of one k and one filter share one batch -- one expansion forward, one impact search.
        `recommend`: a request of positive and negative examples (EmbeddingManager.recommend's dict; needs a
        `recommend_fn`; `text` is not read): requests of one k -- and one filter, which is one alive bitmap per scan --
        share one batch whatever their examples.
        `boost`: a boost spec (an object with a canonical `batch_key()`; needs a `boosted_fn`): the request is ranked with
        that score prior, and requests of one k, filter and spec key share one batch.
        `doc_ids`: answer from these documents only.  With a `scoped_fn`, requests that carry doc_ids and no
        filter_dict share one batch per k whatever their documents; without one (or next to a filter_dict) the
        restriction becomes part of the filter and the request is grouped by it like any other.
        With a `filtered_fn`, requests that carry a filter_dict (doc_ids folded into it included) and neither a boost
        nor a recommend request share one batch per k whatever their filters."""
        if boost is not None and (self.boosted_fn is None or doc_ids is not None):
            raise ValueError("a boosted request needs a boosted_fn and takes no doc_ids")
        if recommend is not None and (self.recommend_fn is None or doc_ids is not None or boost is not None):
            raise ValueError("a recommend request needs a recommend_fn and takes neither doc_ids nor a boost")
        if sparse and (self.sparse_fn is None or doc_ids is not None or boost is not None or recommend is not None):
            raise ValueError("a sparse request needs a sparse_fn and takes no doc_ids, boost or recommend request")
        self.start()
        if doc_ids is not None and (self.scoped_fn is None or filter_dict is not None):
            only = {"doc_id": {"$in": list(doc_ids)}}
            filter_dict, doc_ids = ({"$and": [filter_dict, only]} if filter_dict else only), None
        fut: asyncio.Future = asyncio.get_running_loop().create_future()
        await self._queue.put((text, n_results, filter_dict, fut, doc_ids, boost, recommend, bool(sparse)))
        return await fut

    async def _run(self):
        while True:
            first = await self._queue.get()
            batch = [first]
            deadline = time.monotonic() + self.max_wait
            while len(batch) < self.max_batch:
                try:                                  # whatever is already queued costs no await
                    batch.append(self._queue.get_nowait())
                    continue
                except asyncio.QueueEmpty:
                    pass
                timeout = min(deadline - time.monotonic(), self.idle)
                if timeout <= 0:
                    break
                try:
                    batch.append(await asyncio.wait_for(self._queue.get(), timeout))
                except asyncio.TimeoutError:
                    break
            # one kernel batch per (k, filter) group (per k alone with a filtered_fn, for the requests that carry a
            # filter); the requests with doc_ids are one group per k, the boosted ones
            # one per (k, filter, spec key), the recommend ones one per (k, filter)
            groups: Dict[Any, List[int]] = {}
            for i, (_, k, flt, _, docs, boost, rec, sparse) in enumerate(batch):
                if sparse:
                    key = ("sparse", k, repr(flt))
                elif rec is not None:
                    key = ("recommend", k, repr(flt))
                elif boost is not None:
                    key = ("boosted", k, repr(flt), boost.batch_key())
                elif docs is not None:
                    key = ("scoped", k)
                elif flt is not None and self.filtered_fn is not None:
                    key = ("filtered", k)
                else:
                    key = ("plain", k, repr(flt))
                groups.setdefault(key, []).append(i)
            for key, idxs in groups.items():
                k, flt = batch[idxs[0]][1], batch[idxs[0]][2]
                try:
                    if key[0] == "sparse":
                        results = await self.sparse_fn([batch[i][0] for i in idxs], k, flt)
                    elif key[0] == "recommend":
                        results = await self.recommend_fn([batch[i][6] for i in idxs], k, flt)
                    elif key[0] == "boosted":
                        results = await self.boosted_fn([batch[i][0] for i in idxs], k, flt, batch[idxs[0]][5])
                    elif key[0] == "scoped":
                        results = await self.scoped_fn([batch[i][0] for i in idxs], k, [batch[i][4] for i in idxs])
                    elif key[0] == "filtered":
                        results = await self.filtered_fn([batch[i][0] for i in idxs], k, [batch[i][2] for i in idxs])
                    else:
                        results = await self.batch_fn([batch[i][0] for i in idxs], k, flt)
                    for i, res in zip(idxs, results):
                        fut = batch[i][3]
                        if fut.done():
                            continue
                        if isinstance(res, dict) and "error" in res:
                            # (a recommend_fn raises what is not the request's own fault: its error dicts are all
                            # broken request rules and unknown ids)
                            fut.set_exception(ValueError(res["error"])
                                              if "empty" in res["error"] or key[0] == "recommend"
                                              else RuntimeError(res["error"]))
                        else:
                            fut.set_result(res)
                except Exception as e:  # the whole batch failed
                    for i in idxs:
                        if not batch[i][3].done():
                            batch[i][3].set_exception(e)
                self.stats["batches"] += 1
                self.stats["max_batch_seen"] = max(self.stats["max_batch_seen"], len(idxs))
            self.stats["requests"] += len(batch)
