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


class QueryDispatcher:
    def __init__(self, batch_fn: BatchFn, max_batch: int = 256, max_wait_ms: float = 2.0, idle_ms: float = 0.25,
                 scoped_fn: Optional[ScopedFn] = None, boosted_fn: Optional[BoostedFn] = None):
        self.batch_fn = batch_fn
        self.scoped_fn = scoped_fn
        self.boosted_fn = boosted_fn
        self.max_batch = max_batch
        self.max_wait = max_wait_ms / 1e3
        # a batch also closes when nothing new has arrived for `idle_ms`: with a fixed set of callers that all come back
        # right after their answers, waiting out the whole window for requests that cannot exist is a quarter of the cycle
        self.idle = idle_ms / 1e3
        # (text, k, filter, the caller's future, doc_ids, boost spec)
        self._queue: "asyncio.Queue[Tuple[str, int, Optional[Dict], asyncio.Future, Optional[List[str]], Any]]" = \
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
                     doc_ids: Optional[List[str]] = None, boost: Any = None) -> Dict[str, Any]:
        """`boost`: a boost spec (an object with a canonical `batch_key()`; needs a `boosted_fn`): the request is ranked with
        that score prior, and requests of one k, filter and spec key share one batch.
        `doc_ids`: answer from these documents only.  With a `scoped_fn`, requests that carry doc_ids and no
        filter_dict share one batch per k whatever their documents; without one (or next to a filter_dict) the
        restriction becomes part of the filter and the request is grouped by it like any other."""
        if boost is not None and (self.boosted_fn is None or doc_ids is not None):
            raise ValueError("a boosted request needs a boosted_fn and takes no doc_ids")
        self.start()
        if doc_ids is not None and (self.scoped_fn is None or filter_dict is not None):
            only = {"doc_id": {"$in": list(doc_ids)}}
            filter_dict, doc_ids = ({"$and": [filter_dict, only]} if filter_dict else only), None
        fut: asyncio.Future = asyncio.get_running_loop().create_future()
        await self._queue.put((text, n_results, filter_dict, fut, doc_ids, boost))
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
            # one kernel batch per (k, filter) group; the requests with doc_ids are one group per k, the boosted ones
            # one per (k, filter, spec key)
            groups: Dict[Any, List[int]] = {}
            for i, (_, k, flt, _, docs, boost) in enumerate(batch):
                if boost is not None:
                    key = ("boosted", k, repr(flt), boost.batch_key())
                elif docs is not None:
                    key = ("scoped", k)
                else:
                    key = ("plain", k, repr(flt))
                groups.setdefault(key, []).append(i)
            for key, idxs in groups.items():
                k, flt = batch[idxs[0]][1], batch[idxs[0]][2]
                try:
                    if key[0] == "boosted":
                        results = await self.boosted_fn([batch[i][0] for i in idxs], k, flt, batch[idxs[0]][5])
                    elif key[0] == "scoped":
                        results = await self.scoped_fn([batch[i][0] for i in idxs], k, [batch[i][4] for i in idxs])
                    else:
                        results = await self.batch_fn([batch[i][0] for i in idxs], k, flt)
                    for i, res in zip(idxs, results):
                        fut = batch[i][3]
                        if fut.done():
                            continue
                        if isinstance(res, dict) and "error" in res:
                            fut.set_exception(ValueError(res["error"]) if "empty" in res["error"]
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
