"""Measure answer citations (csrc/attribute.hip) at ONE shape: an answer of 8 sentences against 5 hits of 20 sentences
each -- the `mmrag_attribute` launch alone, the `encode_device` call over the same 108 sentences, and the wall clock of
the whole `EmbeddingManager.attribute_answer`.

    python tools/attribution_bench.py

MiniLM shape with seeded random weights and the hash tokenizer; sentences of 8 random words; fp16 rows, d = 384, 5
sources, m = 3.  `launch_us` is a device-event window around 20 back-to-back calls of the Python entry divided by 20,
median of 5 windows after the same call has been held for 0.5 s (tools/chunk_bench.py's method: the kernel's time plus
whatever of the host's way to the launch is not hidden behind the previous kernel; not a profiler figure).
`encode_device_us`: events around ONE call, median of 5.  `attribute_answer_ms`: the median of 9 wall-clock times after
one warm-up call.  One process.  Prints one JSON object."""
import asyncio
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402
from multimodal_rag_amd import embedder as EM  # noqa: E402
from tools.chunk_bench import sentence, window_us  # noqa: E402

CLAIMS, HITS, PER_HIT = 8, 5, 20


def main():
    EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION = "", "fp16"
    EM.settings.MMRAG_INDEX_DTYPE = "float16"
    engine = EM.HipEngine("sentence-transformers/all-MiniLM-L6-v2")
    rng = np.random.default_rng(8520)
    evidence = [[sentence(rng) for _ in range(PER_HIT)] for _ in range(HITS)]
    claims = [sentence(rng) for _ in range(CLAIMS)]
    passages, answer = [" ".join(hit) for hit in evidence], " ".join(claims)
    texts = [s for hit in evidence for s in hit] + claims
    emb = engine.encode_device(texts)
    d, n_ev = int(emb.shape[1]), HITS * PER_HIT
    rows = torch.zeros((len(texts), _native.padded_dim(d, torch.float16)), dtype=torch.float16, device=emb.device)
    rows[:, :d] = emb.half()

    def i32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(emb.device)

    tables = [i32([n_ev]), i32([CLAIMS]), i32([0]), i32([n_ev]),
              i32(np.concatenate([np.repeat(np.arange(HITS), PER_HIT), np.full(CLAIMS, -1)]))]
    out = _native.attribute(rows, d, *tables, HITS, 3, CLAIMS, want_support=False)
    rec = {"what": "attribute", "claims": CLAIMS, "hits": HITS, "sentences_per_hit": PER_HIT, "dim": d}
    rec["launch_us"] = window_us(lambda: _native.attribute(rows, d, *tables, HITS, 3, CLAIMS, want_support=False,
                                                           out=out), 20)
    rec["encode_device_us"] = window_us(lambda: engine.encode_device(texts), 1, hold=0.0)
    manager = EM.EmbeddingManager(engine=engine, enable_cache=False)
    asyncio.run(manager.initialize())
    times = []
    for _ in range(10):
        t0 = time.perf_counter()
        got = asyncio.run(manager.attribute_answer(answer, passages, threshold=0.5))
        times.append(time.perf_counter() - t0)
    assert got["considered"] == {"claims": CLAIMS, "evidence": n_ev}
    rec["attribute_answer_ms"] = round(float(np.median(times[1:])) * 1e3, 2)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
