"""Measure semantic chunking (csrc/chunk.hip): the `mmrag_chunk_boundaries` launch alone for 256 documents of 64, 128
and 300 sentences, beside the `encode_device` call over the same sentences (which is expected to dominate), and the
wall clock of an `/upload` of one file under MMRAG_CHUNKER=basic (the parent commit's path: `basic_chunk_text`) and
=semantic.

    python tools/chunk_bench.py [--quick] [--sentences 64 128 300]

MiniLM shape with seeded random weights and the hash tokenizer; sentences of 8 random words; fp16 rows, d = 384,
W = 64, max_cost 1000, the automatic tau (auto_scale 0.5), penalty 0.  `launch_us` is a device-event window around 20
back-to-back calls of the Python entry divided by 20, median of 5 windows after the same call has been held for 0.5 s:
the kernels run back to back, so this is the kernel's time once it exceeds the host's way to the launch (some 10 us).
`encode_device_us`: events around ONE call, median of 5.  The upload is the median of 5 wall-clock times of the route
for one text of about 640 sentences, the two settings alternating.  One process.  Prints one JSON object per
measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd import _native  # noqa: E402
from multimodal_rag_amd import embedder as EM  # noqa: E402

WORDS = ("solar panel light power grid cell silicon current inverter storage wind turbine bread dough crust oven "
         "flour water salt yeast river bridge stone arch traffic signal road train station ticket").split()


def sentence(rng, words=8):
    return " ".join(rng.choice(WORDS, words)).capitalize() + "."


def window_us(fn, calls, reps=5, hold=0.5):
    """median over `reps` event windows of (time of `calls` back-to-back calls) / calls, in microseconds"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < hold:
        for _ in range(8):
            fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / calls)
    return round(float(np.median(ts)), 1)


def kernel_and_encoder(engine, docs, per_doc, hold):
    rng = np.random.default_rng(docs * per_doc)
    texts = [sentence(rng) for _ in range(docs * per_doc)]
    emb = engine.encode_device(texts)
    d = int(emb.shape[1])
    rows = torch.zeros((len(texts), _native.padded_dim(d, torch.float16)), dtype=torch.float16, device=emb.device)
    rows[:, :d] = emb.half()

    def i32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(emb.device)

    tables = [i32(np.arange(docs) * per_doc), i32(np.full(docs, per_doc)), i32([len(t) + 1 for t in texts])]
    kw = dict(auto_scale=0.5, penalty=0.0)
    out = _native.chunk_boundaries(rows, d, *tables, 1000, 64, **kw)
    rec = {"what": "chunk_boundaries", "docs": docs, "sentences_per_doc": per_doc, "dim": d}
    rec["launch_us"] = window_us(lambda: _native.chunk_boundaries(rows, d, *tables, 1000, 64, out=out, **kw), 20,
                                 hold=hold)
    rec["encode_device_us"] = window_us(lambda: engine.encode_device(texts), 1, hold=0.0)
    print(json.dumps(rec), flush=True)


def upload(manager, paragraphs=40):
    from starlette.testclient import TestClient

    from multimodal_rag_amd.server import create_app

    rng = np.random.default_rng(1)
    text = "\n\n".join(" ".join(sentence(rng) for _ in range(16)) for _ in range(paragraphs)).encode("utf-8")
    rec = {"what": "upload", "bytes": len(text)}
    times = {"basic": [], "semantic": []}
    for _ in range(6):
        for setting in times:
            EM.settings.MMRAG_CHUNKER = setting
            with TestClient(create_app(embedder=manager)) as client:
                t0 = time.perf_counter()
                up = client.post("/upload", files={"file": ("bench.txt", text, "text/plain")})
                times[setting].append(time.perf_counter() - t0)
                assert up.status_code == 200, up.text
                rec[f"{setting}_chunks"] = up.json()["chunks_processed"]["text"]
    for setting, ts in times.items():
        rec[f"{setting}_ms"] = round(float(np.median(ts[1:])) * 1e3, 2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="no hold, the kernel shapes only (for a rocprofv3 run)")
    ap.add_argument("--sentences", type=int, nargs="*", default=[64, 128, 300], help="sentences per document")
    args = ap.parse_args()
    EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION = "", "fp16"
    engine = EM.HipEngine("sentence-transformers/all-MiniLM-L6-v2")
    for per_doc in args.sentences:
        kernel_and_encoder(engine, 256, per_doc, 0.0 if args.quick else 0.5)
    if not args.quick:
        upload(EM.EmbeddingManager(engine=engine, enable_cache=False))


if __name__ == "__main__":
    main()
