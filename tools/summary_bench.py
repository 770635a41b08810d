"""Measure extractive summaries (csrc/summarize.hip): the `mmrag_summary_select` launch alone for 256 units of 16 and
of 128 sentences, beside the `encode_device` call over the same sentences (which is expected to dominate), and the
wall clock of an `/upload` of one file under MMRAG_SUMMARIZER=fallback and =extractive.

    python tools/summary_bench.py [--quick] [--sentences 16 128]

MiniLM shape with seeded random weights and the hash tokenizer; sentences of 8 random words; fp16 rows, d = 384,
t = 0.1, alpha = 0.15, T = 32, lambda = 0.7, budget 300, k = 16.  `select_us` and `encode_device_us` are HIP events
around ONE call of the Python entry, median of 20 (5) calls after the same call has been held for 0.5 s (DESIGN.md
section 3.1c): for a launch this short that is mostly the host's way to the launch.  The kernel's own time comes from a
separate `tools/prof_cmd.sh <tag> python tools/summary_bench.py --quick --sentences N` run (rocprofv3 kernel stats), one
shape per run so the kernel's row is one shape's.  The upload is the median of 5 wall-clock times of the route, about
40 chunks of about 800 characters.  One process.  Prints one JSON object per measurement."""
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
from multimodal_rag_amd.summarize import summary_parameters  # noqa: E402


def timed(fn, reps=20, hold=0.5):
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
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return round(float(np.median(ts)), 1)

WORDS = ("solar panel light power grid cell silicon current inverter storage wind turbine bread dough crust oven "
         "flour water salt yeast river bridge stone arch traffic signal road train station ticket").split()


def sentence(rng, words=8):
    return " ".join(rng.choice(WORDS, words)).capitalize() + "."


def kernel_and_encoder(engine, units, per_unit, hold):
    rng = np.random.default_rng(units * per_unit)
    texts = [sentence(rng) for _ in range(units * per_unit)]
    emb = engine.encode_device(texts)
    d = int(emb.shape[1])
    rows = torch.zeros((len(texts), _native.padded_dim(d, torch.float16)), dtype=torch.float16, device=emb.device)
    rows[:, :d] = emb.half()

    def i32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(emb.device)

    tables = [i32(np.arange(units) * per_unit), i32(np.full(units, per_unit)),
              i32([len(t) + 1 for t in texts]), i32(np.full(units, 301))]
    k = min(16, per_unit)
    out = _native.summary_select(rows, d, *tables, k, **summary_parameters())
    rec = {"what": "summary_select", "units": units, "sentences_per_unit": per_unit, "dim": d, "k": k}
    rec["select_us"] = timed(lambda: _native.summary_select(rows, d, *tables, k, out=out, **summary_parameters()),
                             hold=hold)
    rec["encode_device_us"] = timed(lambda: engine.encode_device(texts), reps=5, hold=hold)
    print(json.dumps(rec), flush=True)


def upload(manager, chunks=40):
    from starlette.testclient import TestClient

    from multimodal_rag_amd.server import create_app

    rng = np.random.default_rng(1)
    text = "\n\n".join(" ".join(sentence(rng) for _ in range(16)) for _ in range(chunks)).encode("utf-8")
    rec = {"what": "upload", "bytes": len(text)}
    for setting in ("fallback", "extractive"):
        EM.settings.MMRAG_SUMMARIZER = setting
        with TestClient(create_app(embedder=manager)) as client:
            ts = []
            for _ in range(6):
                t0 = time.perf_counter()
                up = client.post("/upload", files={"file": ("bench.txt", text, "text/plain")})
                ts.append(time.perf_counter() - t0)
                assert up.status_code == 200, up.text
                rec["chunks"] = up.json()["chunks_processed"]["text"]
            rec[f"{setting}_ms"] = round(float(np.median(ts[1:])) * 1e3, 2)
    rec["added_ms_per_chunk"] = round((rec["extractive_ms"] - rec["fallback_ms"]) / rec["chunks"], 3)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="no hold, the kernel shapes only (for a rocprofv3 run)")
    ap.add_argument("--sentences", type=int, nargs="*", default=[16, 128], help="sentences per unit of the shapes run")
    args = ap.parse_args()
    EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION = "", "fp16"
    engine = EM.HipEngine("sentence-transformers/all-MiniLM-L6-v2")
    hold = 0.0 if args.quick else 0.5
    for per_unit in args.sentences:
        kernel_and_encoder(engine, 256, per_unit, hold)
    if not args.quick:
        upload(EM.EmbeddingManager(engine=engine, enable_cache=False))


if __name__ == "__main__":
    main()
