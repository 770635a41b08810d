#!/usr/bin/env python3
"""Headline benchmark of the embed-and-retrieve hot path on MI355X.

    python bench.py --gpus 1 --steps 50 --warmup 10
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[2], the configuration the metric is quoted on):
  retrieve: 1,000,000 x 768 fp16 unit-norm corpus, query batch 256, top_k = 5, exact cosine.
            A step = one query batch through the whole retrieve path: fused GEMM+top-k kernel
            on each rank's row shard -> per-rank [256, 5] (score, global row) -> RCCL all-gather
            -> host merge (N > 1) -> results in host memory.  The corpus is fixed at 1M rows
            and split row-wise over the N ranks (strong scaling).
  embed:    (reported under "embed", --full only) encoder forward of bge-base-shaped chunks -> chunks/s.
Inputs are resident in HBM before the timed region.  One JSON line is printed by rank 0.
A plain run times the retrieve steps only; --full adds the measured peaks, the CPU baselines and parity check
against the oracle, the served legs and the embed leg.  --dump-outputs DIR writes the last timed step's results.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_TOTAL = 1_000_000
DIM = 768
BATCH = 256
TOPK = 5
HBM_PEAK_GBS = 8000.0       # vendor: HBM3E 8.0 TB/s (MI355X_MICROARCH.md); the measured copy rate is taken in this run
MFMA_F16_PEAK_TFLOPS = 2500.0  # vendor: dense fp16/bf16 MFMA; the measured MFMA rate is taken in this run
WARMUP_SECONDS = 0.6        # clocks settle over ~100 ms of sustained load: warm up by time, then honour --warmup


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def make_unit_rows(lo: int, hi: int, dim: int, ld: int, dtype, device, base_seed: int) -> torch.Tensor:
    """Rows [lo, hi) of the synthetic corpus: standard normal -> L2-normalise -> storage dtype.
    Generated in 65536-row blocks seeded by block index, so a row's value does not depend on
    how many ranks share the corpus."""
    out = torch.zeros((hi - lo, ld), dtype=dtype, device=device)
    blk = 65536
    g = torch.Generator(device=device)
    b0 = lo // blk
    b1 = (hi + blk - 1) // blk
    for b in range(b0, b1):
        g.manual_seed(base_seed + b)
        x = torch.randn((blk, dim), device=device, generator=g, dtype=torch.float32)
        x = x / x.norm(dim=1, keepdim=True)
        s = max(lo, b * blk)
        e = min(hi, (b + 1) * blk)
        out[s - lo: e - lo, :dim] = x[s - b * blk: e - b * blk].to(dtype)
    return out


def cpu_baseline(q_host: np.ndarray, corpus_host: np.ndarray, k: int):
    """The oracle (numpy sgemm + exact selection) on the host cores: 'port' of the reference's
    CPU search path (chromadb is not installable)."""
    from oracle import search_oracle as O

    threads = torch.get_num_threads()
    try:  # the sgemm runs in numpy's OpenBLAS pool: report ITS thread count
        from threadpoolctl import threadpool_info

        blas = [i["num_threads"] for i in threadpool_info() if i.get("user_api") == "blas"]
        np_blas = [i["num_threads"] for i in threadpool_info()
                   if i.get("user_api") == "blas" and "numpy" in (i.get("filepath") or "") or "openblas" in (i.get("internal_api") or "")]
        if np_blas or blas:
            threads = max(np_blas or blas)
    except Exception:
        pass
    t0 = time.perf_counter()
    s, r = O.cosine_topk(q_host, corpus_host, k)
    t1 = time.perf_counter()
    s, r = O.cosine_topk(q_host, corpus_host, k)
    t2 = time.perf_counter()
    dt = min(t1 - t0, t2 - t1)
    # a GPU box hands one job a share of its cores (16 per GPU): also try the BLAS pool at that size and report
    # the better run with ITS thread count
    try:
        from threadpoolctl import threadpool_limits

        if threads > 16:
            with threadpool_limits(limits=16, user_api="blas"):
                t3 = time.perf_counter()
                O.cosine_topk(q_host, corpus_host, k)
                d16 = time.perf_counter() - t3
            if d16 < dt:
                dt, threads = d16, 16
    except Exception:
        pass
    return s, r, dt, threads


def served_leg(dev, corpus, n_rows: int, seconds: float = 2.0):
    """Wall clock around the calls a user of the reference makes (SURVEY 8d "timing protocol"): queries/s through
    `EmbeddingManager.batch_query` (embedder.py:784-832, here ONE batched encode + ONE batched search per call) and
    through `query()` from 64 concurrent callers with the dynamic-batching dispatcher on (the online /query shape,
    api.py:338).  Text -> tokens -> bge-base-shaped encoder (random weights) -> search over the SAME 1M x 768 index ->
    Chroma-shaped result dicts on the host."""
    import asyncio

    from multimodal_rag_amd import tracing
    from multimodal_rag_amd.embedder import EmbeddingManager, HipEngine

    eng = HipEngine("BAAI/bge-base-en-v1.5", str(dev))
    # a deployment has the checkpoint's vocab.txt and therefore the native WordPiece tokenizer; no vocabulary can be
    # fetched here, so a WordPiece-shaped synthetic one stands in (the pure-Python hash tokenizer HipEngine falls back
    # to without a vocabulary costs 26 us per query -- more than half of a 256-query call)
    from bench_embed import synthetic_vocab
    from multimodal_rag_amd.tokenizer import NativeWordPieceTokenizer

    vocab, words = synthetic_vocab(eng.encoder.cfg.vocab)
    eng.tokenizer = NativeWordPieceTokenizer(vocab)
    m = EmbeddingManager(engine=eng, enable_cache=False)

    async def go():
        await m.initialize()
        ids = [f"doc_{i // 64:012x}_text_{i % 64}" for i in range(n_rows)]
        metas = [{"doc_id": s[:16], "item_id": s[17:], "type": "text"} for s in ids]
        m.collection.add_rows_device(corpus[:n_rows], None, metas, ids)
        texts = [" ".join(words[(i * 7 + j * 131) % len(words)] for j in range(7)) + f" {i % 97}" for i in range(4096)]
        out = {}
        # (a) batch_query, 256 queries per call
        await m.batch_query(texts[:256], n_results=TOPK)
        tracing.reset()
        t_end, n_q, t0 = time.perf_counter() + seconds, 0, time.perf_counter()
        k = 0
        while time.perf_counter() < t_end:
            res = await m.batch_query(texts[k:k + 256], n_results=TOPK)
            assert len(res) == 256 and len(res[0]["ids"]) == TOPK
            n_q += 256
            k = (k + 256) % 3840
        out["batch_query_256"] = {"queries_per_s": round(n_q / (time.perf_counter() - t0), 1), "calls": n_q // 256,
                                  "stage_mean_ms": {k: v["mean_ms"] for k, v in tracing.snapshot().items()}}
        # (a') the same call from three concurrent callers (a server's normal state): one caller's tokenisation and result
        # building overlap the other callers' GPU time (the tokenizer is native and drops the GIL, the GPU wait drops it too)
        t_end, t0 = time.perf_counter() + seconds, time.perf_counter()
        done3 = [0]

        async def batch_caller(j):
            k3 = (j * 1280) % 3840
            while time.perf_counter() < t_end:
                res = await m.batch_query(texts[k3:k3 + 256], n_results=TOPK)
                assert len(res) == 256 and len(res[0]["ids"]) == TOPK
                done3[0] += 256
                k3 = (k3 + 256) % 3840

        await asyncio.gather(*[batch_caller(j) for j in range(3)])
        out["batch_query_256_x3_callers"] = {"queries_per_s": round(done3[0] / (time.perf_counter() - t0), 1),
                                              "calls": done3[0] // 256}
        # (b) query() x 64 concurrent callers through the dispatcher
        disp = m.enable_dynamic_batching(max_batch=256, max_wait_ms=1.0)
        stop_at = time.perf_counter() + seconds
        done = [0]

        async def caller(j):
            i = j
            while time.perf_counter() < stop_at:
                r = await m.query(texts[i % 4096], n_results=TOPK)
                assert len(r["ids"]) == TOPK
                done[0] += 1
                i += 64

        t0 = time.perf_counter()
        await asyncio.gather(*[caller(j) for j in range(64)])
        dt = time.perf_counter() - t0
        st = dict(disp.stats)
        await disp.stop()
        out["query_64_callers_dispatcher"] = {"queries_per_s": round(done[0] / dt, 1), "batches": st["batches"],
                                               "max_batch_seen": st["max_batch_seen"]}
        # (c) one caller, no dispatcher: the single-query latency
        m._dispatcher = None
        lat = []
        for i in range(50):
            t0 = time.perf_counter()
            await m.query(texts[i], n_results=TOPK)
            lat.append(time.perf_counter() - t0)
        out["single_query_latency_ms"] = {"median": round(float(np.median(lat)) * 1e3, 3),
                                          "p90": round(float(np.quantile(lat, 0.9)) * 1e3, 3)}
        return out

    res = asyncio.run(go())
    res["note"] = ("wall clock, host included: native WordPiece (synthetic vocabulary) -> bge-base-shaped encoder "
                   f"(random fp16 weights) -> exact search over {n_rows} x {DIM} -> result dicts; queries are 8 words long")
    del m, eng
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=N_TOTAL, help="total corpus rows (default: the 1M headline)")
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--hnsw-baseline", type=int, default=0, metavar="ROWS",
                    help="also time the HNSW restatement of chromadb's approximate index (oracle/hnsw_oracle.cpp, "
                         "Chroma's defaults) on the first ROWS corpus rows: build time, queries/s, recall@5. Opt-in: "
                         "the graph build takes minutes.")
    ap.add_argument("--no-embed", action="store_true")
    ap.add_argument("--no-served", action="store_true", help="skip the wall-clock EmbeddingManager legs")
    ap.add_argument("--no-peaks", action="store_true", help="skip the stream-copy / MFMA micro-benchmarks")
    ap.add_argument("--merge", choices=["host", "device"], default="host",
                    help="where the G*k -> k merge runs for N > 1 (north star: host)")
    ap.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                    help="gloo = rehearsal on a one-GPU box (collective on host copies); the driver uses nccl (RCCL)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: measured peaks, CPU baselines and the parity check "
                         "against the oracle, the served legs, the embed leg (each can still be dropped with its --no-* "
                         "option). Without it only the retrieve steps are timed.")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the last step's results (scores.npy float32 [batch, k], "
                         "rows.npy float64 [batch, k], global corpus rows) into DIR")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.hnsw_baseline > 0 and not args.full:
        ap.error("--hnsw-baseline is part of --full")
    if not args.full:
        args.no_cpu_baseline = args.no_served = args.no_peaks = args.no_embed = True

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run (one rank per GPU)")
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import torch.distributed as dist

    # MMRAG_BENCH_FORCE_EXCHANGE=1: run the RCCL all-gather + merge with a single rank (one-GPU rehearsal of
    # the N > 1 path; launch through torch.distributed.run --nproc-per-node 1)
    force_exchange = world == 1 and os.environ.get("MMRAG_BENCH_FORCE_EXCHANGE") == "1"
    if world > 1 or force_exchange:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("TORCH_NCCL_HIGH_PRIORITY", "1")  # RCCL's stream: same reason as the side stream
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")

    from multimodal_rag_amd import _native as N

    N.lib()
    dtype = torch.float16
    ld = N.padded_dim(DIM, dtype)
    B, k, n_total = args.batch, TOPK, args.rows
    per = (n_total + world - 1) // world
    lo, hi = min(n_total, rank * per), min(n_total, (rank + 1) * per)
    n_local = hi - lo

    corpus = make_unit_rows(lo, hi, DIM, ld, dtype, dev, base_seed=1234)
    q = make_unit_rows(0, B, DIM, ld, dtype, dev, base_seed=987654)
    # SLOTS workspaces / buffer sets: later batches' corpus scans run while batch i's candidate merge,
    # all-gather and copy-out are still in flight on the side stream.  A batch's scan + tail latency
    # exceeds one host launch at small shards (125k rows: 87 + 40 us vs 60 us), hence more than two.
    SLOTS = 4
    ws = [torch.empty(N.cosine_topk_workspace_bytes(B, n_local, k) + 16, dtype=torch.uint8, device=dev)
          for _ in range(SLOTS)]
    events = {}

    plans = [N.SearchPlan(q, corpus, n_local, DIM, k, ws[i]) for i in range(SLOTS)]
    main_torch = torch.cuda.current_stream(dev)
    main_stream = main_torch.cuda_stream
    side_ptr = [main_stream]

    def local_scan(slot):       # phase 1: the fused GEMM + top-k kernel (the roofline kernel)
        ev = events.get(slot)
        if ev is not None:
            ev[0].record(main_torch)
        plans[slot % SLOTS].scan(main_stream)
        if ev is not None:
            ev[1].record(main_torch)

    def local_finish(slot, out_s, out_r):   # phase 2: per-query merge of the candidate lists (side stream)
        plans[slot % SLOTS].select(lo, out_s.data_ptr(), out_r.data_ptr(), side_ptr[0])

    from multimodal_rag_amd.sharded import ShardedSearch

    ss = ShardedSearch(B, k, world, rank, dev, local_finish, merge=args.merge,
                       collective_on_host=(args.dist_backend == "gloo"), local_scan=local_scan,
                       force_exchange=force_exchange, n_slots=SLOTS)
    # the tail stream stays current for the whole loop (scans get the main stream explicitly): no stream-context
    # switch per batch on the host
    side_ptr[0] = ss.side.cuda_stream
    ss.side_is_current = True
    torch.cuda.set_stream(ss.side)
    final = {}

    host_t = {"launch": 0.0, "finish": 0.0}
    LAG = SLOTS - 1  # batches in flight behind the one whose results the host is merging

    def run(steps):
        pc = time.perf_counter
        for i in range(steps):
            t0 = pc()
            ss.launch(i)
            t1 = pc()
            if i >= LAG:
                final["s"], final["r"] = ss.finish(i - LAG)  # overlaps the device work of steps i-LAG+1 .. i
            host_t["launch"] += t1 - t0
            host_t["finish"] += pc() - t1
        for j in range(max(0, steps - LAG), steps):
            final["s"], final["r"] = ss.finish(j)

    def sync_all():
        torch.cuda.synchronize()
        if world > 1 or force_exchange:
            dist.barrier()
            torch.cuda.synchronize()

    t_warm = time.perf_counter() + WARMUP_SECONDS
    while time.perf_counter() < t_warm:     # by time first (DVFS), then the requested untimed steps
        run(max(8, SLOTS))
        torch.cuda.synchronize()
    run(args.warmup)
    for i in range(args.steps):
        events[i] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    sync_all()
    t0 = time.perf_counter()
    host_t["launch"] = host_t["finish"] = 0.0
    run(args.steps)
    sync_all()
    dt = time.perf_counter() - t0
    log(f"[rank {rank}] host time per step: launch {host_t['launch'] / args.steps * 1e6:.1f} us, "
        f"finish (wait + merge) {host_t['finish'] / args.steps * 1e6:.1f} us")
    if world > 1 or force_exchange:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    torch.cuda.set_stream(main_torch)
    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in events.values()])) if events else float("nan")
    gpu_s = final["s"].clone().numpy()
    gpu_r = final["r"].clone().numpy()
    if rank == 0 and args.dump_outputs:   # every rank holds the same merged results; one copy is enough
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "scores.npy"), gpu_s.astype(np.float32))
        np.save(os.path.join(args.dump_outputs, "rows.npy"), gpu_r.astype(np.float64))

    result = None
    if rank == 0:
        import hashlib

        rows_md5 = hashlib.md5(np.ascontiguousarray(gpu_r).tobytes()).hexdigest()  # identical for every N
        qps = B * args.steps / dt
        alg_bytes = n_local * DIM * 2  # corpus read once per query batch, per GPU
        achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
        flops = 2.0 * B * n_local * DIM
        traffic, traffic_source = None, None
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tpath):
            try:
                t = json.load(open(tpath))
                if t.get("rows_per_gpu") == n_local and t.get("batch") == B:
                    traffic = t.get("hbm_bytes_per_launch")
                    traffic_source = f"profiles/traffic.json ({t.get('source', 'rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes')}; not measured by this run)"
            except Exception:
                pass
        uses_qs = N.search_uses_query_stationary(B, n_local, DIM, k, dtype)
        kernel_name = N.search_kernel_name(B, n_local, DIM, k, dtype)
        dev_info = N.device_info()
        peaks = {}
        if not args.no_peaks:
            try:
                peaks = N.measure_peaks(dev)
            except Exception as e:  # the headline must survive a failure of the micro-benchmarks
                peaks = {"error": str(e)[:200]}
        log(f"[device] {dev_info}  measured peaks: {peaks}")
        result = {
            "metric": "chunks embedded/sec + queries/sec top_k=5 over 1M×768 at 1/2/4/8 GPUs",
            "value": round(qps, 1),
            "unit": "queries/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f16",
            "data": "synthetic",
            "config": {
                "workload": f"retrieve: {n_total}x{DIM} fp16 unit-norm corpus row-sharded over {world} GPU(s), "
                            f"query batch {B}, top_k={k}, exact cosine (fp32 accumulate), "
                            f"{(('RCCL' if args.dist_backend == 'nccl' else 'gloo (rehearsal)') + ' all-gather + ' + args.merge + ' merge') if world > 1 else 'single shard'}, results to host",
                "corpus_rows": n_total, "dim": DIM, "batch": B, "top_k": k, "rows_per_gpu": n_local,
                "parallelism": f"row-shard x{world}", "result_rows_md5": rows_md5,
            },
            "roofline": {
                "bound": "hbm", "kernel": kernel_name,
                "launch": ("one scan = a 4-byte fill of the 258 KB threshold-exchange block + ONE cosine_topk_walk_kernel "
                           "launch over all rows (thresholds are exchanged inside the launch, the last tenth of the tiles "
                           "is handed out by ticket); timed with HIP events around both, every step")
                          if kernel_name == "cosine_topk_walk_kernel" else
                          ("one scan = sample pass (first 65536 rows, best score per query per workgroup) + "
                           "qs_seed_thr_kernel + the walk over all rows, all cosine_topk_qs_kernel; timed with HIP events "
                           "around the three launches of every step") if uses_qs else
                          ("one scan = the launches of mmrag_cosine_topk_lists for this shard (sample pre-pass + merge "
                           "where the shard is long enough, then the main pass); timed with HIP events around them"),
                "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
                "kernel_ms": round(kern_ms, 4),
                # what the fraction is short of (measured): neither memory nor the matrix pipe alone
                "limiter": ("issue slots: one wave per SIMD issues 384 MFMAs and ~370 other instructions per 64-row tile "
                            "(24 LDS-DMA pieces of 45-50 cycles each), at the 1.5-1.9 GHz the board's power limit leaves"
                            if kernel_name == "cosine_topk_walk_kernel" else None),
                "mfma_tflops": round(flops / (kern_ms * 1e-3) / 1e12, 1),
                "mfma_frac": round(flops / (kern_ms * 1e-3) / 1e12 / MFMA_F16_PEAK_TFLOPS, 4),
                "peaks_vendor": {"hbm_GBps": HBM_PEAK_GBS, "mfma_f16_TFLOPs": MFMA_F16_PEAK_TFLOPS},
                "peaks_measured": peaks,
                "frac_of_measured_read": (round(achieved / peaks["stream_read_GBps"], 4)
                                          if peaks.get("stream_read_GBps") else None),
                # against the faster of the two MFMA shapes measured (the scan runs on 16x16x32)
                "mfma_frac_of_measured": (round(flops / (kern_ms * 1e-3) / 1e12 /
                                                max(peaks["mfma_f16_TFLOPs"], peaks.get("mfma_f16_16x16x32_TFLOPs", 0.0)), 4)
                                          if peaks.get("mfma_f16_TFLOPs") else None),
                "device": dev_info,
            },
        }

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        q_host = q[:, :DIM].float().cpu().numpy()
        c_host = corpus[:, :DIM].cpu().numpy()  # fp16 storage; the oracle up-casts exactly
        es, er, cdt, threads = cpu_baseline(q_host, c_host, k)
        from oracle import search_oracle as O

        ok = bool(np.all(np.abs(gpu_s - es) <= 1e-4) and O.same_topk_sets(gpu_r, gpu_s, er, es))
        result["cpu_baseline"] = {
            "value": round(B / cdt, 1), "unit": "queries/s", "cores": threads, "kind": "port",
            "sample": f"oracle/search_oracle.py (numpy/OpenBLAS sgemm + exact top-k) on {B} queries x "
                      f"{n_local} rows, best of 2 (and once at 16 BLAS threads); host cpu_count={os.cpu_count()}",
        }
        result["parity_vs_oracle"] = ok
        if args.hnsw_baseline > 0:
            from oracle.hnsw_oracle import HnswIndex

            m = min(args.hnsw_baseline, n_local)
            sub = np.ascontiguousarray(c_host[:m], dtype=np.float32)
            t0 = time.perf_counter()
            hidx = HnswIndex(sub)
            t_build = time.perf_counter() - t0
            xs, xr = O.cosine_topk(q_host, sub, k)
            leg = {"kind": "restatement of chroma-hnswlib's algorithm, not chromadb (parity unpinned)",
                   "rows": m, "M": 16, "ef_construction": 100, "build_s": round(t_build, 1),
                   "build_threads": hidx.n_threads, "search": []}
            for ef in (10, 100):
                hidx.search(q_host, k, ef, n_threads=1)
                t0 = time.perf_counter()
                hs, hr = hidx.search(q_host, k, ef, n_threads=1)
                t1 = time.perf_counter() - t0
                t0 = time.perf_counter()
                hidx.search(q_host, k, ef)
                tn = time.perf_counter() - t0
                rec = float(np.mean([len(set(a) & set(b)) / k for a, b in zip(hr.tolist(), xr.tolist())]))
                leg["search"].append({"ef": ef, "recall_at_5": round(rec, 3), "queries_per_s_1_thread": round(B / t1, 1),
                                      "queries_per_s_all_threads": round(B / tn, 1)})
            result["cpu_baseline_hnsw"] = leg
            del sub, hidx
        del c_host

    if rank == 0 and world == 1 and not args.no_served:
        try:
            result["served"] = served_leg(dev, corpus, n_local)
        except Exception as e:  # the headline must survive a failure of the extra leg
            result["served"] = {"error": f"{type(e).__name__}: {e}"[:300]}

    if not args.no_embed:
        try:
            import bench_embed

            emb = bench_embed.run(dev, rank, world, steps=max(3, args.steps // 5), warmup=2,
                                  with_cpu_baseline=not args.no_cpu_baseline)
            if rank == 0 and emb is not None:
                result["embed"] = emb
        except ImportError:
            pass

    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1 or force_exchange:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
