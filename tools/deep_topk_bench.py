"""Developer timing of the deep exact top-k (mmrag_cosine_topk_deep, csrc/search_deep.hip); not the judged bench.py.

    python tools/deep_topk_bench.py [--quick]

One JSON line per shape: kernel time from events around a run of calls (us per call), wall time per call on the host
(the call synchronises the stream once), main-pass survivor counts per query (min / mean / max, read from the head of
the workspace, where the library keeps its per-query counters) and the number of queries whose survivors overflowed
the candidate buffer.  k = 20 rows are the existing list kernels (mmrag_cosine_topk), for comparison."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from multimodal_rag_amd import _native as N  # noqa: E402

SHAPES = [(1_000_000, 768, torch.float16), (100_000, 384, torch.float32)]
BS = [1, 256]
KS = [20, 50, 100, 1000, 4096]


def unit(rows, d, ld, dtype, g):
    out = torch.empty((rows, ld), dtype=dtype, device="cuda")
    step = 1 << 18
    for lo in range(0, rows, step):
        hi = min(rows, lo + step)
        x = torch.randn((hi - lo, ld), device="cuda", generator=g)
        x[:, d:] = 0
        x /= x.norm(dim=1, keepdim=True)
        out[lo:hi] = x.to(dtype)
    return out


def time_calls(fn, seconds):
    fn()
    torch.cuda.synchronize()
    t_end = time.time() + seconds / 2          # warm
    while time.time() < t_end:
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = 0
    t0 = time.perf_counter()
    e0.record()
    t_end = time.time() + seconds / 2
    while time.time() < t_end or calls < 5:
        fn()
        calls += 1
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / calls
    return e0.elapsed_time(e1) * 1e3 / calls, wall * 1e6


def main():
    quick = "--quick" in sys.argv
    g = torch.Generator(device="cuda").manual_seed(1)
    for n, d, dtype in SHAPES:
        ld = N.padded_dim(d, dtype)
        c = unit(n, d, ld, dtype, g)
        for B in BS:
            q = unit(B, d, ld, dtype, g)
            for k in KS:
                rec = {"n": n, "d": d, "dtype": str(dtype).replace("torch.", ""), "B": B, "k": k}
                if k <= N.MAX_K:
                    ws = torch.empty(N.cosine_topk_workspace_bytes(B, n, k) + 16, dtype=torch.uint8, device="cuda")
                    fn = lambda: N.cosine_topk(q, c, n, d, k, workspace=ws)  # noqa: E731
                    rec["path"] = "lists"
                else:
                    ws = torch.empty(N.cosine_topk_deep_workspace_bytes(B, n, k), dtype=torch.uint8, device="cuda")
                    fn = lambda: N.cosine_topk_deep(q, c, n, d, k, workspace=ws)  # noqa: E731
                    rec["path"] = "deep"
                rec["kernel_us"], rec["wall_us"] = (round(x, 1) for x in time_calls(fn, 0.3 if quick else 1.0))
                if rec["path"] == "deep":
                    fn()
                    torch.cuda.synchronize()
                    cnt = ws[: 4 * B].view(torch.int32).to(torch.int64).cpu()
                    cap = max(16384, (32 * k + 255) // 256 * 256)
                    rec["survivors_min"], rec["survivors_mean"], rec["survivors_max"] = (
                        int(cnt.min()), round(float(cnt.float().mean()), 1), int(cnt.max()))
                    rec["capacity"] = cap
                    rec["overflowed"] = int((cnt > cap).sum())
                print(json.dumps(rec), flush=True)
            del q
        del c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
