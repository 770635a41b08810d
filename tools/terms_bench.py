"""Measure significant terms (csrc/terms.hip) on the synthetic Zipf corpus of tools/lexical_bench.py (vocabulary 200k,
s = 1.1, ~150 tokens and ~100 distinct terms per row).

    python tools/terms_bench.py [--rows 1000000] [--groups 256] [--top 10] [--quick]

Every row gets one of `groups` labels, uniformly at random: the corpus has no topics, so fgp is bgp plus noise, about
half of the pairs a group holds qualify and a group's candidates can outgrow its slots -- the case that costs the most.
For min_count 2, 5 and 20 it times LexicalIndex.group_terms with HIP events around steady-state repetitions (median of
10 after 3 warm-up calls; the call synchronises once per launch window to read the candidate counts, which the events
include) and reports what the call had to do: the postings of one pass over the CSR, the share of the vocabulary the
df test drops without a visit, the candidates per group and how many groups overflowed their slots and were counted
again alone.  postings_per_s is the postings of ONE pass over the call's time, re-runs included in the time: a rate of
the whole call, not of the kernel.  A few returned counts are recounted on the host.  One JSON object per measurement."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 200_000


def zipf_corpus(n, seed=0, tokens=150):
    g = np.random.default_rng(seed)
    lens = g.integers(tokens // 2, tokens * 3 // 2, n)
    tok = (g.zipf(1.1, int(lens.sum())) - 1) % V
    key = np.repeat(np.arange(n, dtype=np.int64), lens) * V + tok
    uk, cnt = np.unique(key, return_counts=True)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(uk // V, minlength=n), out=off[1:])
    return off, (uk % V).astype(np.int32), cnt.astype(np.int32), lens.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="20 000 rows (a rehearsal, not a measurement)")
    args = ap.parse_args()
    n, G, top = (20_000 if args.quick else args.rows), args.groups, args.top
    off, ids, tfs, dl = zipf_corpus(n)
    labels = np.random.default_rng(2).integers(0, G, n).astype(np.int32)
    sizes = np.bincount(labels, minlength=G).astype(np.int32)
    df = np.bincount(ids, minlength=V)
    print(json.dumps({"what": "corpus", "rows": n, "postings": int(ids.size), "vocabulary": V,
                      "terms_with_postings": int((df > 0).sum()), "groups": G}), flush=True)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("terms_bench needs a GPU: nothing is measured without one")
    from multimodal_rag_amd import _native
    from multimodal_rag_amd.lexical import LexicalIndex

    dev = "cuda:0"
    lex = LexicalIndex(dev)
    lex._max_term = V - 1
    lex.append_postings(off, ids, tfs, dl)
    lex._ensure_csr()
    group = torch.from_numpy(labels).to(dev)
    d_sizes = torch.from_numpy(sizes).to(dev)
    window = _native.terms_limits()["groups"]
    cap = min(_native.candidate_capacity(top), (V + 255) // 256 * 256)
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))

    def timed(fn, reps=10, warm=3):
        for _ in range(warm):
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
        return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))

    for min_count in (2, 5, 20):
        s, t, c = lex.group_terms(group, d_sizes, top, min_count)
        torch.cuda.synchronize()
        # the main pass's true candidate counts of the LAST launch window stay first in the workspace
        last = min(window, G - (G - 1) // window * window)
        cand = lex._terms_ws[: 4 * last].view(torch.int32).cpu().numpy().astype(np.int64)
        t_h, c_h = t.cpu().numpy(), c.cpu().numpy()
        for g in (0, G // 2, G - 1):          # a few returned counts, recounted from the forward log
            for j in range(min(2, top)):
                if t_h[g, j] >= 0:
                    fg = int((labels[row_of[ids == t_h[g, j]]] == g).sum())
                    assert fg == c_h[g, j] >= min_count, (g, j, fg, int(c_h[g, j]))
        us = timed(lambda: lex.group_terms(group, d_sizes, top, min_count))
        print(json.dumps({
            "what": "group_terms", "rows": n, "postings": int(ids.size), "groups": G, "top": top, "min_count": min_count,
            "call_us": round(us[0], 1), "call_p10_p90": [round(us[1], 1), round(us[2], 1)],
            "postings_per_s": round(ids.size / (us[0] * 1e-6), 0),
            "vocabulary_share_skipped_by_df": round(float((df < min_count).mean()), 4),
            "slots_per_group": int(cap), "last_window_groups": int(last),
            "candidates_per_group_mean": float(cand.mean()), "candidates_per_group_max": int(cand.max()),
            "last_window_groups_overflowed": int((cand > cap).sum()),
            "returned_per_group_mean": float((t_h >= 0).sum(1).mean())}), flush=True)


if __name__ == "__main__":
    main()
