"""Measure phrase queries (csrc/phrase.hip) on the synthetic Zipf corpus of tools/lexical_bench.py, built as term-id
SEQUENCES (vocabulary 200k, s = 1.1, ~150 tokens per row) so that every row has positions.

    python tools/phrase_bench.py [--rows 200000] [--quick]

For phrases over frequent, mid and rare terms (two-term phrases taken from the corpus itself, so each occurs somewhere)
at B = 1 and 64 it times, with HIP events around steady-state repetitions (median of 20 after 5 warm-up calls):
  match_us   LexicalIndex.match_phrases alone: the table upload, mmrag_phrase_match and nothing else
  phrase_us  LexicalIndex.topk_phrase_ids: match + mmrag_bm25_phrase_topk, phrase_mode="require"
  plain_us   LexicalIndex.topk_ids for the same loose terms: mmrag_bm25_topk, the code this feature leaves untouched
and reports what the match had to do: the driver list's length, the positions of the first term it walked and the
largest tf of the first term in one row (the work one lane or one wave gets).  Prints one JSON object per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_rag_amd.lexical import LexicalIndex  # noqa: E402

V = 200_000


def zipf_sequences(n, seed=0, tokens=150):
    g = np.random.default_rng(seed)
    lens = g.integers(tokens // 2, tokens * 3 // 2, n)
    tok = ((g.zipf(1.1, int(lens.sum())) - 1) % V).astype(np.int32)
    return np.split(tok, np.cumsum(lens)[:-1]), tok, lens


def timed(fn, reps=20, warm=5):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--quick", action="store_true", help="20 000 rows (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("phrase_bench needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    n = 20_000 if args.quick else args.rows
    seqs, tok, lens = zipf_sequences(n)
    lex = LexicalIndex(dev)
    step = 50_000
    for lo in range(0, n, step):
        lex.append_sequences(seqs[lo: lo + step])
    counts = lex._posting_counts()
    term_off, post_tf = lex._csr[0].cpu().numpy(), lex._csr[2].cpu().numpy()
    print(json.dumps({"what": "corpus", "rows": n, "tokens": int(tok.size), "postings": lex.n_postings,
                      "positions_bytes": lex.positions_bytes}), flush=True)
    g = np.random.default_rng(1)
    # bigrams of the corpus whose FIRST term is frequent / mid / rare (by df)
    first, second = tok[:-1], tok[1:]
    inside = np.ones(tok.size - 1, bool)
    inside[np.cumsum(lens)[:-1] - 1] = False          # not across a row boundary
    classes = {"frequent": counts[first] >= n // 4, "mid": (counts[first] >= n // 400) & (counts[first] < n // 40),
               "rare": (counts[first] >= 2) & (counts[first] < 50)}
    for name, mask in classes.items():
        at = np.nonzero(mask & inside)[0]
        if at.size == 0:
            continue
        for B in (1, 64):
            pick = g.choice(at, B)
            phrases = [(int(first[i]), int(second[i])) for i in pick]
            loose = [list(dict.fromkeys(tok[g.integers(0, tok.size, 3)].tolist())) for _ in range(B)]   # terms the corpus holds
            q_off = np.zeros(B + 1, np.int32)
            np.cumsum([len(q) for q in loose], out=q_off[1:])
            q_terms = np.asarray([t for q in loose for t in q], np.int32)
            distinct = list(dict.fromkeys(phrases))
            info = lex.match_phrases(distinct, 0)
            drivers = info["drivers"]
            first_tf = [int(post_tf[term_off[ph[0]]: term_off[ph[0] + 1]].max()) for ph in distinct]
            for slop in (0, 4):
                match = timed(lambda: lex.match_phrases(distinct, slop))
                whole = timed(lambda: lex.topk_phrase_ids(q_off, q_terms, [[p] for p in phrases], 10, slop=slop))
                plain = timed(lambda: lex.topk_ids(q_off, q_terms, 10))
                print(json.dumps({
                    "what": "phrase_topk", "class": name, "rows": n, "B": B, "slop": slop, "k": 10,
                    "match_us": round(match[0], 1), "match_p10_p90": [round(match[1], 1), round(match[2], 1)],
                    "phrase_us": round(whole[0], 1), "phrase_p10_p90": [round(whole[1], 1), round(whole[2], 1)],
                    "plain_us": round(plain[0], 1), "plain_p10_p90": [round(plain[1], 1), round(plain[2], 1)],
                    "driver_postings_mean": int(np.mean([counts[d] for d in drivers])),
                    "driver_postings_max": int(max(counts[d] for d in drivers)),
                    "first_term_postings_mean": int(np.mean([counts[p[0]] for p in distinct])),
                    "first_term_max_tf_in_a_row": int(max(first_tf)),
                    "rows_holding_mean": float(info["rows"].float().mean().item())}), flush=True)


if __name__ == "__main__":
    main()
