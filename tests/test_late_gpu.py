"""GPU: late-interaction re-ranking -- the MaxSim kernel (csrc/maxsim.hip) against tests/late_ref.py, the encoder's token
rows (mmrag_encoder_forward_tokens) against oracle.encoder_oracle.bert_hidden_states, and the layers above them.

Tolerances
  integer rows ....... entries in {-2..2}: every dot product and every sum is an integer below 2^24, exact in float32;
                       sums, maxima and indices are compared bit for bit
  random unit rows ... best_sim within dedup_ref.TOL (1e-4, the project's tolerance for this tile body) of float64; the
                       mean within 1e-4 + q_len * 2^-23 (q_len float32 additions of values below 1); an index is accepted
                       when the reference similarity at it is within 2 TOL of the reference maximum
  token rows ......... per token max |delta| <= 4e-3 and cosine >= 0.9999 vs the normalised oracle rows (the bound of
                       tests/test_encoder_gpu.py for a CLS-pooled row, which is one token)
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import encoder_oracle as E
from tests import late_ref
from tests.dedup_ref import TOL

pytestmark = pytest.mark.gpu

W = 128     # MMRAG_MAX_LATE_QUERY_TOKENS: the width of best_sim / best_idx
GUARD = 100.0   # rows between sequences: a read outside a sequence shows as a huge similarity


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def layout(seqs, dim, ld, guard_rows=3):
    """sequences (float arrays [len, dim]) -> (rows [n, ld] float32 with GUARD-filled rows before, between and after
    them, pad columns zero; starts; lens)"""
    parts, starts, at = [], [], 0
    for s in seqs:
        parts.append(np.full((guard_rows, ld), GUARD, np.float32))
        at += guard_rows
        body = np.zeros((len(s), ld), np.float32)
        body[:, :dim] = s
        parts.append(body)
        starts.append(at)
        at += len(s)
    parts.append(np.full((guard_rows, ld), GUARD, np.float32))
    rows = np.concatenate(parts)
    rows[:, dim:] = 0.0
    return rows, np.array(starts, np.int32), np.array([len(s) for s in seqs], np.int32)


def run(N, q_seqs, d_seqs, pairs, dim, one_buffer=False, want_best=True, ld=None):
    """-> (sums [P], best_sim [P, W] | None, best_idx | None) as numpy, and the float64 reference list"""
    ld = ld or N.padded_dim(dim, torch.float16)
    if one_buffer:
        rows, starts, lens = layout(list(q_seqs) + list(d_seqs), dim, ld)
        q_rows = d_rows = torch.from_numpy(rows).cuda().half().contiguous()
        nq = len(q_seqs)
        qs, ql, ds, dl = starts[:nq], lens[:nq], starts[nq:], lens[nq:]
    else:
        qr, qs, ql = layout(q_seqs, dim, ld)
        dr, ds, dl = layout(d_seqs, dim, ld, guard_rows=5)
        q_rows = torch.from_numpy(qr).cuda().half().contiguous()
        d_rows = torch.from_numpy(dr).cuda().half().contiguous()
    pq, pd = [a for a, _ in pairs], [b for _, b in pairs]
    sums, bs, bi = N.maxsim_scores(q_rows, d_rows, dim, qs, ql, ds, dl, pq, pd, want_best=want_best)
    torch.cuda.synchronize()
    ref = [late_ref.maxsim(np.asarray(q_seqs[a], np.float16), np.asarray(d_seqs[b], np.float16)) for a, b in pairs]
    return (sums.cpu().numpy(), bs.cpu().numpy() if bs is not None else None,
            bi.cpu().numpy() if bi is not None else None), ref


def assert_exact(got, ref, pairs, q_seqs):
    sums, bs, bi = got
    for p, ((a, _), (r_sim, r_idx, r_sum, _)) in enumerate(zip(pairs, ref)):
        n = len(q_seqs[a])
        assert np.array_equal(bs[p, :n], r_sim.astype(np.float32)), (p, bs[p, :n], r_sim)
        assert np.array_equal(bi[p, :n], r_idx), (p, bi[p, :n], r_idx)
        assert sums[p] == np.float32(r_sum), (p, sums[p], r_sum)


Q_LENS = (1, 15, 16, 17, 64, 65, 128)
D_LENS = (1, 127, 128, 129, 300, 512)


def int_rows(g, n, dim):
    return g.integers(-2, 3, (n, dim)).astype(np.float32)


@pytest.mark.parametrize("at,dim", list(enumerate((64, 128, 384, 768))))
def test_integer_exact_grid(N, at, dim):
    """every q_len against a sample of the d_lens (each (q_len, d_len) pair occurs for two of the four dims); sequences
    at non-zero starts between GUARD rows, queries and passages shared between pairs; P = 21"""
    g = np.random.default_rng(100 + dim)
    q_seqs = [int_rows(g, n, dim) for n in Q_LENS]
    d_seqs = [int_rows(g, n, dim) for n in D_LENS]
    pairs = [(a, b) for a in range(len(Q_LENS)) for b in range(len(D_LENS)) if (a + b + at) % 2 == 0]
    got, ref = run(N, q_seqs, d_seqs, pairs, dim, one_buffer=(at % 2 == 1))
    assert_exact(got, ref, pairs, q_seqs)
    # identical calls give identical bits; the optional outputs may be left out
    again, _ = run(N, q_seqs, d_seqs, pairs, dim, one_buffer=(at % 2 == 1))
    for x, y in zip(got, again):
        n_of = [len(q_seqs[a]) for a, _ in pairs]
        if x.ndim == 1:
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
        else:
            assert all(np.array_equal(x[p, :n].view(np.int32), y[p, :n].view(np.int32)) for p, n in enumerate(n_of))
    (sums_only, none_a, none_b), _ = run(N, q_seqs, d_seqs, pairs, dim, one_buffer=(at % 2 == 1), want_best=False)
    assert none_a is None and none_b is None
    assert np.array_equal(sums_only.view(np.int32), got[0].view(np.int32))


@pytest.mark.parametrize("P", [1, 3, 70])
def test_pair_counts_share_sequences(N, P):
    dim = 128
    g = np.random.default_rng(P)
    q_seqs = [int_rows(g, n, dim) for n in (5, 128, 33)]
    d_seqs = [int_rows(g, n, dim) for n in (140, 7, 512, 129)]
    pairs = [(p % 3, (p * 5 + p // 3) % 4) for p in range(P)]
    got, ref = run(N, q_seqs, d_seqs, pairs, dim, ld=256)       # a padded width wider than mmrag_padded_dim's
    assert_exact(got, ref, pairs, q_seqs)


@pytest.mark.parametrize("dups,d_len", [((127, 128), 300), ((63, 64), 300), ((60, 70, 127, 128, 200), 300),
                                        ((100, 130), 140), ((3, 19), 40), ((3, 4), 40), ((255, 256, 384), 512),
                                        ((511,), 512), ((0, 511), 512), ((128,), 129), ((35, 99), 100)])
def test_duplicated_passage_tokens_lowest_index_wins(N, dups, d_len):
    """the same row at several passage positions -- across the tile boundary (127 | 128), the two wave columns
    (63 | 64), two registers of one lane (3, 19), two lanes (3, 4) -- and every query token equal to it: its dot with
    itself, 4 dim, is the strict maximum (entries +-2: any other row in {-2..2} scores less), attained at every copy"""
    dim = 64
    g = np.random.default_rng(sum(dups) + d_len)
    v = g.choice([-2.0, 2.0], dim).astype(np.float32)
    d = int_rows(g, d_len, dim)
    d[np.all(d == v, axis=1)] = 0.0
    d[list(dups)] = v
    q = np.tile(v, (17, 1))
    q[5] = int_rows(g, 1, dim)[0]       # and one ordinary token
    got, ref = run(N, [q], [d], [(0, 0)], dim)
    assert_exact(got, ref, [(0, 0)], [q])
    assert got[2][0, 0] == min(dups) and got[1][0, 0] == 4.0 * dim


@pytest.mark.parametrize("d_len", [1, 5, 129, 300])
def test_all_negative_similarities_padding_does_not_win(N, d_len):
    """every similarity is negative: the zero rows past d_len (similarity 0) must not be the maximum"""
    dim = 64
    g = np.random.default_rng(d_len)
    q = g.integers(1, 3, (20, dim)).astype(np.float32)
    d = -g.integers(1, 3, (d_len, dim)).astype(np.float32)
    got, ref = run(N, [q], [d], [(0, 0)], dim)
    assert_exact(got, ref, [(0, 0)], [q])
    assert (got[1][0, :20] < 0).all() and got[0][0] < 0 and (got[2][0, :20] < d_len).all()


def test_device_side_refusal_of_a_bad_pair(N):
    """the tables are device data: the wrapper checks its host copies, and the kernel itself answers a pair that is out
    of range with NaN and reads nothing (the C entry, called with tables the wrapper would refuse)"""
    dim = 64
    rows = torch.zeros((40, 64), dtype=torch.float16, device="cuda")
    rows[:, 0] = 1.0
    tables = torch.tensor([0, 10, 30,      # q_start
                           10, 129, 11,    # q_len: sequence 1 too long, sequence 2 past the 40 rows
                           0, 5,           # d_start
                           5, 0,           # d_len: sequence 1 empty
                           0, 1, 2, 0, 0, 3,     # pair_q: 3 is no sequence
                           0, 0, 0, 1, -1, 0],   # pair_d: -1 is no sequence
                          dtype=torch.int32, device="cuda")
    out = torch.full((6,), 7.0, dtype=torch.float32, device="cuda")
    p = tables.data_ptr()
    st = N.lib().mmrag_maxsim_scores(rows.data_ptr(), 40, 64, rows.data_ptr(), 40, 64, dim, p, p + 12, 3, p + 24, p + 32,
                                     2, p + 40, p + 64, 6, out.data_ptr(), None, None,
                                     torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[0] == 10.0 and np.isnan(got[1:]).all(), got


@pytest.mark.parametrize("skip", ["best_sim", "best_idx"])
def test_either_optional_output_alone_may_be_null(N, skip):
    """the C entry with ONE of out_best_sim / out_best_idx NULL: the other and out_sum are what the full call writes"""
    dim = 64
    g = np.random.default_rng(9)
    q_seqs, d_seqs, pairs = [int_rows(g, 17, dim), int_rows(g, 128, dim)], [int_rows(g, 129, dim)], [(0, 0), (1, 0)]
    (sums, bs, bi), _ = run(N, q_seqs, d_seqs, pairs, dim)
    rows, starts, lens = layout(q_seqs + d_seqs, dim, 64)
    dev = torch.from_numpy(rows).cuda().half().contiguous()
    t = torch.tensor(np.concatenate([starts[:2], lens[:2], starts[2:], lens[2:], [0, 1], [0, 0]]), dtype=torch.int32,
                     device="cuda")
    out = torch.zeros(2, dtype=torch.float32, device="cuda")
    o_sim = torch.full((2, W), -7.0, dtype=torch.float32, device="cuda")
    o_idx = torch.full((2, W), -7, dtype=torch.int32, device="cuda")
    p, n = t.data_ptr(), dev.shape[0]
    st = N.lib().mmrag_maxsim_scores(dev.data_ptr(), n, 64, dev.data_ptr(), n, 64, dim, p, p + 8, 2, p + 16, p + 20, 1,
                                     p + 24, p + 32, 2, out.data_ptr(),
                                     None if skip == "best_sim" else o_sim.data_ptr(),
                                     None if skip == "best_idx" else o_idx.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), sums)
    for a, n_q in ((0, 17), (1, 128)):
        if skip == "best_sim":
            assert np.array_equal(o_idx.cpu().numpy()[a, :n_q], bi[a, :n_q]) and (o_sim == -7.0).all()
        else:
            assert np.array_equal(o_sim.cpu().numpy()[a, :n_q], bs[a, :n_q]) and (o_idx == -7).all()
    assert (o_sim[0, 17:] == -7.0).all() and (o_idx[0, 17:] == -7).all()      # slots i >= q_len are not written


def unit_rows(g, n, dim):
    x = g.standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("at,dim", list(enumerate((64, 128, 384, 768))))
def test_random_unit_rows(N, at, dim):
    g = np.random.default_rng(200 + dim)
    q_seqs = [unit_rows(g, n, dim) for n in Q_LENS]
    d_seqs = [unit_rows(g, n, dim) for n in D_LENS]
    pairs = [(a, b) for a in range(len(Q_LENS)) for b in range(len(D_LENS)) if (a + b + at) % 2 == 1]
    (sums, bs, bi), ref = run(N, q_seqs, d_seqs, pairs, dim, one_buffer=(at % 2 == 0))
    worst = 0.0
    for p, ((a, b), (r_sim, _, _, r_mean)) in enumerate(zip(pairs, ref)):
        n = len(q_seqs[a])
        full = late_ref.sims(np.asarray(q_seqs[a], np.float16), np.asarray(d_seqs[b], np.float16))
        worst = max(worst, float(np.abs(bs[p, :n] - r_sim).max()))
        assert np.abs(bs[p, :n] - r_sim).max() <= TOL, (p, float(np.abs(bs[p, :n] - r_sim).max()))
        assert abs(float(sums[p]) / n - r_mean) <= 1e-4 + n * 2.0 ** -23, (p, float(sums[p]) / n, r_mean)
        idx = bi[p, :n]
        assert ((idx >= 0) & (idx < len(d_seqs[b]))).all(), (p, idx)
        assert (full[np.arange(n), idx] >= r_sim - 2 * TOL).all(), p      # every token is checked
    print(f"dim {dim}: max |best_sim - float64| = {worst:.2e}")


# ---------------------------------------------------------------- token rows of the encoder
SHAPES = {"tiny": dataclasses.replace(E.TINY, max_pos=256),
          "h384": E.BertShape(2, 384, 12, 1536, vocab=1000, max_pos=256)}
_token_cases = {}


def token_case(name, pool):
    """(encoder, fp16-rounded weights, shape), built once per (shape, pool)"""
    from multimodal_rag_amd.encoder import DeviceEncoder, EncoderConfig

    if (name, pool) not in _token_cases:
        shape = SHAPES[name]
        w = E.make_bert_weights(shape, 31)
        cfg = EncoderConfig(name, shape.n_layers, shape.hidden, shape.n_heads, shape.intermediate, shape.vocab,
                            shape.max_pos, max_seq_length=shape.max_pos, pool=pool, ln_eps=shape.ln_eps)
        _token_cases[(name, pool)] = (DeviceEncoder(cfg, w, "cuda:0"), E.round_weights_fp16(w), shape)
    return _token_cases[(name, pool)]


_oracle_rows = {}


def oracle_hidden(name, seqs):
    """float64 last hidden states of each sequence (computed once per (shape, lengths); the weights do not depend on
    the pool setting)"""
    key = (name, tuple(len(s) for s in seqs))
    if key not in _oracle_rows:
        _, w16, shape = token_case(name, "mean")
        _oracle_rows[key] = [np.asarray(E.bert_hidden_states(shape, w16, s), np.float64) for s in seqs]
    return _oracle_rows[key]


def normalised(x):
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


def as_arrays(seqs):
    ids = np.zeros((len(seqs), max(len(s) for s in seqs)), np.int32)
    for i, s in enumerate(seqs):
        ids[i, : len(s)] = s
    return ids, np.array([len(s) for s in seqs], np.int32)


def sequences(name, lens):
    g = np.random.default_rng(sum(lens) + len(lens))
    return [g.integers(1, SHAPES[name].vocab, n).tolist() for n in lens]


@pytest.mark.parametrize("name", ["tiny", "h384"])
@pytest.mark.parametrize("lens", [[37], [1, 63, 64, 65, 200]], ids=["one", "batch"])
@pytest.mark.parametrize("pool", ["mean", "cls"])
def test_token_rows_vs_oracle(N, name, lens, pool):
    """one sequence of <= 64 tokens (h384: the folded-LayerNorm body) and a batch (the general body), with both pool
    settings in the desc: the token rows do not depend on it"""
    enc, _, shape = token_case(name, pool)
    seqs = sequences(name, lens)
    before = enc.encode_ids(seqs).clone()
    tokens, cu = enc.encode_tokens(*as_arrays(seqs))
    after = enc.encode_ids(seqs)
    torch.cuda.synchronize()
    # the pooled bits are unchanged by a tokens call in between.  The batch case shares the encoder's workspace with it;
    # the single sequence goes through its captured graph, which owns a workspace, so there this only shows that the
    # tokens call left the graph's buffers and the weights alone
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    H = shape.hidden
    # out_dim is a multiple of 64: the padded width is out_dim itself, the rows have no pad columns
    assert N.padded_dim(H, torch.float16) == H
    assert tokens.dtype == torch.float16 and tokens.shape == (sum(lens), H) and tokens.is_contiguous()
    assert cu.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    got = tokens.float().cpu().numpy().astype(np.float64)
    worst_err, worst_cos = 0.0, 1.0
    for b, hs in enumerate(oracle_hidden(name, seqs)):
        want = normalised(hs)
        mine = got[cu[b]: cu[b + 1], :H]
        err = np.abs(mine - want).max(axis=1)
        cos = (mine * want).sum(1) / np.linalg.norm(mine, axis=1)
        worst_err, worst_cos = max(worst_err, float(err.max())), min(worst_cos, float(cos.min()))
        assert err.max() <= 4e-3 and cos.min() >= 0.9999, (b, float(err.max()), float(cos.min()))
    print(f"{name} {lens} {pool}: max |delta| = {worst_err:.2e}, min cosine = {worst_cos:.6f}")
    if pool == "cls":
        # token row 0 of a sequence is its CLS-pooled embedding, rounded to fp16 once
        pooled = before.cpu().numpy().astype(np.float64)
        first = got[cu[:-1], :H]
        assert np.abs(first - pooled).max() <= 2.0 ** -12 + 1e-6, float(np.abs(first - pooled).max())


@pytest.mark.parametrize("name", ["tiny", "h384"])
@pytest.mark.parametrize("lens", [[37], [1, 63, 64, 65, 200]], ids=["one", "batch"])
def test_projected_token_rows(N, name, lens):
    enc, _, shape = token_case(name, "mean")
    seqs = sequences(name, lens)
    H, out_dim = shape.hidden, 128 if name == "h384" else 64
    g = np.random.default_rng(7)
    proj = (g.standard_normal((out_dim, H)) * 0.05).astype(np.float16)
    tokens, cu = enc.encode_tokens(*as_arrays(seqs), proj=torch.from_numpy(proj))
    torch.cuda.synchronize()
    assert tokens.shape == (sum(lens), out_dim) and N.padded_dim(out_dim, torch.float16) == out_dim
    got = tokens.float().cpu().numpy().astype(np.float64)
    for b, hs in enumerate(oracle_hidden(name, seqs)):
        want = normalised(hs @ proj.astype(np.float64).T)
        mine = got[cu[b]: cu[b + 1], :out_dim]
        err = np.abs(mine - want).max()
        cos = ((mine * want).sum(1) / np.linalg.norm(mine, axis=1)).min()
        assert err <= 4e-3 and cos >= 0.9999, (b, float(err), float(cos))


def test_encode_tokens_refuses_fp32_mode(N):
    from multimodal_rag_amd.encoder import DeviceEncoder, EncoderConfig

    shape = SHAPES["tiny"]
    cfg = EncoderConfig("t", shape.n_layers, shape.hidden, shape.n_heads, shape.intermediate, shape.vocab, shape.max_pos,
                        max_seq_length=shape.max_pos, pool="mean", ln_eps=shape.ln_eps)
    enc = DeviceEncoder(cfg, E.make_bert_weights(shape, 1), "cuda:0", precision="fp32")
    with pytest.raises(RuntimeError, match="fp16"):
        enc.encode_tokens(*as_arrays([[5, 6, 7]]))


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def manager(N):
    from multimodal_rag_amd import embedder as EM

    saved = (EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION, EM.settings.MMRAG_RERANKER_DIR)
    EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION, EM.settings.MMRAG_RERANKER_DIR = "", "fp16", ""
    try:
        yield EM.EmbeddingManager(engine=EM.HipEngine("sentence-transformers/all-MiniLM-L6-v2"), enable_cache=False)
    finally:
        EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION, EM.settings.MMRAG_RERANKER_DIR = saved


DOCS = ["the quick brown fox jumps over the lazy dog " * 3, "how do solar panels turn light into power",
        "a recipe for sourdough bread with a long cold proof " * 12, None, "solar power",
        "wind turbines and solar panels feed the grid " * 40]
QUERY = "how do solar panels turn light into power"


def hits(docs):
    n = len(docs)
    return {"ids": [f"id{i}" for i in range(n)], "distances": [0.1 * i for i in range(n)],
            "metadatas": [{"i": i} for i in range(n)], "documents": list(docs)}


def test_late_rerank_end_to_end(N, manager):
    import asyncio

    assert manager.has_late_reranker()
    res = hits(DOCS)
    out = asyncio.run(manager.rerank_results(QUERY, res, top_k=4, method="late", explain=True))
    assert set(out) == {"ids", "distances", "metadatas", "documents", "rerank_scores", "late_matches"}
    assert len(out["ids"]) == 4 and out["rerank_scores"] == sorted(out["rerank_scores"], reverse=True)
    # the candidate whose text IS the query: every query token finds itself
    assert out["ids"][0] == "id1" and out["rerank_scores"][0] >= 0.9996, out["rerank_scores"]
    # the scores are late_ref over the device's own token rows
    scorer = manager._get_late()
    docs = [d if d is not None else "" for d in DOCS]
    pairs = [(0, j) for j in range(len(docs))]
    plan = scorer.plan([QUERY], docs, pairs)
    tokens, _ = scorer.encoder.encode_tokens(plan["ids"], plan["lens"])
    rows = tokens.float().cpu().numpy().astype(np.float64)
    ref = late_ref.score_tables(rows, rows, plan["q_start"], plan["q_len"], plan["d_start"], plan["d_len"],
                                plan["pair_q"], plan["pair_d"])
    full = asyncio.run(manager.late_rerank(QUERY, res, explain=True))
    by_id = dict(zip(full["ids"], full["rerank_scores"]))
    for j, (_, r_idx, _, r_mean) in enumerate(ref):
        assert abs(by_id[f"id{j}"] - r_mean) <= 1e-4, (j, by_id[f"id{j}"], r_mean)
    # the matches name real tokens of the passage
    match_of = dict(zip(full["ids"], full["late_matches"]))
    for j in range(len(docs)):
        d_len = int(plan["d_len"][plan["pair_d"][j]])
        assert len(match_of[f"id{j}"]) == int(plan["q_len"][0])
        assert all(0 <= m["doc_index"] < d_len for m in match_of[f"id{j}"]), j
    assert [m["doc_index"] for m in match_of["id1"]] == list(range(int(plan["q_len"][0])))


def test_batch_late_rerank_equals_single_calls(N, manager):
    """one scoring call for all questions against one call per question: the same answers, list against list -- ids,
    distances, metadatas, documents and rerank_scores, in order, the scores bit for bit.  A token row's bits depend on
    its own sequence alone: every GEMM of the forward adds a row's K products in one order whatever tile kernel the
    batch size selects, and attention reads only the sequence's own keys; MaxSim then scores a pair from its two
    sequences' rows in a fixed order.  The three questions here meet different GEMM tile kernels and attention paths
    alone (a few hundred tokens, longest 122 / 256) and together."""
    import asyncio

    qs = [QUERY, "bread", "a fox and a dog"]
    lists = [hits(DOCS), hits(DOCS[:3]), hits([])]
    got = asyncio.run(manager.batch_late_rerank(qs, lists, top_k=3))
    single = [asyncio.run(manager.late_rerank(q, r, top_k=3)) for q, r in zip(qs, lists)]
    for q, mine, alone in zip(qs, got, single):
        print(q, mine["ids"], mine["rerank_scores"], alone["rerank_scores"])
    assert got == single
    assert [len(g["ids"]) for g in got] == [3, 3, 0] and got[0]["ids"][0] == "id1"
    assert all(set(g) == {"ids", "distances", "metadatas", "documents", "rerank_scores"} for g in got)


def test_query_route_late_rerank(N, manager):
    from starlette.testclient import TestClient

    from multimodal_rag_amd import server

    assert not server.settings.MMRAG_RERANKER_DIR
    with TestClient(server.create_app(embedder=manager)) as c:
        for i, body in enumerate(["alpha beta gamma delta. " * 3, "solar panels turn light into power. " * 3,
                                  "zeta eta theta. " * 30]):
            r = c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
        q = {"query": "solar panels turn light into power", "top_k": 2, "rerank": True, "rerank_method": "late"}
        r = c.post("/query", json=q)
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert 1 <= len(src) <= 2 and all(-1.0 <= s["rerank_score"] <= 1.0 + 1e-3 for s in src)
        assert [s["rerank_score"] for s in src] == sorted((s["rerank_score"] for s in src), reverse=True)
        assert all("matches" not in s for s in src)
        r = c.post("/query", json={**q, "explain": True})
        assert r.status_code == 200, r.text
        scorer = manager._get_late()
        for s in r.json()["sources"]:
            stored = manager.collection.get(ids=[s["doc_id"]])["documents"][0] or ""
            d_len = int(scorer.plan(["x"], [stored], [(0, 0)])["d_len"][0])
            assert len(s["matches"]) == 6                     # the query's six words
            assert all(0 <= m["doc_index"] < d_len and -1.0 <= m["similarity"] <= 1.0 + 1e-3 for m in s["matches"])
        # the cross method still needs its model
        r = c.post("/query", json={"query": "solar", "rerank": True})
        assert r.status_code == 400 and "MMRAG_RERANKER_DIR" in r.json()["detail"]
