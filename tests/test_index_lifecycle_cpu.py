"""tests/index_model.py proved on the CPU: the generator's exactness claims, the model's add / delete / compact / reset
bookkeeping against a naive list implementation over a few hundred random operations, its answers against brute force,
and the property the GPU lifecycle test leans on -- an answer expressed as ids does not change across a compaction."""
import copy

import numpy as np
import pytest
import torch

from tests import f8_ref
from tests import index_model as M


def test_generator_rows_are_exact_in_every_storage_format():
    x = M.exact_rows(np.random.default_rng(1), 600)
    assert set(np.count_nonzero(x, axis=1).tolist()) == {4, 16, 64}          # the three kinds, mixed
    assert np.array_equal(np.einsum("ij,ij->i", x, x), np.ones(600))         # norm exactly 1.0
    x32 = x.astype(np.float32)
    assert np.array_equal(np.sqrt(np.einsum("ij,ij->i", x32, x32)), np.ones(600, np.float32))
    dots = (x @ x.T) * 64
    assert np.array_equal(dots, np.rint(dots)) and np.abs(dots).max() <= 64  # integer dot products after scaling by 64
    for dt in (torch.float16, torch.bfloat16):
        assert np.array_equal(torch.from_numpy(x32).to(dt).to(torch.float32).numpy(), x32)
    codes = f8_ref.encode(x32)
    assert np.array_equal(f8_ref.decode(codes), x * f8_ref.SCALE)            # exact as the E4M3 code of x * 256
    assert set(np.abs(f8_ref.decode(codes)).reshape(-1).tolist()) == {0.0, 32.0, 64.0, 128.0}
    # the bf16 split of the fp32 path: the high half is the value, the low half zero
    hi = torch.from_numpy(x32).to(torch.bfloat16).to(torch.float32).numpy()
    assert not np.any(x32 - hi)


def test_generator_plants_duplicates_and_fields():
    gen = M.Generator(3)
    rows = gen.rows(120)
    twins = [c for c in range(120) if c % 5 == 0 and c >= 9]
    assert twins and all(np.array_equal(rows[c]["vec"], rows[c - 9]["vec"]) for c in twins)
    assert all(np.array_equal(rows[c]["tok"], rows[c - 9]["tok"]) for c in twins)
    assert all(1 <= r["tok"].shape[0] <= 40 or r["tok"].shape[0] == 0 for r in rows)
    assert any(r["tok"].shape[0] == 0 for r in rows) and any("sec" not in r["meta"] for r in rows)
    assert any(np.isnan(r["time"]) for r in rows)
    for r in rows:
        assert np.all(np.diff(r["sp_terms"]) > 0) and np.all((r["sp_imps"] >= 1) & (r["sp_imps"] <= 255))
        assert np.isnan(r["time"]) or (M.NOW - r["time"]) / M.HOUR in (0.0, 1.0, 2.0, 3.0)
    spec = (1.0, M.HOUR, {"tag": {"a": 0.5, "b": -0.25}}, M.NOW)
    m = M.IndexModel()
    m.add(rows)
    prior = m.prior_column(spec).astype(np.float64) * 8
    assert np.array_equal(prior, np.rint(prior))                              # priors are multiples of 1/8


class Naive:
    """the collection semantics restated over one plain list of (id, payload, live) with no shortcuts"""

    def __init__(self, min_dead):
        self.items, self.min_dead = [], min_dead

    def add(self, batch):
        for row in batch:
            if not any(live and i == row["id"] for i, _, live in self.items):
                self.items.append([row["id"], row, True])

    def delete(self, ids=None, where=None):
        gone = []
        for it in self.items:
            if it[2] and (ids is None or it[0] in ids) and M.match_where(it[1]["meta"], where):
                it[2] = False
                gone.append(it[0])
        dead = sum(not it[2] for it in self.items)
        if gone and dead >= self.min_dead and dead > 0.25 * len(self.items):
            self.compact()
        return sorted(gone)

    def compact(self):
        self.items = [it for it in self.items if it[2]]


def test_bookkeeping_against_a_naive_list_over_random_operations():
    g = np.random.default_rng(7)
    gen = M.Generator(8)
    model, naive = M.IndexModel(compact_min_dead=8), Naive(8)
    ever = []
    for step in range(300):
        op = g.integers(0, 10)
        if op < 5:
            m = int(g.integers(1, 9))
            ids = None
            if ever and g.integers(0, 2):       # ids that exist, that were deleted, and one repeated inside the batch
                ids = [ever[int(i)] for i in g.integers(0, len(ever), m)]
                ids[-1] = ids[0]
            batch = gen.rows(m, ids)
            kept = model.add(batch)
            naive.add(batch)
            ever += [r["id"] for r in batch]
            assert len(set(batch[i]["id"] for i in kept)) == len(kept)
        elif op < 8 and ever:
            if g.integers(0, 2):
                ids = [ever[int(i)] for i in g.integers(0, len(ever), int(g.integers(1, 6)))]
                assert model.delete(ids=ids) == naive.delete(ids=ids)
            else:
                where = [{"tag": "b"}, {"n": {"$gte": 8}}, {"doc_id": f"d{int(g.integers(0, 40))}"}][int(g.integers(0, 3))]
                assert model.delete(where=where) == naive.delete(where=where)
        elif op == 8:
            model.compact()
            naive.compact()
        elif step % 97 == 0:
            model.reset()
            naive.items = []
        assert [(r["id"], r["live"]) for r in model.rows] == [(i, live) for i, _, live in naive.items]
        assert all(r is it[1] or np.array_equal(r["vec"], it[1]["vec"]) for r, it in zip(model.rows, naive.items))
        live = model.live_ids()
        assert len(set(live)) == len(live) == model.count()
        assert model.get(ids=live[:3])["ids"] == live[:3]
    assert model.n > 50 and model.n - model.count() > 0      # the run ends with tombstones in place


@pytest.fixture(scope="module")
def filled():
    gen = M.Generator(21)
    model = M.IndexModel()
    model.enable_grouping("doc_id")
    model.add(gen.rows(260))
    model.enable_grouping("sec")
    model.set_prior("pin", [(i % 9 - 4) / 8 for i in range(260)])
    model.delete(ids=["r0", "r259", "r10", "r91"])            # r10's twin r1 and r91's twin r100 stay alive
    model.delete(where={"doc_id": "d7"})
    return gen, model


def test_dense_answers_equal_brute_force(filled):
    gen, model = filled
    q = gen.queries(3, [model.rows[model.row_of("r5")]["vec"]])
    where = {"$and": [{"n": {"$gte": 2}}, {"tag": {"$in": ["a", "b"]}}, {"$added_at": {"$gte": M.NOW - 1.5 * M.HOUR}}]}
    for w in (None, where):
        s, r = model.search(q, 21, w)
        for b in range(3):
            cand = [(-float(np.dot(q[b].astype(np.float64), row["vec"])), i) for i, row in enumerate(model.rows)
                    if row["live"] and (w is None or (row["meta"]["n"] >= 2 and row["meta"]["tag"] in "ab"
                                                      and row["time"] >= M.NOW - 1.5 * M.HOUR))]
            want = sorted(cand)[:21]
            assert r[b].tolist()[: len(want)] == [i for _, i in want]
            assert s[b].tolist()[: len(want)] == [-v for v, _ in want]
    assert model.ids_of(model.search(q, 5)[1][0])[0] == "r5" and model.search(q, 5)[0][0, 0] == 1.0
    twin = model.search(model.rows[model.row_of("r100")]["vec"][None].astype(np.float32), 3)
    assert model.ids_of(twin[1][0])[0] == "r100" and twin[0][0, 0] == 1.0 and twin[0][0, 1] < 1.0     # r91 is dead


def test_boosted_sparse_and_duplicates_equal_brute_force(filled):
    gen, model = filled
    q = gen.queries(2)
    spec = (1.0, M.HOUR, {"tag": {"a": 0.5, "b": -0.25}}, M.NOW)
    for prior in ("pin", spec):
        s, r, boosts = model.boosted(q, 9, prior, 0.5)
        col = model.prior_column(prior).astype(np.float64)
        for b in range(2):
            cand = sorted((-(float(np.dot(q[b].astype(np.float64), row["vec"])) + 0.5 * col[i]), i)
                          for i, row in enumerate(model.rows) if row["live"])[:9]
            assert r[b].tolist() == [i for _, i in cand] and s[b].tolist() == [-v for v, _ in cand]
            assert boosts[b].tolist() == [0.5 * col[i] for _, i in cand]
    sq = gen.sparse_queries(3)
    s, r = model.sparse(sq, 7)
    for b in range(3):
        qw = dict(zip(sq[1][sq[0][b]: sq[0][b + 1]].tolist(), sq[2][sq[0][b]: sq[0][b + 1]].tolist()))
        score = [sum(qw.get(int(t), 0) * int(w) for t, w in zip(row["sp_terms"], row["sp_imps"])) for row in model.rows]
        cand = sorted((-v, i) for i, (v, row) in enumerate(zip(score, model.rows)) if v > 0 and row["live"])[:7]
        assert [i for i in r[b].tolist() if i >= 0] == [i for _, i in cand]
    pairs, groups = model.near_duplicates(1.0)
    want = {(i, j) for i in range(model.n) for j in range(i + 1, model.n)
            if model.rows[i]["live"] and model.rows[j]["live"] and np.array_equal(model.rows[i]["vec"], model.rows[j]["vec"])}
    assert set(pairs) == want and want and all(g_ == sorted(g_) for g_ in groups)


def answers(gen_seed, model):
    """every mode of the model as ids and score bytes"""
    gen = M.Generator(gen_seed)
    q = gen.queries(3, [model.rows[model.row_of("r5")]["vec"]])
    ids = model.ids_of
    where = {"$and": [{"n": {"$gte": 2}}, {"tag": {"$in": ["a", "b"]}}, {"$added_at": {"$gte": M.NOW - 1.5 * M.HOUR}}]}
    out = {}
    s, r = model.search(q, 21, where)
    out["search"] = (s.tobytes(), ids(r))
    ms, mr, _, mv = model.mmr(q, 5, 32, 0.5)
    out["mmr"] = (ms.tobytes(), mv.tobytes(), ids(mr))
    out["grouped"] = [(c, a[0].tobytes(), ids(a[1]), [model.groups["sec"][o] if o >= 0 else o for o in a[3]])
                      for c, a in model.grouped(q, 4, 2, "sec")]
    s, r = model.scoped(q, 5, [["d1", "d2"], ["d3"], ["nope"]], "doc_id")
    out["scoped"] = (s.tobytes(), ids(r))
    c, t, s, r = model.range(q, 0.25, 10, [None, where, None], ["sec"])
    out["range"] = (c.tolist(), [dict(zip(model.groups["sec"] + [None], row)) for row in t[0].tolist()], s.tobytes(), ids(r))
    docs = model.power_of_two_documents()
    sim, grp, cov, best, brow = model.related([{"value": docs[0]}, q[:2].astype(np.float64)], 4, "doc_id", 0.75)
    out["related"] = (sim.tobytes(), [model.groups["doc_id"][o] if o >= 0 else o for o in grp.reshape(-1)], cov.tolist(),
                      best.tobytes(), ids(brow))
    s, r, b = model.boosted(q, 7, "pin", [1.0, 0.25, 2.0])
    out["boosted"] = (s.tobytes(), b.tobytes(), ids(r))
    rec = model.recommend([["r5", q[1]], [q[2]]], [[q[0]], []], 6, 0.5)
    out["recommend"] = (rec[0].tobytes(), ids(rec[1]), rec[2].tobytes(), rec[3].tobytes(), rec[4].tolist(), rec[5].tolist())
    f = model.fused(q, [0, 2, 3], 8, 50, weights=[1.0, 0.5, 1.0], method="max")
    out["fused"] = (f[0].tobytes(), ids(f[1]), f[2].tobytes(), f[3].tolist(), f[4].tolist())
    qt = M.exact_rows(np.random.default_rng(5), 7, M.TOKEN_DIM)
    for f8 in (False, True):
        s, r = model.late(qt, [0, 3], [3, 4], 6, f8=f8)
        out["late", f8] = (s.tobytes(), ids(r))
    out["lexical"] = ids(model.lexical_rows("học máy gpu", 10))
    s, r = model.sparse(gen.sparse_queries(3), 7)
    out["sparse"] = (s.tobytes(), ids(r))
    pairs, groups = model.near_duplicates(0.75)
    out["dups"] = ([(model.rows[a]["id"], model.rows[b]["id"], v) for (a, b), v in sorted(pairs.items())],
                   [ids(g_) for g_ in groups])
    return out


def test_answers_as_ids_do_not_change_across_a_compaction(filled):
    model = copy.deepcopy(filled[1])
    assert model.n - model.count() >= 10
    before = answers(33, model)
    n_before = model.n
    model.compact()
    assert model.n < n_before and model.n == model.count()
    after = answers(33, model)
    assert before.keys() == after.keys()
    for key in before:
        assert before[key] == after[key], key
    assert before["late", False] == before["late", True]      # exact token rows: the FP8 definition gives the same numbers
