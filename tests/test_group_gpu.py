"""GPU: grouping search hits by a per-row key (csrc/group.hip through _native.group_select, VectorIndex,
EmbeddingManager and POST /query) against tests/group_ref.py.  Nothing here is arithmetic: every comparison with the
reference is exact, scores bit for bit."""
import asyncio

import numpy as np
import pytest
import torch

from tests import group_ref as R

pytestmark = pytest.mark.gpu

TORCH_DT = {"fp16": torch.float16, "fp32": torch.float32}
GS = [(1, 1), (5, 1), (5, 3), (256, 16), (7, 16)]
BC = [(1, 1), (3, 63), (3, 64), (3, 65), (5, 200), (2, 4096)]
TOL = 1e-4          # tests/test_search_gpu.py: cosine scores within 1e-4, every dtype


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return "cuda:0"


# ---------------------------------------------------------------- 1. the kernel against the reference
def bits_equal(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def run_kernel(dev, scores, rows, gor, n_rows, G, S):
    from multimodal_rag_amd import _native

    out = _native.group_select(torch.from_numpy(scores).to(dev), torch.from_numpy(rows).to(dev),
                               torch.from_numpy(gor).to(dev), n_rows, G, S)
    return [t.cpu().numpy() for t in out]


def check_against_reference(dev, scores, rows, gor, n_rows, what, gs=GS):
    for G, S in gs:
        got = run_kernel(dev, scores, rows, gor, n_rows, G, S)
        for b in range(len(rows)):
            want = R.select_padded(scores[b], rows[b], gor, n_rows, G, S)
            for name, g_, w_ in zip(("scores", "rows", "positions", "groups", "info"), got, want):
                assert bits_equal(g_[b], w_), (what, G, S, b, name, g_[b].ravel()[:12], w_.ravel()[:12])


def make_lists(B, C, n_rows, seed, row_range=None, ties=False):
    """B candidate lists of C distinct rows, scores descending with -0.0, a denormal and exact repeats among them"""
    g = np.random.default_rng(seed)
    rows = np.stack([g.choice(row_range or n_rows, C, replace=False) for _ in range(B)]).astype(np.int64)
    scores = -np.sort(-g.standard_normal((B, C)).astype(np.float32), axis=1)
    if ties:
        scores = (np.round(scores * 1.5) / 1.5).astype(np.float32)       # long runs of equal scores
    if not ties and C > 2:                                                # bit patterns a float comparison would lose
        scores[:, C // 2] = np.float32(-0.0)
        scores[:, -1] = np.float32(-1e-42)
    return np.ascontiguousarray(scores), rows


PATTERNS = ["equal", "distinct", "mult4096", "mult8192", "mixed", "oob", "cut", "ties", "late"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("B,C", BC)
def test_kernel_equals_reference(dev, B, C, pattern):
    n_rows = 6000
    g = np.random.default_rng(1000 * C + B)
    scores, rows = make_lists(B, C, n_rows, seed=C + 7 * B, ties=pattern == "ties",
                              row_range=n_rows + max(C // 3, 2) if pattern == "oob" else None)
    if pattern == "equal":
        gor = np.full(n_rows, 3, np.int32)
    elif pattern == "distinct":                       # C = 4096: 4096 groups against G = 256
        gor = np.arange(n_rows, dtype=np.int32)
    elif pattern in ("mult4096", "mult8192"):         # every ordinal lands in slot 0 of a 1024-, 4096- or 8192-slot table
        step = 4096 if pattern == "mult4096" else 8192
        gor = (step * g.integers(0, 300 if pattern == "mult4096" else 40, n_rows)).astype(np.int32)
    elif pattern == "late":
        # group 5 gets exactly S members early (for S = 1, 3, 16 alike: its 16 first members sit in the first chunk when
        # C allows) and one more at the very last position; the rest are spread over 11 other groups
        gor = g.integers(6, 17, n_rows).astype(np.int32)
        for b in range(B):
            early = list(range(0, min(16, C - 1)))
            gor[rows[b, early]] = 5
            gor[rows[b, C - 1]] = 5
    else:
        gor = g.integers(0, 37, n_rows).astype(np.int32)
        gor[g.random(n_rows) < 0.2] = -1
        gor[g.random(n_rows) < 0.05] = -12345
    if pattern == "cut":
        for at in (0, 1, 64, C - 1):
            if at < C:
                s2, r2 = scores.copy(), rows.copy()
                s2[B // 2:, at:], r2[B // 2:, at:] = -np.inf, -1       # half the batch is cut, and what follows the
                r2[B // 2:, at + 1:] = rows[B // 2:, at + 1:]             # first -1 is live rows again: not to be read
                check_against_reference(dev, s2, r2, gor, n_rows, (pattern, at))
        return
    check_against_reference(dev, scores, rows, gor, n_rows, pattern)


def test_late_member_and_full_groups_at_the_chunk_edges(dev):
    """a group's S-th member at the last lane of a chunk and its S+1-th at the first lane of the next, and at C - 1"""
    n_rows, C = 5000, 4096
    for S in (1, 3, 16):
        scores, rows = make_lists(2, C, n_rows, seed=S)
        gor = np.arange(100, 100 + n_rows, dtype=np.int32)
        # group 7: its S-th member in lane 63, the next in lane 0 of the following chunk, more in the last chunk
        members = [63, 64, 4032, C - 1] if S == 1 else [0] + list(range(65 - S, 64)) + [64, 4032, C - 1]
        # group 8: exactly S members in the first chunk, the S+1-th in the last one
        second = list(range(1, S + 1)) + [C - 2]
        assert len(set(members) & set(second)) == 0 and len([m for m in members if m < 64]) == S
        for b in range(2):
            gor[rows[b, members]] = 7
            gor[rows[b, second]] = 8
        check_against_reference(dev, scores, rows, gor, n_rows, ("edge", S), gs=[(3, S), (256, S), (1, S)])


def test_native_argument_checks(dev):
    from multimodal_rag_amd import _native

    def call(C=10, G=2, S=2, B=2, n_rows=100, gor_len=100):
        s = torch.zeros((B, C), dtype=torch.float32, device=dev)
        r = torch.zeros((B, C), dtype=torch.int64, device=dev)
        return _native.group_select(s, r, torch.zeros(gor_len, dtype=torch.int32, device=dev), n_rows, G, S)

    for bad in (dict(C=0), dict(C=4097), dict(G=0), dict(G=257), dict(S=0), dict(S=17), dict(n_rows=-1),
                dict(n_rows=101)):
        with pytest.raises(_native.MMRagNativeError):
            call(**bad)
    for good in (dict(C=1), dict(C=4096), dict(G=1), dict(G=256), dict(S=1), dict(S=16)):
        out = call(**good)
        assert out[4][:, 0].tolist() == [1, 1]                               # rows all 0: one group
    assert call(n_rows=0, gor_len=0)[4].tolist() == [[2, 10], [2, 10]]       # no row has a key: G groups of one
    s = torch.zeros((2, 10), dtype=torch.float32, device=dev)
    r = torch.zeros((2, 10), dtype=torch.int64, device=dev)
    gor = torch.zeros(100, dtype=torch.int32, device=dev)
    for args in ((s.cpu(), r, gor), (s, r.int(), gor), (s.t().contiguous().t(), r, gor), (s, r, gor.long()),
                 (s, r[:, :5], gor)):
        with pytest.raises(_native.MMRagNativeError):
            _native.group_select(*args, 100, 2, 2)


def test_graph_capture_replays_the_same_bits(dev):
    from multimodal_rag_amd import _native

    scores, rows = make_lists(8, 200, 3000, seed=3)
    gor = np.random.default_rng(4).integers(-1, 25, 3000).astype(np.int32)
    s, r, g = (torch.from_numpy(x).to(dev) for x in (scores, rows, gor))
    eager = [t.clone() for t in _native.group_select(s, r, g, 3000, 5, 3)]
    side = torch.cuda.Stream()                                             # one stream, no parallel branches
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _native.group_select(s, r, g, 3000, 5, 3)                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _native.group_select(s, r, g, 3000, 5, 3)
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_a_query_block_does_not_depend_on_its_batch(dev):
    B, C, n_rows = 9, 300, 4000
    scores, rows = make_lists(B, C, n_rows, seed=11)
    rows[3, 100:] = -1
    rows[6, 0] = -1
    gor = np.random.default_rng(12).integers(-1, 30, n_rows).astype(np.int32)
    base = run_kernel(dev, scores, rows, gor, n_rows, 7, 4)
    perm = np.random.default_rng(13).permutation(B)
    mixed = run_kernel(dev, np.ascontiguousarray(scores[perm]), np.ascontiguousarray(rows[perm]), gor, n_rows, 7, 4)
    for a, b in zip(base, mixed):
        assert bits_equal(a[perm], b)
    alone = run_kernel(dev, scores[4:5].copy(), rows[4:5].copy(), gor, n_rows, 7, 4)
    for a, b in zip(base, alone):
        assert bits_equal(a[4:5], b)


# ---------------------------------------------------------------- 2. through VectorIndex
def document_rows(d, seed, n_docs=44, planted=70):
    """n_docs documents of 1..30 unit-norm rows around their own centre, plus one PLANTED document of `planted` rows
    packed tightly around a centre of its own; returns rows, per-row document name, and the planted centre"""
    g = np.random.default_rng(seed)
    sizes = g.integers(1, 31, n_docs)
    sizes[:3] = (1, 30, 17)
    centres = g.standard_normal((n_docs + 1, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    owner = np.repeat(np.arange(n_docs), sizes)
    x = centres[owner] + 0.6 * g.standard_normal((len(owner), d)) / np.sqrt(d)
    tight = centres[n_docs] + 0.05 * g.standard_normal((planted, d)) / np.sqrt(d)
    x = np.concatenate([x, tight])
    owner = np.concatenate([owner, np.full(planted, n_docs)])
    order = g.permutation(len(owner))                                     # a document's rows are not contiguous
    x, owner = x[order], owner[order]
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return x, [f"doc{o}" for o in owner], centres[n_docs]


def make_queries(rows, planted_centre, seed, n_plain=8, n_planted=4):
    """unit queries: n_plain near stored rows of ordinary documents, n_planted near the planted document's centre"""
    g = np.random.default_rng(seed)
    d = rows.shape[1]
    ordinary = np.nonzero(rows @ planted_centre < 0.9)[0]
    plain = rows[g.choice(ordinary, n_plain)] + 0.3 * g.standard_normal((n_plain, d)) / np.sqrt(d)
    hot = planted_centre + 0.02 * g.standard_normal((n_planted, d)) / np.sqrt(d)
    q = np.concatenate([plain[: n_plain // 2], hot, plain[n_plain // 2:]])
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def build_index(dev, rows, names, dtype=torch.float16, extra_meta=None, **kw):
    from multimodal_rag_amd.index import VectorIndex

    n, d = rows.shape
    idx = VectorIndex(dim=d, dtype=dtype, device=dev, capacity=n, **kw)
    metas = [{"doc_id": names[i], "i": i, **(extra_meta(i) if extra_meta else {})} for i in range(n)]
    idx.add(rows, documents=[f"text {i}" for i in range(n)], metadatas=metas, ids=[f"id{i}" for i in range(n)])
    return idx


def host_column(idx, key="doc_id"):
    st = idx.enable_grouping(key)
    return st["col"][: idx.rows_in_use].cpu().numpy(), st["values"]


def structure(idx, ans, values):
    """(key, ids) per group of one query's answer blocks"""
    out = []
    for gi in range(int(ans[4][0])):
        rows = [int(r) for r in ans[1][gi] if r >= 0]
        out.append((values[ans[3][gi]] if ans[3][gi] >= 0 else None, [idx._ids[r] for r in rows]))
    return out


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
@pytest.mark.parametrize("d", [384, 768])
def test_grouped_search_equals_reference_over_search(dev, dt, d):
    rows, names, centre = document_rows(d, seed=d)
    idx = build_index(dev, rows, names, TORCH_DT[dt])
    assert not idx._groups                                                 # nothing built until the first grouped call
    q = make_queries(rows, centre, seed=d + 1, n_planted=0)
    G, S = 3, 2                                                            # 64 hits of documents of <= 30 rows: >= 3 groups
    C0 = R.first_depth(G, S)
    assert C0 == 64
    *got, depths = idx.grouped_search(q, G, S)
    got = [t.cpu().numpy() for t in got]
    assert depths == [C0] * len(q) and list(idx._groups) == ["doc_id"]
    gor, values = host_column(idx)
    assert [values[o] for o in gor] == names                               # ordinals by first appearance in row order
    assert gor[0] == 0 and (np.diff(np.maximum.accumulate(gor)) <= 1).all()
    s, r = (t.cpu().numpy() for t in idx.search(q, C0))
    for b in range(len(q)):
        want = R.select_padded(s[b], r[b], gor, idx.rows_in_use, G, S)
        for g_, w_ in zip(got, want):
            assert bits_equal(g_[b], w_), (b, g_[b], w_)
    # explicit fetch_k: one pass, clipped to [G, 4096]
    for fetch_k, depth in ((1, G), (40, 40), (10 ** 6, 4096)):
        *one, depths = idx.grouped_search(q[:3], G, S, fetch_k=fetch_k)
        assert depths == [depth] * 3
        s, r = (t.cpu().numpy() for t in idx.search(q[:3], depth))
        for b in range(3):
            want = R.select_padded(s[b], r[b], gor, idx.rows_in_use, G, S)
            for g_, w_ in zip(one, want):
                assert bits_equal(g_[b].cpu().numpy(), w_)


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
@pytest.mark.parametrize("d", [384, 768])
def test_mixed_ladder_only_some_queries_deepen(dev, dt, d):
    rows, names, centre = document_rows(d, seed=3 * d)
    idx = build_index(dev, rows, names, TORCH_DT[dt])
    q = make_queries(rows, centre, seed=3 * d + 1)
    B, n = len(q), len(rows)
    G, S = 3, 2
    res = idx.grouped_query(q, n_groups=G, group_size=S)
    gor, values = host_column(idx)
    full_s, full_r = (t.cpu().numpy() for t in idx.search(q, n))          # the exact ranking of every row
    plain = idx.query(q, n_results=n)
    hot = list(range(4, 8))
    for b in range(B):
        assert (len({names[r] for r in full_r[b][:70]}) == 1) == (b in hot)   # the planted document owns the top 70
        C, want = R.ladder(full_s[b], full_r[b], gor, n, G, S)
        assert C == (256 if b in hot else 64) and res["fetch_k"][b] == C and res["exhaustive"][b] is True
        got = [(g["key"], g["ids"]) for g in res["groups"][b]]
        assert got == structure(idx, want, values), (b, got)
        dist_of = dict(zip(plain["ids"][b], plain["distances"][b]))
        for g in res["groups"][b]:
            assert len(g["ids"]) == len(g["distances"]) == len(g["metadatas"]) == len(g["documents"]) <= S
            assert all(m["doc_id"] == g["key"] for m in g["metadatas"])
            assert all(abs(x - dist_of[i]) <= TOL for i, x in zip(g["ids"], g["distances"]))
            assert g["distances"] == sorted(g["distances"])
        best = [g["distances"][0] for g in res["groups"][b]]
        assert best == sorted(best) and len(res["groups"][b]) == G
    for b in (0, hot[0], hot[-1], B - 1):                                  # alone: the identical answer
        alone = idx.grouped_query(q[b:b + 1], n_groups=G, group_size=S)
        assert alone["groups"][0] == res["groups"][b] and alone["fetch_k"] == [res["fetch_k"][b]]
    # tensors of the batch: each query's block is its own pass's block
    *blocks, depths = idx.grouped_search(q, G, S)
    for b in (1, hot[1]):
        *one, depth = idx.grouped_search(q[b:b + 1], G, S)
        assert depth == [depths[b]]
        for whole, part in zip(blocks, one):
            assert torch.equal(whole[b].view(torch.uint8), part[0].view(torch.uint8))


def test_ladder_ends_at_4096_not_exhaustive(dev):
    d, n = 64, 4400
    g = np.random.default_rng(8)
    u = np.zeros(d)
    u[0] = 1.0
    # 4300 rows of one document on the query's side (cos about 0.7), 100 other documents opposite it: the first 4300
    # hits are one document
    x = g.standard_normal((n, d)) / np.sqrt(d) + np.where(np.arange(n) < 4300, 1.0, -1.0)[:, None] * u
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    idx = build_index(dev, x, ["only"] * 4300 + [f"tail{i}" for i in range(100)])
    q = u.astype(np.float32)[None]
    s_all, r_all = (t.cpu().numpy() for t in idx.search(q, 4096))
    res = idx.grouped_query(q, n_groups=2, group_size=1)
    gor, values = host_column(idx)
    C, want = R.ladder(s_all[0], r_all[0], gor, n, 2, 1)
    assert C == 4096 and res["fetch_k"] == [4096]
    assert res["exhaustive"] == [False] and not R.complete(want, C, 2)
    assert (r_all[0] < 4300).all()
    assert [(g_["key"], g_["ids"]) for g_ in res["groups"][0]] == structure(idx, want, values)


def test_state_deletes_filters_compact_adds_and_keys(dev):
    d = 384
    rows, names, centre = document_rows(d, seed=77)
    n = len(rows)
    idx = build_index(dev, rows, names, extra_meta=lambda i: ({"parity": i % 2, "shelf": f"s{i % 5}"} if i % 7 else
                                                            {"parity": i % 2, "shelf": None}))
    q = make_queries(rows, centre, seed=78)
    G, S = 4, 3
    gone = {f"id{i}" for i in range(0, n, 3)}
    idx.delete(ids=sorted(gone))

    def flat(res):
        return [[i for g in groups for i in g["ids"]] for groups in res["groups"]]

    before = idx.grouped_query(q, n_groups=G, group_size=S)
    assert not gone & {i for x in flat(before) for i in x}
    odd = idx.grouped_query(q, n_groups=G, group_size=S, where={"parity": 1})
    assert all(m["parity"] == 1 for groups in odd["groups"] for g in groups for m in g["metadatas"])
    assert not gone & {i for x in flat(odd) for i in x}
    # the reference over the live rows' exact ranking, tombstones in place
    gor, values = host_column(idx)
    live = idx.count()
    s_all, r_all = (t.cpu().numpy() for t in idx.search(q, live))
    for b in range(len(q)):
        _, want = R.ladder(s_all[b], r_all[b], gor, idx.rows_in_use, G, S)
        assert [(g["key"], g["ids"]) for g in before["groups"][b]] == structure(idx, want, values)
    idx.compact()
    assert idx.rows_in_use == idx.count() == live
    after = idx.grouped_query(q, n_groups=G, group_size=S)
    assert [[(g["key"], g["ids"]) for g in groups] for groups in after["groups"]] == \
        [[(g["key"], g["ids"]) for g in groups] for groups in before["groups"]]
    gor2, values2 = host_column(idx)
    assert [values2[o] for o in gor2] == [m["doc_id"] for m in idx._metadatas]
    # rows added after enable_grouping (past the capacity: the column grows with the matrix) are grouped
    g = np.random.default_rng(79)
    new = q[0] + 0.01 * g.standard_normal((5, d)).astype(np.float32) / np.sqrt(d)
    new = (new / np.linalg.norm(new, axis=1, keepdims=True)).astype(np.float32)
    cap = idx.matrix.shape[0]
    filler = rows[: cap - idx.rows_in_use + 3]
    idx.add(filler, metadatas=[{"doc_id": "filler"}] * len(filler), ids=[f"f{i}" for i in range(len(filler))],
            documents=None)
    assert idx.matrix.shape[0] > cap and idx._groups["doc_id"]["col"].shape[0] == idx.matrix.shape[0]
    idx.add(new, metadatas=[{"doc_id": "fresh"}, {"doc_id": "fresh"}, {"doc_id": "doc1"}, {}, {"doc_id": ["x"]}],
            ids=[f"new{i}" for i in range(5)], documents=[f"new text {i}" for i in range(5)])
    res = idx.grouped_query(q[:1], n_groups=4, group_size=3, fetch_k=5)
    assert sorted(i for g in res["groups"][0] for i in g["ids"]) == [f"new{i}" for i in range(5)]
    by_key = {str(g["key"]): g["ids"] for g in res["groups"][0] if g["key"] is not None}
    assert sorted(by_key["fresh"]) == ["new0", "new1"] and by_key["doc1"] == ["new2"]
    solo = [g for g in res["groups"][0] if g["key"] is None]
    assert sorted(g["ids"][0] for g in solo) == ["new3", "new4"] and all(len(g["ids"]) == 1 for g in solo)
    gor3, values3 = host_column(idx)
    assert [values3[o] if o >= 0 else None for o in gor3] == \
        [m.get("doc_id") if isinstance(m.get("doc_id"), str) else None for m in idx._metadatas]
    # a second key, with None values: rows without it are groups of their own
    shelf = idx.grouped_query(q, n_groups=6, group_size=2, group_by="shelf", where={"parity": {"$in": [0, 1]}})
    assert set(idx._groups) == {"doc_id", "shelf"}
    gor_s, values_s = host_column(idx, "shelf")
    s_all, r_all = (t.cpu().numpy() for t in idx.search(q, idx.count(), where={"parity": {"$in": [0, 1]}}))
    for b in range(len(q)):
        _, want = R.ladder(s_all[b], r_all[b], gor_s, idx.rows_in_use, 6, 2)
        assert [(g["key"], g["ids"]) for g in shelf["groups"][b]] == structure(idx, want, values_s)
        keyed = [g["key"] for g in shelf["groups"][b] if g["key"] is not None]
        assert len(keyed) == len(set(keyed)) <= 5
        assert all(len(g["ids"]) == 1 and g["metadatas"][0]["shelf"] is None
                   for g in shelf["groups"][b] if g["key"] is None)
    with pytest.raises(ValueError):
        idx.grouped_query(q, n_groups=257)
    with pytest.raises(ValueError):
        idx.grouped_query(q, n_groups=0)
    with pytest.raises(ValueError):
        idx.grouped_query(q, n_groups=3, group_size=17)
    idx.reset()
    assert not idx._groups
    assert idx.grouped_query(q[:2], n_groups=3)["groups"] == [[], []]


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
def test_degenerate_shapes_equal_query(dev, dt):
    d = 384
    rows, names, centre = document_rows(d, seed=91)
    q = make_queries(rows, centre, seed=92)
    idx = build_index(dev, rows, names, TORCH_DT[dt])
    one = idx.grouped_query(q, n_groups=1, group_size=1)
    plain = idx.query(q, n_results=1)
    assert [[g["ids"] for g in groups] for groups in one["groups"]] == [[ids] for ids in plain["ids"]]
    assert all(abs(groups[0]["distances"][0] - dist[0]) <= TOL for groups, dist in zip(one["groups"], plain["distances"]))
    # every row its own document, S = 1: query(n_results=G) in order
    own = build_index(dev, rows, [f"own{i}" for i in range(len(rows))], TORCH_DT[dt])
    for G in (5, 20):
        res = own.grouped_query(q, n_groups=G, group_size=1)
        plain = own.query(q, n_results=G)
        assert [[g["ids"][0] for g in groups] for groups in res["groups"]] == plain["ids"]
        assert all(abs(g["distances"][0] - x) <= TOL for groups, dist in zip(res["groups"], plain["distances"])
                   for g, x in zip(groups, dist))
        assert [[g["documents"][0] for g in groups] for groups in res["groups"]] == plain["documents"]


def test_f8_collection_with_a_rescore_plane(dev):
    d = 384
    rows, names, centre = document_rows(d, seed=101)
    q = make_queries(rows, centre, seed=102, n_planted=0)
    idx = build_index(dev, rows, names, torch.float8_e4m3fn, rescore_dtype=torch.float16)
    G, S, C = 3, 2, 64
    res = idx.grouped_query(q, n_groups=G, group_size=S, fetch_k=C)
    gor, values = host_column(idx)
    s, r = (t.cpu().numpy() for t in idx.search(q, C))                     # the collection's own re-scored hits
    plain = idx.query(q, n_results=C)
    for b in range(len(q)):
        want = R.select_padded(s[b], r[b], gor, idx.rows_in_use, G, S)
        assert [(g["key"], g["ids"]) for g in res["groups"][b]] == structure(idx, want, values)
        dist_of = dict(zip(plain["ids"][b], plain["distances"][b]))
        assert all(g["distances"][j] == dist_of[i] for g in res["groups"][b] for j, i in enumerate(g["ids"]))
    # capacity mode: allowed, the scores are the quantised collection's own
    lean = build_index(dev, rows, names, torch.float8_e4m3fn, rescore_dtype=None)
    res = lean.grouped_query(q, n_groups=G, group_size=S, fetch_k=C)
    s, r = (t.cpu().numpy() for t in lean.search(q, C))
    gor, values = host_column(lean)
    for b in range(len(q)):
        want = R.select_padded(s[b], r[b], gor, lean.rows_in_use, G, S)
        assert [(g["key"], g["ids"]) for g in res["groups"][b]] == structure(lean, want, values)


# ---------------------------------------------------------------- 3. end to end
def test_through_embedding_manager(dev):
    from multimodal_rag_amd.embedder import EmbeddingManager

    m = EmbeddingManager()
    asyncio.run(m.initialize())
    assert m.supports_grouping()
    words = ["học", "máy", "dữ", "liệu", "gpu", "kernel", "bảng", "ảnh", "văn", "bản", "mô", "hình"]
    g = np.random.default_rng(61)
    for doc, count in (("long", 120), ("mid", 30), ("short", 4), ("tiny", 1)):
        texts = [" ".join(g.choice(words, int(g.integers(3, 9)))) for _ in range(count)]
        items = [{"id": f"{doc}_{i}", "type": "text", "summary": t} for i, t in enumerate(texts)]
        asyncio.run(m.embed_and_store(items, doc))
    queries = ["học máy dữ liệu", "gpu kernel", "bảng và ảnh"]
    before = m.stats["total_queries"]
    out = asyncio.run(m.grouped_query(queries[0], n_groups=3, group_size=2))
    assert m.stats["total_queries"] == before + 1
    assert set(out) == {"ids", "distances", "metadatas", "documents", "groups", "exhaustive", "fetch_k"}
    vec = np.asarray(asyncio.run(m.embed_texts_batch(queries)), np.float32)
    res = m.collection.grouped_query(vec, n_groups=3, group_size=2)
    assert out["groups"] == res["groups"][0] and out["fetch_k"] == res["fetch_k"][0]
    assert out["ids"] == [i for grp in out["groups"] for i in grp["ids"]]
    assert len({grp["key"] for grp in out["groups"]}) == len(out["groups"]) == 3
    assert all(meta["doc_id"] == grp["key"] for grp in out["groups"] for meta in grp["metadatas"])
    many = asyncio.run(m.batch_grouped_query(queries + [" "], n_groups=3, group_size=2))
    assert m.stats["total_queries"] == before + 1 + 3
    for b in range(3):
        assert many[b]["groups"] == res["groups"][b] and many[b]["exhaustive"] == res["exhaustive"][b]
    assert many[3]["error"] == "Query text cannot be empty" and many[3]["groups"] == []
    with pytest.raises(ValueError):
        asyncio.run(m.grouped_query("  "))
    asyncio.run(m.cleanup())


def test_query_endpoint_group_by_document(dev):
    from fastapi.testclient import TestClient

    from multimodal_rag_amd.server import create_app

    with TestClient(create_app()) as c:
        bodies = [" ".join(f"Học máy là gì, phần {i}." for i in range(60)), "GPU kernel và dữ liệu. " * 3,
                  "Machine learning cơ bản, học máy. " * 3, "Bảng và ảnh. " * 3]
        uploaded = []
        for i, body in enumerate(bodies):
            r = c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
            uploaded.append(r.json()["doc_id"])
        plain = c.post("/query", json={"query": "học máy", "top_k": 3})
        assert plain.status_code == 200
        assert all("document" not in s and "document_rank" not in s for s in plain.json()["sources"])
        r = c.post("/query", json={"query": "học máy", "top_k": 3, "group_by_document": True})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert [s["document_rank"] for s in src] == [1, 2, 3] and len({s["document"] for s in src}) == 3
        assert {s["document"] for s in src} <= set(uploaded)
        assert src[0]["doc_id"] == plain.json()["sources"][0]["doc_id"]
        r = c.post("/query", json={"query": "học máy", "top_k": 2, "group_by_document": True, "per_document": 2})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        ranks = [s["document_rank"] for s in src]
        assert ranks == sorted(ranks) and set(ranks) == {1, 2} and 2 <= len(src) <= 4
        assert len({(s["document_rank"], s["document"]) for s in src}) == 2
        for other in ("mmr", "hybrid", "rerank"):
            assert c.post("/query", json={"query": "học máy", "group_by_document": True, other: True}).status_code == 400
