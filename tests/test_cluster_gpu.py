"""GPU: topic clustering (csrc/kmeans.hip through _native.kmeans_assign / cluster_sums, VectorIndex.cluster and
EmbeddingManager.cluster_topics) against tests/cluster_ref.py.

Assignments are compared through the band of cluster_ref: every score within TOL of the float64 dot of the stored rows;
a row whose float64 margin is at least BAND must get the reference's centroid; a row inside the band may get any
centroid whose float64 score is within BAND of the best; the share of band rows is capped on the reference alone."""
import asyncio
import functools

import numpy as np
import pytest
import torch

from tests import cluster_ref as R

pytestmark = pytest.mark.gpu

NK = ((0, 1), (1, 1), (127, 2), (128, 127), (129, 128), (513, 129), (1025, 300))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return "cuda:0"


def pack(dev, x, dtype, rows=None):
    """float32 [n, d] -> the stored layout [max(rows or n, 1), ld], zero pad columns"""
    from multimodal_rag_amd import _native

    n, d = x.shape
    out = torch.zeros((max(rows or n, 1), _native.padded_dim(d, R.TORCH_DT[dtype])), dtype=R.TORCH_DT[dtype], device=dev)
    if n:
        out[:n, :d] = torch.from_numpy(x).to(dev).to(R.TORCH_DT[dtype])
    return out


def bitmap(dev, flags):
    words = np.zeros((len(flags) + 31) // 32 + 8, np.uint32)
    idx = np.nonzero(np.asarray(flags, bool))[0]
    np.bitwise_or.at(words, idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    return torch.from_numpy(words.view(np.int32)).to(dev)


def run_assign(dev, x, c, dtype, alive=None, n=None):
    from multimodal_rag_amd import _native

    n = len(x) if n is None else n
    a, s = _native.kmeans_assign(pack(dev, x, dtype), n, x.shape[1], pack(dev, c, dtype),
                                 alive=None if alive is None else bitmap(dev, alive))
    assert a.shape == (n,) and s.shape == (n,) and a.dtype == torch.int32 and s.dtype == torch.float32
    return a.cpu().numpy(), s.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(n, k, d, dtype):
    """(rows, centroids: float32 rounded to dtype; the same as stored float64; the reference's (arg, best, margin)).
    The seed is the first of a fixed sequence whose band share stays under the cap -- decided on the reference alone;
    the cap is asserted again where the data is used."""
    for seed in range(1000 * d + n + k, 1000 * d + n + k + 200):
        x = R.unit_rows(n, d, seed, dtype)
        c = R.centroids_of(x, k, seed, dtype) if n >= k else R.unit_rows(k, d, seed + 1, dtype)
        x64, c64 = R.stored(x, dtype), R.stored(c, dtype)
        ref = R.assign(x64, c64)
        if R.band_share(ref[2]) <= R.MAX_BAND_SHARE:
            return x, c, x64, c64, ref
    raise AssertionError(f"no seed keeps the band share under the cap for n={n} k={k} d={d} {dtype}")


def check_assign(got_a, got_s, x64, c64, ref, alive, what):
    """the band comparison of the module docstring, on the alive rows; dead rows hold (-1, -inf)"""
    arg, best, margin = ref
    n, k = len(x64), len(c64)
    live = np.ones(n, bool) if alive is None else np.asarray(alive, bool)
    assert R.band_share(margin, live) <= R.MAX_BAND_SHARE, what
    assert np.all(got_a[~live] == -1) and np.all(np.isneginf(got_s[~live])), what
    if not live.any():
        return
    print(what, "live", int(live.sum()), "max |score - float64|", float(np.abs(got_s[live] - best[live]).max()),
          "band rows", int((margin[live] < R.BAND).sum()))
    assert np.all(np.abs(got_s[live] - best[live]) <= R.TOL), what
    assert np.all((got_a[live] >= 0) & (got_a[live] < k)), what
    strict = live & (margin >= R.BAND)
    assert np.array_equal(got_a[strict], arg[strict]), (what, np.nonzero(strict & (got_a != arg))[0][:8])
    loose = np.nonzero(live & (margin < R.BAND))[0]
    s = x64[loose] @ c64.T
    assert np.all(s[np.arange(len(loose)), got_a[loose]] >= best[loose] - R.BAND), what


# ---------------------------------------------------------------- 1. kmeans_assign against the reference
@pytest.mark.parametrize("dtype,d", [(t, d) for t in ("fp16", "bf16", "fp32") for d in (8, 64, 72, 384)]
                         + [("fp32", 32), ("fp16", 768)])
def test_assign_against_reference(dev, dtype, d):
    for n, k in NK:
        x, c, x64, c64, ref = case(n, k, d, dtype)
        got_a, got_s = run_assign(dev, x, c, dtype)
        check_assign(got_a, got_s, x64, c64, ref, None, (dtype, d, n, k))


# ---------------------------------------------------------------- 2. ties, padding and the bitmap
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_ties_go_to_the_lower_index(dev, dtype):
    d, k = 64, 256
    c = R.unit_rows(k, d, 41, dtype)
    c[200], c[128] = c[3], c[127]                  # twins: (3, 200), and (127, 128) across the tile edge
    g = np.random.default_rng(42)
    want = np.repeat([3, 127, 200, 128, 5, 250], 50)[g.permutation(300)]          # the centroid each row is built around
    x = c[want].astype(np.float64) + 0.02 * g.standard_normal((300, d))
    x = R.stored(x / np.linalg.norm(x, axis=1, keepdims=True), dtype).astype(np.float32)
    x64, c64 = R.stored(x, dtype), R.stored(c, dtype)
    s = x64 @ c64.T
    lower = np.where(want == 200, 3, np.where(want == 128, 127, want))
    others = s.copy()
    for a, b in ((3, 200), (127, 128)):
        others[(lower == a)[:, None] & np.isin(np.arange(k), (a, b))[None, :]] = -np.inf
    others[np.arange(300), lower] = -np.inf
    assert np.all(s[np.arange(300), lower] - others.max(axis=1) >= R.BAND)         # on the reference: nothing else is near
    assert np.array_equal(R.assign(x64, c64)[0], lower)                             # the reference's rule: the lowest
    got_a, got_s = run_assign(dev, x, c, dtype)
    assert np.array_equal(got_a, lower), np.nonzero(got_a != lower)[0][:8]
    assert np.all(np.abs(got_s - s[np.arange(300), lower]) <= R.TOL)


@pytest.mark.parametrize("k", [129, 1])
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_all_negative_rows_never_pick_a_padded_centroid(dev, dtype, k):
    d, n = 64, 300
    for seed in range(500, 700):
        g = np.random.default_rng(seed)
        e = np.zeros(d)
        e[0] = 1.0
        c = e + 0.06 * g.standard_normal((k, d))                                   # centroids in one cone: cosines > 0
        c = R.stored(c / np.linalg.norm(c, axis=1, keepdims=True), dtype).astype(np.float32)
        x = -c[g.integers(0, k, n)].astype(np.float64) + 0.03 * g.standard_normal((n, d))
        x = R.stored(x / np.linalg.norm(x, axis=1, keepdims=True), dtype).astype(np.float32)
        x64, c64 = R.stored(x, dtype), R.stored(c, dtype)
        ref = R.assign(x64, c64)
        if R.band_share(ref[2]) <= R.MAX_BAND_SHARE:
            break
    else:
        raise AssertionError("no seed keeps the band share under the cap")
    assert (x64 @ c64.T).max() < -0.1                       # every score negative: a zero (padded) column would win
    got_a, got_s = run_assign(dev, x, c, dtype)
    check_assign(got_a, got_s, x64, c64, ref, None, ("negative", dtype, k))
    assert np.all(got_s < 0)


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
def test_bitmap_and_position_independence(dev, dtype):
    n, k, d = 513, 129, 64
    x, c, x64, c64, ref = case(n, k, d, dtype)
    g = np.random.default_rng(9)
    alive = g.random(n) > 0.3
    alive[128:256] = False                                   # one whole tile of dead rows
    full_a, full_s = run_assign(dev, x, c, dtype)
    got_a, got_s = run_assign(dev, x, c, dtype, alive=alive)
    masked = R.assign(x64, c64, alive)
    check_assign(got_a, got_s, x64, c64, masked, alive, ("bitmap", dtype))
    assert np.array_equal(got_a[alive], full_a[alive]) and got_s[alive].tobytes() == full_s[alive].tobytes()
    ones_a, ones_s = run_assign(dev, x, c, dtype, alive=np.ones(n, bool))
    assert np.array_equal(ones_a, full_a) and ones_s.tobytes() == full_s.tobytes()
    # the same rows at other positions of a larger n (another grid, other tiles, other lanes)
    big_n = 1200
    at = np.sort(g.choice(big_n, n, replace=False))[g.permutation(n)]
    big = R.unit_rows(big_n, d, 77, dtype)
    big[at] = x
    big_a, big_s = run_assign(dev, big, c, dtype)
    assert np.array_equal(big_a[at], full_a) and big_s[at].tobytes() == full_s.tobytes()
    part_a, part_s = run_assign(dev, x, c, dtype, n=300)     # a prefix: another n
    assert np.array_equal(part_a, full_a[:300]) and part_s.tobytes() == full_s[:300].tobytes()


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
def test_assign_and_join_scores_are_the_same_bits(dev, dtype):
    """The assign kernel and the similarity join run one tile body (csrc/pair_tile.h): a pair of rows has the same score
    bits in both.  The first k rows are the centroids; ragged last tiles in both dimensions, a padded last K-slab."""
    from multimodal_rag_amd import _native

    n, d, k = 300, 72, 130
    x = np.abs(np.random.default_rng(130).standard_normal((n, d)))     # every dot product is positive
    x = R.stored(x / np.linalg.norm(x, axis=1, keepdims=True), dtype).astype(np.float32)
    rows = pack(dev, x, dtype)
    pairs, scores, total = _native.sim_join(rows, n, d, 1e-6, capacity=1 << 16)
    assert total == n * (n - 1) // 2 == 44850 and len(scores) == total        # nothing is left out
    pairs, scores = pairs.cpu().numpy(), scores.cpu().numpy()
    join = np.full((n, n), -np.inf, np.float32)
    join[pairs[:, 0], pairs[:, 1]] = scores                                    # join[j, i], j < i
    got_a, got_s = _native.kmeans_assign(rows, n, d, rows[:k])
    got_a, got_s = got_a.cpu().numpy(), got_s.cpu().numpy()
    want = join[:k, k:]                                                        # centroid j < k against row i >= k
    assert np.array_equal(got_s[k:].view(np.int32), want.max(axis=0).view(np.int32))
    assert np.array_equal(got_a[k:], want.argmax(axis=0))                      # argmax: the lowest j at the maximum


# ---------------------------------------------------------------- 3. cluster_sums
SEGMENTS = (0, 1, 255, 256, 257, 1025, 0, 37)


def run_sums(dev, rows, d, members):
    """members: one ascending row array per cluster"""
    from multimodal_rag_amd import _native

    order = torch.from_numpy(np.concatenate(members).astype(np.int32)).to(dev)
    seg = torch.from_numpy(np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)).to(dev)
    out = _native.cluster_sums(rows, d, order, seg, len(members))
    assert out.shape == (len(members), d) and out.dtype == torch.float32
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype,d", [(t, d) for t in ("fp16", "bf16", "fp32") for d in (8, 72, 384)])
def test_cluster_sums(dev, dtype, d):
    n = 2000
    x = R.unit_rows(n, d, 300 + d, dtype)
    x64 = R.stored(x, dtype)
    rows = pack(dev, x, dtype)
    g = np.random.default_rng(d)
    perm = g.permutation(n)
    members, at = [], 0
    for length in SEGMENTS:
        members.append(np.sort(perm[at: at + length]))
        at += length
    got = run_sums(dev, rows, d, members)
    for c, m in enumerate(members):
        want = x64[m].sum(axis=0)
        bound = 2.0 * max(len(m) - 1, 0) * 2.0 ** -24 * np.abs(x64[m]).sum(axis=0)
        assert np.all(np.abs(got[c] - want) <= bound), (dtype, d, c, len(m), float(np.abs(got[c] - want).max()))
    assert np.all(got[0] == 0) and np.all(got[6] == 0)                   # empty segments: written, zero
    assert np.array_equal(got[1], x[members[1][0]])                      # one member: the row itself
    assert run_sums(dev, rows, d, members).tobytes() == got.tobytes()    # a second call: identical bits
    # cluster 5 keeps its bits when the others lose members, move, or go away
    other = [members[5], members[4][::-1].copy(), members[2][:100]]
    again = run_sums(dev, rows, d, other)
    assert again[0].tobytes() == got[5].tobytes()
    alone = run_sums(dev, rows, d, [members[5]])
    assert alone[0].tobytes() == got[5].tobytes()


# ---------------------------------------------------------------- 4. VectorIndex.cluster
def build_index(dev, x, kind="fp16", doc=lambda i: "a", **kw):
    from multimodal_rag_amd.index import VectorIndex

    n, d = x.shape
    if kind == "f8+fp16":
        kw = dict(dtype=torch.float8_e4m3fn, rescore_dtype=torch.float16, **kw)
    else:
        kw = dict(dtype=R.TORCH_DT[kind], **kw)
    idx = VectorIndex(dim=d, device=dev, capacity=n, **kw)
    idx.add(x, documents=[f"text {i}" for i in range(n)], metadatas=[{"doc_id": doc(i)} for i in range(n)],
            ids=[f"id{i}" for i in range(n)])
    assert idx.count() == n
    return idx


def row_dtype(kind):
    return "fp16" if kind == "f8+fp16" else kind


@functools.lru_cache(maxsize=None)
def blob_case(dtype, init_rows, twin=None, min_cos=0.95, min_iterations=2):
    """(rows, blob of each row, the reference's run from init_rows): 8 blobs x 60 rows, d = 64, members at cosine
    >= min_cos to their centre.  `twin` = (i, j): row j is made a copy of row i.  The seed is the first of a fixed
    sequence for which the reference's run converges in at least min_iterations iterations and keeps every margin and
    every re-seed gap at or above BAND -- decided on the reference alone, asserted again at the use."""
    for seed in range(20, 120):
        x, owner, _ = R.blobs(8, 60, 64, seed, dtype, min_cos=min_cos)
        if twin:
            x[twin[1]] = x[twin[0]]
        ref = R.lloyd(x, dtype, list(init_rows))
        if (ref["min_margin"] >= R.BAND and ref["min_reseed_gap"] >= R.BAND and ref["converged"]
                and ref["iterations"] >= min_iterations):
            return x, owner, ref
    raise AssertionError("no seed keeps the reference's margins at or above the band")


ONE_PER_BLOB = tuple(b * 60 + 7 for b in range(8))
TWO_IN_ONE = (0, 1) + tuple(b * 60 for b in range(1, 7))        # two seeds in blob 0, none in blob 7
TWIN_SEEDS = (0, 60, 61) + tuple(b * 60 for b in range(2, 7))   # rows 60 and 61 identical: cluster 2 starts empty


def labels_of(rep, n):
    return np.array([rep["labels"].get(f"id{r}", -1) for r in range(n)])


@pytest.mark.parametrize("kind", ["fp16", "fp32", "f8+fp16"])
def test_cluster_recovers_planted_blobs(dev, kind):
    dtype = row_dtype(kind)
    x, owner, ref = blob_case(dtype, ONE_PER_BLOB)
    assert ref["min_margin"] >= R.BAND and ref["converged"]
    n = len(x)
    idx = build_index(dev, x, kind, doc=lambda i: f"blob{i // 60}")
    rep = idx.cluster(init=[f"id{r}" for r in ONE_PER_BLOB], return_labels=True)
    assert set(rep) == {"n_clusters", "iterations", "converged", "objective", "clusters", "centroids", "labels"}
    assert rep["n_clusters"] == 8 and rep["converged"] is True and rep["iterations"] == ref["iterations"] == 2
    assert np.array_equal(labels_of(rep, n), owner)
    assert [c["size"] for c in rep["clusters"]] == [60] * 8 and [c["cluster"] for c in rep["clusters"]] == list(range(8))
    cent = rep["centroids"]
    assert cent.shape == (8, 64) and cent.dtype == torch.float32 and cent.is_cuda
    x64, c64 = R.stored(x, dtype), R.stored(cent.cpu().numpy(), dtype)
    assert np.abs(np.linalg.norm(cent.cpu().numpy().astype(np.float64), axis=1) - 1).max() <= 1e-5
    assert len(rep["objective"]) == 2 and abs(rep["objective"][-1] - ref["objective"][-1]) <= R.TOL
    for c in rep["clusters"]:
        b = c["cluster"]
        assert set(c) == {"cluster", "size", "cohesion", "representatives", "documents"}
        assert c["documents"] == [(f"blob{b}", 60)]
        cos = x64[owner == b] @ c64[b]
        assert abs(c["cohesion"] - cos.mean()) <= R.TOL
        hits = c["representatives"]
        assert len(hits) == 3 and all(owner[int(i[2:])] == b for i, _ in hits)
        assert all(abs(s - x64[int(i[2:])] @ c64[b]) <= R.TOL for i, s in hits)
        assert [s for _, s in hits] == sorted((s for _, s in hits), reverse=True)
        assert min(s for _, s in hits) >= np.sort(cos)[-3] - R.BAND           # nothing better was left out
    assert "labels" not in idx.cluster(init=[f"id{r}" for r in ONE_PER_BLOB])
    assert len(idx.cluster(n_clusters=8, representatives=1)["clusters"][0]["representatives"]) == 1


@pytest.mark.parametrize("dtype,init_rows,twin", [("fp16", TWO_IN_ONE, None), ("fp32", TWO_IN_ONE, None),
                                                  ("fp16", TWIN_SEEDS, (60, 61))])
def test_cluster_follows_the_reference_step_by_step(dev, dtype, init_rows, twin):
    """Two seeds inside one blob (the update step, the re-normalisation and the stop rule), and two identical seed rows
    (an empty cluster, re-seeded from the row with the lowest score): the labels of every assign equal cluster_ref.lloyd's.
    cluster(max_iter=t) ends with the assign that follows t updates, which is the reference's assign number t + 1."""
    x, owner, ref = blob_case(dtype, init_rows, twin, min_cos=0.75, min_iterations=4)     # wide blobs: rows do move
    assert ref["min_margin"] >= R.BAND and ref["min_reseed_gap"] >= R.BAND
    assert ref["converged"] and 4 <= ref["iterations"] <= 25
    if twin:
        assert not np.any(ref["labels"][0] == 2) and ref["min_reseed_gap"] != np.inf     # the re-seed did happen
    n = len(x)
    idx = build_index(dev, x, dtype)
    init = [f"id{r}" for r in init_rows]
    for t in range(1, ref["iterations"]):
        rep = idx.cluster(init=init, max_iter=t, return_labels=True)
        assert rep["iterations"] == t and rep["converged"] is False and len(rep["objective"]) == t + 1
        assert np.array_equal(labels_of(rep, n), ref["labels"][t]), (t, int((labels_of(rep, n) != ref["labels"][t]).sum()))
    rep = idx.cluster(init=init, return_labels=True)
    assert rep["iterations"] == ref["iterations"] and rep["converged"] is True
    assert np.array_equal(labels_of(rep, n), ref["labels"][-1])
    obj = rep["objective"]
    print("objective", obj)
    assert len(obj) == len(ref["objective"]) and all(abs(a - b) <= R.TOL for a, b in zip(obj, ref["objective"]))
    assert all(b >= a - R.TOL for a, b in zip(obj, obj[1:]))                              # non-decreasing within TOL
    assert np.abs(rep["centroids"].cpu().numpy() - ref["centroids"]).max() <= 1e-5
    sizes = np.bincount(ref["labels"][-1], minlength=8)
    assert [(c["cluster"], c["size"]) for c in rep["clusters"]] == sorted(enumerate(sizes.tolist()), key=lambda cs: (-cs[1], cs[0]))


def test_cluster_where_labels_seed_and_refusals(dev, monkeypatch):
    from multimodal_rag_amd import config

    x, owner, _ = blob_case("fp16", ONE_PER_BLOB)
    n = len(x)
    idx = build_index(dev, x, "fp16", doc=lambda i: "even" if (i // 60) % 2 == 0 else "odd")
    idx.delete(ids=["id3", "id64", "id130"])
    even = [r for r in range(n) if (r // 60) % 2 == 0 and r not in (3, 130)]
    rep = idx.cluster(n_clusters=4, where={"doc_id": "even"}, seed=5, return_labels=True)
    assert set(rep["labels"]) == {f"id{r}" for r in even}                        # exactly the live matching ids
    assert sum(c["size"] for c in rep["clusters"]) == len(even)
    assert all(v == "even" for c in rep["clusters"] for v, _ in c["documents"])
    again = idx.cluster(n_clusters=4, where={"doc_id": "even"}, seed=5, return_labels=True)
    assert torch.equal(again.pop("centroids"), rep.pop("centroids")) and again == rep     # reproducible from the seed
    whole = idx.cluster(n_clusters=8, seed=1, return_labels=True)
    assert set(whole["labels"]) == {f"id{r}" for r in range(n) if r not in (3, 64, 130)}
    assert all(b >= a - R.TOL for a, b in zip(whole["objective"], whole["objective"][1:]))
    # the default k: MMRAG_TOPICS, whose 0 is the automatic rule, capped at the live rows
    monkeypatch.setattr(config.settings, "MMRAG_TOPICS", 0)
    assert idx.cluster()["n_clusters"] == config.auto_topics(n - 3) == 15
    monkeypatch.setattr(config.settings, "MMRAG_TOPICS", 5)
    assert idx.cluster()["n_clusters"] == 5
    tiny = idx.cluster(where={"doc_id": {"$in": ["none"]}})
    assert tiny["n_clusters"] == 0 and tiny["clusters"] == [] and tiny["objective"] == [] and tiny["centroids"].shape == (0, 64)
    idx.delete(ids=[f"id{r}" for r in range(4, n)])
    assert idx.count() == 3                                                       # id0, id1, id2
    assert idx.cluster()["n_clusters"] == 3                                       # 5 topics asked by default: capped
    for bad in (dict(n_clusters=4), dict(n_clusters=0), dict(n_clusters=4097), dict(init=["id0", "id0"]),
                dict(init=["id0", "id3"]), dict(init=["id0", "nothing"]), dict(n_clusters=3, init=["id0", "id1"]),
                dict(max_iter=0), dict(tol=-1.0)):
        with pytest.raises(ValueError):
            idx.cluster(**bad)
    one = idx.cluster(n_clusters=1, return_labels=True)
    assert one["labels"] == {"id0": 0, "id1": 0, "id2": 0} and one["clusters"][0]["size"] == 3


def test_capacity_mode_is_refused(dev):
    x, _, _ = blob_case("fp16", ONE_PER_BLOB)
    from multimodal_rag_amd.index import VectorIndex

    lean = VectorIndex(dim=64, dtype=torch.float8_e4m3fn, device=dev, rescore_dtype=None)     # MMRAG_F8_RESCORE=none
    lean.add(x[:100], ids=[f"id{i}" for i in range(100)])
    with pytest.raises(ValueError, match="needs full-precision rows"):
        lean.cluster(n_clusters=4)


# ---------------------------------------------------------------- 5. end to end
def test_through_embedding_manager(dev, monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd.embedder import EmbeddingManager

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    words = ["học", "máy", "dữ", "liệu", "gpu", "kernel", "bảng", "ảnh", "văn", "bản", "mô", "hình", "sông", "núi",
             "trời", "biển", "sách", "bút", "đường", "phố"]
    g = np.random.default_rng(62)
    texts = sorted({" ".join(g.choice(words, int(g.integers(2, 25)))) for _ in range(60)})
    m = EmbeddingManager()
    asyncio.run(m.initialize())
    assert m.supports_clustering()
    docs = {"docA": texts[:20], "docB": texts[20:40], "docC": texts[40:]}
    for doc_id, part in docs.items():
        items = [{"id": f"item{i}", "type": "text", "summary": t} for i, t in enumerate(part)]
        assert asyncio.run(m.embed_and_store(items, doc_id))["text"] == len(part)

    def check(rep, total, doc_ids):
        assert set(rep) == {"n_clusters", "iterations", "converged", "objective", "clusters"}      # no tensor
        assert rep["n_clusters"] == 4 == len(rep["clusters"]) and sum(c["size"] for c in rep["clusters"]) == total
        for c in rep["clusters"]:
            assert c["size"] >= 1 and 1 <= len(c["representatives"]) <= 2
            for hit in c["representatives"]:
                assert set(hit) == {"id", "score", "document", "metadata"}
                doc = hit["metadata"]["doc_id"]
                assert doc in doc_ids and hit["id"].startswith(doc + "_") and hit["document"] in docs[doc]
                assert -1.0 <= hit["score"] <= 1.0 + R.TOL
            assert {v for v, _ in c["documents"]} <= set(doc_ids)
            assert sum(n for _, n in c["documents"]) == c["size"]

    check(asyncio.run(m.cluster_topics(n_topics=4, representatives=2)), len(texts), ("docA", "docB", "docC"))
    only = asyncio.run(m.cluster_topics(n_topics=2, doc_id="docB"))
    assert sum(c["size"] for c in only["clusters"]) == 20
    with pytest.raises(ValueError):
        asyncio.run(m.cluster_topics(n_topics=len(texts) + 1))
    asyncio.run(m.delete_document("docA"))
    check(asyncio.run(m.cluster_topics(n_topics=4, representatives=2)), len(texts) - 20, ("docB", "docC"))
    asyncio.run(m.cleanup())
