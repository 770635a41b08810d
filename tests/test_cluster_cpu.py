"""CPU: topic clustering without a device -- the numpy reference against plain loops, its Lloyd loop on planted blobs,
the MMRAG_TOPICS setting, the library's argument checks through ctypes, GET /topics over a fake collection, and the
kernels' resources as compiled for gfx950."""
import ctypes
import re

import numpy as np
import pytest
from starlette.testclient import TestClient

from tests import asm_util
from tests import cluster_ref as R
from tests.fakes import FakeCollection, FakeEngine


# ---------------------------------------------------------------- 1. the reference itself
def test_reference_assign_against_loops():
    g = np.random.default_rng(3)
    for n, k, d in ((1, 1, 4), (5, 1, 3), (37, 2, 3), (64, 9, 2), (50, 17, 8)):
        x = g.standard_normal((n, d))
        c = g.standard_normal((k, d))
        alive = g.random(n) > 0.3
        for mask in (None, alive):
            arg, best, margin = R.assign(x, c, mask)
            for r in range(n):
                if mask is not None and not mask[r]:
                    assert arg[r] == -1 and best[r] == -np.inf and margin[r] == np.inf
                    continue
                scores = [float(np.dot(x[r], c[j])) for j in range(k)]
                top = max(scores)
                assert arg[r] == scores.index(top) and abs(best[r] - top) < 1e-12
                rest = scores[: arg[r]] + scores[arg[r] + 1:]
                assert margin[r] == np.inf if k == 1 else abs(margin[r] - (top - max(rest))) < 1e-12


def test_reference_tie_rule_and_margin():
    c = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0]])
    x = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, -1.0], [0.6, 0.8]])
    arg, best, margin = R.assign(x, c)
    assert arg.tolist() == [0, 1, 0, 1]                       # twins: the lower index; all equal: the lowest
    assert best.tolist() == [1.0, 1.0, -1.0, 0.8] and margin.tolist()[:3] == [0.0, 0.0, 0.0]
    assert abs(margin[3]) < 1e-12                             # its twin ties it; R.BAND is what tells such rows apart
    assert R.BAND == 2 * R.TOL == 2e-4 and R.MAX_BAND_SHARE == 0.05
    assert R.band_share(np.array([0.0, 1e-4, 2e-4, 1.0])) == 0.5
    assert R.assign(np.zeros((0, 2)), c)[0].shape == (0,)


def test_reference_sums_against_loops():
    g = np.random.default_rng(4)
    x = g.standard_normal((40, 5))
    labels = g.integers(-1, 6, 40)
    labels[labels == 3] = 2                                   # cluster 3 stays empty
    got = R.sums(x, labels, 6)
    for c in range(6):
        want = np.zeros(5)
        for r in range(40):
            if labels[r] == c:
                want += x[r]
        assert np.allclose(got[c], want, atol=1e-12)
    assert np.all(got[3] == 0)


def test_lloyd_recovers_planted_blobs():
    for dtype in ("fp16", "fp32"):
        x, owner, centres = R.blobs(8, 60, 64, 5, dtype)
        x64 = R.stored(x, dtype)
        assert np.all(np.einsum("ij,ij->i", x64, centres[owner]) >= 0.95)
        assert np.abs(centres @ centres.T - np.eye(8)).max() <= 0.3
        run = R.lloyd(x, dtype, [b * 60 + 7 for b in range(8)])
        assert run["converged"] and run["iterations"] == 2 and len(run["labels"]) == 2
        assert np.array_equal(run["labels"][-1], owner)
        assert run["min_margin"] >= R.BAND and run["min_reseed_gap"] == np.inf
        assert abs(np.linalg.norm(run["centroids"], axis=1) - 1).max() < 1e-12
        # two seeds inside blob 0, none in blob 7: still a partition into 8, and the objective never falls
        bad = R.lloyd(x, dtype, [0, 1] + [b * 60 for b in range(1, 7)])
        obj = bad["objective"]
        assert all(b >= a - 1e-12 for a, b in zip(obj, obj[1:])), obj
        assert len(obj) == len(bad["labels"]) and bad["iterations"] >= 2
        assert sorted(np.unique(bad["labels"][-1])) == list(range(8))
        dead = np.ones(len(x), bool)
        dead[60:120] = False                                   # blob 1 is dead: its seed must not be used
        part = R.lloyd(x, dtype, [b * 60 for b in range(8) if b != 1], alive=dead)
        assert np.all(part["labels"][-1][60:120] == -1) and part["converged"]
        assert np.array_equal(part["labels"][-1][dead], np.where(owner > 1, owner - 1, owner)[dead])


def test_lloyd_reseeds_an_empty_cluster():
    x, owner, _ = R.blobs(4, 30, 32, 9, "fp32")
    x[31] = x[30]                                              # two identical seeds: the higher index gets no row
    run = R.lloyd(x, "fp32", [0, 30, 31, 60])
    first = run["labels"][0]
    assert not np.any(first == 2) and np.all(first[30:60] == 1)
    assert run["min_reseed_gap"] > 0 and run["min_reseed_gap"] != np.inf
    # the re-seed took the row with the lowest score: a row of blob 3, which no seed covers
    final = run["labels"][-1]
    assert len(np.unique(final)) == 4 and len(np.unique(final[90:])) == 1 and final[90] == 2


# ---------------------------------------------------------------- 2. settings
def test_settings_topics(monkeypatch):
    from multimodal_rag_amd.config import Settings, auto_topics

    monkeypatch.delenv("MMRAG_TOPICS", raising=False)
    assert Settings().MMRAG_TOPICS == 0 and Settings().topics() == 0
    for good in ("1", "12", "4096"):
        monkeypatch.setenv("MMRAG_TOPICS", good)
        assert Settings().topics() == int(good)
    for bad in ("-1", "4097"):
        monkeypatch.setenv("MMRAG_TOPICS", bad)
        with pytest.raises(ValueError, match="MMRAG_TOPICS"):
            Settings()
    monkeypatch.setenv("MMRAG_TOPICS", "many")
    with pytest.raises(ValueError):
        Settings()
    # min(256, max(2, round(sqrt(live / 2)))), halves rounded up
    assert [auto_topics(v) for v in (0, 1, 8, 9, 12, 13, 200, 5000, 131072, 10 ** 6)] == [2, 2, 2, 2, 2, 3, 10, 50, 256, 256]


# ---------------------------------------------------------------- 3. the library's argument checks
def test_argument_checks_need_no_device():
    from multimodal_rag_amd import _native

    L = _native.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)       # never dereferenced: every call below returns before anything is launched
    EINVAL, EUNSUPPORTED = 1, 4

    def assign(rows=p, n=100, ld=64, dtype=_native.F16, d=64, cent=p, k=8, alive=None, out_a=p, out_s=p):
        return L.mmrag_kmeans_assign(rows, n, ld, dtype, d, cent, k, alive, out_a, out_s, None)

    def sums(rows=p, ld=64, dtype=_native.F16, d=64, order=p, seg=p, k=8, out=p):
        return L.mmrag_cluster_sums(rows, ld, dtype, d, order, seg, k, out, None)

    assert assign(rows=None) == EINVAL and assign(cent=None) == EINVAL
    assert assign(out_a=None) == EINVAL and assign(out_s=None) == EINVAL
    assert assign(n=-1) == EINVAL and assign(n=1 << 31) == EINVAL
    assert assign(k=0) == EINVAL and assign(k=4097) == EINVAL and assign(k=-2) == EINVAL
    assert assign(d=0) == EINVAL and assign(d=-3) == EINVAL and assign(ld=63) == EINVAL
    assert assign(dtype=7) == EINVAL and assign(dtype=-1) == EINVAL
    assert assign(dtype=_native.F8E4M3, ld=128, d=64) == EUNSUPPORTED
    assert b"re-scoring plane" in L.mmrag_last_error()
    assert assign(n=0) == 0                                    # nothing to do, nothing launched
    assert sums(rows=None) == EINVAL and sums(order=None) == EINVAL and sums(seg=None) == EINVAL
    assert sums(out=None) == EINVAL and sums(k=0) == EINVAL and sums(k=4097) == EINVAL
    assert sums(d=0) == EINVAL and sums(ld=63) == EINVAL and sums(dtype=9) == EINVAL
    assert sums(dtype=_native.F8E4M3, ld=128, d=64) == EUNSUPPORTED
    assert _native.MAX_CLUSTERS == 4096 and L.mmrag_abi_version() == 1


# ---------------------------------------------------------------- 4. embedder + server over a fake collection
class ClusterCollection(FakeCollection):
    """FakeCollection plus VectorIndex.cluster, computed by tests/cluster_ref.py"""

    def cluster(self, n_clusters=None, where=None, max_iter=25, tol=1e-3, seed=0, init=None, representatives=3,
                return_labels=False):
        from multimodal_rag_amd.config import auto_topics, settings
        from multimodal_rag_amd.index import match_where

        alive = np.array([match_where(m, where) for m in self.metas], bool)
        live = int(alive.sum())
        if n_clusters is None:
            k = min(settings.topics() or auto_topics(live), live)
        else:
            k = int(n_clusters)
            if not 1 <= k <= 4096 or (live and k > live):
                raise ValueError(f"cluster: n_clusters={k} is outside what {live} live rows allow")
        if live == 0:
            return {"n_clusters": 0, "iterations": 0, "converged": True, "objective": [], "clusters": [], "centroids": None}
        seeds = np.random.default_rng(seed).choice(np.nonzero(alive)[0], k, replace=False)
        run = R.lloyd(self.vecs, "fp32", seeds, alive, max_iter, tol)
        labels = run["labels"][-1]
        cent = run["centroids"]
        clusters = []
        for c in range(k):
            mine = np.nonzero(labels == c)[0]
            cos = self.vecs[mine].astype(np.float64) @ cent[c]
            best = mine[np.argsort(-cos, kind="stable")][:representatives]
            docs = {}
            for r in mine:
                docs[self.metas[r]["doc_id"]] = docs.get(self.metas[r]["doc_id"], 0) + 1
            clusters.append({"cluster": c, "size": len(mine), "cohesion": float(cos.mean()) if len(mine) else 0.0,
                             "representatives": [(self.ids[r], float(self.vecs[r].astype(np.float64) @ cent[c])) for r in best],
                             "documents": sorted(docs.items(), key=lambda kv: -kv[1])[:5]})
        clusters.sort(key=lambda c: (-c["size"], c["cluster"]))
        return {"n_clusters": k, "iterations": run["iterations"], "converged": run["converged"],
                "objective": run["objective"], "clusters": clusters, "centroids": cent}


class ClusterEngine(FakeEngine):
    def new_collection(self, name, metadata=None):
        c = ClusterCollection(self.dim, name, metadata)
        self.collections.append(c)
        return c


def make_client(engine):
    from multimodal_rag_amd.embedder import EmbeddingManager
    from multimodal_rag_amd.server import create_app

    async def no_sleep(_):
        return None

    manager = EmbeddingManager(engine=engine)
    manager._sleep = no_sleep
    return TestClient(create_app(embedder=manager)), manager


def document(word: str, paragraphs: int) -> bytes:
    return "\n\n".join(f"{word} paragraph number {i} about {word} engines. " * 25 for i in range(paragraphs)).encode()


def upload(client, name, data):
    r = client.post("/upload", files={"file": (name, data, "text/plain")})
    assert r.status_code == 200, r.text
    return r.json()


def test_topics_route(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    monkeypatch.setattr(config.settings, "MMRAG_TOPICS", 0)
    plain, plain_manager = make_client(FakeEngine())
    topical, manager = make_client(ClusterEngine())
    with plain as c0, topical as c1:
        # an embedder whose collection cannot cluster: the 400 that /duplicates gives for an unsupported collection
        upload(c0, "a.txt", document("alpha", 4))
        r, dup = c0.get("/topics"), c0.get("/duplicates")
        assert r.status_code == dup.status_code == 400
        assert "Topic clustering is not available with this embedder" in r.json()["detail"]
        assert r.json()["detail"].split(":", 1)[1].replace("cluster_topics", "find_duplicates") == dup.json()["detail"].split(":", 1)[1]
        assert not plain_manager.supports_clustering() and not plain_manager.supports_dedup()

        empty = c1.get("/topics").json()                          # nothing stored yet: a report without topics
        assert empty == {"n_topics": 0, "iterations": 0, "converged": True, "objective": None, "topics": []}
        a = upload(c1, "a.txt", document("alpha", 6))
        b = upload(c1, "b.txt", document("beta", 5))
        n = a["chunks_processed"]["text"] + b["chunks_processed"]["text"]
        assert manager.supports_clustering()

        rep = c1.get("/topics", params={"n_topics": 3, "representatives": 2, "seed": 4})
        assert rep.status_code == 200, rep.text
        rep = rep.json()
        assert set(rep) == {"n_topics", "iterations", "converged", "objective", "topics"}
        assert rep["n_topics"] == 3 and len(rep["topics"]) == 3 and isinstance(rep["objective"], float)
        assert rep["iterations"] >= 1 and isinstance(rep["converged"], bool)
        assert sum(t["size"] for t in rep["topics"]) == n
        assert [t["size"] for t in rep["topics"]] == sorted((t["size"] for t in rep["topics"]), reverse=True)
        for t in rep["topics"]:
            assert set(t) == {"topic", "size", "cohesion", "representatives", "documents"}
            assert 1 <= len(t["representatives"]) <= 2 and -1.0 <= t["cohesion"] <= 1.0 + 1e-6
            for hit in t["representatives"]:
                assert set(hit) == {"id", "score", "document", "metadata"}
                assert hit["metadata"]["doc_id"] in (a["doc_id"], b["doc_id"]) and hit["id"].startswith(hit["metadata"]["doc_id"])
                assert isinstance(hit["document"], str) and hit["document"]
            assert t["documents"] and all(set(x) == {"doc_id", "count"} for x in t["documents"])
            assert sum(x["count"] for x in t["documents"]) == t["size"]
        assert c1.get("/topics", params={"n_topics": 3, "representatives": 2, "seed": 4}).json() == rep     # reproducible

        auto = c1.get("/topics").json()                           # MMRAG_TOPICS=0: the automatic rule
        assert auto["n_topics"] == config.auto_topics(n)
        monkeypatch.setattr(config.settings, "MMRAG_TOPICS", 4)
        assert c1.get("/topics").json()["n_topics"] == 4
        only = c1.get("/topics", params={"doc_id": b["doc_id"], "n_topics": 2}).json()
        assert sum(t["size"] for t in only["topics"]) == b["chunks_processed"]["text"]
        assert all(x["doc_id"] == b["doc_id"] for t in only["topics"] for x in t["documents"])
        assert c1.get("/topics", params={"doc_id": "doc_nothing"}).json()["n_topics"] == 0

        # parameter validation and the error mapping: 400 as /duplicates maps a ValueError; 422 for a non-number
        for bad in ({"representatives": 0}, {"representatives": 11}, {"n_topics": 0}, {"n_topics": n + 1},
                    {"n_topics": 4097}, {"n_topics": -3}):
            r = c1.get("/topics", params=bad)
            assert r.status_code == 400 and r.json()["detail"], bad
        assert c1.get("/topics", params={"n_topics": "many"}).status_code == 422
        assert c1.get("/duplicates", params={"threshold": 1.5}).status_code == 400

        def boom(**kw):
            raise RuntimeError("injected engine failure")

        monkeypatch.setattr(manager.collection, "cluster", boom)
        assert c1.get("/topics").status_code == 500


# ---------------------------------------------------------------- 5. the kernels as compiled
def test_kernel_resources(tmp_path):
    asm = asm_util.compile_asm("kmeans.hip", tmp_path)
    meta = {m.group(1): m.group(2) for m in re.finditer(r"- \.agpr_count:.*?\.name:\s+(\w+)(.*?)\.wavefront_size", asm, re.S)}
    # assign: two workgroups per CU (half of the 160 KiB of LDS each, two waves per SIMD of 512 registers);
    # sums: a small streaming kernel, at least four workgroups per CU
    for kernel, max_lds, max_vgprs in (("kmeans_assign_kernel", 80 * 1024, 256), ("cluster_sums_kernel", 16 * 1024, 128)):
        kernels = re.findall(r"\.amdhsa_kernel (\w*%s\w*)(.*?)\.end_amdhsa_kernel" % kernel, asm, re.S)
        assert len(kernels) == 3, [k for k, _ in kernels]           # float32, float16, bfloat16
        for name, body in kernels:
            lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
            scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
            vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
            assert scratch == 0, (name, scratch)
            assert 0 < lds <= max_lds, (name, lds)
            assert vgprs <= max_vgprs, (name, vgprs)
            assert name in meta and int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta[name]).group(1)) == 0, name
