"""CPU: near-duplicate detection without a device -- the numpy reference against a second brute force, the component and
greedy rules, the join's tile mapping and argument checks through the library's exports, settings, the /duplicates and
/upload surface over a fake collection, and the kernel's resources as compiled for gfx950."""
import ctypes
import re

import numpy as np
import pytest
from starlette.testclient import TestClient

from tests import asm_util
from tests import dedup_ref as R
from tests.fakes import FakeCollection, FakeEngine


# ---------------------------------------------------------------- 1. the reference itself
def test_reference_pairs_against_loops():
    g = np.random.default_rng(3)
    for n, d, t in ((1, 4, 0.5), (2, 4, 0.1), (37, 3, 0.8), (64, 2, 0.95)):
        x = g.standard_normal((n, d))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        alive = g.random(n) > 0.3
        for mask in (None, alive):
            want = {}
            for i in range(n):
                for j in range(i + 1, n):
                    s = float(np.dot(x[i], x[j]))
                    if s >= t and (mask is None or (mask[i] and mask[j])):
                        want[(i, j)] = s
            got = R.pairs(x, mask, t)
            assert set(got) == set(want)
            assert all(abs(got[k] - want[k]) < 1e-12 for k in want)


def test_reference_recipe_separates_planted_from_unplanted():
    for dtype in ("fp16", "bf16", "fp32"):
        x, planted = R.make_rows(513, 64, 11, dtype)
        x64 = R.stored(x, dtype)
        g = R.gram(x64)
        for i, j, c in planted:
            assert abs(g[i, j] - c) < 1.1e-3, (dtype, i, j, c, g[i, j])
        assert {(i, j) for i, j, _ in planted} >= {(0, 1), (255, 256), (127, 128), (126, 129), (5, 511)}
        mask = np.ones_like(g, bool)
        for i, j, _ in planted:
            mask[i, j] = mask[j, i] = False
        np.fill_diagonal(mask, False)
        assert g[mask].max() <= 0.6
        assert R.band_is_empty(x64, R.T_JOIN)


def test_components_chains_and_stars():
    assert R.components([]) == []
    assert R.components([(3, 9), (9, 4), (4, 20)]) == [[3, 4, 9, 20]]                 # a chain: one component
    assert R.components([(7, 1), (7, 2), (7, 30), (5, 6)]) == [[1, 2, 7, 30], [5, 6]]  # a star and a pair, keeper order
    g = np.random.default_rng(5)
    for _ in range(20):
        n = 40
        edges = [(int(a), int(b)) for a, b in g.integers(0, n, (25, 2)) if a != b]
        comps = R.components(edges)
        label = list(range(n))
        for _ in range(n):                      # second method: label propagation to the minimum
            for a, b in edges:
                label[a] = label[b] = min(label[a], label[b])
        touched = sorted({v for e in edges for v in e})
        want = {}
        for v in touched:
            want.setdefault(label[v], []).append(v)
        assert comps == [want[k] for k in sorted(want)]
        assert all(c[0] == min(c) for c in comps) and [c[0] for c in comps] == sorted(c[0] for c in comps)


def test_greedy_rule():
    # chain a~b~c without a~c: a kept, b skipped for a, c kept (its only partner was skipped)
    assert R.greedy([None] * 3, [(0, 1), (1, 2)], 3) == ([0, 2], {1: ("batch", 0)})
    # a stored duplicate wins over a batch one, and a row skipped for a stored row shields nobody
    kept, skipped = R.greedy([None, 17, None], [(0, 1), (1, 2)], 3)
    assert kept == [0, 2] and skipped == {1: ("stored", 17)}
    kept, skipped = R.greedy([4, None, None], [(0, 1), (0, 2), (1, 2)], 3)
    assert kept == [1] and skipped == {0: ("stored", 4), 2: ("batch", 1)}
    # the lowest KEPT partner is reported
    assert R.greedy([None] * 4, [(0, 3), (1, 3), (0, 1)], 4) == ([0, 2], {1: ("batch", 0), 3: ("batch", 0)})
    assert R.greedy([None] * 5, [(i, j) for i in range(5) for j in range(i + 1, 5)], 5)[0] == [0]


# ---------------------------------------------------------------- 2. the library's host-side exports
@pytest.fixture(scope="module")
def native():
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def row_start(T, r):
    return r * T - r * (r - 1) // 2


@pytest.mark.parametrize("T", [1, 2, 3, 33, 7813, 65536])
def test_join_tile_row_ends(native, T):
    rows = range(T)
    if T == 65536:
        g = np.random.default_rng(1)
        rows = sorted(set(range(64)) | set(range(T - 64, T)) | set(int(v) for v in g.integers(0, T, 4096 - 128)))
    for ti in rows:
        first, last = row_start(T, ti), row_start(T, ti + 1) - 1
        assert native.join_tile(T, first) == (ti, ti), (T, ti)
        assert native.join_tile(T, last) == (ti, T - 1), (T, ti)
        # the kernel's own order holds the same tiles band by band: the band's first and last slot stay inside the band
        b0 = ti // 8 * 8
        a, b = native.join_tile(T, first, slot_order=True)
        assert b0 <= a <= b < T and a < b0 + 8


@pytest.mark.parametrize("T", [1, 2, 3, 7, 8, 9, 16, 17, 33])
def test_join_tile_is_one_to_one(native, T):
    total = T * (T + 1) // 2
    want = [(i, j) for i in range(T) for j in range(i, T)]
    assert [native.join_tile(T, at) for at in range(total)] == want          # row-major, in order
    banded = [native.join_tile(T, at, slot_order=True) for at in range(total)]
    assert sorted(banded) == want and len(set(banded)) == total
    for at, (ti, tj) in enumerate(banded):                                    # a band holds the ids of its own rows
        assert row_start(T, ti // 8 * 8) <= at < row_start(T, min(T, ti // 8 * 8 + 8))
    for bad in (-1, total):
        with pytest.raises(native.MMRagNativeError):
            native.join_tile(T, bad)


def test_sim_join_argument_checks_need_no_device(native):
    L = native.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)       # never dereferenced: every call below returns before anything is launched
    EINVAL, EUNSUPPORTED = 1, 4

    def call(rows=p, n=100, ld=64, dtype=native.F16, d=64, alive=None, t=0.9, pairs=p, scores=p, cap=16, count=p):
        return L.mmrag_sim_join(rows, n, ld, dtype, d, alive, t, pairs, scores, cap, count, None)

    assert call(rows=None) == EINVAL and call(pairs=None) == EINVAL
    assert call(scores=None) == EINVAL and call(count=None) == EINVAL
    assert call(n=-1) == EINVAL and call(d=0) == EINVAL and call(d=-3) == EINVAL
    assert call(ld=63) == EINVAL                                  # ld < d
    assert call(cap=-1) == EINVAL and call(cap=native.MAX_JOIN_PAIRS + 1) == EINVAL
    assert call(t=0.0) == EINVAL and call(t=-0.5) == EINVAL and call(t=float("nan")) == EINVAL
    assert call(dtype=7) == EINVAL and call(dtype=-1) == EINVAL
    assert call(dtype=native.F8E4M3, ld=128, d=64) == EUNSUPPORTED
    assert b"re-scoring plane" in L.mmrag_last_error()
    assert native.MAX_JOIN_PAIRS == 1 << 26 and L.mmrag_abi_version() == 1


# ---------------------------------------------------------------- 3. settings
def test_settings_parsing(monkeypatch):
    from multimodal_rag_amd.config import Settings

    monkeypatch.delenv("MMRAG_DEDUP_THRESHOLD", raising=False)
    monkeypatch.delenv("MMRAG_DEDUP_REPORT_THRESHOLD", raising=False)
    s = Settings()
    assert s.MMRAG_DEDUP_THRESHOLD == 0.0 and s.dedup_threshold() == 0.0 and s.MMRAG_DEDUP_REPORT_THRESHOLD == 0.98
    monkeypatch.setenv("MMRAG_DEDUP_THRESHOLD", "0.95")
    monkeypatch.setenv("MMRAG_DEDUP_REPORT_THRESHOLD", "0.9")
    s = Settings()
    assert s.dedup_threshold() == 0.95 and s.MMRAG_DEDUP_REPORT_THRESHOLD == 0.9
    monkeypatch.setenv("MMRAG_DEDUP_THRESHOLD", "1")
    assert Settings().dedup_threshold() == 1.0
    for bad in ("1.5", "-0.1", "nan"):
        monkeypatch.setenv("MMRAG_DEDUP_THRESHOLD", bad)
        with pytest.raises(ValueError, match="MMRAG_DEDUP_THRESHOLD"):
            Settings()


# ---------------------------------------------------------------- 4. embedder + server over a fake collection
class DedupCollection(FakeCollection):
    """FakeCollection plus the near-duplicate calls of VectorIndex, computed by tests/dedup_ref.py"""

    def near_duplicates(self, threshold=None, where=None, max_pairs=1 << 20):
        from multimodal_rag_amd.config import settings
        from multimodal_rag_amd.index import match_where

        t = settings.MMRAG_DEDUP_REPORT_THRESHOLD if threshold is None else threshold
        if not 0.0 < t <= 1.0:
            raise ValueError(f"threshold must be a cosine in (0, 1] (got {t!r})")
        alive = [match_where(m, where) for m in self.metas]
        found = R.pairs(self.vecs.astype(np.float64), alive, t)
        order = sorted(found)[:max_pairs]
        return {"threshold": t, "total_pairs": len(found), "truncated": len(found) > len(order),
                "pairs": [(self.ids[a], self.ids[b], found[(a, b)]) for a, b in order],
                "groups": [[self.ids[r] for r in comp] for comp in R.components(order)]}

    def drop_duplicates(self, threshold=None, where=None, max_pairs=1 << 20):
        from multimodal_rag_amd.index import DuplicateReportTruncated

        report = self.near_duplicates(threshold, where, max_pairs)
        if report["truncated"]:
            raise DuplicateReportTruncated("truncated report; nothing was deleted")
        return self.delete(ids=[s for g in report["groups"] for s in g[1:]])

    def add(self, embeddings, documents=None, metadatas=None, ids=None, dedup_threshold=None):
        if dedup_threshold is None:
            return super().add(embeddings, documents, metadatas, ids)
        e = np.asarray(embeddings, np.float64).reshape(-1, self.dim)
        old = self.vecs.astype(np.float64)
        best = [None] * len(e)
        if len(old):
            s = e @ old.T
            best = [int(np.argmax(row)) if row.max() >= dedup_threshold else None for row in s]
        kept, skipped = R.greedy(best, sorted(R.pairs(e, None, dedup_threshold)), len(e))
        super().add(e[kept], [documents[j] for j in kept], [metadatas[j] for j in kept], [ids[j] for j in kept])
        return {"added": [ids[j] for j in kept],
                "skipped": [(ids[j], self.ids[w] if kind == "stored" else ids[w], 1.0) for j, (kind, w) in skipped.items()]}


class DedupEngine(FakeEngine):
    def new_collection(self, name, metadata=None):
        c = DedupCollection(self.dim, name, metadata)
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


DOC = ("Alpha paragraph about retrieval engines. " * 30 + "\n\n" + "Beta paragraph on matrix cores. " * 40).encode()


def upload(client, name="a.txt", data=DOC):
    r = client.post("/upload", files={"file": (name, data, "text/plain")})
    assert r.status_code == 200, r.text
    return r.json()


def test_upload_and_duplicates_routes_with_the_setting_off(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    plain, _ = make_client(FakeEngine())
    dedup, _ = make_client(DedupEngine())
    with plain as c0, dedup as c1:
        a0, a1 = upload(c0), upload(c1)
        # setting 0: the answer is today's, whatever the collection can do
        assert set(a0) == set(a1) == {"doc_id", "filename", "doc_type", "chunks_processed", "message", "processing_time"}
        assert a0["chunks_processed"] == a1["chunks_processed"] and set(a1["chunks_processed"]) == {"text", "table", "image"}
        assert re.fullmatch(r"Processed in \d+\.\d\ds", a0["message"]) and re.fullmatch(r"Processed in \d+\.\d\ds", a1["message"])
        n = a1["chunks_processed"]["text"]
        assert n >= 2
        upload(c1, "b.txt")                                            # the same file again: stored again in full
        assert c1.get("/stats").json()["documents"]["total_chunks"] == 2 * n

        # a collection without near_duplicates: 400 with the MODE_NEEDS-style detail, on both routes
        for r in (c0.get("/duplicates"), c0.delete("/duplicates")):
            assert r.status_code == 400 and "Near-duplicate detection is not available" in r.json()["detail"]

        rep = c1.get("/duplicates", params={"threshold": 0.99}).json()
        assert set(rep) == {"threshold", "total_pairs", "truncated", "pairs", "groups"}
        assert rep["total_pairs"] == n and rep["truncated"] is False and len(rep["pairs"]) == n
        assert all(set(p) == {"a", "b", "cosine"} and p["cosine"] >= 0.99 for p in rep["pairs"])
        assert len(rep["groups"]) == n and all(set(g) == {"keep", "duplicates"} for g in rep["groups"])
        assert all(g["keep"].startswith(a1["doc_id"]) and len(g["duplicates"]) == 1 for g in rep["groups"])
        cut = c1.get("/duplicates", params={"threshold": 0.99, "limit": 1}).json()
        assert len(cut["pairs"]) == 1 and cut["total_pairs"] == n and len(cut["groups"]) == n
        assert c1.get("/duplicates").json()["threshold"] == config.settings.MMRAG_DEDUP_REPORT_THRESHOLD
        only = c1.get("/duplicates", params={"threshold": 0.99, "doc_id": a1["doc_id"]}).json()
        assert only["total_pairs"] == 0 and only["groups"] == []      # one document alone holds no copies
        assert c1.get("/duplicates", params={"threshold": 1.5}).status_code == 400

        gone = c1.delete("/duplicates", params={"threshold": 0.99}).json()
        assert gone["deleted"] == n and len(gone["ids"]) == n and not any(i.startswith(a1["doc_id"]) for i in gone["ids"])
        assert c1.get("/stats").json()["documents"]["total_chunks"] == n
        assert c1.get("/duplicates", params={"threshold": 0.99}).json()["total_pairs"] == 0
        assert c1.delete("/duplicates", params={"threshold": 0.99}).json() == {"deleted": 0, "ids": []}


def test_delete_duplicates_answers_409_when_truncated(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    client, manager = make_client(DedupEngine())
    with client as c:
        n = upload(c)["chunks_processed"]["text"]
        upload(c, "b.txt")
        col = manager.collection
        full = col.near_duplicates
        monkeypatch.setattr(col, "near_duplicates", lambda threshold=None, where=None, max_pairs=0: full(threshold, where, 1))
        r = c.delete("/duplicates", params={"threshold": 0.99})
        assert r.status_code == 409 and "nothing was deleted" in r.json()["detail"]
        assert c.get("/stats").json()["documents"]["total_chunks"] == 2 * n


def test_upload_with_the_setting_on(monkeypatch, caplog):
    from multimodal_rag_amd import config, embedder

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.95)
    client, _ = make_client(DedupEngine())
    with client as c:
        first = upload(c)
        n = first["chunks_processed"]["text"]
        assert first["chunks_processed"] == {"text": n, "table": 0, "image": 0, "duplicates_skipped": 0}
        assert re.fullmatch(r"Processed in \d+\.\d\ds", first["message"])          # nothing skipped: today's message
        again = upload(c, "b.txt")
        assert again["chunks_processed"] == {"text": n, "table": 0, "image": 0, "duplicates_skipped": n}
        assert again["message"].endswith(f", {n} duplicates skipped")
        assert c.get("/stats").json()["documents"]["total_chunks"] == n
        assert c.get("/duplicates", params={"threshold": 0.95}).json()["total_pairs"] == 0

    # set but unsupported: one warning per process, stored as today
    monkeypatch.setattr(embedder, "_dedup_warned", False)
    plain, _ = make_client(FakeEngine())
    with plain as c, caplog.at_level("WARNING", logger=embedder.logger.name):
        a = upload(c)
        b = upload(c, "b.txt")
        assert set(a["chunks_processed"]) == set(b["chunks_processed"]) == {"text", "table", "image"}
        assert c.get("/stats").json()["documents"]["total_chunks"] == 2 * a["chunks_processed"]["text"]
    assert sum("MMRAG_DEDUP_THRESHOLD" in rec.getMessage() for rec in caplog.records) == 1


# ---------------------------------------------------------------- 5. the kernel as compiled
def test_kernel_resources(tmp_path):
    asm = asm_util.compile_asm("simjoin.hip", tmp_path)
    kernels = re.findall(r"\.amdhsa_kernel (\w*sim_join_kernel\w*)(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert len(kernels) == 3, [k for k, _ in kernels]           # float32, float16, bfloat16
    meta = {m.group(1): m.group(2) for m in re.finditer(r"- \.agpr_count:.*?\.name:\s+(\w+)(.*?)\.wavefront_size", asm, re.S)}
    for name, body in kernels:
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        assert scratch == 0, (name, scratch)
        assert 0 < lds <= 80 * 1024, (name, lds)                 # two workgroups per CU: half of the 160 KiB
        assert vgprs <= 256, (name, vgprs)                       # two waves per SIMD (512 registers)
        assert name in meta and int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta[name]).group(1)) == 0, name
