"""Significant terms through the embedder and the server without a GPU: GET /topics?terms=n and
GET /documents/{doc_id}/keywords over a fake collection whose terms come from tests/terms_ref.py."""
import numpy as np

from tests import terms_ref as R
from tests.fakes import FakeEngine
from tests.test_cluster_cpu import ClusterCollection, ClusterEngine, document, make_client, upload


class TermsCollection(ClusterCollection):
    """ClusterCollection plus VectorIndex.significant_terms and cluster(terms=...), computed by tests/terms_ref.py"""

    def _lists(self, group, G, top, min_count, min_length, exclude=()):
        from multimodal_rag_amd.lexical import LEX_DOCUMENTS, Lexicon, analyze, label_allowed

        lex = Lexicon()
        off, ids, _, _ = lex.analyze_batch(self.docs, LEX_DOCUMENTS)
        words = lex.terms(0, len(lex))
        drop = {t for w in exclude for t in analyze(w)}
        mask = np.asarray([label_allowed(w, min_length) and w not in drop for w in words], bool)
        df = R.live_df(off, ids, np.ones(len(self.docs), bool), len(words))
        sizes = np.bincount(group[group >= 0], minlength=G)
        s, t, c = R.group_terms(off, ids, group, sizes, df, len(self.docs), mask, min_count, top)
        return sizes, [[{"term": words[j], "score": float(s[g, i]), "count": int(c[g, i]), "background": int(df[j])}
                        for i, j in enumerate(t[g]) if j >= 0] for g in range(G)]

    def significant_terms(self, where=None, key=None, values=None, labels=None, top=10, min_count=2, min_length=3,
                          exclude=()):
        if key is None or values is None or where is not None or labels is not None:
            raise ValueError("the fake groups by key + values only")
        if not 1 <= top <= 4096 or min_count < 1:
            raise ValueError("significant terms: top must be in 1..4096 and min_count at least 1")
        at = {v: g for g, v in enumerate(values)}
        group = np.asarray([at.get(m.get(key), -1) for m in self.metas], np.int64).reshape(-1)
        sizes, lists = self._lists(group, len(values), top, min_count, min_length, exclude)
        return [{"group": v, "size": int(sizes[g]), "terms": lists[g]} for g, v in enumerate(values)]

    def cluster(self, n_clusters=None, where=None, max_iter=25, tol=1e-3, seed=0, init=None, representatives=3,
                return_labels=False, terms=0):
        from multimodal_rag_amd.index import match_where

        out = super().cluster(n_clusters, where, max_iter, tol, seed, init, representatives, return_labels)
        if terms and out["n_clusters"]:
            alive = np.array([match_where(m, where) for m in self.metas], bool)
            group = np.where(alive, np.argmax(self.vecs @ np.asarray(out["centroids"], np.float32).T, axis=1), -1)
            sizes, lists = self._lists(group, out["n_clusters"], terms, 2, 3)
            for c in out["clusters"]:
                assert c["size"] == sizes[c["cluster"]]
                c["terms"] = lists[c["cluster"]]
        return out


class TermsEngine(FakeEngine):
    def new_collection(self, name, metadata=None):
        c = TermsCollection(self.dim, name, metadata)
        self.collections.append(c)
        return c


TERM_KEYS = {"term", "score", "count", "background"}
TOPIC_KEYS = {"topic", "size", "cohesion", "representatives", "documents"}


def test_topics_with_terms_and_labels(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    monkeypatch.setattr(config.settings, "MMRAG_TOPICS", 0)
    monkeypatch.setattr(config.settings, "MMRAG_TOPIC_TERMS", 0)
    client, manager = make_client(TermsEngine())
    with client as c:
        upload(c, "a.txt", document("alpha", 6))
        upload(c, "b.txt", document("beta", 5))
        assert manager.supports_terms() and manager.supports_clustering()
        ask = {"n_topics": 2, "representatives": 2, "seed": 4}
        plain = c.get("/topics", params=ask).json()
        assert all(set(t) == TOPIC_KEYS for t in plain["topics"])                 # without `terms`: exactly as it was
        assert c.get("/topics", params={**ask, "terms": 0}).json() == plain
        rep = c.get("/topics", params={**ask, "terms": 3})
        assert rep.status_code == 200, rep.text
        rep = rep.json()
        assert set(rep) == set(plain) and len(rep["topics"]) == 2
        for t, before in zip(rep["topics"], plain["topics"]):
            assert set(t) == TOPIC_KEYS | {"terms", "label"}
            assert {k: t[k] for k in TOPIC_KEYS} == before
            assert len(t["terms"]) <= 3 and all(set(x) == TERM_KEYS for x in t["terms"])
            assert t["label"] == ", ".join(x["term"] for x in t["terms"][:3])
            scores = [x["score"] for x in t["terms"]]
            assert scores == sorted(scores, reverse=True) and all(x["count"] >= 2 for x in t["terms"])
        assert any(t["terms"] for t in rep["topics"])
        five = c.get("/topics", params={**ask, "terms": 5}).json()
        assert all(t["label"] == ", ".join(x["term"] for x in t["terms"][:3]) for t in five["topics"])
        monkeypatch.setattr(config.settings, "MMRAG_TOPIC_TERMS", 3)               # the default of a request that says nothing
        assert c.get("/topics", params=ask).json() == rep
        assert c.get("/topics", params={**ask, "terms": 0}).json() == plain
        for bad in (33, -1):
            r = c.get("/topics", params={**ask, "terms": bad})
            assert r.status_code == 400 and "terms must be in 0..32" in r.json()["detail"]
        assert c.get("/topics", params={**ask, "terms": "few"}).status_code == 422


def test_document_keywords_route(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    monkeypatch.setattr(config.settings, "MMRAG_TOPIC_TERMS", 0)
    client, manager = make_client(TermsEngine())
    with client as c:
        a = upload(c, "a.txt", document("alpha", 6))
        b = upload(c, "b.txt", document("beta", 5))
        r = c.get(f"/documents/{a['doc_id']}/keywords")
        assert r.status_code == 200, r.text
        got = r.json()
        assert set(got) == {"doc_id", "chunks", "keywords"}
        assert got["doc_id"] == a["doc_id"] and got["chunks"] == a["chunks_processed"]["text"] >= 2
        words = [x["term"] for x in got["keywords"]]
        assert "alpha" in words and "beta" not in words and all(set(x) == TERM_KEYS for x in got["keywords"])
        assert all(x["count"] >= 2 and len(x["term"]) >= 3 for x in got["keywords"])
        other = c.get(f"/documents/{b['doc_id']}/keywords", params={"top": 1, "min_count": 1}).json()
        assert [x["term"] for x in other["keywords"]] == ["beta"] and other["chunks"] == b["chunks_processed"]["text"]
        monkeypatch.setattr(config.settings, "MMRAG_KEYWORD_MIN_LENGTH", 6)        # "alpha" has five code points
        assert "alpha" not in [x["term"] for x in c.get(f"/documents/{a['doc_id']}/keywords").json()["keywords"]]
        monkeypatch.setattr(config.settings, "MMRAG_KEYWORD_MIN_LENGTH", 3)
        missing = c.get("/documents/doc_nothing/keywords")
        assert missing.status_code == 404 and "doc_nothing" in missing.json()["detail"]
        for bad in ({"top": 0}, {"top": 101}, {"min_count": 0}):
            assert c.get(f"/documents/{a['doc_id']}/keywords", params=bad).status_code == 400, bad
        assert c.get(f"/documents/{a['doc_id']}/keywords", params={"top": "all"}).status_code == 422
        assert c.get(f"/documents/{a['doc_id']}/related").status_code in (200, 400)   # the sibling route still answers


def test_embedders_that_cannot(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    monkeypatch.setattr(config.settings, "MMRAG_TOPIC_TERMS", 0)
    plain, plain_manager = make_client(FakeEngine())
    topical, manager = make_client(ClusterEngine())
    with plain as c0, topical as c1:
        a = upload(c0, "a.txt", document("alpha", 4))
        r = c0.get(f"/documents/{a['doc_id']}/keywords")
        assert r.status_code == 400 and "Significant terms are not available with this embedder" in r.json()["detail"]
        assert not plain_manager.supports_terms()
        # a collection that clusters but keeps no terms: /topics answers, /topics?terms=n is the same 400
        b = upload(c1, "b.txt", document("beta", 4))
        assert manager.supports_clustering() and not manager.supports_terms()
        assert c1.get("/topics", params={"n_topics": 2}).status_code == 200
        r = c1.get("/topics", params={"n_topics": 2, "terms": 3})
        assert r.status_code == 400 and "Significant terms are not available with this embedder" in r.json()["detail"]
        assert c1.get(f"/documents/{b['doc_id']}/keywords").status_code == 400
