"""GPU: phrase queries -- mmrag_phrase_match and mmrag_bm25_phrase_topk on synthetic term-id sequences against
tests/phrase_ref.py (ptf, counts and bitmaps exactly; scores through bm25_ref.assert_topk, rtol 1e-5), the overflow
re-run, bit identity, and the index, hybrid and /query levels on texts."""
import numpy as np
import pytest
import torch

from tests import bm25_ref
from tests import phrase_ref as R

pytestmark = pytest.mark.gpu

A, B_, C, D = 0, 1, 2, 3
FILL = 9
E8 = list(range(20, 28))          # an 8-term phrase of rare terms
P, Q = 30, 31                     # the slop rows
K0, Z = 40, 50                    # K0 + i: a term held by exactly SEAMS[i] rows; Z: its partner, held by many more
DEAD_ONLY = 60                    # held by one dead row: in the lexicon, live df 0
N_TERMS = 61


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return "cuda:0"


def limits():
    from multimodal_rag_amd.lexical import phrase_limits

    return phrase_limits()


def seams():
    lim = limits()
    sizes = sorted({lim["match_block"], lim["lane_starts"], lim["wave_lanes"]})
    return [s + d for s in sizes for d in (-1, 0, 1)]


class Corpus:
    """n = 2 SCORE_R + 3 rows: two full scoring blocks and one of three rows"""

    def __init__(self):
        lim = limits()
        self.R = SR = lim["score_rows"]
        self.n = n = 2 * SR + 3
        g = np.random.default_rng(7)
        seqs = [g.choice(8, int(g.integers(0, 13)), p=[.25, .2, .15, .1, .1, .1, .05, .05]).tolist() for _ in range(n)]
        self.planted = [0, SR - 1, SR, n - 1]
        seqs[0] = E8 + [4, 5]                       # the phrase at the first position of a row
        seqs[SR - 1] = [4, 5] + E8                  # and at the last
        seqs[SR] = [4] + E8 + [5]
        seqs[n - 1] = list(E8)
        self.edge_dead = [1, SR - 2, SR + 1, n - 2]  # dead rows at the block edges, holding what the queries look for
        for r in self.edge_dead:
            seqs[r] = [A, B_, A] + E8
        seqs[SR + 1] = seqs[SR + 1] + [DEAD_ONLY]
        seqs[5] = []                                # dl 0
        seqs[6] = [A]                               # dl 1
        self.long_row = 7                           # the first term more often than a wave has lanes
        seqs[7] = [A] * (3 * lim["wave_lanes"] + 8) + [B_]
        self.lane_rows = {}
        for at, c in enumerate((lim["lane_starts"] - 1, lim["lane_starts"], lim["lane_starts"] + 1)):
            seqs[8 + at] = [A] * (c - 1) + [B_, A]  # starts one below, at and one above what a lane walks alone
            self.lane_rows[c] = 8 + at
        self.slop_rows = {0: 20, 1: 21, 16: 22}     # matches at that slop, fails at one less
        seqs[20] = [P, Q]
        seqs[21] = [P, FILL, Q]
        seqs[22] = [P] + [FILL] * 16 + [Q]
        seqs[23] = [P] + [FILL] * 17 + [Q]          # fails at every allowed slop
        special = set(self.planted + self.edge_dead + [5, 6, 7, 8, 9, 10, 20, 21, 22, 23])
        free = [r for r in g.permutation(n).tolist() if r not in special]
        self.seams = seams()
        at = 0
        for i, c in enumerate(self.seams):          # driver lists one below, at and one above each partition size
            for j, r in enumerate(free[at: at + c]):
                seqs[r] = seqs[r] + ([K0 + i, Z] if j % 3 else [K0 + i, FILL, Z])
            at += c
        for r in free[at: at + 1200]:
            seqs[r] = seqs[r] + [Z]
        self.seqs = seqs
        dead = np.zeros(n, bool)
        dead[self.edge_dead] = True
        dead[g.permutation(free)[:30]] = True
        self.live = ~dead
        where = g.random(n) < 0.75
        where[self.planted] = True
        self.where = where
        self.ref = R.PhraseRef(seqs)
        k = [K0 + i for i in range(len(self.seams))]
        self.pool = ([([A, B_], []), ([C], [(A, B_)]), ([], [(A, A)]), ([D], [(A, B_, A)]), ([], [tuple(E8)]),
                      ([A], [(C,)])] + [([], [(t, Z)]) for t in k] +
                     [([], [(P, Q)]), ([A], [(A, DEAD_ONLY)]), ([B_], [(A, -1)]),
                      ([4], [(A, B_), (B_, C), (C,), (A, A)]), ([], []), ([5, 6], [(B_, A), (A, B_)])])
        self.four = len(self.pool) - 3
        self._scored = {}

    def queries(self, B):
        if B == 1:
            return [self.pool[self.four]]
        if B == 3:
            return [self.pool[0], self.pool[1], self.pool[self.four]]      # 0, 1 and 4 phrases in one batch
        return [self.pool[i % len(self.pool)] for i in range(B)]

    def scored(self, at, slop, mode, use_where):
        key = (at, slop, mode, use_where)
        if key not in self._scored:
            loose, phrases = self.pool[at]
            visible = self.live & self.where if use_where else self.live
            self._scored[key] = self.ref.scores(loose, [list(p) for p in phrases], self.live, slop, mode, visible=visible)
        return self._scored[key]


@pytest.fixture(scope="module")
def corpus():
    return Corpus()


@pytest.fixture(scope="module")
def lex(dev, corpus):
    from multimodal_rag_amd.lexical import LexicalIndex

    lx = LexicalIndex(dev)
    lx.append_sequences(corpus.seqs[:1500])
    lx.append_sequences(corpus.seqs[1500:])         # the second append grows the plane
    lx.delete_rows(np.nonzero(~corpus.live)[0])
    assert lx.positions_enabled and lx.n == corpus.n and lx.n_terms == N_TERMS
    assert lx._pos_total == sum(len(s) for s in corpus.seqs) == lx.sum_dl + int(sum(len(corpus.seqs[r]) for r in
                                                                                    np.nonzero(~corpus.live)[0]))
    return lx


def bits_of(flags, dev):
    from multimodal_rag_amd import _native

    return torch.from_numpy(R.bitmap(flags, _native.filter_words(len(flags))).view(np.int32)).to(dev)


def flat(queries):
    q_off = np.zeros(len(queries) + 1, np.int32)
    np.cumsum([len(l) for l, _ in queries], out=q_off[1:])
    return q_off, np.asarray([t for l, _ in queries for t in l], np.int32), [list(p) for _, p in queries]


def test_corpus_holds_the_cases(corpus):
    c, ref = corpus, corpus.ref
    lim = limits()
    assert [len(ref.holders[K0 + i]) for i in range(len(c.seams))] == c.seams and len(ref.holders[Z]) > max(c.seams)
    assert {lim["match_block"] + d for d in (-1, 0, 1)} <= set(c.seams)
    assert {lim["lane_starts"] + d for d in (-1, 0, 1)} <= set(c.seams)
    for s, r in c.slop_rows.items():
        assert ref.tf([P, Q], s)[r] == 1 and (s == 0 or ref.tf([P, Q], s - 1)[r] == 0)
    assert ref.tf([P, Q], 16)[23] == 0
    assert ref.tf([A, A], 0)[c.long_row] == 3 * lim["wave_lanes"] + 7 > lim["wave_lanes"]     # overlapping occurrences
    assert ref.tf([A, B_], 0)[c.long_row] == 1 and ref.tf([A, B_], 16)[c.long_row] == 17
    for n_a, r in c.lane_rows.items():
        assert c.seqs[r].count(A) == n_a and ref.tf([A, B_, A], 0)[r] == 1 and ref.tf([A, B_, A], 1)[r] == 2
    assert all(ref.tf(E8, 0)[r] == 1 for r in c.planted + c.edge_dead)
    assert c.seqs[0][:8] == E8 and c.seqs[c.R - 1][-8:] == E8 and not c.live[c.edge_dead].any()
    assert ref.known([A, B_], c.live) and not ref.known([A, DEAD_ONLY], c.live) and not ref.known([A, -1], c.live)


CASES = [(130, 5, 0, "require", False), (130, 21, 1, "require", True), (130, 4096, 16, "require", False),
         (130, 1, 0, "prefer", True), (130, 5, 16, "prefer", False), (130, 21, 1, "prefer", False),
         (3, 5, 0, "require", True), (3, 4096, 1, "prefer", False), (3, 21, 16, "require", False),
         (1, 1, 0, "require", False), (1, 5, 1, "prefer", True), (1, 4096, 16, "require", True)]


@pytest.mark.parametrize("B,k,slop,mode,use_where", CASES)
def test_match_and_score_against_the_reference(dev, corpus, lex, B, k, slop, mode, use_where):
    c, ref = corpus, corpus.ref
    queries = c.queries(B)
    visible = c.live & c.where if use_where else c.live
    q_off, q_terms, q_phrases = flat(queries)
    got_s, got_r, info = lex.topk_phrase_ids(q_off, q_terms, q_phrases, k, bits_of(visible, dev), slop=slop,
                                             phrase_mode=mode, bitmaps=True)
    torch.cuda.synchronize()
    # the match: drivers, ptf per driver posting, counts
    ptf, held = info["ptf"].cpu().numpy(), info["rows"].cpu().numpy()
    assert len(info["phrases"]) == len({tuple(p) for _, ps in queries for p in ps})
    for i, ph in enumerate(info["phrases"]):
        known = ref.known(ph, c.live)
        assert bool(info["known"][i]) == known, ph
        lo, hi = int(info["ptf_off"][i]), int(info["ptf_off"][i + 1])
        if not known:
            assert info["drivers"][i] == -1 and lo == hi and held[i] == 0
            continue
        counts = [len(ref.holders[t]) for t in ph]
        assert info["drivers"][i] == ph[int(np.argmin(counts))], ph          # fewest postings, ties to the earlier
        rows = np.asarray(ref.holders[int(info["drivers"][i])])               # the driver's CSR list: sorted by row
        want = np.where(visible[rows], ref.tf(list(ph), slop)[rows], 0)
        assert hi - lo == rows.size and np.array_equal(ptf[lo:hi], want), (ph, np.nonzero(ptf[lo:hi] != want)[0][:8])
        assert held[i] == int((want > 0).sum()), ph
    # the bitmaps: rows holding every phrase of the query; every row below n without phrases
    maps = info["bitmaps"].cpu().numpy().view(np.uint32)
    assert maps.shape == (B, 4 * ((c.n + 127) // 128))
    for b, (_, phrases) in enumerate(queries):
        flags = np.ones(c.n, bool)
        for ph in phrases:
            flags &= (visible & (ref.tf(list(ph), slop) > 0)) if ref.known(ph, c.live) else False
        assert np.array_equal(maps[b], R.bitmap(flags, maps.shape[1])), b
    # the scores and the hits
    got_s, got_r = got_s.cpu().numpy(), got_r.cpu().numpy()
    assert got_s.shape == (B, k) and got_s.dtype == np.float32 and got_r.dtype == np.int64
    for b in range(B):
        acc, hit = c.scored(b % len(c.pool) if B > 3 else c.pool.index(queries[b]), slop, mode, use_where)
        bm25_ref.assert_topk(got_s[b], got_r[b], acc, hit, visible, k)
        if mode == "require" and queries[b][1] and all(ref.known(p, c.live) for p in queries[b][1]):
            want_rows = np.nonzero(hit & visible)[0]
            if want_rows.size <= k:          # a query returns exactly the rows that hold its phrases
                assert sorted(got_r[b][got_r[b] >= 0].tolist()) == want_rows.tolist()


def test_overflow_rerun(dev):
    """every row holds the phrase and n exceeds the candidate slots of a query: the overflow re-run answers"""
    from multimodal_rag_amd.lexical import LexicalIndex, bm25_phrase_workspace_bytes

    n = 16384 + limits()["score_rows"] + 5
    seqs = [[A, B_] + [C] * (r * 7 % 11) for r in range(n)]
    lx = LexicalIndex(dev)
    lx.append_sequences(seqs)
    ref = R.PhraseRef(seqs)
    live = np.ones(n, bool)
    queries = [([], [(A, B_)]), ([C], []), ([], [(B_, A)])]
    q_off, q_terms, q_phrases = flat(queries)
    got_s, got_r, info = lx.topk_phrase_ids(q_off, q_terms, q_phrases, 5)
    assert info["rows"].cpu().tolist() == [n, 0] and bm25_phrase_workspace_bytes(3, n, 5) > 16384 * 8 * 3
    got_s, got_r = got_s.cpu().numpy(), got_r.cpu().numpy()
    for b, (loose, phrases) in enumerate(queries):
        acc, hit = ref.scores(loose, [list(p) for p in phrases], live)
        bm25_ref.assert_topk(got_s[b], got_r[b], acc, hit, live, 5)
    assert (got_r[0] >= 0).all() and (got_r[2] == -1).all()
    assert all(len(seqs[r]) == 2 for r in got_r[0])          # the shortest rows score highest


def test_scores_are_bit_identical_alone_in_a_batch_and_twice(dev, corpus, lex):
    queries = corpus.pool
    bits = bits_of(corpus.live & corpus.where, dev)
    for mode in ("require", "prefer"):
        q_off, q_terms, q_phrases = flat(queries)
        s1, r1, _ = lex.topk_phrase_ids(q_off, q_terms, q_phrases, 21, bits, slop=1, phrase_mode=mode)
        s2, r2, _ = lex.topk_phrase_ids(q_off, q_terms, q_phrases, 21, bits, slop=1, phrase_mode=mode)
        assert torch.equal(s1, s2) and torch.equal(r1, r2)
        for b in (0, 1, 3, corpus.four, len(queries) - 1):
            o, t, p = flat(queries[b: b + 1])
            s, r, _ = lex.topk_phrase_ids(o, t, p, 21, bits, slop=1, phrase_mode=mode)
            assert torch.equal(s[0], s1[b]) and torch.equal(r[0], r1[b]), (mode, b)
        shuffled = list(reversed(queries))
        o, t, p = flat(shuffled)
        s3, r3, _ = lex.topk_phrase_ids(o, t, p, 21, bits, slop=1, phrase_mode=mode)
        assert torch.equal(s3.flip(0), s1) and torch.equal(r3.flip(0), r1)


def test_a_batch_without_phrases_is_topk_ids_bit_for_bit(dev, corpus, lex):
    queries = [([A, B_], []), ([C], []), ([D, 4, 5], []), ([], []), ([A], []), ([Z, K0], []), (list(range(8)), [])]
    q_off, q_terms, q_phrases = flat(queries)
    for k, bits in ((21, None), (4096, bits_of(corpus.live & corpus.where, dev)), (1, bits_of(corpus.live, dev))):
        want_s, want_r = lex.topk_ids(q_off, q_terms, k, bits)
        for mode in ("require", "prefer"):
            s, r, info = lex.topk_phrase_ids(q_off, q_terms, q_phrases, k, bits, slop=3, phrase_mode=mode)
            assert torch.equal(s, want_s) and torch.equal(r, want_r), (k, mode)
            assert info["phrases"] == [] and info["ptf_off"].tolist() == [0]
    assert (want_r[3] == -1).all()


def test_python_argument_checks(dev, lex):
    q_off, q_terms, q_phrases = flat([([A], [(A, B_)])])
    for bad in (dict(slop=17), dict(slop=-1), dict(phrase_mode="must"), dict(k=0), dict(k=4097)):
        kw = dict(k=5, slop=0, phrase_mode="require")
        kw.update(bad)
        with pytest.raises(ValueError):
            lex.topk_phrase_ids(q_off, q_terms, q_phrases, kw.pop("k"), None, **kw)
    for phrases in ([[tuple(range(9))]], [[()]], [[(A, N_TERMS)]], [[(A,), (B_,), (C,), (D,), (4,)]]):
        with pytest.raises(ValueError):
            lex.topk_phrase_ids(q_off, q_terms, phrases, 5)
    with pytest.raises(ValueError):
        lex.append_postings(np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.int32))


# ---- the index, on texts -----------------------------------------------------------------------------------------------------
DOCS = [
    "new york is a big city",
    "york is new to me",
    "the new city of york",
    "error code 0x80070005 occurred during setup",
    "code error: 0x80070005",
    "the force majeure clause applies",
    "majeure force",
    "to be or not to be that is the question",
    "new york new york",
    "a big city is new",
    "not to be or to be",
    "the clause applies to the city",
] + [f"filler document number {i} about retrieval and ranking" for i in range(28)]
DIM = 32
HOLDS_NEW_YORK = [0, 8]


def unit_rows(n, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, DIM)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def make_index(dev, docs=DOCS, ids=None):
    from multimodal_rag_amd.index import VectorIndex

    idx = VectorIndex(DIM, dtype=torch.float32, device=dev)
    idx.add(unit_rows(len(docs), 0), documents=list(docs),
            metadatas=[{"g": i % 3, "ny": int("new york" in d)} for i, d in enumerate(docs)],
            ids=ids or [f"id{i}" for i in range(len(docs))])
    return idx


@pytest.fixture(scope="module")
def index(dev):
    return make_index(dev)


def test_lazy_build_and_the_query_language(index):
    plain = index.lexical_query(['"new york"', "new york"], n_results=10)
    assert plain["ids"][0] == plain["ids"][1] and "phrases" not in plain            # quotes are punctuation today
    assert index.lexical_enabled and not index.positions_enabled and index.positions_bytes() == 0
    none = index.lexical_query(["new york"], n_results=10, phrases=True)
    assert none["phrases"] == [[]] and not index.positions_enabled                   # no phrase in the batch: no plane
    assert {k: v for k, v in none.items() if k != "phrases"} == index.lexical_query(["new york"], n_results=10)
    got = index.lexical_query(['"new york"', 'big "New York!" city', "“force majeure”", '"york new"',
                               '"quantum york"', '"to be or not to be"', 'city "new york" "big city"'],
                              n_results=10, phrases=True)
    assert index.positions_enabled and index.positions_bytes() > 0 and index._lex.position_builds == 1
    assert sorted(got["ids"][0]) == ["id0", "id8"] and got["ids"][0][0] == "id8"     # two starts in the shorter row
    assert sorted(got["ids"][1]) == ["id0", "id8"] and got["ids"][1][0] == "id0"     # the loose terms add score
    assert got["ids"][2] == ["id5"] and got["ids"][3] == ["id8"] and got["ids"][4] == []
    assert got["ids"][5] == ["id7"] and got["ids"][6] == ["id0"]
    assert got["phrases"][0] == [{"text": "new york", "terms": ["new", "york"], "known": True, "rows": 2}]
    assert got["phrases"][4] == [{"text": "quantum york", "terms": ["quantum", "york"], "known": False, "rows": 0}]
    assert [p["rows"] for p in got["phrases"][6]] == [2, 2]
    assert got["phrases"][5][0]["terms"] == ["to", "be", "or", "not", "to", "be"]
    # slop and mode
    assert sorted(index.lexical_query(['"new york"'], n_results=10, phrases=True, slop=1)["ids"][0]) == ["id0", "id8"]
    assert sorted(index.lexical_query(['"new york"'], n_results=10, phrases=True, slop=2)["ids"][0]) == \
        ["id0", "id2", "id8"]
    prefer = index.lexical_query(['city "new york"'], n_results=40, phrases=True, phrase_mode="prefer")
    assert set(prefer["ids"][0]) == {"id0", "id8", "id2", "id9", "id11"} and prefer["ids"][0][0] == "id0"
    where = index.lexical_query(['"new york"'], n_results=10, phrases=True, where={"g": 0})
    assert where["ids"] == [["id0"]] and where["phrases"][0][0]["rows"] == 1
    # fuzzy rewrites the loose terms, never a phrase's
    fz = index.lexical_query(['citty "new york"', '"new yrok"'], n_results=10, phrases=True, fuzzy="auto")
    assert fz["corrections"] == [[{"term": "citty", "matched": "city", "edits": 1}], []]
    assert fz["ids"][0][0] == "id0" and fz["ids"][1] == [] and fz["phrases"][1][0]["known"] is False
    for bad in ('"a b c d e f g h i"', '"a" "b" "c" "d" "e"'):
        with pytest.raises(ValueError):
            index.lexical_query([bad], n_results=5, phrases=True)
    with pytest.raises(ValueError):
        index.lexical_query(['"new york"'], n_results=5, phrases=True, slop=17)
    assert index._lex.position_builds == 1


def rows_as_tokens(idx):
    """every row's token sequence, rebuilt from the forward log, the positions plane and the lexicon's strings"""
    lex = idx._lex
    names = lex.lexicon.terms(0, len(lex.lexicon))
    P = lex.n_postings
    off = lex._fwd_off[: lex.n + 1].cpu().numpy()
    term = lex._fwd_term[:P].cpu().numpy()
    tf = lex._fwd_tf[:P].cpu().numpy()
    pos_off = lex._pos_off[: P + 1].cpu().numpy()
    pos = lex._pos[: lex._pos_total].cpu().numpy()
    assert np.array_equal(np.diff(pos_off), tf) and pos_off[0] == 0 and pos_off[-1] == lex._pos_total
    out = []
    for r in range(lex.n):
        seq = {}
        for j in range(off[r], off[r + 1]):
            for p in pos[pos_off[j]: pos_off[j + 1]]:
                seq[int(p)] = names[term[j]]
        assert sorted(seq) == list(range(len(seq)))
        out.append([seq[p] for p in range(len(seq))])
    return out


def test_lifecycle_equals_a_fresh_index(dev):
    from multimodal_rag_amd.lexical import analyze

    idx = make_index(dev, DOCS[:20])
    queries = ['"new york"', 'city "big city"', '"to be" question', '"retrieval and ranking" filler', '"force majeure"']
    first = idx.lexical_query(queries, n_results=10, phrases=True)
    assert idx.positions_enabled and sorted(first["ids"][0]) == ["id0", "id8"]
    idx.add(unit_rows(6, 3), documents=DOCS[20:26], metadatas=[{"g": 0, "ny": 0}] * 6, ids=[f"id{i}" for i in range(20, 26)])
    assert rows_as_tokens(idx) == [analyze(d) for d in DOCS[:26]]                    # append keeps the plane current
    idx.delete(ids=["id8", "id3", "id21"])
    gone = idx.lexical_query(queries, n_results=10, phrases=True)
    assert gone["ids"][0] == ["id0"] and gone["phrases"][0][0]["rows"] == 1         # the alive bits mask the match
    idx.compact()
    extra = ["new york once more", "the question of new york"]
    idx.add(unit_rows(2, 4), documents=extra, metadatas=[{"g": 1, "ny": 1}] * 2, ids=["x0", "x1"])
    kept = [i for i in range(26) if i not in (8, 3, 21)]
    docs = [DOCS[i] for i in kept] + extra
    ids = [f"id{i}" for i in kept] + ["x0", "x1"]
    assert rows_as_tokens(idx) == [analyze(d) for d in docs]
    fresh = make_index(dev, docs, ids)
    got = idx.lexical_query(queries, n_results=10, phrases=True, slop=1)
    want = fresh.lexical_query(queries, n_results=10, phrases=True, slop=1)
    assert rows_as_tokens(fresh) == rows_as_tokens(idx)
    for key in ("ids", "lexical_scores", "phrases", "documents"):
        assert got[key] == want[key], key                                            # bit-equal scores
    assert sorted(got["ids"][0]) == ["id0", "x0", "x1"] and idx._lex.position_builds == 1
    idx.reset()
    assert not idx.positions_enabled and idx.positions_bytes() == 0
    idx.add(unit_rows(2, 5), documents=["a new start", "new york again"], ids=["r0", "r1"])
    assert idx.lexical_query(['"new york"'], n_results=5, phrases=True)["ids"] == [["r1"]]


def test_hybrid_require_takes_the_dense_leg_from_the_phrase_rows(index, monkeypatch):
    from multimodal_rag_amd.config import settings

    n = len(DOCS)
    q = unit_rows(4, 9)
    texts = ['"new york"', "big city", 'city "new york"', '"quantum york" city']
    plain = index.hybrid_query(q, texts, n_results=n)
    got = index.hybrid_query(q, texts, n_results=n, phrases=True)
    assert set(got) == set(plain) | {"phrases"}
    assert sorted(got["ids"][0]) == sorted(got["ids"][2]) == ["id0", "id8"] and got["ids"][3] == []
    for key in ("ids", "hybrid_scores", "lexical_scores"):
        assert got[key][1] == plain[key][1], key                    # a query without phrases is answered as before
    assert got["distances"][1] == pytest.approx(plain["distances"][1], abs=1e-6)     # (by the filtered scan's kernel)
    # the dense side is the filtered scan over the same rows: the metadata flag "ny" marks them
    f_s, f_r = index.filtered_search(q[:1], n, {"ny": 1})
    dense = {f"id{r}": 1.0 - s for s, r in zip(f_s[0].cpu().tolist(), f_r[0].cpu().tolist()) if r >= 0}
    assert sorted(dense) == ["id0", "id8"]
    assert dict(zip(got["ids"][0], got["distances"][0])) == pytest.approx(dense, abs=1e-6)
    order = [i for i, _ in sorted(dense.items(), key=lambda kv: kv[1])]
    lex_order = index.lexical_query(texts[:1], n_results=n, phrases=True)["ids"][0]
    want = bm25_ref.rrf([int(i[2:]) for i in order], [int(i[2:]) for i in lex_order], settings.MMRAG_HYBRID_RRF_K)
    assert got["ids"][0] == [f"id{r}" for r, _ in want] and got["hybrid_scores"][0] == [s for _, s in want]
    # `where` and the tombstones restrict both legs
    assert index.hybrid_query(q[:1], texts[:1], n_results=n, phrases=True, where={"g": 2})["ids"] == [["id8"]]
    # one bitmap per launch gives the same answer
    monkeypatch.setattr(settings, "MMRAG_FILTER_BITMAP_BYTES", 1)
    cut = index.hybrid_query(q, texts, n_results=n, phrases=True)
    monkeypatch.undo()
    for key in got:
        if key == "distances":
            assert all(a == pytest.approx(b, abs=1e-6) for a, b in zip(cut[key], got[key]))
        else:
            assert cut[key] == got[key], key
    # prefer: the dense leg is today's, so every row is fused in
    prefer = index.hybrid_query(q, texts, n_results=n, phrases=True, phrase_mode="prefer")
    for b in range(4):
        assert sorted(prefer["ids"][b]) == sorted(plain["ids"][b])
        assert dict(zip(prefer["ids"][b], prefer["distances"][b])) == dict(zip(plain["ids"][b], plain["distances"][b]))
    at = prefer["ids"][0].index("id8")
    assert prefer["lexical_scores"][0][at] > 0 and prefer["phrases"] == got["phrases"]


def test_query_endpoint_with_phrases(dev):
    from fastapi.testclient import TestClient

    from multimodal_rag_amd.embedder import EmbeddingManager
    from multimodal_rag_amd.server import create_app

    m = EmbeddingManager()
    with TestClient(create_app(embedder=m)) as c:
        bodies = ["New York is a big city. " * 3, "York is new to me, and the city is big. " * 3,
                  "A new clause applies in the city of York. " * 3]
        for i, body in enumerate(bodies):
            r = c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
        plain = c.post("/query", json={"query": 'the "new york" city', "top_k": 3, "hybrid": True})
        assert plain.status_code == 200 and len(plain.json()["sources"]) == 3 and "phrases" not in plain.json()
        r = c.post("/query", json={"query": 'the "new york" city', "top_k": 3, "hybrid": True, "phrases": True})
        assert r.status_code == 200, r.text
        out = r.json()
        rows = out["phrases"][0]["rows"]
        assert out["phrases"] == [{"text": "new york", "terms": ["new", "york"], "known": True, "rows": rows}]
        assert 1 <= len(out["sources"]) <= min(3, rows) and all("hybrid_score" in s for s in out["sources"])
        assert m.collection.positions_enabled and m.collection.positions_bytes() > 0
        r = c.post("/query", json={"query": '"new york"', "top_k": 3, "hybrid": True, "phrases": True, "slop": 16})
        assert r.status_code == 200 and r.json()["phrases"][0]["rows"] >= 1
        assert c.post("/query", json={"query": '"new york"', "top_k": 3, "phrases": True}).status_code == 400
