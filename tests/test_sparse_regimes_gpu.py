"""GPU: the learned sparse leg at its edges, on the structured inputs of tests/sparse_regimes.py whose answers are fully
determined (tests/test_sparse_regimes_cpu.py proves the generators).

  impact   mmrag_impact_topk (csrc/sparse_score.hip) on corpora by signature class: rows and integer scores exactly,
           alone and inside a batch of 130 between queries of other regimes, under the test hook's small capacity and
           without bound stages, and the REGIME itself by the main pass's per-query counters (the first B words of the
           workspace, csrc/candidate_select.h)
  pool     mmrag_sparse_pool (csrc/sparse_expand.hip) bit for bit: the query shape (many pieces per tile), a real
           vocabulary with the run of vocabulary tiles taken from the grid, padded pitches, dim 128 and 1024
  select   mmrag_sparse_select on a real vocabulary: long tie runs cut at wave boundaries, +inf / NaN / saturation,
           scale 1024, skip bits at word edges
  rows     the token rows of mmrag_sparse_expand_forward (csrc/encoder.hip: both encoder bodies, then the masked-LM
           tail) against float64 over the fp16-rounded matrices

Tolerance of the token rows.  The rows are un-normalised LayerNorm outputs in fp16; rounding is the only error source.
Measured on an MI355X against float64 (worst over the tokens of a case, relative row error |got - want|_2 / |want|_2):
see EXPAND_MEASURED below, and DESIGN.md's sparse section.  ROW_TOL is 4 x the worst of them rounded up to one
significant digit (the margin covers other seeds and shapes)."""
import numpy as np
import pytest
import torch

import lexical_regimes as LR
import sparse_ref as R
import sparse_regimes as SR
from tests.test_sparse_cpu import E2E_SHAPE, e2e_sequences, e2e_weights

pytestmark = pytest.mark.gpu

# (worst relative row error, lowest cosine) per encoder and length set, as measured: the bound below comes from these
EXPAND_MEASURED = {
    ("e2e", (1,)): (7.659e-04, 0.9999997), ("e2e", (8,)): (1.004e-03, 0.9999995),
    ("e2e", (37,)): (9.416e-04, 0.9999996), ("e2e", (64,)): (1.159e-03, 0.9999993),
    ("e2e", (1, 63, 64, 8)): (1.199e-03, 0.9999993), ("e2e", (1, 63, 37, 64, 8)): (1.199e-03, 0.9999993),
    ("h384", (1,)): (1.007e-03, 0.9999995), ("h384", (8,)): (1.039e-03, 0.9999995),
    ("h384", (37,)): (1.063e-03, 0.9999994), ("h384", (64,)): (1.044e-03, 0.9999995),
    ("h384", (65,)): (1.087e-03, 0.9999994), ("h384", (1, 63, 64, 65, 200)): (1.106e-03, 0.9999994),
    ("h384", (1, 63, 37, 64, 65, 200)): (1.106e-03, 0.9999994),
}
ROW_TOL = 5e-3        # 4 x 1.199e-3 = 4.8e-3, rounded up to one significant digit
ROW_COS = 0.9999      # implied by ROW_TOL: a relative error e costs a cosine about e^2 / 2 = 1.25e-5
assert ROW_TOL == 5e-3 >= 4 * max(e for e, _ in EXPAND_MEASURED.values()) > 4e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return "cuda:0"


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def test_restated_constants(dev):
    from multimodal_rag_amd import _native

    assert _native.sparse_limits() == SR.LIMITS
    for k in (1, 5, 100, 512, 4096):
        assert _native.candidate_capacity(k) == SR.candidate_capacity(k)
    for n in (2049, 16640, 20_000, SR.BIG):
        for k in (1, 5, 512, 4096):
            assert _native.bound_plan(n, k) == SR.bound_plan(n, k)
            assert _native.bound_plan(n, k, 256) == SR.bound_plan(n, k, 256)


# ---------------------------------------------------------------------------------------------------- impact
def new_index(dev, corpus):
    """the corpus appended in two pieces (one when it has a single row)"""
    from multimodal_rag_amd.sparse import ImpactIndex

    off, terms, imps = corpus.log
    idx = ImpactIndex(dev, SR.V)
    m = corpus.n * 2 // 5
    for lo, hi in ((0, m), (m, corpus.n)):
        if hi > lo:
            idx.append(off[lo: hi + 1] - off[lo], terms[off[lo]: off[hi]], imps[off[lo]: off[hi]])
    assert idx.n == corpus.n
    return idx


def search(idx, qs, k, allowed=None, cap=0, dbg=0):
    """(scores [B, k], rows [B, k], the main pass's survivors per query [B]) on the host"""
    alive = None if allowed is None or allowed.all() else torch.from_numpy(LR.alive_words(allowed)).to(idx.device)
    s, r = idx.topk(*SR.pack(qs), k, alive, cap, dbg)
    counts = idx._search_ws[: 4 * len(qs)].view(torch.int32).cpu().numpy().astype(np.int64)
    return s.cpu().numpy(), r.cpu().numpy(), counts


class Regimes:
    """what the impact tests share: one ImpactIndex (and its workspace) per case, the reference scores of every query
    over it, and the first answer of every (case, k)"""

    def __init__(self, dev):
        self.dev, self.index, self.first, self.score, self.answer = dev, {}, {}, {}, {}

    def index_of(self, case):
        if case.id not in self.index:
            self.index[case.id] = new_index(self.dev, SR.build(case).corpus)
        return self.index[case.id]

    def scores(self, case, q):
        key = (case.id, tuple(q[0]), tuple(q[1]))
        if key not in self.score:
            self.score[key] = R.scores(*SR.build(case).corpus.log, SR.V, *q)
        return self.score[key]

    def want(self, case, q, k, allowed=None):
        if allowed is not None:
            return R.topk(self.scores(case, q), k, allowed)
        key = (case.id, tuple(q[0]), tuple(q[1]), k)
        if key not in self.answer:
            self.answer[key] = R.topk(self.scores(case, q), k, SR.build(case).allowed)
        return self.answer[key]

    def run(self, case, k, **hook):
        b = SR.build(case)
        return search(self.index_of(case), [(b.qt, b.qw)], k, b.allowed, **hook)

    def first_run(self, case, k):
        if (case.id, k) not in self.first:
            self.first[(case.id, k)] = self.run(case, k)
        return self.first[(case.id, k)]


@pytest.fixture(scope="module")
def regimes(dev):
    shared = Regimes(dev)
    yield shared
    shared.index.clear()


def assert_answer(got_s, got_r, want):
    assert np.array_equal(got_r, want[1])
    assert np.array_equal(_bits(got_s), _bits(want[0]))


@pytest.mark.parametrize("case", SR.CASES, ids=SR.CASE_IDS)
def test_impact_regimes(regimes, case):
    b = SR.build(case)
    q = (b.qt, b.qw)
    idx = regimes.index_of(case)
    hits = int(((b.level >= 0) & b.allowed).sum())
    batch = [q if i in SR.BATCH_AT else SR.fillers(b)[i % 4] for i in range(SR.BATCH)]
    assert len(batch) == 130
    for k in case.ks:
        cap, stages = SR.bound_plan(case.n, k)
        want = regimes.want(case, q, k)
        named = LR.named_topk(b.level, b.allowed, k)
        assert np.array_equal(want[1][: named.size], named) and (want[1][named.size:] == -1).all()
        # alone
        s, r, cnt = regimes.first_run(case, k)
        assert_answer(s[0], r[0], want)
        # the regime, not just the answer
        print(f"{case.id} k={k}: stages {stages}, survivors {int(cnt[0])} of {hits} matching live rows, {cap} slots")
        if not stages:
            assert cnt[0] == hits
        if case.regime == "few":
            assert stages and cnt[0] <= cap and k <= cnt[0] <= k + 3 and cnt[0] * 16 < case.n
        if case.regime == "all":
            assert stages and cnt[0] == hits > cap
        # in a batch of 130 between queries of other regimes: no bit depends on the batch
        sb, rb, cb = search(idx, batch, k, b.allowed)
        for i in range(SR.BATCH):
            if i in SR.BATCH_AT:
                assert np.array_equal(rb[i], r[0]) and np.array_equal(_bits(sb[i]), _bits(s[0])), i
                assert cb[i] == cnt[0], i
            else:
                assert_answer(sb[i], rb[i], regimes.want(case, batch[i], k))
        assert (rb[1] >= 0).sum() == int(b.allowed[b.lone_row]) and (rb[3] == -1).all()     # one row; nothing
        if case.n > cap and case.layout in ("plateau", "planted:unsampled_blocks"):
            assert cb[4] > cap                                                              # the plateau's term overflows
        # fewer slots than matches (stages, overflow, re-runs of many queries of one call), and no bound stages
        sc, rc, _ = search(idx, batch, k, b.allowed, cap=256)
        assert np.array_equal(rc, rb) and np.array_equal(_bits(sc), _bits(sb))
        sd, rd, cd = regimes.run(case, k, dbg=1)
        assert_answer(sd[0], rd[0], want)
        assert cd[0] == hits
        s2, r2, _ = regimes.run(case, k, cap=256, dbg=1)
        assert_answer(s2[0], r2[0], want)


def test_reverse_sweep_gives_the_same_bits(regimes):
    first = {(case.id, k): regimes.first_run(case, k) for case in SR.CASES for k in case.ks}
    for case in reversed(SR.CASES):
        for k in reversed(case.ks):
            s, r, cnt = regimes.run(case, k)
            f = first[(case.id, k)]
            assert np.array_equal(_bits(s), _bits(f[0])) and np.array_equal(r, f[1]), (case.id, k)
            assert np.array_equal(cnt, f[2]), (case.id, k)


def test_top_of_the_integer_range(regimes):
    case = SR.case("block-edges-top-4099")
    s, r, _ = regimes.first_run(case, 5)
    assert s[0].tolist() == [SR.MAX_SCORE] * 3 + [SR.MAX_SCORE - 255] * 2 and SR.MAX_SCORE == 4_161_600


@pytest.mark.parametrize("case_id", ["block-edges-4099", "word-edges-4099"])
def test_deletes_by_alive_bits_and_compaction(dev, regimes, case_id):
    case = SR.case(case_id)
    b = SR.build(case)
    idx = new_index(dev, b.corpus)
    dead = LR.delete_set(b.level) | ~b.allowed
    live = ~dead
    q = (b.qt, b.qw)
    before = {}
    for k in case.ks:
        s, r, cnt = search(idx, [q], k, live)
        assert_answer(s[0], r[0], regimes.want(case, q, k, live))
        named = LR.named_topk(b.level, live, k)
        assert np.array_equal(r[0][: named.size], named)
        assert cnt[0] == int(((b.level >= 0) & live).sum())
        before[k] = (s, r)
    idx.compact(np.nonzero(live)[0])
    assert idx.n == int(live.sum())
    new_row = np.cumsum(live) - 1
    for k in case.ks:
        s, r, _ = search(idx, [q], k)
        old = before[k][1][0]
        assert np.array_equal(_bits(s), _bits(before[k][0]))                   # the same bits for the same live rows
        assert np.array_equal(r[0], np.where(old >= 0, new_row[np.maximum(old, 0)], -1))


# ---------------------------------------------------------------------------------------------------- pool
def pool_on(dev, pc, vrun=0, tok=None, cu=None, E=None):
    from multimodal_rag_amd import _native

    t = torch.from_numpy(pc.tok if tok is None else tok).to(dev)
    c = torch.from_numpy(np.asarray(pc.cu if cu is None else cu, np.int32)).to(dev)
    e = torch.from_numpy(pc.E).to(dev) if E is None else E
    return _native.sparse_pool(t, c, e, pc.dim, vrun=vrun).cpu().numpy()


@pytest.mark.parametrize("name", SR.POOL_CASES)
def test_pool_bit_exact_in_every_shape(dev, name):
    pc = SR.pool_case(name)
    ref = SR.pool_ref(pc)
    E = torch.from_numpy(pc.E).to(dev)
    got = pool_on(dev, pc, E=E)
    assert got.shape == ref.shape
    assert np.array_equal(_bits(got), _bits(ref))
    if pc.signed:
        neg = np.arange(pc.cu.size - 1) % 2 == 0
        assert (got[neg] < 0).all() and (got[~neg] > 0).all()
    T, Vt = pc.tok.shape[0], pc.E.shape[0]
    vt = (Vt + SR.PT - 1) // SR.PT
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    print(f"pool {name}: T={T} V={Vt} dim={pc.dim}, {cus} CUs, default run of vocabulary tiles "
          f"{SR.default_vrun(T, Vt, cus)}")
    if name == "real_vocab" and cus <= 256:
        assert SR.default_vrun(T, Vt, cus) > 1          # the run taken from the grid, as in production
    # the bits do not depend on the run
    for vrun in sorted({1, 3, SR.SP_VRUN, vt}):
        assert np.array_equal(_bits(pool_on(dev, pc, vrun, E=E)), _bits(got)), vrun
    if name == "eights":                                # nor on the packing: chunks alone, one per call
        for c in SR.EIGHTS_SAMPLE:
            rows = np.ascontiguousarray(pc.tok[pc.cu[c]: pc.cu[c + 1]])
            one = pool_on(dev, pc, tok=rows, cu=[0, rows.shape[0]], E=E)
            assert np.array_equal(_bits(one[0]), _bits(got[c])), c


# ---------------------------------------------------------------------------------------------------- select
@pytest.fixture(scope="module")
def select_inputs(dev):
    pooled, bias, skip, scale, _ = SR.select_case()
    return (torch.from_numpy(pooled).to(dev), torch.from_numpy(bias).to(dev),
            torch.from_numpy(R.bool_to_bits(skip)).to(dev), R.impacts(pooled, bias, scale), skip, scale)


@pytest.mark.parametrize("m", SR.SELECT_MS)
def test_select_exact_on_a_real_vocabulary(dev, select_inputs, m):
    from multimodal_rag_amd import _native

    d_pooled, d_bias, d_skip, imp, skip, scale = select_inputs
    ref_cnt, ref_terms, ref_imp = R.select_batch(imp, m, skip)
    cnt, terms, imps = _native.sparse_select(d_pooled, d_bias, scale, m, d_skip)
    assert np.array_equal(cnt.cpu().numpy(), ref_cnt)
    assert np.array_equal(terms.cpu().numpy(), ref_terms)
    assert np.array_equal(imps.cpu().numpy(), ref_imp)
    assert ref_cnt.tolist() == [m, m, min(m, 10), m]
    # without skip bits the would-be 200s under them win
    ref0 = R.select_batch(imp, m)
    got0 = _native.sparse_select(d_pooled, d_bias, scale, m)
    for g, w in zip(got0, ref0):
        assert np.array_equal(g.cpu().numpy(), w)
    assert (ref0[2][0] == 200).all()


# ---------------------------------------------------------------------------------------------------- expansion rows
H384 = (2, 384, 12, 1536, 1000, 256)       # tests/test_late_gpu.py's h384 shape: the folded-LayerNorm body for T <= 64
LENGTH_SETS = [[1], [8], [37], [64], [65], [1, 63, 64, 65, 200], [1, 63, 37, 64, 65, 200]]


def head_weights(H, V, seed):
    g = np.random.default_rng(seed)
    return {"cls.predictions.transform.dense.weight": (g.standard_normal((H, H)) * 0.05).astype(np.float32),
            "cls.predictions.transform.dense.bias": (g.standard_normal(H) * 0.05).astype(np.float32),
            "cls.predictions.transform.LayerNorm.weight": (1.0 + g.standard_normal(H) * 0.1).astype(np.float32),
            "cls.predictions.transform.LayerNorm.bias": (g.standard_normal(H) * 0.1).astype(np.float32),
            "cls.predictions.bias": (g.standard_normal(V) * 0.1).astype(np.float32)}


class Expander:
    def __init__(self, dev, name):
        from multimodal_rag_amd.encoder import EncoderConfig
        from multimodal_rag_amd.sparse import DeviceSparseEncoder

        self.name = name
        if name == "e2e":
            self.shape, w = E2E_SHAPE, e2e_weights()
        else:
            from oracle import encoder_oracle as E

            self.shape = H384
            L, H, heads, inter, V, max_pos = H384
            w = E.make_bert_weights(E.BertShape(L, H, heads, inter, vocab=V, max_pos=max_pos), 31)
            w.update(head_weights(H, V, 32))
        L, H, heads, inter, V, max_pos = self.shape
        cfg = EncoderConfig(name + "-mlm", L, H, heads, inter, V, max_pos, max_pos, "cls", 1e-12)
        self.enc = DeviceSparseEncoder(cfg, w, dev, scale=64.0, skip_ids=list(range(5)))
        self.w, self.w16, self._rows = w, R.round_matrices_fp16(w), {}

    def sequence(self, n):
        """the sequence of n tokens: one per length, whatever batch it sits in"""
        return np.random.default_rng(1000 + n).integers(5, self.shape[4], n).tolist()

    def want(self, n):
        """float64 token rows of the sequence of n tokens over the fp16-rounded matrices, computed once"""
        if n not in self._rows:
            L, _, heads = self.shape[:3]
            self._rows[n] = R.mlm_transform(R.bert_hidden(self.w16, self.sequence(n), L, heads, 1e-12), self.w16, 1e-12)
        return self._rows[n]

    def rows(self, lens):
        seqs = [self.sequence(n) for n in lens]
        ids = np.zeros((len(seqs), max(lens)), np.int32)
        for i, s in enumerate(seqs):
            ids[i, : len(s)] = s
        with self.enc._launch_lock:
            tok, cu = self.enc._token_rows(ids, np.asarray(lens, np.int32))
            tok = tok.float().cpu().numpy().astype(np.float64)
        assert cu.cpu().tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist() and tok.shape == (sum(lens), self.shape[1])
        return tok


@pytest.fixture(scope="module")
def expanders(dev):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Expander(dev, name)
        return cache[name]
    yield get
    cache.clear()


def row_errors(got, want):
    rel = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return float(rel.max()), float(cos.min())


@pytest.mark.parametrize("lens", LENGTH_SETS, ids=["-".join(map(str, x)) for x in LENGTH_SETS])
@pytest.mark.parametrize("name", ["e2e", "h384"])
def test_expansion_rows_vs_float64(expanders, name, lens):
    """h384: one sequence of <= 64 tokens takes the folded-LayerNorm body, everything else the general one; at
    E2E_SHAPE (hidden 128, which the folded body does not serve, and 64 positions) every length set that fits runs
    the general body.  The sequence of 37 tokens is the same in [37] and inside the batch: both its folded and its
    general rows are held against the same float64 rows."""
    x = expanders(name)
    if max(lens) > x.shape[5]:
        lens = [n for n in lens if n <= x.shape[5]] + [8]       # E2E_SHAPE has 64 positions: the lengths that fit
    got = x.rows(lens)
    at, worst, lowest = 0, 0.0, 1.0
    for n in lens:
        rel, cos = row_errors(got[at: at + n], x.want(n))
        print(f"{name} {lens}: sequence of {n}: worst relative row error {rel:.3e}, lowest cosine {cos:.7f}")
        worst, lowest = max(worst, rel), min(lowest, cos)
        at += n
    print(f"{name} {lens}: worst relative row error {worst:.3e}, lowest cosine {lowest:.7f} (bound {ROW_TOL:g})")
    assert worst <= ROW_TOL and lowest >= ROW_COS, (worst, lowest)


def test_impacts_through_the_single_sequence_path(expanders):
    """tests/test_sparse_gpu.py's end-to-end assertions with every sequence expanded ALONE (T <= 64)"""
    x = expanders("e2e")
    enc, w = x.enc, x.w
    L, H, heads, inter, V, max_pos = E2E_SHAPE
    seqs = e2e_sequences()
    pooled = R.expand(R.round_matrices_fp16(w), seqs, L, heads, 1e-12)
    ws = R.weights(pooled, w["cls.predictions.bias"], 64.0)
    ws[:, :5] = 0.0                                             # the skipped ids
    ref_imp = np.minimum(np.rint(ws), 255).astype(np.int64)
    checked = 0
    for m in (1, 2, 4, 8, 32, 256):
        for i, seq in enumerate(seqs):
            off, t, q = enc.expand_ids(np.asarray([seq], np.int32), np.asarray([len(seq)], np.int32), m)
            assert off.tolist() == [0, t.size] and t.size == q.size
            assert (np.diff(t) > 0).all() and t.size <= m and (q >= 1).all() and (t >= 5).all()
            assert (np.abs(q - ref_imp[i, t]) <= 1).all(), (m, i)
            order = np.sort(ws[i])[::-1]
            n_pos = int((ref_imp[i] >= 1).sum())
            if n_pos > m and order[m - 1] - order[m] > 1.0 and order[m - 1] >= 1.5:
                assert set(t.tolist()) == set(np.argsort(-ws[i], kind="stable")[:m].tolist()), (m, i)
                checked += 1
            elif n_pos <= m and (np.abs(ws[i] - 0.5) > 0.5)[ref_imp[i] <= 1].all():
                assert set(t.tolist()) == set(np.nonzero(ref_imp[i] >= 1)[0].tolist()), (m, i)
                checked += 1
            if t.size and n_pos > m:
                assert ws[i, t].min() >= order[m - 1] - 1.0, (m, i)
    assert checked > 0
