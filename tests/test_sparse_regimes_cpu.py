"""CPU: the generators of tests/sparse_regimes.py and their expected answers, before any kernel is involved.

For every case the GPU file runs: the rows the layout names are the reference's top-k (tests/sparse_ref.py), the levels
give strictly rising integer scores, the sampled / unsampled layouts put their winners where the restated plan and
block mapping say, the pool planes have the pieces per tile and tiles per workgroup they claim and two formulations
of their maxima agree, the select grid keeps clear of half-integers and its ties end where the pins say, and the
restated constants are the library's."""
import os

import numpy as np
import pytest

import lexical_regimes as LR
import sparse_ref as R
import sparse_regimes as SR


@pytest.fixture(scope="module")
def native():
    from multimodal_rag_amd import _native, build

    build.build(verbose=False)
    _native.lib()
    return _native


PLAN_POINTS = [(n, k) for n in (1, 100, 2048, 2049, 4099, 16384, 16385, 16640, 20_000, 140_000, 1_000_000, 5_000_000)
               for k in (1, 5, 100, 512, 513, 4096)]


def test_restated_constants(native):
    assert native.sparse_limits() == SR.LIMITS
    assert SR.IMP_R == LR.SCORE_R and SR.IMP_R % SR.PT == 0
    assert (R.MAX_CHUNK_TOKENS, R.MAX_TERMS, R.MAX_QUERY_TERMS) == (
        native.MAX_SPARSE_CHUNK_TOKENS, native.MAX_SPARSE_TERMS, native.MAX_SPARSE_QUERY_TERMS)
    for k in (1, 5, 100, 512, 513, 4096):
        assert native.candidate_capacity(k) == SR.candidate_capacity(k)
    for n, k in PLAN_POINTS:
        assert native.bound_plan(n, k) == SR.bound_plan(n, k), (n, k)
        assert native.bound_plan(n, k, 256) == SR.bound_plan(n, k, 256), (n, k)
        assert native.bound_plan(n, k, 0, 1) == SR.bound_plan(n, k, 0, True), (n, k)


def test_limits_export_is_internal():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "mmrag_internal_sparse_limits" not in open(os.path.join(root, "include", "mmrag.h")).read()


def test_the_plans_the_cases_are_built_on():
    assert SR.bound_plan(16640, 5) == (16384, [96])
    assert SR.stage_blocks(16640, 96) == [0, 1, 3, 4, 6, 7] and SR.blocks(16640) == 9
    assert SR.sampled_blocks(16640, 5) == ([0, 1, 3, 4, 6, 7], [2, 5, 8])
    assert SR.bound_plan(SR.BIG, 512) == (16384, [96, 137]) and SR.blocks(SR.BIG) == 69
    assert SR.stage_blocks(SR.BIG, 96) == [0, 11, 23, 34, 46, 57]
    assert SR.stage_blocks(SR.BIG, 137) == [0, 7, 15, 23, 30, 38, 46, 53, 61]
    every, never = SR.sampled_blocks(SR.BIG, 512)
    assert every == [0, 23, 46] and len(never) == 69 - 12 and 68 in never
    # the second stage of (140 000, 512) holds more rows than a stage has slots: on a plateau the stage overflows
    assert 9 * SR.IMP_R == 18432 > SR.candidate_capacity(512) == 16384
    # the main pass visits every block, in order
    for n in (1, 2049, 16640, SR.BIG):
        assert SR.stage_blocks(n, (n + SR.PT - 1) // SR.PT) == list(range(SR.blocks(n)))
    assert SR.bound_plan(4099, 512) == (16384, []) and SR.bound_plan(16640, 4096) == (131072, [])


@pytest.mark.parametrize("case", SR.CASES, ids=SR.CASE_IDS)
def test_names_are_the_reference_answer(case):
    from multimodal_rag_amd.sparse import check_sparse_rows

    b = SR.build(case)
    off, terms, imps = b.corpus.log
    check_sparse_rows(off, terms, imps, SR.V, case.n, R.MAX_TERMS)
    check_sparse_rows(*SR.pack([(b.qt, b.qw)]), SR.V, 1, R.MAX_QUERY_TERMS)
    assert len(b.qt) == case.T and case.T in (1, R.MAX_QUERY_TERMS)
    if case.n == SR.BIG:
        assert off[-1] <= 3 * case.n                        # two or three pairs per row
    score = R.scores(off, terms, imps, SR.V, b.qt, b.qw)
    assert np.array_equal(score, b.corpus.scores(b.qt, b.qw))          # by postings and by class
    assert np.array_equal(score > 0, b.level >= 0)
    steps = SR.level_scores(b)
    assert all(x < y for x, y in zip(steps, steps[1:])) and steps[0] > 0 and steps[-1] <= SR.MAX_SCORE
    hits = int(((b.level >= 0) & b.allowed).sum())
    for k in case.ks:
        s, r = R.topk(score, k, b.allowed)
        want = LR.named_topk(b.level, b.allowed, k)
        assert want.size == min(k, hits)
        assert np.array_equal(r[: want.size], want) and (r[want.size:] == -1).all()
        assert np.array_equal(s[: want.size].astype(np.int64), score[want])       # float32 holds every score
    # the lone row, and the queries of the batch
    assert (terms == SR.LONE).sum() == 1 and (terms == SR.NONE).sum() == 0
    if case.T > 1 and case.mode != "top":
        assert SR.LONE in b.qt and b.qt == sorted(b.qt) and b.level[b.lone_row] == b.level.max()
        assert (b.level == b.level.max()).sum() == 1
        held = set(terms.tolist())
        assert sum(t not in held for t in b.qt) >= 50                 # most query terms have no posting
    low, lone, top, none = (R.scores(off, terms, imps, SR.V, t, w) for t, w in SR.fillers(b))
    assert np.array_equal(low > 0, b.level >= 0)                      # the plateau's term: every matching row
    assert (lone > 0).sum() == 1 and lone[b.lone_row] == 2 * 255 and not none.any() and (top > 0).sum() > 0
    if case.regime == "all":
        assert hits > SR.candidate_capacity(case.plan_k or case.ks[0])


def test_top_of_the_integer_range():
    b = SR.build(SR.case("block-edges-top-4099"))
    steps = SR.level_scores(b)
    assert steps == [255, SR.MAX_SCORE - 2 * 255, SR.MAX_SCORE - 255, SR.MAX_SCORE] and SR.MAX_SCORE == 4_161_600
    assert all(float(np.float32(s)) == s for s in steps) and SR.MAX_SCORE < 2 ** 24
    top = np.nonzero(b.level == 3)[0]
    assert top.size == 3 and all(len(b.corpus.classes[c]) >= R.MAX_QUERY_TERMS for c in b.corpus.row_class[top])
    below = b.corpus.classes[b.corpus.row_class[np.nonzero(b.level == 2)[0][0]]]
    assert sorted(i for _, i in below) == [254] + [255] * 63


@pytest.mark.parametrize("case_id", ["sampled-16640", "unsampled-16640", "sampled-140000", "unsampled-140000"])
def test_sampled_layouts_are_where_they_claim(case_id):
    """recomputed from the plan alone: which rows each stage sees, and what tau the stages can reach"""
    case = SR.case(case_id)
    b = SR.build(case)
    n, k = case.n, case.plan_k
    score = b.corpus.scores(b.qt, b.qw)
    win = np.nonzero(b.level >= 1)[0]
    assert win.size == k + 3
    cap, stages = SR.bound_plan(n, k)
    assert stages and n > cap
    true_kth = np.sort(score)[::-1][k - 1]
    tau = -np.inf
    for tiles in stages:
        walk = (tiles + 15) // 16
        seen = np.zeros(n, bool)
        for i in range(walk):
            blk = i * ((n + 2047) // 2048) // walk
            seen[blk * 2048: (blk + 1) * 2048] = True
        if case.layout.endswith(":sampled_blocks"):
            assert seen[win].all()
        else:
            assert not seen[win].any()
        cand = np.sort(score[seen & (score >= tau)])[::-1]
        # a stage of more candidates than slots keeps an arbitrary subset: here they are then all of one score
        assert cand.size <= cap or np.unique(cand).size == 1
        tau = max(tau, cand[k - 1])
    survivors = int((score >= tau).sum())
    if case.regime == "few":
        assert tau == true_kth and survivors <= k + 3
    else:
        assert tau == score[b.level == 0][0] < true_kth and survivors == n > cap
    # winners sit on both edges of their blocks
    assert (win % 2048 == 0).any() and ((win % 2048 == 2047) | (win == n - 1)).any()


def test_plateau_overflows_its_second_stage():
    case = SR.case("plateau-140000")
    b = SR.build(case)
    assert (b.level == 0).all() and np.unique(b.corpus.scores(b.qt, b.qw)).size == 1
    cap, stages = SR.bound_plan(case.n, 512)
    assert len(SR.stage_blocks(case.n, stages[1])) * SR.IMP_R > cap
    assert np.array_equal(LR.named_topk(b.level, b.allowed, 512), np.arange(512))


def test_masked_cases_and_delete_sets():
    S = SR.IMP_R
    b = SR.build(SR.case("word-edges-4099"))
    for r in (S - 33, S - 32, S - 1, S, S + 31, S + 32, S + 63, S + 64):     # bits 31 | 0 on both sides of the block edge
        assert b.allowed[r] and b.level[r] >= 1
    assert not b.allowed[S - 2] and b.level[S - 2] >= 1
    d = SR.build(SR.case("dead-term-4099"))
    assert not d.allowed[d.lone_row] and (d.level[~d.allowed] >= 2).all() and (~d.allowed).sum() >= 40
    for case_id in ("block-edges-4099", "word-edges-4099"):
        b = SR.build(SR.case(case_id))
        dead = LR.delete_set(b.level) | ~b.allowed
        win = b.level >= 1
        assert dead[win].any() and (~dead)[win].any() and dead[b.level == 3].all() and dead[b.level == 0].any()
        score = b.corpus.scores(b.qt, b.qw)
        for k in SR.case(case_id).ks:
            want = LR.named_topk(b.level, ~dead, k)
            assert np.array_equal(R.topk(score, k, ~dead)[1][: want.size], want)


# ---------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("name", SR.POOL_CASES)
def test_pool_references_agree(name):
    pc = SR.pool_case(name)
    ref = SR.pool_ref(pc)
    assert np.array_equal(ref.view(np.int32), SR.pool_by_plane(pc).view(np.int32))
    T = pc.tok.shape[0]
    good = np.array([R.chunk_ok(int(pc.cu[c]), int(pc.cu[c + 1]), T) for c in range(pc.cu.size - 1)])
    assert np.isneginf(ref[~good]).all() and np.isfinite(ref[good]).all()
    assert np.abs(ref[good]).max() < 2 ** 24 and (ref[good] == np.rint(ref[good])).all()
    assert pc.tok.dtype == pc.E.dtype == np.float16 and pc.tok.shape[1] % 64 == 0 and pc.E.shape[1] % 64 == 0
    if pc.signed:
        neg = np.arange(pc.cu.size - 1) % 2 == 0
        assert (ref[neg] < 0).all() and (ref[~neg] > 0).all()


def test_pool_planes_have_the_structure_they_claim():
    B, PT = SR.SP_BATCH, SR.PT
    pc = SR.pool_case("eights")
    assert pc.cu.size - 1 == 256 and SR.pieces_per_tile(pc.cu, pc.tok.shape[0]).tolist() == [2 * B] * 16
    s = set(SR.EIGHTS_SAMPLE)                  # first and last of a tile (16 chunks) and of a batch of 8
    assert len(s) == 16 and {0, 7, 8, 15, 16, 255, 248} <= s and max(s) < 256
    pc = SR.pool_case("ones")
    assert SR.pieces_per_tile(pc.cu, pc.tok.shape[0]).tolist() == [16 * B, 1]
    pc = SR.pool_case("batch_edges")
    T = pc.tok.shape[0]
    assert SR.pieces_per_tile(pc.cu, T).tolist() == [B, B + 1, 2 * B, 2 * B + 1, 2]
    for edge in range(PT, T, PT):              # one chunk lies across every tile edge
        assert ((pc.cu[:-1] < edge) & (pc.cu[1:] > edge)).sum() == 1
    pc = SR.pool_case("invalid_between")
    lens = np.diff(pc.cu)
    assert 0 in lens and R.MAX_CHUNK_TOKENS + 1 in lens and (lens[(lens > 0) & (lens < 513)] == 8).all()
    per = SR.pieces_per_tile(pc.cu, pc.tok.shape[0])
    # the refused chunks take no slot: tile 0 has a batch of 8 and one of 2, tiles 1 .. 3 lie inside the long chunk
    assert per.tolist() == [10, 0, 0, 0, 6, 1]
    for name, ld, ld_e in (("pitch_128_192", 128, 192), ("pitch_192_128", 192, 128)):
        pc = SR.pool_case(name)
        assert pc.dim == 64 and pc.tok.shape[1] == ld and pc.E.shape[1] == ld_e
        assert (np.abs(pc.tok[:, 64:]) == 7).all() and (np.abs(pc.E[:, 64:]) == 7).all()
    assert SR.pool_case("dim_128").dim == 128 and SR.pool_case("dim_1024").dim == 1024
    pc = SR.pool_case("real_vocab")
    T, Vt = pc.tok.shape[0], pc.E.shape[0]
    assert (T, Vt) == (1200, 30522) and (Vt + PT - 1) // PT == 239 and Vt - 238 * PT == 58
    assert SR.default_vrun(T, Vt, 256) == 2 and SR.default_vrun(T, Vt, 304) == 1 and SR.default_vrun(1 << 20, Vt, 256) == 16
    assert len(set(np.diff(pc.cu).tolist())) > 10
    pc = SR.pool_case("run_tail")
    vt = (pc.E.shape[0] + PT - 1) // PT
    assert vt == SR.SP_VRUN + 2 and (vt + SR.SP_VRUN - 1) // SR.SP_VRUN == 2 and pc.E.shape[0] - (vt - 1) * PT == 5
    # every other case runs one vocabulary tile per workgroup by default on a device of 64 or more compute units
    for name in SR.POOL_CASES:
        pc = SR.pool_case(name)
        if name != "real_vocab":
            assert SR.default_vrun(pc.tok.shape[0], pc.E.shape[0], 64) == 1


# ---------------------------------------------------------------------------------------------------- select
def test_select_case_is_on_the_grid_and_the_ties_end_at_the_pins():
    pooled, bias, skip, scale, at = SR.select_case()
    Vt = pooled.shape[1]
    assert Vt == SR.REAL_V and scale == 1024.0 and pooled.dtype == np.float32
    ws = R.weights(pooled, bias, scale)
    fin = np.isfinite(ws)
    assert (np.abs(ws[fin] - np.rint(ws[fin])) <= 0.25 + 1e-3).all()
    imp = R.impacts(pooled, bias, scale)
    # chunk 2: +inf -> 255, NaN -> 0, -inf -> 0, saturation
    assert np.isposinf(pooled[2, at[0]]) and np.isnan(pooled[2, at[1]]) and np.isneginf(pooled[2, at[2]])
    assert imp[2, at].tolist() == [255, 0, 0, 255, 255, 255, 255, 255, 254, 100, 1, 0] and imp[2, Vt - 1] == 255
    assert (imp[2] > 0).sum() == 10 and imp[3].max() == 255 and (imp[3] == 255).sum() > 256
    # chunks 0 and 1: the run of ties, in every step of 256 terms
    for c, above in ((0, 0), (1, SR.ABOVE)):
        live = np.where(skip, 0, imp[c])
        ties = np.nonzero(live == SR.TIE_IMPACT)[0]
        assert ties.size == SR.TIE_RUN and ties[0] == SR.TIE_FIRST and (live > SR.TIE_IMPACT).sum() == above
        assert np.unique(ties // SR.SEL_T).size == (Vt + SR.SEL_T - 1) // SR.SEL_T == 120
        assert (imp[c][skip] == 200).all()
    ties = np.nonzero(np.where(skip, 0, imp[0]) == SR.TIE_IMPACT)[0]
    for m, lane in ((63, 63), (64, 64), (65, 65), (255, 127), (256, 128)):
        assert ties[m - 1] % SR.SEL_T == lane and ties[m - 1] // SR.SEL_T >= 5        # the last tie kept at this m
        t, q = R.select(imp[0], m, skip)
        assert np.array_equal(t, ties[:m]) and (q == SR.TIE_IMPACT).all()
    for m in SR.SELECT_MS:
        t, q = R.select(imp[1], m, skip)
        assert t.size == m and (q == 9).sum() == min(m, SR.ABOVE) and (q >= SR.TIE_IMPACT).all()
    for t in SR.SKIP_AT:
        assert skip[t] and t % 32 in (0, 31)
    words = sorted({t // 32 for t in SR.SKIP_AT})
    assert (5 * SR.SEL_T + 64) // 32 in words and (20 * SR.SEL_T + 128) // 32 in words
    assert np.array_equal(R.bits_to_bool(R.bool_to_bits(skip), Vt), skip)
