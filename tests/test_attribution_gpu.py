"""GPU: answer citations -- the kernel (csrc/attribute.hip, mmrag_attribute) against tests/attribution_ref.py (float64),
and the layers above it.

Every kernel case packs its units back to back in one plane -- a unit's claims, then its evidence -- with rows of POISON
(large values, source ordinal 0) between and around them, so a read past a unit's `len` shows as a huge score for
source 0.  The first unit starts at row 0 and the last ends at the last row.

Tolerances (derived, not fitted)
  exact data  row entries are multiples of 1/8 (one entry of 64 in the planted rows), few of them non-zero: every S_ij
              is a multiple of 1/64 of at most 64, exact in float32 whatever the order of the sum.  All four outputs
              bit-equal.
  random rows |S_ij - ref| <= d 2^-24 sum_k |x_k e_k| <= d 2^-24 for rows of norm at most 1 (the float32 accumulation
              of d exact products; tests/test_summary_gpu.py uses the same bound for S).  Every score is within it of
              the reference value of the evidence row it names; every pick (a source, and the evidence row inside it)
              is within it of the best eligible reference value; where the reference's margin exceeds twice the bound
              the pick is the reference's.
"""
import asyncio

import numpy as np
import pytest
import torch

from tests import attribution_ref as R

pytestmark = pytest.mark.gpu

DS = (384, 768, 100)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
POISON = 100.0
EINVAL, EUNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def as_stored(x, dtype):
    """the numbers a plane of `dtype` holds for x, as float64"""
    return torch.from_numpy(np.asarray(x, np.float32)).to(dtype).to(torch.float64).numpy()


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def pack(N, units, dtype, d, lead=0, gap=2):
    """units [(X [C, d], E [E, d], sources [E]) ...] -> (rows tensor [n_rows, ld] on the device, claim_start,
    claim_len, ev_start, ev_len, ev_source [n_rows]): claims then evidence per unit, `gap` POISON rows between any two
    blocks and `lead` before the first"""
    ld = N.padded_dim(d, dtype)
    parts, ords, tables, at = [], [], [[], [], [], []], 0

    def put(block, block_ords):
        nonlocal at
        body = np.zeros((len(block), ld), np.float32)
        body[:, :d] = block
        parts.append(body)
        ords.append(np.asarray(block_ords, np.int32))
        at += len(block)

    def poison(n):
        if n:
            put(np.full((n, d), POISON, np.float32), np.zeros(n, np.int32))

    poison(lead)
    for u, (X, E, sources) in enumerate(units):
        if u:
            poison(gap)
        tables[0].append(at)
        tables[1].append(len(X))
        put(X, np.zeros(len(X), np.int32))
        if len(E):
            poison(gap)
        tables[2].append(at)
        tables[3].append(len(E))
        if len(E):
            put(E, sources)
    rows = torch.from_numpy(np.concatenate(parts)).to(dtype).cuda().contiguous()
    return (rows,) + tuple(np.asarray(t, np.int32) for t in tables) + (np.concatenate(ords),)


def launch(N, rows, d, cs, cl, es, el, src_of, n_sources, m, max_claims, want_support=True, out=None):
    got = N.attribute(rows, d, dev_i32(cs), dev_i32(cl), dev_i32(es), dev_i32(el), dev_i32(src_of), n_sources, m,
                      max_claims, want_support=want_support, out=out)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in got)


def sentinels(n_units, max_claims, m, n_sources, support=True):
    shape = (n_units, max_claims, m)
    return (torch.full(shape, 77, dtype=torch.int32).cuda(), torch.full(shape, 77, dtype=torch.int32).cuda(),
            torch.full(shape, 77.0).cuda(),
            torch.full((n_units, max_claims, n_sources), 77.0).cuda() if support else None)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------- 1: exact data
def exact_rows(rng, n, d):
    """multiples of 1/8, 6 non-zeros per row: 4 among the first 12 columns (so rows overlap and many scores tie), 1
    anywhere, 1 in the last column of the ragged slab"""
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        cols = np.concatenate([rng.choice(12, 4, replace=False), rng.integers(12, d, 1), [d - 1]])
        x[i, cols] = rng.integers(-2, 9, len(cols)) / 8.0
    return x


# (C, E, the ordinals the evidence draws from -- out-of-range ones included)
EXACT_UNITS = (
    (1, 0, (0,)),
    (2, 1, (1,)),
    (16, 127, (0, 1)),
    (17, 128, (5, 0, 62, 63, 64, -1)),
    (64, 129, tuple(range(0, 64, 2))),                # the odd sources have no evidence
    (65, 257, tuple(range(64))),
    (127, 1000, tuple(range(70)) + (-7, 1000)),       # ordinals out of range at every n_sources
    (128, 4096, tuple(range(64))),
    (128, 300, (63, 1, 0)),
    (3, 130, (0,)),
    (33, 128, (1, 0)),
)
# (n_sources, m): m larger than the sources with evidence (2 sources, m = 8); every claim-source pair at 64 x 8
EXACT_CALLS = ((1, 1), (2, 8), (63, 3), (64, 8))


def exact_unit(rng, C, E, pool, d):
    X, Ev = exact_rows(rng, C, d), exact_rows(rng, E, d)
    X[:, 20:22], Ev[:, 20:22] = 0.0, 0.0             # two columns for the planted matches alone
    sources = np.asarray(pool, np.int32)[rng.integers(0, len(pool), E)]       # interleaved, unsorted
    if E >= 4:
        # exact ties: row 2 again in the same source (the lowest j wins) and in another source (the lowest s wins)
        Ev[E // 2], sources[E // 2] = Ev[2], sources[2]
        Ev[E // 2 + 1] = Ev[2]
        sources[E // 2 + 1] = pool[(list(pool).index(sources[2]) + 1) % len(pool)]
    if E >= 2 and C >= 2:
        # the best match of claim 0 in the LAST row of the last (ragged) evidence tile, of claim 1 in row 0: a score of
        # 64 where every other one is below |x| |e| < 7
        X[0, 20], X[1, 21] = 1.0, 1.0
        Ev[E - 1], Ev[0] = 0.0, 0.0
        Ev[E - 1, 20], Ev[0, 21] = 64.0, 64.0
        sources[E - 1] = sources[0] = 0
    return X, Ev, sources


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_exact_data_is_bit_equal_to_the_reference(N, name, d):
    dtype = DTYPES[name]
    rng = np.random.default_rng(2000 + d + len(name))
    units = [exact_unit(rng, C, E, pool, d) for C, E, pool in EXACT_UNITS]
    rows, cs, cl, es, el, src_of = pack(N, units, dtype, d)
    assert cs[0] == 0 and es[-1] + el[-1] == rows.shape[0]
    Ss = [R.similarities(as_stored(X, dtype), as_stored(E, dtype)) for X, E, _ in units]
    for S in Ss:
        assert np.array_equal(S.astype(np.float32).astype(np.float64), S)      # the data IS exact
    max_claims = 128
    planted = ties = 0
    for n_sources, m in EXACT_CALLS:
        out = sentinels(len(units), max_claims, m, n_sources)
        src, ev, score, sup = launch(N, rows, d, cs, cl, es, el, src_of, n_sources, m, max_claims, out=out)
        for u, (C, E, _) in enumerate(EXACT_UNITS):
            tag = f"exact {name} d={d} C={C} E={E} n_sources={n_sources} m={m}"
            M, J = R.support(Ss[u], units[u][2], n_sources)
            r_src, r_ev, r_score = R.rank(M, J, m)
            assert np.array_equal(src[u, :C], r_src), tag
            assert np.array_equal(ev[u, :C], r_ev), tag
            assert np.array_equal(bits(score[u, :C]), bits(r_score)), tag
            assert np.array_equal(bits(sup[u, :C]), bits(M)), tag
            # rows past C: padding in the three lists, nothing written in the matrix
            assert np.all(src[u, C:] == -1) and np.all(ev[u, C:] == -1) and np.all(np.isneginf(score[u, C:])), tag
            assert np.all(sup[u, C:] == 77.0), tag
            if E >= 2 and C >= 2:
                assert r_ev[0, 0] == E - 1 and r_ev[1, 0] == 0 and r_src[0, 0] == 0, tag
                planted += 1
            have = (J >= 0).sum(axis=1)
            assert np.all((r_src >= 0).sum(axis=1) == np.minimum(have, m)), tag
            if n_sources == 64 and E >= 4:
                ties += int(sum(len(set(M[i, J[i] >= 0])) < have[i] for i in range(C)))
        if n_sources == 2:
            assert np.all(src[:, :, 2:] == -1)          # m = 8 above the two sources there are
    assert planted >= 30 and ties >= 100, (planted, ties)     # the cases the data was built for are there


# ---------------------------------------------------------------- 2: random unit rows
def unit_rows(rng, n, d, centres):
    """normalised rows around one of a few centres, cast to fp16; scaled so the norm stays at most 1 in any dtype"""
    x = centres[rng.integers(0, len(centres), n)] + 0.6 * rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True) * (1.0 + 2.0 ** -7)
    return x.astype(np.float16)


RANDOM_UNITS = ((17, 300, 5), (128, 1000, 64), (65, 129, 2), (1, 128, 1), (30, 4096, 64))


def check_random_unit(tag, X, E, sources, n_sources, m, src, ev, score, sup, bound):
    C = len(X)
    S = R.similarities(X, E)
    M, J = R.support(S, sources, n_sources)
    finite = np.isfinite(M)
    assert np.array_equal(np.isfinite(sup[:C]), finite), tag
    err = np.abs(sup[:C].astype(np.float64)[finite] - M[finite]).max() if finite.any() else 0.0
    decisive = steps = 0
    for i in range(C):
        got, left = R.margins(S[i], sources, n_sources, src[i], ev[i])
        assert len(got) == min(m, len(got) + left), (tag, i)
        for t, (s_val, m_val, best, margin, ref_pick, mine) in enumerate(got):
            assert mine, (tag, i, t)
            assert abs(float(score[i, t]) - s_val) <= bound, (tag, i, t, score[i, t], s_val)
            assert m_val - s_val <= bound, (tag, i, t)             # the evidence row is (close to) its source's best
            assert best - m_val <= bound, (tag, i, t, best, m_val)  # the source is (close to) the best one left
            steps += 1
            if margin > 2 * bound:
                decisive += 1
                assert src[i, t] == ref_pick, (tag, i, t, src[i, t], ref_pick, margin)
            rows = np.nonzero(np.asarray(sources) == src[i, t])[0]
            order = np.sort(S[i, rows])[::-1]
            if len(order) < 2 or order[0] - order[1] > 2 * bound:
                assert ev[i, t] == J[i, src[i, t]], (tag, i, t)
        assert np.all(src[i, len(got):] == -1) and np.all(np.isneginf(score[i, len(got):])), (tag, i)
    print(f"{tag}: support err {err:.3e} (bound {bound:.3e}), decisive {decisive} of {steps}")
    assert err <= bound, (tag, err, bound)
    return decisive, steps


@pytest.mark.parametrize("name,d", [("f16", 384), ("f16", 768), ("f16", 100), ("bf16", 384), ("f32", 100)])
def test_random_rows_against_float64(N, name, d):
    dtype = DTYPES[name]
    rng = np.random.default_rng([7, d, len(name)])
    centres = rng.standard_normal((6, d))
    units = []
    for C, E, n_src in RANDOM_UNITS:
        pool = np.concatenate([np.arange(n_src), [-1, 64]])
        units.append((unit_rows(rng, C, d, centres), unit_rows(rng, E, d, centres),
                      pool[rng.integers(0, len(pool), E)].astype(np.int32)))
    rows, cs, cl, es, el, src_of = pack(N, units, dtype, d)
    bound = d * 2.0 ** -24
    n_sources, m = 64, 8
    src, ev, score, sup = launch(N, rows, d, cs, cl, es, el, src_of, n_sources, m, 128)
    decisive = steps = 0
    for u, (X, E, sources) in enumerate(units):
        Xs, Es = as_stored(X, dtype), as_stored(E, dtype)
        assert np.linalg.norm(Xs, axis=1).max() <= 1.0 and np.linalg.norm(Es, axis=1).max() <= 1.0
        got = check_random_unit(f"random {name} d={d} u={u}", Xs, Es, sources, n_sources, m, src[u], ev[u], score[u],
                                sup[u], bound)
        decisive, steps = decisive + got[0], steps + got[1]
    assert decisive >= 0.85 * steps, f"the inputs are not decisive enough for the tolerance to mean anything"


# ---------------------------------------------------------------- 3: independence
def test_a_unit_has_the_same_bits_wherever_it_runs(N):
    d, C, E, n_sources, m = 384, 65, 300, 7, 4
    rng = np.random.default_rng(11)
    centres = rng.standard_normal((4, d))
    unit = (unit_rows(rng, C, d, centres), unit_rows(rng, E, d, centres), rng.integers(0, n_sources, E))

    def bits_of(out, u, support=True):
        src, ev, score, sup = out
        return (src[u, :C].tobytes(), ev[u, :C].tobytes(), score[u, :C].tobytes()) + \
            ((sup[u, :C].tobytes(),) if support else ())

    packed = pack(N, [unit], torch.float16, d)
    alone = bits_of(launch(N, *packed[:1], d, *packed[1:], n_sources, m, C), 0)
    assert bits_of(launch(N, *packed[:1], d, *packed[1:], n_sources, m, C), 0) == alone
    # out_support NULL
    assert bits_of(launch(N, *packed[:1], d, *packed[1:], n_sources, m, C, want_support=False), 0, False) == alone[:3]
    # at another place in the plane
    moved = pack(N, [unit], torch.float16, d, lead=37)
    assert bits_of(launch(N, *moved[:1], d, *moved[1:], n_sources, m, C), 0) == alone
    # in a batch of 50 (the unit is number 31; the others are smaller and different), with a larger max_claims
    others = [(unit_rows(rng, 1 + u % 9, d, centres), unit_rows(rng, 3 + 5 * u, d, centres),
               rng.integers(0, n_sources, 3 + 5 * u)) for u in range(50)]
    others[31] = unit
    batch = pack(N, others, torch.float16, d, gap=1)
    assert bits_of(launch(N, *batch[:1], d, *batch[1:], n_sources, m, 128), 31) == alone
    # under graph capture and replay
    tables = [dev_i32(a) for a in packed[1:]]
    out = sentinels(1, C, m, n_sources)

    def call():
        N.attribute(packed[0], d, *tables, n_sources, m, C, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert bits_of(tuple(t.cpu().numpy() for t in out), 0) == alone


# ---------------------------------------------------------------- 4: refusals
def test_bad_arguments_are_refused_and_nothing_is_launched(N):
    d = 384
    rng = np.random.default_rng(12)
    unit = (exact_rows(rng, 16, d), exact_rows(rng, 40, d), rng.integers(0, 4, 40))
    rows, cs, cl, es, el, src_of = pack(N, [unit], torch.float16, d)
    tables = [dev_i32(a) for a in (cs, cl, es, el, src_of)]
    out = sentinels(1, 16, 3, 4)
    f8 = torch.zeros((rows.shape[0], 384), dtype=torch.uint8).cuda().view(torch.float8_e4m3fn)

    def status(rows=rows, ld=None, dtype=1, d=d, n_rows=None, tables=tables, n_units=1, n_sources=4, m=3, max_claims=16,
               null=None):
        ptrs = [rows.data_ptr()] + [t.data_ptr() for t in tables] + [t.data_ptr() for t in out[:3]]
        if null is not None:
            ptrs[null] = None
        st = N.lib().mmrag_attribute(ptrs[0], rows.shape[1] if ld is None else ld, dtype, d,
                                     rows.shape[0] if n_rows is None else n_rows, ptrs[1], ptrs[2], ptrs[3], ptrs[4],
                                     n_units, ptrs[5], n_sources, m, max_claims, ptrs[6], ptrs[7], ptrs[8],
                                     out[3].data_ptr(), None)
        return st

    assert status(rows=f8, dtype=3) == EUNSUPPORTED                 # FP8 rows are not attributed
    for null in range(9):                                           # every pointer but out_support
        assert status(null=null) == EINVAL, null
    assert status(ld=100, d=100) == EINVAL and status(ld=d - 64) == EINVAL     # a pitch of 200 bytes; ld < d
    assert status(d=0) == EINVAL and status(dtype=7) == EINVAL
    assert status(n_rows=0) == EINVAL and status(n_rows=2 ** 31) == EINVAL
    assert status(n_units=0) == EINVAL and status(n_units=2 ** 24 + 1) == EINVAL
    assert status(n_sources=0) == EINVAL and status(n_sources=65) == EINVAL
    assert status(m=0) == EINVAL and status(m=9) == EINVAL
    assert status(max_claims=0) == EINVAL and status(max_claims=129) == EINVAL
    with pytest.raises(N.MMRagNativeError, match="status 4"):
        N.attribute(f8, d, *tables, 4, 3, 16, out=out)
    with pytest.raises(N.MMRagNativeError):
        N.attribute(rows.cpu(), d, *tables, 4, 3, 16)                          # host tensors
    with pytest.raises(N.MMRagNativeError):
        N.attribute(rows, d, *tables[:4], tables[4][:5], 4, 3, 16)             # ev_source: one entry per row
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out)


def test_a_unit_with_a_bad_table_entry_is_marked_and_its_neighbours_are_untouched(N):
    d, n_sources, m, max_claims = 768, 6, 3, 40
    rng = np.random.default_rng(13)
    units = [(exact_rows(rng, C, d), exact_rows(rng, E, d), rng.integers(0, n_sources, E))
             for C, E in ((17, 140), (16, 50), (40, 129))]
    rows, cs, cl, es, el, src_of = pack(N, units, torch.bfloat16, d)
    n_rows = rows.shape[0]
    good = launch(N, rows, d, cs, cl, es, el, src_of, n_sources, m, max_claims)
    for u, (X, E, sources) in enumerate(units):
        r_src, r_ev, r_score, M = R.attribute(as_stored(X, torch.bfloat16), as_stored(E, torch.bfloat16), sources,
                                              n_sources, m)
        assert np.array_equal(good[0][u, :len(X)], r_src) and np.array_equal(good[1][u, :len(X)], r_ev)
        assert np.array_equal(bits(good[2][u, :len(X)]), bits(r_score))
    # the entries a device table may hold by mistake.  None of them indexes memory: the unit is marked, its neighbours
    # are what they were.  (claim_start, claim_len, ev_start, ev_len) of unit 1
    for bad in ((cs[1], 0, es[1], 50), (cs[1], 41, es[1], 50), (cs[1], 129, es[1], 50), (cs[1], -3, es[1], 50),
                (-1, 16, es[1], 50), (n_rows - 3, 16, es[1], 50), (2 ** 31 - 8, 16, es[1], 50),
                (cs[1], 16, es[1], -1), (cs[1], 16, es[1], 4097), (cs[1], 16, -1, 50), (cs[1], 16, n_rows - 3, 50),
                (cs[1], 16, 2 ** 31 - 8, 50)):
        tabs = [t.copy() for t in (cs, cl, es, el)]
        for t, v in zip(tabs, bad):
            t[1] = v
        src, ev, score, sup = launch(N, rows, d, *tabs, src_of, n_sources, m, max_claims,
                                     out=sentinels(3, max_claims, m, n_sources))
        assert np.isnan(score[1, 0, 0]) and np.all(src[1] == -1) and np.all(ev[1] == -1), bad
        assert np.all(sup[1] == 77.0), bad
        for u in (0, 2):
            C = cl[u]
            assert np.array_equal(src[u], good[0][u]) and np.array_equal(ev[u], good[1][u]), bad
            assert np.array_equal(bits(score[u]), bits(good[2][u])), bad
            assert np.array_equal(bits(sup[u, :C]), bits(good[3][u, :C])), bad


# ---------------------------------------------------------------- 5: through the product
@pytest.fixture(scope="module")
def manager(N):
    from multimodal_rag_amd import embedder as EM

    names = ("MMRAG_MODEL_DIR", "MMRAG_ENCODER_PRECISION", "MMRAG_INDEX_DTYPE", "MMRAG_SUMMARIZER")
    saved = [getattr(EM.settings, n) for n in names]
    EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION = "", "fp16"
    EM.settings.MMRAG_INDEX_DTYPE, EM.settings.MMRAG_SUMMARIZER = "float16", "fallback"
    try:
        m = EM.EmbeddingManager(engine=EM.HipEngine("sentence-transformers/all-MiniLM-L6-v2"), enable_cache=False)
        asyncio.run(m.initialize())
        yield m
    finally:
        for n, v in zip(names, saved):
            setattr(EM.settings, n, v)


SOLAR = ["Solar panels turn sunlight into electric power.", "A panel is built from many silicon cells.",
         "Each cell frees electrons when light strikes it.", "An inverter turns the direct current into grid power."]
BREAD = ["Sourdough bread starts from a living culture of flour and water.", "The dough proofs overnight in the cold.",
         "A hot cast iron pot gives the loaf its crust.", "Steam in the first minutes lets the loaf rise."]
RIVER = ["The river floods the lower meadows every spring.", "Herons nest in the reeds along its banks."]
UNRELATED = "Quarterly invoices, 4711 and 0815, were mailed to zip code 90210?"


def test_copied_sentences_cite_their_passages_and_a_foreign_one_is_unsupported(N, manager):
    passages = [" ".join(SOLAR), " ".join(BREAD), " ".join(RIVER)]
    answer = " ".join([BREAD[2], SOLAR[0], RIVER[1], SOLAR[3]])
    expect = [(1, BREAD[2]), (0, SOLAR[0]), (2, RIVER[1]), (0, SOLAR[3])]
    got = asyncio.run(manager.attribute_answer(answer, passages, threshold=0.99, max_citations=1))
    assert got["considered"] == {"claims": 4, "evidence": 10} and got["groundedness"] == 1.0
    assert got["support"] == pytest.approx([(len(SOLAR[0]) + len(SOLAR[3])) / sum(len(t) for _, t in expect),
                                            len(BREAD[2]) / sum(len(t) for _, t in expect),
                                            len(RIVER[1]) / sum(len(t) for _, t in expect)])
    for entry, (source, text) in zip(got["citations"], expect):
        assert answer[entry["start"]: entry["end"]] == entry["text"] == text and entry["supported"]
        assert [c["source"] for c in entry["sources"]] == [source]
        cite = entry["sources"][0]
        assert passages[cite["passage"]][cite["start"]: cite["end"]] == cite["text"] == text
        assert abs(cite["score"] - 1.0) <= 2e-3 and entry["score"] == cite["score"]     # fp16 rows of a unit vector
    # an appended sentence of unrelated text: unsupported under a threshold between the two observed scores (seeded
    # random weights give no meaningful absolute scale, so the threshold comes from the scores)
    longer = answer + " " + UNRELATED
    loose = asyncio.run(manager.attribute_answer(longer, passages, threshold=-0.999, max_citations=8))
    scores = [entry["score"] for entry in loose["citations"]]
    assert len(scores) == 5 and min(scores[:4]) > scores[4], scores
    assert all(len(entry["sources"]) == 3 for entry in loose["citations"])       # every source, best first
    assert all(entry["sources"][0]["score"] >= entry["sources"][1]["score"] >= entry["sources"][2]["score"]
               for entry in loose["citations"])
    between = (min(scores[:4]) + scores[4]) / 2.0
    print(f"copied {min(scores[:4]):.4f}, unrelated {scores[4]:.4f}, threshold {between:.4f}")
    cut = asyncio.run(manager.attribute_answer(longer, passages, threshold=between))
    assert [entry["supported"] for entry in cut["citations"]] == [True] * 4 + [False]
    assert cut["citations"][4]["sources"] == [] and cut["citations"][4]["score"] == scores[4]
    assert cut["groundedness"] == pytest.approx(sum(len(t) for _, t in expect) /
                                                (sum(len(t) for _, t in expect) + len(UNRELATED)))
    # owners: passages 0 and 2 are one source; a batch is one call and gives what the single calls give
    owned = asyncio.run(manager.attribute_answer(answer, passages, owner=[0, 1, 0], threshold=0.99, max_citations=1))
    assert [entry["sources"][0]["source"] for entry in owned["citations"]] == [1, 0, 0, 0]
    assert [entry["sources"][0]["passage"] for entry in owned["citations"]] == [1, 0, 2, 0]
    both = asyncio.run(manager.batch_attribute_answers([answer, longer, ""], [passages, passages, passages],
                                                       threshold=between))
    assert both[1] == cut and both[0]["groundedness"] == 1.0 and both[2]["citations"] == []


def test_query_with_citations_matches_attribute_answer(N, manager):
    from starlette.testclient import TestClient

    from multimodal_rag_amd.server import create_app

    chunk = " ".join(SOLAR + BREAD)
    with TestClient(create_app(embedder=manager)) as client:
        up = client.post("/upload", files={"file": ("solar.txt", chunk.encode("utf-8"), "text/plain")})
        assert up.status_code == 200, up.text
        try:
            plain = client.post("/query", json={"query": "how do solar panels make power", "top_k": 2,
                                                "extractive_answer": True}).json()
            assert "citations" not in plain and "groundedness" not in plain
            assert all("cited_by" not in src and "support" not in src for src in plain["sources"])
            got = client.post("/query", json={"query": "how do solar panels make power", "top_k": 2,
                                              "extractive_answer": True, "citations": True,
                                              "citation_threshold": 0.99, "max_citations": 2}).json()
            assert got["answer"] == plain["answer"] and got["answer"]
            assert [{k: v for k, v in src.items() if k not in ("cited_by", "support")} for src in got["sources"]] == \
                plain["sources"]
            direct = asyncio.run(manager.attribute_answer(got["answer"], [chunk], owner=[0], threshold=0.99,
                                                          max_citations=2))
            assert got["citations"] == direct["citations"] and got["groundedness"] == direct["groundedness"] == 1.0
            # an extractive answer quotes the hit: every sentence cites source 0
            assert got["sources"][0]["cited_by"] == list(range(len(got["citations"])))
            assert got["sources"][0]["support"] == 1.0
            away = client.post("/attribute", json={"answer": got["answer"], "passages": [chunk],
                                                   "citation_threshold": 0.99, "max_citations": 2}).json()
            assert away["citations"] == direct["citations"] and away["groundedness"] == 1.0
        finally:
            manager.collection.delete(where={"doc_id": up.json()["doc_id"]})
