"""GPU: extractive selection by sentence centrality -- the kernel (csrc/summarize.hip, mmrag_summary_select) against
tests/summary_ref.py (float64), and the layers above it.

Every kernel case packs its units back to back in one plane: one unit starts at row 0, one ends at the last row, and
rows of POISON (large values) sit between units, so a read past a unit's `len` shows as a huge similarity.
n in {1, 2, 3, 16, 17, 64, 65, 127, 128} (tile and 16-row-block seams, one- and two-wave row halves), d in {384, 768,
100} (100: a padded pitch and a ragged last slab), the three storage dtypes.

Tolerances (derived, not fitted)
  rel ....... |rel - ref| <= 2 (n + 2) 2^-24 / alpha, relative to the reference's maximum (which is 1): each step's
              sums carry a relative error of at most (n + 2) 2^-24, the iteration contracts the 1-norm by 1 - alpha,
              so errors accumulate to at most 1 / alpha times one step's.  n = 128, alpha = 0.15: about 1e-4.
  picks ..... for each kernel pick, given the kernel's own earlier picks, the reference v of the pick is within
              tol_v = 1e-4 of the best eligible reference v (lambda times the bound above plus (1 - lambda) d 2^-24
              for S); where the reference's margin between its best and second-best eligible value exceeds 2 tol_v
              the pick must be the reference's.
  exact data  row entries are multiples of 1/8, few of them non-zero: every S_ij is exact in float32.
"""
import asyncio

import numpy as np
import pytest
import torch

from tests import summary_ref as R

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 16, 17, 64, 65, 127, 128)
DS = (384, 768, 100)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
POISON = 100.0
TOL_V = 1e-4
PARAMS = dict(edge_threshold=0.1, alpha=0.15, iterations=32, lam=0.7)


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def rel_bound(n, alpha):
    return 2.0 * (n + 2) * 2.0 ** -24 / alpha


def as_stored(x, dtype):
    """the numbers a plane of `dtype` holds for x, as float64"""
    return torch.from_numpy(np.asarray(x, np.float32)).to(dtype).to(torch.float64).numpy()


def pack(N, units, costs, dtype, d, lead=0, gap=2, bias=None):
    """units (float arrays [n, d]) back to back with `gap` POISON rows between them (and `lead` before the first) ->
    (rows tensor [n_rows, ld] on the device, starts, lens, cost [n_rows], bias tensor or None)"""
    ld = N.padded_dim(d, dtype)
    parts, cost_parts, starts, at = [], [], [], 0
    if lead:
        parts.append(np.full((lead, ld), POISON, np.float32))
        cost_parts.append(np.ones(lead, np.int32))
        at += lead
    for u, (x, c) in enumerate(zip(units, costs)):
        if u:
            parts.append(np.full((gap, ld), POISON, np.float32))
            cost_parts.append(np.ones(gap, np.int32))
            at += gap
        body = np.zeros((len(x), ld), np.float32)
        body[:, :d] = x
        parts.append(body)
        cost_parts.append(np.asarray(c, np.int32))
        starts.append(at)
        at += len(x)
    rows = np.concatenate(parts)
    rows[:, d:] = 0.0
    rows_t = torch.from_numpy(rows).to(dtype).cuda().contiguous()
    bias_t = None
    if bias is not None:
        b = np.zeros((len(bias), ld), np.float32)
        b[:, :d] = bias
        bias_t = torch.from_numpy(b).to(dtype).cuda().contiguous()
    return (rows_t, np.asarray(starts, np.int32), np.asarray([len(x) for x in units], np.int32),
            np.concatenate(cost_parts), bias_t)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def launch(N, rows, d, starts, lens, cost, budgets, k, params=PARAMS, bias=None, unit_bias=None, out=None):
    got = N.summary_select(rows, d, dev_i32(starts), dev_i32(lens), dev_i32(cost), dev_i32(budgets), k,
                           bias_rows=bias, unit_bias=None if unit_bias is None else dev_i32(unit_bias), out=out,
                           **params)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in got)


def check_unit(tag, X, q, cost, budget, k, params, pos, val, rel, used, d):
    """one unit's outputs against the reference (X, q: the stored numbers as float64)"""
    n = len(X)
    S, s = R.similarities(X, q)
    ref_rel = R.centrality(S, s, params["edge_threshold"], params["alpha"], params["iterations"])
    bound = rel_bound(n, params["alpha"])
    err = np.abs(rel.astype(np.float64) - ref_rel).max()
    print(f"{tag}: rel err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (tag, err, bound)
    picks = [int(p) for p in pos if p >= 0]
    m = len(picks)
    assert np.all(pos[m:] == -1) and np.all(np.isneginf(val[m:])) and m <= min(k, n), (tag, pos, val)
    assert len(set(picks)) == m and all(0 <= p < n for p in picks), (tag, picks)
    steps, remaining = R.margins(ref_rel, S, cost, budget, params["lam"], picks)
    for t, (v_pick, v_best, margin, eligible, ref_pick) in enumerate(steps):
        assert eligible, (tag, t, picks)
        assert v_best - v_pick <= TOL_V, (tag, t, picks[t], v_pick, v_best)
        assert abs(float(val[t]) - v_pick) <= TOL_V + 2.0 ** -23 * max(1.0, abs(v_pick)), (tag, t, val[t], v_pick)
        if margin > 2 * TOL_V:
            assert picks[t] == ref_pick, (tag, t, picks[t], ref_pick, margin)
    assert remaining >= 0 and used == budget - remaining, (tag, used, budget, remaining)
    if m < k:       # the kernel stopped: nothing free may fit what is left
        _, ok = R.step_values(ref_rel, S, cost, remaining, picks, params["lam"])
        assert not ok.any(), (tag, picks, remaining)


# ---------------------------------------------------------------- 1: exact data
def exact_rows(rng, n, d):
    """multiples of 1/8, 6 non-zeros per row: 4 among the first 12 columns (so rows overlap), 2 anywhere -- the last
    column of the ragged slab included"""
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        cols = np.concatenate([rng.choice(12, 4, replace=False), rng.integers(12, d, 1), [d - 1]])
        x[i, cols] = rng.integers(-2, 9, len(cols)) / 8.0
    return x


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_exact_data_against_the_reference(N, name, d):
    dtype = DTYPES[name]
    rng = np.random.default_rng(1000 + d + len(name))
    units = [exact_rows(rng, n, d) for n in NS]
    costs = [rng.integers(1, 9, n) for n in NS]
    budgets = np.asarray([max(1, int(c.sum()) // 2) for c in costs], np.int32)
    bias = exact_rows(rng, 2, d)
    unit_bias = np.asarray([(u % 3) - 1 for u in range(len(NS))], np.int32)      # -1, 0, 1, ...
    k = 16
    rows, starts, lens, cost, bias_t = pack(N, units, costs, dtype, d, bias=bias)
    assert starts[0] == 0 and starts[-1] + lens[-1] == rows.shape[0]
    for with_bias in (False, True):
        pos, val, rel, used = launch(N, rows, d, starts, lens, cost, budgets, k, bias=bias_t if with_bias else None,
                                     unit_bias=unit_bias if with_bias else None)
        for u, n in enumerate(NS):
            q = as_stored(bias[unit_bias[u]], dtype) if with_bias and unit_bias[u] >= 0 else None
            check_unit(f"exact {name} d={d} n={n} bias={with_bias}", as_stored(units[u], dtype), q, costs[u],
                       int(budgets[u]), k, PARAMS, pos[u], val[u], rel[starts[u]: starts[u] + n], int(used[u]), d)


# ---------------------------------------------------------------- 2: real-shaped data
def clustered_rows(rng, n, d):
    """4 Gaussian centres in d dimensions; each sentence is a random centre plus 0.6 x standard normal noise,
    normalised, cast to fp16"""
    centres = rng.standard_normal((4, d))
    x = centres[rng.integers(0, 4, n)] + 0.6 * rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16)


def real_cases(d, seeds=(0, 1, 2, 3)):
    out = []
    for seed in seeds:
        for n in NS:
            rng = np.random.default_rng([seed, n, d])
            x = clustered_rows(rng, n, d)
            q = clustered_rows(rng, 1, d)[0]
            out.append((x, q, rng.integers(20, 160, n)))
    return out


def decisive_share(cases, with_bias, k=16, budget=300):
    """the share of the REFERENCE's own steps whose margin exceeds 2 tol_v"""
    flags = []
    for x, q, cost in cases:
        X = x.astype(np.float64)
        rel, picks, _, _ = R.summarize(X, cost, budget, k, PARAMS["edge_threshold"], PARAMS["alpha"],
                                       PARAMS["iterations"], PARAMS["lam"], q.astype(np.float64) if with_bias else None)
        S, _ = R.similarities(X)
        steps, _ = R.margins(rel, S, cost, budget, PARAMS["lam"], picks)
        flags += [m > 2 * TOL_V for _, _, m, _, _ in steps]
    return float(np.mean(flags)), len(flags)


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("with_bias", (False, True))
def test_real_shaped_data_against_the_reference(N, with_bias, d):
    cases = real_cases(d)
    share, steps = decisive_share(cases, with_bias)
    print(f"decisive steps: {share:.3f} of {steps}")
    assert share >= 0.85, f"the inputs are not decisive enough for the tolerance to mean anything: {share:.3f}"
    k, budget = 16, 300
    rows, starts, lens, cost, bias_t = pack(N, [x for x, _, _ in cases], [c for _, _, c in cases], torch.float16, d,
                                            bias=np.stack([q for _, q, _ in cases]) if with_bias else None)
    budgets = np.full(len(cases), budget, np.int32)
    pos, val, rel, used = launch(N, rows, d, starts, lens, cost, budgets, k, bias=bias_t,
                                 unit_bias=np.arange(len(cases)) if with_bias else None)
    for u, (x, q, c) in enumerate(cases):
        n = len(x)
        check_unit(f"real d={d} u={u} n={n} bias={with_bias}", x.astype(np.float64),
                   q.astype(np.float64) if with_bias else None, c, budget, k, PARAMS, pos[u], val[u],
                   rel[starts[u]: starts[u] + n], int(used[u]), d)


# ---------------------------------------------------------------- 3: edges
def test_budget_zero_and_budget_below_every_cost(N):
    rng = np.random.default_rng(3)
    units = [exact_rows(rng, 17, 384), exact_rows(rng, 5, 384)]
    costs = [np.full(17, 7), np.full(5, 3)]
    rows, starts, lens, cost, _ = pack(N, units, costs, torch.float16, 384)
    pos, val, rel, used = launch(N, rows, 384, starts, lens, cost, [0, 2], 4)
    assert np.all(pos == -1) and np.all(np.isneginf(val)) and np.all(used == 0)
    assert np.isfinite(rel[starts[0]: starts[0] + 17]).all()       # the centrality is still there


@pytest.mark.parametrize("k", (1, 128))
def test_k_one_and_k_above_n(N, k):
    rng = np.random.default_rng(4)
    units = [exact_rows(rng, 17, 100), exact_rows(rng, 3, 100)]
    costs = [np.ones(17, np.int32), np.ones(3, np.int32)]
    rows, starts, lens, cost, _ = pack(N, units, costs, torch.float32, 100)
    budgets = [1000, 1000]
    pos, val, rel, used = launch(N, rows, 100, starts, lens, cost, budgets, k)
    for u, n in enumerate((17, 3)):
        assert (pos[u] >= 0).sum() == min(k, n) and used[u] == min(k, n)
        check_unit(f"k={k} n={n}", as_stored(units[u], torch.float32), None, costs[u], budgets[u], k, PARAMS, pos[u],
                   val[u], rel[starts[u]: starts[u] + n], int(used[u]), 100)


def test_identical_sentences_all_zero_rows_and_a_threshold_above_everything(N):
    d = 384
    same = np.zeros((9, d), np.float32)
    same[:, :8] = 0.5          # <x, x> = 2 for every pair
    zero = np.zeros((6, d), np.float32)
    rng = np.random.default_rng(5)
    other = exact_rows(rng, 16, d)
    units, costs = [same, zero, other], [np.ones(9, np.int32), np.ones(6, np.int32), np.ones(16, np.int32)]
    rows, starts, lens, cost, _ = pack(N, units, costs, torch.float16, d)
    pos, val, rel, used = launch(N, rows, d, starts, lens, cost, [100, 100, 100], 4)
    # identical sentences: rel is 1 everywhere (bit for bit: every thread runs the same sums), the first pick is
    # sentence 0 at v = lambda, every later one ties at lambda - (1 - lambda) 2 and goes to the lowest free index
    lam, oml = R.weights(PARAMS["lam"])
    assert np.all(rel[starts[0]: starts[0] + 9] == 1.0)
    assert pos[0].tolist() == [0, 1, 2, 3]
    assert val[0, 0] == np.float32(lam) and np.all(val[0, 1:] == np.float32(np.float32(lam) - np.float32(oml * 2.0)))
    # all-zero rows: deg = 0 everywhere, p stays alpha b after the first step, rel is uniform; picks in index order
    assert np.all(rel[starts[1]: starts[1] + 6] == 1.0) and pos[1].tolist() == [0, 1, 2, 3]
    # a threshold above every similarity: the graph has no edge, rel is uniform (the prior's), picks by redundancy
    high = dict(PARAMS, edge_threshold=1000.0)
    pos2, val2, rel2, used2 = launch(N, rows, d, starts, lens, cost, [100, 100, 100], 4, params=high)
    assert np.all(rel2[starts[2]: starts[2] + 16] == 1.0)
    check_unit("t above all", as_stored(other, torch.float16), None, costs[2], 100, 4, high, pos2[2], val2[2],
               rel2[starts[2]: starts[2] + 16], int(used2[2]), d)


def test_an_invalid_unit_between_valid_ones_and_mixed_bias(N):
    d = 768
    rng = np.random.default_rng(6)
    units = [exact_rows(rng, 17, d), exact_rows(rng, 16, d), exact_rows(rng, 65, d)]
    costs = [rng.integers(1, 5, len(x)) for x in units]
    bias = exact_rows(rng, 1, d)
    rows, starts, lens, cost, bias_t = pack(N, units, costs, torch.bfloat16, d, bias=bias)
    n_rows = rows.shape[0]
    k = 8
    good = launch(N, rows, d, starts, lens, cost, [20, 20, 20], k, bias=bias_t, unit_bias=[0, -1, 0])
    for u in range(3):
        q = as_stored(bias[0], torch.bfloat16) if u != 1 else None
        check_unit(f"mixed bias u={u}", as_stored(units[u], torch.bfloat16), q, costs[u], 20, k, PARAMS, good[0][u],
                   good[1][u], good[2][starts[u]: starts[u] + lens[u]], int(good[3][u]), d)
    # the entries a device table may hold by mistake: a length of 0, above 128, negative; a start below 0; rows past the
    # plane; a bias index outside the bias rows.  None of them indexes memory: the unit is marked, its neighbours are
    # what they were
    for bad_start, bad_len, bad_bias in ((starts[1], 0, -1), (starts[1], 129, -1), (starts[1], -5, -1),
                                         (-1, 16, -1), (n_rows - 3, 16, -1), (2 ** 31 - 8, 16, -1),
                                         (starts[1], 16, 1), (starts[1], 16, -2)):
        s2, l2 = starts.copy(), lens.copy()
        s2[1], l2[1] = bad_start, bad_len
        sentinel = (torch.full((3, k), 77, dtype=torch.int32).cuda(), torch.full((3, k), 77.0).cuda(),
                    torch.full((n_rows,), 77.0).cuda(), torch.full((3,), 77, dtype=torch.int32).cuda())
        pos, val, rel, used = launch(N, rows, d, s2, l2, cost, [20, 20, 20], k, bias=bias_t,
                                     unit_bias=[0, bad_bias, 0], out=sentinel)
        assert np.isnan(val[1, 0]) and np.all(pos[1] == -1) and used[1] == 0, (bad_start, bad_len, bad_bias)
        assert np.all(rel[starts[1]: starts[1] + 16] == 77.0)
        for u in (0, 2):
            assert np.array_equal(pos[u], good[0][u]) and np.array_equal(val[u].view(np.int32), good[1][u].view(np.int32))
            assert used[u] == good[3][u]
            lo, hi = starts[u], starts[u] + lens[u]
            assert np.array_equal(rel[lo:hi].view(np.int32), good[2][lo:hi].view(np.int32))


# ---------------------------------------------------------------- 4: reproducible
def test_a_unit_has_the_same_bits_wherever_it_runs(N):
    d, n, k = 384, 65, 16
    rng = np.random.default_rng(7)
    x = clustered_rows(rng, n, d)
    q = clustered_rows(rng, 1, d)
    c = rng.integers(20, 160, n)

    def bits_of(out, u, start):
        pos, val, rel, used = out
        return (pos[u].tobytes(), val[u].tobytes(), rel[start: start + n].tobytes(), int(used[u]))

    rows, starts, lens, cost, bias_t = pack(N, [x], [c], torch.float16, d, bias=q)
    alone = bits_of(launch(N, rows, d, starts, lens, cost, [300], k, bias=bias_t, unit_bias=[0]), 0, 0)
    again = bits_of(launch(N, rows, d, starts, lens, cost, [300], k, bias=bias_t, unit_bias=[0]), 0, 0)
    assert alone == again
    # at another plane offset
    rows2, starts2, lens2, cost2, _ = pack(N, [x], [c], torch.float16, d, lead=37)
    moved = bits_of(launch(N, rows2, d, starts2, lens2, cost2, [300], k, bias=bias_t, unit_bias=[0]), 0, 37)
    assert moved == alone
    # in a batch of 300 units (the unit is number 211; the others are smaller and different)
    others = [clustered_rows(rng, 1 + (u % 20), d) for u in range(300)]
    others[211] = x
    costs = [rng.integers(20, 160, len(o)) for o in others]
    costs[211] = c
    rows3, starts3, lens3, cost3, _ = pack(N, others, costs, torch.float16, d, gap=1)
    ub = np.full(300, -1, np.int32)
    ub[211] = 0
    batch = launch(N, rows3, d, starts3, lens3, cost3, np.full(300, 300), k, bias=bias_t, unit_bias=ub)
    assert bits_of(batch, 211, int(starts3[211])) == alone
    # under graph capture and replay
    tables = [dev_i32(a) for a in (starts, lens, cost, [300], [0])]
    out = (torch.zeros((1, k), dtype=torch.int32).cuda(), torch.zeros((1, k)).cuda(), torch.zeros(n).cuda(),
           torch.zeros(1, dtype=torch.int32).cuda())

    def call():
        N.summary_select(rows, d, tables[0], tables[1], tables[2], tables[3], k, bias_rows=bias_t, unit_bias=tables[4],
                         out=out, **PARAMS)

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
    assert bits_of(tuple(t.cpu().numpy() for t in out), 0, 0) == alone


# ---------------------------------------------------------------- 5: argument checks
def test_bad_arguments_are_refused_and_nothing_is_launched(N):
    d = 384
    rng = np.random.default_rng(8)
    rows, starts, lens, cost, bias_t = pack(N, [exact_rows(rng, 16, d)], [np.ones(16, np.int32)], torch.float16, d,
                                            bias=exact_rows(rng, 1, d))
    tables = [dev_i32(a) for a in (starts, lens, cost, [10])]
    out = (torch.full((1, 4), 77, dtype=torch.int32).cuda(), torch.full((1, 4), 77.0).cuda(),
           torch.full((16,), 77.0).cuda(), torch.full((1,), 77, dtype=torch.int32).cuda())

    def refused(rows=rows, d=d, k=4, tables=tables, **kw):
        params = dict(PARAMS, **{key: kw.pop(key) for key in list(kw) if key in PARAMS})
        with pytest.raises(N.MMRagNativeError):
            N.summary_select(rows, d, *tables, k, out=out, **params, **kw)

    refused(k=0)
    refused(k=129)
    refused(iterations=-1)
    refused(iterations=65)
    refused(alpha=0.0)
    refused(alpha=1.5)
    refused(alpha=float("nan"))
    refused(lam=-0.1)
    refused(lam=1.1)
    refused(edge_threshold=-0.5)
    refused(edge_threshold=float("inf"))
    refused(d=0)
    refused(d=rows.shape[1] + 1)
    refused(rows=torch.zeros((16, 100), dtype=torch.float16).cuda(), d=100)         # a pitch of 200 bytes
    refused(rows=torch.zeros((16, 384), dtype=torch.uint8).cuda().view(torch.float8_e4m3fn))   # FP8: not summarised
    refused(rows=rows.cpu())                                                          # host tensors
    refused(tables=[tables[0], tables[1], tables[2][:5], tables[3]])                  # cost: one entry per row
    refused(tables=[tables[0][:0], tables[1][:0], tables[2], tables[3][:0]])          # no unit
    refused(bias_rows=bias_t)                                                         # a bias triple given in part
    refused(bias_rows=bias_t.float(), unit_bias=dev_i32([0]))                         # bias rows of another dtype
    st = N.lib().mmrag_summary_select(rows.data_ptr(), rows.shape[1], 1, d, rows.shape[0], tables[0].data_ptr(),
                                      tables[1].data_ptr(), 1, tables[2].data_ptr(), tables[3].data_ptr(),
                                      bias_t.data_ptr(), 0, None, 0.1, 0.15, 32, 0.7, 4, out[0].data_ptr(),
                                      out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None)
    assert st == 1      # MMRAG_EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out)


# ---------------------------------------------------------------- 6: through the product
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
         "Each cell frees electrons when light strikes it.", "An inverter turns the direct current into grid power.",
         "Panels lose a little output every year they age.", "Dust on the glass lowers what a panel yields."]
BREAD = ["Sourdough bread starts from a living culture of flour and water.", "The dough proofs overnight in the cold.",
         "A hot cast iron pot gives the loaf its crust.", "Steam in the first minutes lets the loaf rise.",
         "Scoring the dough decides where the crust opens.", "The crumb sets while the loaf cools on a rack."]


def check_summary(text, got, max_length):
    assert len(got["summary"]) <= max_length and got["summary"]
    assert got["summary"] == " ".join(text[a:b] for a, b in got["spans"])
    assert got["spans"] == sorted(got["spans"]) and len(set(got["spans"])) == len(got["spans"])     # order, no duplicate
    assert all(0 <= a < b <= len(text) and text[a:b] == text[a:b].strip() for a, b in got["spans"])
    assert all(b <= a2 for (_, b), (a2, _) in zip(got["spans"], got["spans"][1:]))                 # no overlap
    assert len(got["scores"]) == len(got["spans"]) and all(0.0 <= s <= 1.0 for s in got["scores"])


def test_summarize_texts_on_the_seeded_encoder(N, manager):
    from multimodal_rag_amd.ingest import fallback_summary

    assert manager.supports_summaries()
    two_topics = " ".join(a + " " + b for a, b in zip(SOLAR, BREAD))
    short = "  A short text is its own summary.  "
    many = " ".join(f"Sentence number {i} talks about topic {i % 7}." for i in range(300))
    assert len(two_topics) > 300
    got = asyncio.run(manager.summarize_texts([two_topics, short, many, ""], max_length=300))
    check_summary(two_topics, got[0], 300)
    assert len(got[0]["spans"]) >= 2
    assert got[1]["summary"] == fallback_summary(short, 300) == short.strip()
    check_summary(many, got[2], 300)        # more than 128 sentences: three sections share the budget
    assert got[3]["summary"] == fallback_summary("", 300)
    # the same call again gives the same answer, and a question moves nothing it should not
    assert asyncio.run(manager.summarize_texts([two_topics, short, many, ""], max_length=300)) == got
    asked = asyncio.run(manager.summarize_texts([two_topics], max_length=200, questions=["how does bread rise"]))
    check_summary(two_topics, asked[0], 200)


def test_extract_answer_quotes_map_back_to_the_passages(N, manager):
    passages = [" ".join(SOLAR), " ".join(BREAD), "", "One more passage. It has two sentences."]
    got = asyncio.run(manager.extract_answer("how do solar panels make power", passages, max_chars=200,
                                             top_sentences=3))
    assert got["considered"] == len(SOLAR) + len(BREAD) + 2
    assert 1 <= len(got["quotes"]) <= 3 and len(got["answer"]) <= 200
    keys = [(q["passage"], q["start"]) for q in got["quotes"]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for q in got["quotes"]:
        assert passages[q["passage"]][q["start"]: q["end"]] == q["text"] and q["text"] and 0.0 <= q["score"] <= 1.0
    assert got["answer"] == " ".join(q["text"] for q in got["quotes"])
    # more than 128 sentences: the rest is dropped and the count says so
    long = [" ".join(f"Fact {i} of passage {p}." for i in range(50)) for p in range(4)]
    assert asyncio.run(manager.extract_answer("fact 3", long))["considered"] == 128
    assert asyncio.run(manager.extract_answer("anything", ["", "   "])) == {"answer": "", "quotes": [], "considered": 0}


def test_upload_embeds_the_central_sentence_under_the_extractive_setting(N, manager, monkeypatch):
    """a chunk whose distinctive LAST sentence is repeated in paraphrase across the chunk: it is central, so the stored
    summary holds it; under the default setting the stored summary is the 300-character prefix, unchanged"""
    from starlette.testclient import TestClient

    from multimodal_rag_amd import embedder as EM
    from multimodal_rag_amd.ingest import fallback_summary
    from multimodal_rag_amd.server import create_app

    last = "The reactor valve must stay closed during the pressure test."
    fillers = ["Lunch is served at noon in the canteen.", "The parking lot is repainted in spring.",
               "Visitors sign the book at the front desk.", "The library closes early on Fridays.",
               "Coffee machines are cleaned every week.", "The choir meets on Tuesday evenings."]
    # the echoes are the two halves of the last sentence: it shares half of its words with each of them and they share
    # none with one another, so it is the hub of the family whatever the encoder makes of word overlap (the seeded
    # random-weight encoder makes every pair of sentences similar, which compresses rel but keeps its order)
    echoes = ["The reactor valve must stay closed.", "During the pressure test."]
    body = []
    for i, filler in enumerate(fillers):
        body.append(filler)
        if i < len(echoes):
            body.append(echoes[i])
    chunk = " ".join(body + [last])
    assert 300 < len(chunk) <= 1000 and last not in chunk[:300]
    for setting in ("extractive", "fallback"):
        monkeypatch.setattr(EM.settings, "MMRAG_SUMMARIZER", setting)
        with TestClient(create_app(embedder=manager)) as client:
            up = client.post("/upload", files={"file": ("valve.txt", chunk.encode("utf-8"), "text/plain")})
            assert up.status_code == 200, up.text
            stored = manager.collection.get(where={"doc_id": up.json()["doc_id"]})["documents"]
            assert len(stored) == 1
            if setting == "extractive":
                assert len(stored[0]) <= 300 and stored[0] != fallback_summary(chunk, 300)
                assert last in stored[0], stored[0]        # the central sentence made it into the summary
                got = client.post("/query", json={"query": "reactor valve pressure test", "top_k": 1,
                                                  "extractive_answer": True}).json()
                assert got["sources"] and got["sources"][0]["quotes"]
                for quote in got["sources"][0]["quotes"]:
                    assert chunk[quote["start"]: quote["end"]] == quote["text"]
                assert got["answer"] == " ".join(quote["text"] for quote in got["sources"][0]["quotes"])
            else:
                assert stored[0] == fallback_summary(chunk, 300)
            manager.collection.delete(where={"doc_id": up.json()["doc_id"]})
