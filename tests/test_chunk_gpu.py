"""GPU: semantic chunking -- the kernel (csrc/chunk.hip, mmrag_chunk_boundaries) against tests/chunk_ref.py, and the
layers above it.

Every kernel case packs its documents back to back in one plane: one document starts at row 0, one ends at the last
row, and rows of POISON (large values) sit between documents, so a read past a document's `len` shows as a huge
similarity.  n in {1, 2, 63, 64, 65, 127, 128, 129, 191, 193, 300}: the seams of the 64-sentence step, the end of the
128-row tile, a `best` carried over more than two steps, a ragged last tile.  W in {1, 2, 17, 64}, d in {384, 768, 100}
(100: a padded pitch and a ragged last slab), the three storage dtypes.

Exact data: row entries are multiples of 1/8, six of them non-zero, tau and beta multiples of 1/64: every S_ij is
exact in float32, and the float32 model (chunk_ref.segment with np.float32, the kernel's order of operations) must
give the kernel's outputs bit for bit -- with a fixed tau every sum is exact too; with the automatic tau (a rounded
division) the sums round, in the same order on both sides.

Real-shaped data: the bound E (derived, not fitted).  The kernel maximises its own float32 evaluation F~ of a
partition's objective F; float32 addition is monotone, so best[n] >= F~(P) for every admissible P.  If |F~(P) - F(P)|
<= E for every P then F(kernel's partition) >= F~(kernel's) - E >= F~(optimum) - E >= F(optimum) - 2 E, and best[n]
lies within E of F(optimum).  For a partition into chunks of m_c <= W sentences (sum m_c = n):
  pairs      P = sum m_c (m_c - 1) / 2 <= n (W - 1) / 2
  S_ij       at most (d + 1) 2^-24 each for unit rows (d products, d additions in float32, values <= 1)
  roundings  per pair one subtraction S - tau and one addition into R; per chunk m_c - 1 additions into G, one
             G - beta and one best + (.): at most 2 P + 3 n in all, each at most 2^-24 M with M the largest magnitude
             among the partial sums and differences the float64 reference forms
  E = n (W - 1) / 2 * (d + 1) 2^-24 + (n (W - 1) + 3 n) 2^-24 M
(F itself is evaluated in float64 with the kernel's own tau; its error, some 2^-53 M per operation, is far below
2^-24 of anything above.)  tau: |tau - ref| <= (d + 2) 2^-24 auto_scale.
"""
import asyncio

import numpy as np
import pytest
import torch

from tests import chunk_ref as R

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 193, 300)
WS = (1, 2, 17, 64)
DS = (384, 768, 100)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
POISON = 100.0
TAU, BETA, CAP = 12 / 64.0, 1 / 64.0, 40
EINVAL = 1


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def pack(N, docs, costs, dtype, d, lead=0, gap=2):
    """docs (float arrays [n, d]) back to back with `gap` POISON rows between them (and `lead` before the first) ->
    (rows tensor [n_rows, ld] on the device, starts, lens, cost [n_rows])"""
    ld = N.padded_dim(d, dtype)
    parts, cost_parts, starts, at = [], [], [], 0
    for u, (x, c) in enumerate(zip(docs, costs)):
        fill = lead if u == 0 else gap
        if fill:
            parts.append(np.full((fill, ld), POISON, np.float32))
            cost_parts.append(np.ones(fill, np.int32))
            at += fill
        body = np.zeros((len(x), ld), np.float32)
        body[:, :d] = x
        parts.append(body)
        cost_parts.append(np.asarray(c, np.int32))
        starts.append(at)
        at += len(x)
    rows = np.concatenate(parts)
    rows[:, d:] = 0.0
    return (torch.from_numpy(rows).to(dtype).cuda().contiguous(), np.asarray(starts, np.int32),
            np.asarray([len(x) for x in docs], np.int32), np.concatenate(cost_parts))


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def launch(N, rows, d, starts, lens, cost, max_cost, W, out=None, **kw):
    got = N.chunk_boundaries(rows, d, dev_i32(starts), dev_i32(lens), dev_i32(cost), max_cost, W, out=out, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in got)


def sentinels(n_rows, n_docs):
    return (torch.full((n_rows,), 77, dtype=torch.int32).cuda(), torch.full((n_rows,), 77.0).cuda(),
            torch.full((n_docs,), 77.0).cuda(), torch.full((n_docs,), 77.0).cuda())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------- 1: exact data
def exact_rows(rng, n, d):
    """multiples of 1/8, 6 non-zeros per row: 4 among the first 12 columns (so rows overlap), 2 anywhere -- the last
    column of the ragged slab included"""
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        cols = np.concatenate([rng.choice(12, 4, replace=False), rng.integers(12, d, 1), [d - 1]])
        x[i, cols] = rng.integers(-2, 9, len(cols)) / 8.0
    return x


def exact_docs(d):
    rng = np.random.default_rng(2000 + d)
    docs = [exact_rows(rng, n, d) for n in NS]
    same = np.zeros((9, d), np.float32)
    same[:, :3] = 0.25                      # <x, x> = 3/16 = TAU for every pair: every gain ties
    docs += [same, np.zeros((6, d), np.float32)]
    costs = [rng.integers(1, 9, len(x)) for x in docs]
    return docs, costs


_MODEL = {}


def exact_model(d, W, auto_scale, max_cost=CAP):
    """the float32 model of every document of exact_docs(d), computed once and shared by the three dtypes (the rows
    are exact in each of them)"""
    key = (d, W, auto_scale, max_cost)
    if key not in _MODEL:
        docs, costs = exact_docs(d)
        out = []
        for x, c in zip(docs, costs):
            S = R.similarities(x)
            tau = R.auto_tau(S, auto_scale, np.float32) if auto_scale else np.float32(TAU)
            prev, best = R.segment(S, c, max_cost, W, tau, BETA, np.float32)
            out.append((prev, best, tau))
        _MODEL[key] = out
    return _MODEL[key]


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_exact_data_bit_for_bit(N, name, d):
    docs, costs = exact_docs(d)
    rows, starts, lens, cost = pack(N, docs, costs, DTYPES[name], d)
    assert starts[0] == 0 and starts[-1] + lens[-1] == rows.shape[0]
    for W in WS:
        for auto_scale in (0.0, 0.5):
            prev, best, tau, score = launch(N, rows, d, starts, lens, cost, CAP, W, threshold=TAU,
                                            auto_scale=auto_scale, penalty=BETA)
            for u, (ref_prev, ref_best, ref_tau) in enumerate(exact_model(d, W, auto_scale)):
                tag = (name, d, W, auto_scale, int(lens[u]))
                lo, hi = starts[u], starts[u] + lens[u]
                assert np.array_equal(prev[lo:hi], ref_prev), tag
                assert np.array_equal(bits(best[lo:hi]), bits(ref_best)), tag
                assert bits(tau[u]) == bits(ref_tau) and bits(score[u]) == bits(ref_best[-1]), tag


def test_exact_data_the_cap_binds_in_some_chunks_and_not_in_others():
    """a statement about the inputs of the test above (no GPU work): under W = 64 the cap changes the segmentation of
    the long documents, and some of their chunks are well below it"""
    d = 384
    docs, costs = exact_docs(d)
    changed = slack = 0
    for u, (prev, _, _) in enumerate(exact_model(d, 64, 0.0)):
        free = exact_model(d, 64, 0.0, max_cost=10 ** 9)[u][0]
        changed += not np.array_equal(prev, free)
        cuts = R.cuts_of(prev)
        sums = [int(costs[u][a:b].sum()) for a, b in zip(cuts, cuts[1:] + [len(prev)])]
        slack += any(s + 8 <= CAP for s in sums)
    assert changed >= 5 and slack >= 5, (changed, slack)


# ---------------------------------------------------------------- 2: real-shaped data
def topic_runs(rng, n, d):
    """Gaussian topic runs of 3..40 sentences: each sentence is its run's centre plus 0.6 x standard normal noise,
    normalised, cast to fp16 -> (rows, the planted chunk starts)"""
    starts, at = [], 0
    while at < n:
        starts.append(at)
        at += int(rng.integers(3, 41))
    if n - starts[-1] < 3 and len(starts) > 1:
        starts.pop()
    x = np.empty((n, d))
    for a, b in zip(starts, starts[1:] + [n]):
        x[a:b] = rng.standard_normal(d) + 0.6 * rng.standard_normal((b - a, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16), starts


def bound(n, d, W, peak):
    pairs = n * (W - 1) / 2.0
    return pairs * (d + 1) * 2.0 ** -24 + (2 * pairs + 3 * n) * 2.0 ** -24 * peak


@pytest.mark.parametrize("d", DS)
def test_real_shaped_data_reaches_the_optimum(N, d):
    W, scale, beta, huge = 64, 0.5, 0.0, 10 ** 9
    cases = []
    for n in (65, 129, 300):
        rng = np.random.default_rng([n, d])
        x, planted = topic_runs(rng, n, d)
        cases.append((x, planted, rng.integers(20, 160, n)))
    rows, starts, lens, cost = pack(N, [x for x, _, _ in cases], [c for _, _, c in cases], torch.float16, d)
    for max_cost in (huge, 1000):                   # no cap; a cap that cuts the longer runs
        prev, best, tau, score = launch(N, rows, d, starts, lens, cost, max_cost, W, auto_scale=scale, penalty=beta)
        for u, (x, planted, c) in enumerate(cases):
            n = len(x)
            S = R.similarities(x.astype(np.float64))
            ref_tau = float(R.auto_tau(S, scale))
            tau_bound = (d + 2) * 2.0 ** -24 * scale
            print(f"d={d} n={n} cap={max_cost}: tau {tau[u]:.7f} ref {ref_tau:.7f} "
                  f"err {abs(float(tau[u]) - ref_tau):.3e} (bound {tau_bound:.3e})")
            assert abs(float(tau[u]) - ref_tau) <= tau_bound
            stats = {}
            ref_prev, ref_best = R.segment(S, c, max_cost, W, float(tau[u]), beta, np.float64, stats)
            E = bound(n, d, W, stats["peak"])
            lo = int(starts[u])
            cuts = R.cuts_of(prev[lo: lo + n])
            assert cuts[0] == 0 and cuts == sorted(set(cuts)) and R.admissible(cuts, n, c, max_cost, W)
            got = R.objective(S, cuts, float(tau[u]), beta)
            print(f"   objective {got:.6f} optimum {ref_best[-1]:.6f} gap {ref_best[-1] - got:.3e} "
                  f"score err {abs(float(score[u]) - ref_best[-1]):.3e} (E {E:.3e}, peak {stats['peak']:.1f})")
            assert got >= ref_best[-1] - 2 * E
            assert abs(float(score[u]) - ref_best[-1]) <= E and score[u] == best[lo + n - 1]
            if max_cost == huge:
                assert cuts == planted, (d, n, cuts, planted)
            else:       # cuts are added only inside the runs that exceed the cap
                assert set(planted) <= set(cuts)
                for a, b in zip(planted, planted[1:] + [n]):
                    if c[a:b].sum() <= max_cost:
                        assert not any(a < cut < b for cut in cuts), (a, b, cuts)


# ---------------------------------------------------------------- 3: edges
def test_edges_singletons_one_sentence_and_chunks_as_long_as_admissible(N):
    d = 384
    rng = np.random.default_rng(3)
    docs = [exact_rows(rng, 70, d), exact_rows(rng, 1, d), exact_rows(rng, 150, d)]
    same = np.zeros((140, d), np.float32)
    same[:, :3] = 0.25
    docs.append(same)
    costs = [rng.integers(3, 9, len(x)) for x in docs]
    rows, starts, lens, cost = pack(N, docs, costs, torch.float16, d)

    def cuts(prev, u):
        return R.cuts_of(prev[starts[u]: starts[u] + lens[u]])

    # max_cost below every cost: all singletons, best[b] = -b beta
    prev, best, tau, score = launch(N, rows, d, starts, lens, cost, 2, 64, threshold=TAU, penalty=BETA)
    for u in range(4):
        assert cuts(prev, u) == list(range(lens[u]))
        assert np.array_equal(best[starts[u]: starts[u] + lens[u]], -BETA * np.arange(1, lens[u] + 1, dtype=np.float32))
    # n = 1: one chunk whatever the parameters; the automatic tau of a single sentence is 0
    prev, best, tau, score = launch(N, rows, d, starts, lens, cost, 1, 64, auto_scale=0.5, penalty=0.25)
    assert prev[starts[1]] == 0 and best[starts[1]] == -0.25 == score[1] and tau[1] == 0.0
    # max_cost huge with W = 64, and beta large enough that no partition has a chunk more than it needs: ceil(n / 64)
    # chunks (which ones, the gains decide: the model's, bit for bit -- every sum is a multiple of 1/64 below 2^14)
    prev, best, tau, score = launch(N, rows, d, starts, lens, cost, 2 ** 31 - 1, 64, threshold=TAU, penalty=4096.0)
    assert [len(cuts(prev, u)) for u in range(4)] == [2, 1, 3, 3]
    for u in (0, 1, 2):
        S = R.similarities(docs[u])
        ref_prev, ref_best = R.segment(S, costs[u], 2 ** 31 - 1, 64, TAU, 4096.0, np.float32)
        assert np.array_equal(prev[starts[u]: starts[u] + lens[u]], ref_prev)
        assert np.array_equal(bits(best[starts[u]: starts[u] + lens[u]]), bits(ref_best))
    # the same under a cap: each chunk holds as many sentences as the cap admits, counted from the END
    cap = 30
    prev, _, _, _ = launch(N, rows, d, starts, lens, cost, cap, 64, threshold=TAU, penalty=4096.0)
    assert np.array_equal(prev[starts[2]: starts[2] + 150], R.segment(R.similarities(docs[2]), costs[2], cap, 64, TAU,
                                                                      4096.0, np.float32)[0])
    # identical sentences with S = tau and beta = 0: every gain is 0, every candidate ties, the lowest a wins
    prev, best, _, _ = launch(N, rows, d, starts, lens, cost, 2 ** 31 - 1, 64, threshold=TAU, penalty=0.0)
    assert np.array_equal(prev[starts[3]: starts[3] + 140], np.maximum(np.arange(1, 141) - 64, 0))
    assert np.all(best[starts[3]: starts[3] + 140] == 0.0)


# ---------------------------------------------------------------- 4: invalid documents
def test_invalid_documents_between_valid_ones(N):
    d = 768
    rng = np.random.default_rng(4)
    docs = [exact_rows(rng, 70, d), exact_rows(rng, 16, d), exact_rows(rng, 130, d)]
    costs = [rng.integers(1, 9, len(x)) for x in docs]
    rows, starts, lens, cost = pack(N, docs, costs, torch.bfloat16, d)
    n_rows = rows.shape[0]
    kw = dict(threshold=TAU, auto_scale=0.5, penalty=BETA)
    good = launch(N, rows, d, starts, lens, cost, CAP, 17, **kw)
    assert np.isfinite(good[3]).all()
    # the entries a device table may hold by mistake: none of them indexes memory, the document is marked, its rows of
    # the outputs stay as they were and its neighbours are what they were
    for bad_start, bad_len in ((starts[1], 0), (starts[1], -5), (-1, 16), (n_rows - 3, 16), (2 ** 31 - 8, 16),
                               (2 ** 31 - 1, 2 ** 31 - 1)):
        s2, l2 = starts.copy(), lens.copy()
        s2[1], l2[1] = bad_start, bad_len
        prev, best, tau, score = launch(N, rows, d, s2, l2, cost, CAP, 17, out=sentinels(n_rows, 3), **kw)
        assert np.isnan(score[1]) and tau[1] == 77.0, (bad_start, bad_len)
        valid = np.zeros(n_rows, bool)
        for u in (0, 2):
            valid[starts[u]: starts[u] + lens[u]] = True
            assert bits(tau[u]) == bits(good[2][u]) and bits(score[u]) == bits(good[3][u])
        assert np.array_equal(prev[valid], good[0][valid]) and np.array_equal(bits(best[valid]), bits(good[1][valid]))
        assert np.all(prev[~valid] == 77) and np.all(best[~valid] == 77.0)


# ---------------------------------------------------------------- 5: reproducible
def test_a_document_has_the_same_bits_wherever_it_runs(N):
    d, n, W = 384, 193, 64
    rng = np.random.default_rng(7)
    x, _ = topic_runs(rng, n, d)
    c = rng.integers(20, 160, n)
    kw = dict(auto_scale=0.5, penalty=0.125)

    def bits_of(out, u, start):
        prev, best, tau, score = out
        return (prev[start: start + n].tobytes(), best[start: start + n].tobytes(), tau[u].tobytes(), score[u].tobytes())

    rows, starts, lens, cost = pack(N, [x], [c], torch.float16, d)
    alone = bits_of(launch(N, rows, d, starts, lens, cost, 1000, W, **kw), 0, 0)
    assert bits_of(launch(N, rows, d, starts, lens, cost, 1000, W, **kw), 0, 0) == alone
    # at another plane offset
    rows2, starts2, lens2, cost2 = pack(N, [x], [c], torch.float16, d, lead=37)
    assert bits_of(launch(N, rows2, d, starts2, lens2, cost2, 1000, W, **kw), 0, 37) == alone
    # in a batch of 300 documents (the document is number 211; the others are smaller and different)
    others = [topic_runs(rng, 1 + (u % 20), d)[0] for u in range(300)]
    others[211] = x
    costs = [rng.integers(20, 160, len(o)) for o in others]
    costs[211] = c
    rows3, starts3, lens3, cost3 = pack(N, others, costs, torch.float16, d, gap=1)
    batch = launch(N, rows3, d, starts3, lens3, cost3, 1000, W, **kw)
    assert bits_of(batch, 211, int(starts3[211])) == alone
    # under graph capture and replay
    tables = [dev_i32(a) for a in (starts, lens, cost)]
    out = (torch.zeros(n, dtype=torch.int32).cuda(), torch.zeros(n).cuda(), torch.zeros(1).cuda(), torch.zeros(1).cuda())

    def call():
        N.chunk_boundaries(rows, d, tables[0], tables[1], tables[2], 1000, W, out=out, **kw)

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


# ---------------------------------------------------------------- 6: argument checks
def test_bad_arguments_are_refused_and_nothing_is_launched(N):
    d = 384
    rng = np.random.default_rng(8)
    rows, starts, lens, cost = pack(N, [exact_rows(rng, 16, d)], [np.ones(16, np.int32)], torch.float16, d)
    tables = [dev_i32(a) for a in (starts, lens, cost)]
    out = sentinels(16, 1)
    good = dict(max_cost=10, max_sentences=8, threshold=0.25, auto_scale=0.0, penalty=0.0)

    def refused(rows=rows, d=d, tables=tables, **kw):
        with pytest.raises(N.MMRagNativeError):
            N.chunk_boundaries(rows, d, *tables, out=out, **dict(good, **kw))

    def raw(rows=rows, ld=None, dtype=1, d=d, n_docs=1, **kw):
        p = dict(good, **kw)
        return N.lib().mmrag_chunk_boundaries(
            rows.data_ptr(), rows.shape[1] if ld is None else ld, dtype, d, rows.shape[0], tables[0].data_ptr(),
            tables[1].data_ptr(), n_docs, tables[2].data_ptr(), p["max_cost"], p["max_sentences"], p["threshold"],
            p["auto_scale"], p["penalty"], out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
            None)

    nan, inf = float("nan"), float("inf")
    for bad in (dict(max_cost=0), dict(max_cost=-3), dict(max_sentences=0), dict(max_sentences=65), dict(threshold=nan),
                dict(threshold=inf), dict(threshold=-inf), dict(auto_scale=-0.5), dict(auto_scale=inf),
                dict(auto_scale=nan), dict(penalty=-0.1), dict(penalty=inf), dict(penalty=nan)):
        refused(**bad)
        assert raw(**bad) == EINVAL, bad
    refused(d=0)
    refused(d=rows.shape[1] + 1)
    assert raw(d=0) == EINVAL and raw(d=rows.shape[1] + 1) == EINVAL
    assert raw(ld=100) == EINVAL                                                      # a pitch of 200 bytes
    refused(rows=torch.zeros((16, 100), dtype=torch.float16).cuda(), d=100)
    f8 = torch.zeros((16, 384), dtype=torch.uint8).cuda()
    refused(rows=f8.view(torch.float8_e4m3fn))                                        # FP8: not segmented
    assert raw(rows=f8, dtype=3) == EINVAL and raw(dtype=7) == EINVAL
    assert raw(n_docs=0) == EINVAL and raw(n_docs=-1) == EINVAL
    refused(rows=rows.cpu())                                                          # host tensors
    refused(tables=[tables[0].cpu(), tables[1], tables[2]])
    refused(tables=[tables[0], tables[1], tables[2][:5]])                             # cost: one entry per row
    refused(tables=[tables[0][:0], tables[1][:0], tables[2]])                         # no document
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out)
    assert raw() == 0                                                                 # and the good call is taken
    torch.cuda.synchronize()
    assert not bool((out[0] == 77).any())


# ---------------------------------------------------------------- 7: through the product
@pytest.fixture(scope="module")
def manager(N):
    from multimodal_rag_amd import embedder as EM

    names = ("MMRAG_MODEL_DIR", "MMRAG_ENCODER_PRECISION", "MMRAG_INDEX_DTYPE", "MMRAG_CHUNKER")
    saved = [getattr(EM.settings, n) for n in names]
    EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION = "", "fp16"
    EM.settings.MMRAG_INDEX_DTYPE, EM.settings.MMRAG_CHUNKER = "float16", "basic"
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
TWO_TOPICS = " ".join(SOLAR) + "\n\n" + " ".join(BREAD)
MANY = " ".join(f"Sentence number {i} talks about topic {i // 40}." for i in range(300))


def check_chunks(text, chunks, chunk_size):
    from multimodal_rag_amd.summarize import split_sentences

    spans = split_sentences(text, chunk_size)
    assert sum(c["sentences"] for c in chunks) == len(spans)
    at = 0
    for c in chunks:
        assert (c["start"], c["end"]) == (spans[at][0], spans[at + c["sentences"] - 1][1])
        at += c["sentences"]
        assert c["content"] == text[c["start"]: c["end"]] == c["content"].strip() and 0 < len(c["content"]) <= chunk_size
    assert all(p["end"] <= c["start"] for p, c in zip(chunks, chunks[1:]))


def test_chunk_texts_on_the_seeded_encoder(N, manager):
    from multimodal_rag_amd.chunking import DeviceChunker, semantic_costs
    from multimodal_rag_amd.config import settings
    from multimodal_rag_amd.summarize import split_sentences

    assert manager.supports_chunking()
    texts = [TWO_TOPICS, MANY, "Only one sentence here.", ""]
    size = 400
    got = asyncio.run(manager.chunk_texts(texts, chunk_size=size))
    assert [len(g) for g in got[2:]] == [1, 0] and got[2][0]["content"] == texts[2]
    for text, chunks in zip(texts[:2], got):
        check_chunks(text, chunks, size)
        assert len(chunks) >= 2
    assert asyncio.run(manager.chunk_texts(texts, chunk_size=size)) == got              # repeatable
    # the cuts against the float64 optimum over the rows the encoder gives for the same sentences, cast to the
    # chunker's dtype: the objective check of the real-shaped kernel test, whatever a seeded encoder thinks of topics
    params = settings.chunk_parameters()
    params.pop("overlap")
    worker = DeviceChunker(manager._engine, torch.float16)
    for text in texts[:2]:
        spans = split_sentences(text, size)
        flat = [text[a:b] for a, b in spans]
        costs = semantic_costs(text, spans)
        found = worker.segment([flat], [costs], size, **params)[0]
        # (the text on its own: the encoder call is then the one `segment` makes, sentence for sentence)
        chunks = asyncio.run(manager.chunk_texts([text], chunk_size=size))[0]
        assert [(b - a) for a, b, _ in found["runs"]] == [c["sentences"] for c in chunks]
        assert [g for _, _, g in found["runs"]] == [c["gain"] for c in chunks]
        order = sorted(range(len(flat)), key=lambda i: len(flat[i]))
        emb = manager._engine.encode_device([flat[i] for i in order])
        x = np.empty((len(flat), emb.shape[1]))
        x[order] = emb.to(torch.float16).to(torch.float64).cpu().numpy()
        n, d, W = len(flat), int(emb.shape[1]), params["max_sentences"]
        S = R.similarities(x)
        tau_bound = (d + 2) * 2.0 ** -24 * params["auto_scale"]
        ref_tau = float(R.auto_tau(S, params["auto_scale"]))
        print(f"n={n}: tau {found['tau']:.7f} ref {ref_tau:.7f} (bound {tau_bound:.3e})")
        assert abs(found["tau"] - ref_tau) <= tau_bound
        stats = {}
        _, ref_best = R.segment(S, costs, size, W, found["tau"], params["penalty"], np.float64, stats)
        E = bound(n, d, W, stats["peak"])
        cuts = [a for a, _, _ in found["runs"]]
        assert R.admissible(cuts, n, costs, size, W)
        value = R.objective(S, cuts, found["tau"], params["penalty"])
        print(f"   objective {value:.6f} optimum {ref_best[-1]:.6f} gap {ref_best[-1] - value:.3e} (E {E:.3e})")
        assert value >= ref_best[-1] - 2 * E and abs(found["score"] - ref_best[-1]) <= E


def test_upload_under_the_semantic_and_the_basic_setting(N, manager, monkeypatch):
    from starlette.testclient import TestClient

    from multimodal_rag_amd import embedder as EM
    from multimodal_rag_amd.ingest import basic_chunk_text, fallback_summary
    from multimodal_rag_amd.server import create_app

    monkeypatch.setattr(EM.settings, "CHUNK_SIZE", 300)         # chunks of at most 300 characters are their own summary
    monkeypatch.setattr(EM.settings, "CHUNK_OVERLAP", 50)
    for setting in ("semantic", "basic"):
        monkeypatch.setattr(EM.settings, "MMRAG_CHUNKER", setting)
        with TestClient(create_app(embedder=manager)) as client:
            up = client.post("/upload", files={"file": ("topics.txt", TWO_TOPICS.encode("utf-8"), "text/plain")})
            assert up.status_code == 200, up.text
            stored = manager.collection.get(where={"doc_id": up.json()["doc_id"]})
            docs, metas = stored["documents"], stored["metadatas"]
            if setting == "semantic":
                assert len(docs) >= 2 and up.json()["chunks_processed"]["text"] == len(docs)
                spans = sorted((m["char_start"], m["char_end"]) for m in metas)
                assert sorted(TWO_TOPICS[a:b] for a, b in spans) == sorted(docs)         # the raw chunk
                assert all(b <= a2 for (_, b), (a2, _) in zip(spans, spans[1:]))
                assert all(m["chunker"] == "semantic" and m["sentence_count"] >= 1 for m in metas)
                assert sum(m["sentence_count"] for m in metas) == len(SOLAR) + len(BREAD)
                preview = client.post("/chunk", json={"text": TWO_TOPICS, "chunk_size": 300}).json()
                assert sorted(c["content"] for c in preview["chunks"]) == sorted(docs)
                got = client.post("/query", json={"query": "how does bread rise", "top_k": 2})
                assert got.status_code == 200 and got.json()["sources"]
            else:
                want = [fallback_summary(c, 300) for c in basic_chunk_text(TWO_TOPICS, 300, 50)]
                assert sorted(docs) == sorted(want) and not any("chunker" in m or "char_start" in m for m in metas)
            manager.collection.delete(where={"doc_id": up.json()["doc_id"]})
