"""GPU: the walk kernel (csrc/search_qsw.hip) with its last Q k-step parked in LDS and the cold tile ends built on the
registers that frees (tile 0's maxima published before its selection, thresholds picked up before a selection, a
lane's k best of a tile taken from its sorted scores once some lane has many hits).

Every case runs the walk (`DBG_FORCE_QS`) against the CPU oracle and bit for bit against the slab-ring kernel
(`DBG_NO_QS`), which shares none of this."""
import numpy as np
import pytest
import torch

from oracle import search_oracle as O
from test_search_gpu import check, run, to_dev, unit_rows

pytestmark = pytest.mark.gpu

PARKED = 32   # dimensions of the last k-step of the 16x16x32 shape


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def alive_bits(alive):
    words = np.zeros((alive.shape[0] + 31) // 32 + 8, dtype=np.uint32)
    idx = np.nonzero(alive)[0]
    np.bitwise_or.at(words, idx // 32, (np.uint32(1) << (idx % 32).astype(np.uint32)))
    return torch.from_numpy(words.view(np.int32)).to("cuda")


def walk_vs_oracle_and_slab_ring(N, q, c, k, dtype, alive=None, exact=False):
    """the walk's answer: checked against the oracle (bit for bit if `exact`), equal to the slab-ring kernel's"""
    s, r, es, er = run(N, q, c, k, dtype, alive=alive, dbg=N.DBG_FORCE_QS)
    if exact:
        assert np.array_equal(s, es) and np.array_equal(r, er)
    else:
        check(s, r, es, er)
    qd, _ = to_dev(N, q, dtype)
    cd, _ = to_dev(N, c, dtype)
    bits = None if alive is None else alive_bits(alive)
    s2, r2 = N.cosine_topk(qd, cd, c.shape[0], c.shape[1], k, alive_bits=bits, dbg=N.DBG_NO_QS)
    assert np.array_equal(r2.cpu().numpy(), r) and np.array_equal(s2.cpu().numpy(), s)
    return s, r


def parked_signal(B, n, d, seed, planted=20):
    """queries and `planted` rows per query that are zero outside the last PARKED dimensions; every other row random.
    A query's planted rows are the only ones whose score comes near 1, and all of that score is made by the parked
    k-step: a stale, misplaced or missing parked fragment changes the top-5 outright."""
    g = np.random.default_rng(seed)
    q = np.zeros((B, d), dtype=np.float32)
    q[:, d - PARKED:] = unit_rows(B, PARKED, seed + 1)
    c = unit_rows(n, d, seed + 2)
    rows = g.choice(n, size=B * planted, replace=False)
    tail = np.repeat(q[:, d - PARKED:], planted, axis=0)
    tail = tail + 0.05 * np.tile(np.arange(1, planted + 1, dtype=np.float32), B)[:, None] * unit_rows(B * planted, PARKED, seed + 3)
    c[rows] = 0.0
    c[rows, d - PARKED:] = tail / np.linalg.norm(tail, axis=1, keepdims=True)
    return q, c, rows.reshape(B, planted)


@pytest.mark.parametrize("B,n,d,dtype", [
    (256, 400_003, 768, torch.float16),     # 3 x 4 ring
    (300, 250_000, 384, torch.bfloat16),    # two query groups, 768-byte rows
    (256, 420_000, 512, torch.float16),     # 1024-byte rows: the 2 x 6 ring, the last k-step sits in another stage
])
def test_signal_only_in_the_parked_dimensions(N, B, n, d, dtype):
    q, c, rows = parked_signal(B, n, d, 101)
    s, r = walk_vs_oracle_and_slab_ring(N, q, c, 5, dtype)
    assert np.all(s[:, 4] > 0.5)                               # the planted rows, not the random ones
    assert all(set(r[i]) <= set(rows[i]) for i in range(B))


@pytest.mark.parametrize("B,n", [(200, 200_000), (130, 393_300)])   # the exchange without tickets; a half-empty group
def test_padding_query_slots(N, B, n):
    """56 / 126 dead query slots per workgroup: their zeroed parked fragments (and zero scores everywhere) must never open
    the insertion path or reach the exchange; the planted signal sits in the parked dimensions here too"""
    q, c, rows = parked_signal(B, n, 768, 111)
    s, r = walk_vs_oracle_and_slab_ring(N, q, c, 5, torch.float16)
    assert all(set(r[i]) <= set(rows[i]) for i in range(B))
    walk_vs_oracle_and_slab_ring(N, unit_rows(B, 768, 112), unit_rows(n, 768, 113), 5, torch.float16)


@pytest.fixture(scope="module")
def integer_data():
    g = np.random.default_rng(121)
    ci = g.integers(-2, 3, size=(400_003, 384)).astype(np.float32)
    qi = g.integers(-2, 3, size=(256, 384)).astype(np.float32)
    return qi, ci


@pytest.mark.parametrize("k", [1, 3, 5])
def test_ties_through_the_cold_path(N, integer_data, k):
    """integer data in -2 .. 2: exact scores, ties everywhere (a lane's k-th largest score of a tile is shared by
    several rows) -> the lower row wins, bit for bit as the oracle has it"""
    qi, ci = integer_data
    walk_vs_oracle_and_slab_ring(N, qi, ci, k, torch.float16, exact=True)


def test_ties_with_three_live_rows(N, integer_data):
    """an alive mask that leaves 3 rows: no lane ever gets a threshold, every tile goes through the sorted scores with
    -inf everywhere else"""
    qi, ci = integer_data
    few = np.zeros(ci.shape[0], dtype=bool)
    few[[7, 200_000, ci.shape[0] - 1]] = True
    walk_vs_oracle_and_slab_ring(N, qi, ci, 5, torch.float16, alive=few, exact=True)


def test_second_launch_on_the_same_workspace(N):
    """one shape twice on one workspace with other queries in between: nothing of a launch (exchange block, parked
    fragments, lists) may reach the next"""
    B, n, d = 256, 400_003, 768
    q, c, _ = parked_signal(B, n, d, 131)
    qd, _ = to_dev(N, q, torch.float16)
    cd, _ = to_dev(N, c, torch.float16)
    q2d, _ = to_dev(N, unit_rows(B, d, 132), torch.float16)
    ws = torch.empty(N.cosine_topk_workspace_bytes(B, n, 5), dtype=torch.uint8, device="cuda")
    first = [t.cpu().numpy() for t in N.cosine_topk(qd, cd, n, d, 5, workspace=ws, dbg=N.DBG_FORCE_QS)]
    other = [t.cpu().numpy() for t in N.cosine_topk(q2d, cd, n, d, 5, workspace=ws, dbg=N.DBG_FORCE_QS)]
    again = [t.cpu().numpy() for t in N.cosine_topk(qd, cd, n, d, 5, workspace=ws, dbg=N.DBG_FORCE_QS)]
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    assert not np.array_equal(other[1], first[1])
    es, er = O.cosine_topk(qd[:, :d].float().cpu().numpy(), cd[:n, :d].float().cpu().numpy(), 5)
    check(first[0], first[1], es, er)
