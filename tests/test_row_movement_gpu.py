"""GPU: the row-movement kernels of csrc/common.hip called directly -- append_rows (the float32 -> storage cast every
`add` and every packed query goes through), gather_rows (compaction, stored examples) and fetch_rows_f32 (`get`).

append_rows is compared BIT FOR BIT with torch's CPU cast (round to nearest even) over values chosen at the rounding
edges of fp16 and bf16; pad columns must come out zero and every byte outside the written rows must stay as it was.
gather_rows and fetch_rows_f32 move bits and are compared as bytes.  The sizes cross the grid cap of 8 * CUs * 256
threads once each, so the grid-stride loops take a second trip."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
POISON = 0x7F
EINVAL = 1


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _native():
    from multimodal_rag_amd import _native

    return _native


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def near(x):
    """x, the float32 just below it and the one just above it, and their negatives"""
    x = np.float32(x)
    v = np.array([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))], np.float32)
    return np.concatenate([v, -v])


def edge_values() -> np.ndarray:
    """float32 values at the rounding edges of the two 16-bit formats"""
    parts = [
        # fp16 (10 mantissa bits): halfway between 1 and 1 + 2^-10 (ties to even: down), halfway between 1 + 2^-10 and
        # 1 + 2^-9 (up), each with its two float32 neighbours, which are no ties
        near(1.0 + 2.0 ** -11), near(1.0 + 3 * 2.0 ** -11), near(1024.0 + 0.5), near(1024.0 + 1.5),
        # bf16 (7 mantissa bits): the same two ties
        near(1.0 + 2.0 ** -8), near(1.0 + 3 * 2.0 ** -8), near(256.0 + 1.0), near(256.0 + 3.0),
        # fp16 subnormals: the smallest, an odd multiple, half the smallest (a tie: to zero), just under and just over
        # it, one and a half (a tie: up to 2 * 2^-24), the largest subnormal and the smallest normal
        near(2.0 ** -24), near(3 * 2.0 ** -24), near(2.0 ** -25), near(1.5 * 2.0 ** -24), near(2.0 ** -14 - 2.0 ** -24),
        near(2.0 ** -14), near(2.0 ** -14 + 2.0 ** -25),
        # zeros, the largest fp16, the first float32 above it (rounds back to it), 65520 = the tie that rounds to inf,
        # and the float32 just below it (the last that rounds to 65504)
        np.array([0.0, -0.0], np.float32), near(65504.0), near(65520.0), near(65536.0),
        # the edges of bf16's range: the largest bf16, the float32 values above it that round to inf
        f32([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0xFF7FFFFF]),
        # float32 subnormals and the smallest normal (bf16 keeps float32's exponent range)
        f32([0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00800000, 0x80008000]),
        np.array([np.inf, -np.inf, np.nan], np.float32),
    ]
    return np.concatenate(parts).astype(np.float32)


def source(m: int, d: int, seed: int) -> np.ndarray:
    """[m, d] float32: the edge values first, then seeded values of every magnitude a row can hold"""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(m * d) * np.exp2(g.integers(-26, 17, m * d))).astype(np.float32)
    e = edge_values()
    x[: min(e.size, x.size)] = e[: x.size]
    if x.size > 2 * e.size:
        x[-e.size:] = e[::-1]          # and again at the end: the last row, the second trip of the loop
    return x.reshape(m, d)


def bits_of(t: torch.Tensor) -> np.ndarray:
    t = t.contiguous().cpu()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def assert_same_numbers(got: torch.Tensor, want: torch.Tensor):
    """bit for bit, NaN compared as "is NaN" """
    nan = torch.isnan(want.float())
    assert torch.equal(torch.isnan(got.float()), nan)
    g, w = bits_of(got), bits_of(want)
    keep = ~nan.numpy()
    bad = np.argwhere((g != w) & keep)
    assert not bad.size, (bad[:4].tolist(), [hex(int(g[tuple(i)]) & 0xFFFFFFFF) for i in bad[:4]],
                          [hex(int(w[tuple(i)]) & 0xFFFFFFFF) for i in bad[:4]])


def poisoned(rows: int, ld: int, dtype) -> torch.Tensor:
    """[rows, ld] of `dtype` whose every byte is 0x7F"""
    raw = torch.full((rows, ld * torch.empty(0, dtype=dtype).element_size()), POISON, dtype=torch.uint8, device=DEV)
    return raw.view(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("d,m", [(1, 300), (3, 131), (64, 37), (70, 37), (100, 37), (768, 5), (768, 1024)])
def test_append_rows_rounds_to_nearest_even_and_zeroes_the_pad(dtype, d, m):
    nat = _native()
    ld = nat.padded_dim(d, dtype)
    assert ld >= d
    if m == 1024:
        info = torch.cuda.get_device_properties(0)
        assert m * ld > 8 * info.multi_processor_count * 256          # the grid-stride loop takes a second trip
    n_used, tail = 3, 2
    x = source(m, d, 11 * d + m)
    dst = poisoned(n_used + m + tail, ld, dtype)
    nat.append_rows(dst, n_used, torch.from_numpy(x).to(DEV), d)
    torch.cuda.synchronize()
    got = dst.cpu()
    want = torch.from_numpy(x).to(dtype)                               # the CPU cast: round to nearest even
    assert_same_numbers(got[n_used: n_used + m, :d], want)
    assert not got[n_used: n_used + m, d:].contiguous().view(torch.uint8).any()    # pad columns [d, ld): zero bytes
    outside = torch.cat([got[:n_used], got[n_used + m:]]).view(torch.uint8)
    assert bool((outside == POISON).all())                             # rows outside [n_used, n_used + m): untouched


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_append_rows_edge_values_round_as_the_formats_say(dtype):
    """the reference itself pinned where the format decides: the ties and the overflow edges of fp16 / bf16"""
    if dtype == torch.float32:
        x = edge_values()
        assert_same_numbers(torch.from_numpy(x).to(dtype), torch.from_numpy(x))
        return
    if dtype == torch.float16:
        cases = [(1.0 + 2.0 ** -11, 1.0), (1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -9), (2.0 ** -25, 0.0),
                 (np.nextafter(np.float32(2.0 ** -25), np.float32(1.0)), 2.0 ** -24), (1.5 * 2.0 ** -24, 2.0 ** -23),
                 (np.nextafter(np.float32(65520.0), np.float32(0.0)), 65504.0), (65520.0, np.inf), (-65520.0, -np.inf)]
    else:
        cases = [(1.0 + 2.0 ** -8, 1.0), (1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -6), (257.0, 256.0), (259.0, 260.0),
                 (float(f32([0x7F7F7FFF])[0]), float(f32([0x7F7F0000])[0])), (float(f32([0x7F7F8000])[0]), np.inf)]
    x = np.array([c[0] for c in cases], np.float32)
    want = np.array([c[1] for c in cases], np.float32)
    assert np.array_equal(torch.from_numpy(x).to(dtype).float().numpy(), want)       # the CPU reference agrees
    nat = _native()
    dst = poisoned(1, nat.padded_dim(len(cases), dtype), dtype)
    nat.append_rows(dst, 0, torch.from_numpy(x[None]).to(DEV), len(cases))
    assert np.array_equal(dst[0, : len(cases)].float().cpu().numpy(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_append_rows_of_no_rows_writes_nothing(dtype):
    nat = _native()
    dst = poisoned(4, nat.padded_dim(70, dtype), dtype)
    nat.append_rows(dst, 2, torch.zeros((0, 70), device=DEV), 70)
    nat.append_rows(dst, 4, torch.zeros((0, 70), device=DEV), 70)      # n_used == capacity is fine for m = 0
    torch.cuda.synchronize()
    assert bool((dst.view(torch.uint8) == POISON).all())


def random_bytes(rows: int, row_bytes: int, seed: int) -> torch.Tensor:
    g = np.random.default_rng(seed)
    return torch.from_numpy(g.integers(0, 256, (rows, row_bytes), dtype=np.uint8))


GATHER_DTYPES = DTYPES + [torch.float8_e4m3fn]


@pytest.mark.parametrize("dtype", GATHER_DTYPES, ids=str)
@pytest.mark.parametrize("ld", [64, 128, 768])
def test_gather_rows_moves_whole_rows_and_nothing_else(dtype, ld):
    nat = _native()
    esize = torch.empty(0, dtype=dtype).element_size()
    n = 301
    src_h = random_bytes(n, ld * esize, ld + esize)
    src = src_h.to(DEV).view(dtype)
    g = np.random.default_rng(ld)
    subset = np.sort(g.choice(n, 97, replace=False))
    subset[-1] = n - 1                                                  # the last stored row among them
    for keep in (subset, np.arange(n), np.array([n - 1]), np.array([0])):
        tail = 5
        dst = poisoned(len(keep) + tail, ld, dtype)
        nat.gather_rows(dst, src, torch.from_numpy(keep).to(DEV))
        torch.cuda.synchronize()
        got = dst.view(torch.uint8).cpu()
        assert torch.equal(got[: len(keep)], src_h[keep]), len(keep)    # src[keep] as bytes
        assert bool((got[len(keep):] == POISON).all())                  # the destination's tail: untouched
    dst = poisoned(2, ld, dtype)
    nat.gather_rows(dst, src, torch.zeros(0, dtype=torch.int64, device=DEV))       # m = 0
    torch.cuda.synchronize()
    assert bool((dst.view(torch.uint8) == POISON).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float8_e4m3fn], ids=str)
def test_gather_rows_above_the_grid_cap(dtype):
    """m * row_vec above 8 * CUs * 256 sixteen-byte chunks: the second trip of the loop"""
    nat = _native()
    ld, esize = 768, torch.empty(0, dtype=dtype).element_size()
    row_vec = ld * esize // 16
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256
    n = cap // row_vec * 9 // 8 + 500
    src_h = random_bytes(n, ld * esize, 5)
    src = src_h.to(DEV).view(dtype)
    keep = np.nonzero(np.arange(n) % 9 != 4)[0]                        # strictly increasing, most rows
    assert len(keep) * row_vec > cap
    dst = poisoned(len(keep) + 1, ld, dtype)
    nat.gather_rows(dst, src, torch.from_numpy(keep).to(DEV))
    torch.cuda.synchronize()
    got = dst.view(torch.uint8).cpu()
    assert torch.equal(got[:-1], src_h[keep]) and bool((got[-1] == POISON).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("d", [3, 70, 100, 700])
def test_fetch_rows_f32_is_the_exact_upcast(dtype, d):
    nat = _native()
    ld = nat.padded_dim(d, dtype)
    assert d < ld
    n = 211
    x = source(n, ld, d)
    x[np.isnan(x)] = 1.0
    stored = torch.from_numpy(x).to(dtype)                              # any bits the format holds, pad columns too
    g = np.random.default_rng(d)
    rows = np.concatenate([[n - 1, 0, n - 1], g.integers(0, n, 600), [n - 1]])     # any order, repeats, the last row
    got = nat.fetch_rows_f32(stored.to(DEV), torch.from_numpy(rows).to(DEV), d).cpu()
    want = stored[rows, :d].float()
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert np.array_equal(got.numpy().view(np.int32), want.numpy().view(np.int32))


def test_fetch_rows_f32_above_the_grid_cap():
    nat = _native()
    d, ld = 700, 704
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256
    n = 400
    stored = torch.from_numpy(np.random.default_rng(3).standard_normal((n, ld)).astype(np.float32)).to(torch.bfloat16)
    m = cap // d + 300
    rows = np.random.default_rng(4).integers(0, n, m)
    rows[-1] = n - 1
    got = nat.fetch_rows_f32(stored.to(DEV), torch.from_numpy(rows).to(DEV), d).cpu()
    assert m * d > cap and torch.equal(got, stored[rows, :d].float())


# ---------------------------------------------------------------- argument checks: a status, and nothing launched
def test_argument_checks_return_their_status_and_launch_nothing():
    nat = _native()
    lib = nat.lib()
    F16, F32, BAD = 1, 0, 7
    dst = poisoned(8, 128, torch.float16)
    src = torch.ones((4, 70), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def append(capacity=8, ld=128, dtype=F16, n_used=0, m=4, d=70, corpus=None):
        return lib.mmrag_append_rows(dst.data_ptr() if corpus is None else corpus, capacity, ld, dtype, n_used,
                                     src.data_ptr(), m, d, stream)

    assert append() == 0
    torch.cuda.synchronize()
    assert bool((dst[:4, :70] == 1).all())
    dst.view(torch.uint8).fill_(POISON)
    assert append(n_used=5) == EINVAL and b"exceed capacity" in lib.mmrag_last_error()     # rows past the capacity
    assert append(n_used=-1) == EINVAL and append(m=-1) == EINVAL
    assert append(dtype=BAD) == EINVAL and b"bad dtype" in lib.mmrag_last_error()
    assert append(dtype=-1) == EINVAL
    assert append(ld=64) == EINVAL and b"d <= ld" in lib.mmrag_last_error()                # ld < d
    assert append(d=0) == EINVAL
    assert append(corpus=0) == EINVAL and b"null" in lib.mmrag_last_error()
    with pytest.raises(nat.MMRagNativeError, match="exceed capacity"):
        nat.append_rows(dst, 5, src, 70)

    keep = torch.tensor([1, 0], dtype=torch.int64, device=DEV)
    rows16 = torch.zeros((4, 128), dtype=torch.float16, device=DEV)

    def gather(dst_ptr=None, src_ptr=None, ld=128, dtype=F16, m=2):
        return lib.mmrag_gather_rows(dst.data_ptr() if dst_ptr is None else dst_ptr,
                                     rows16.data_ptr() if src_ptr is None else src_ptr, ld, dtype, keep.data_ptr(), m, stream)

    assert gather(dtype=BAD) == EINVAL and b"bad dtype" in lib.mmrag_last_error()
    assert gather(ld=3) == EINVAL and b"multiple of 16" in lib.mmrag_last_error()          # 6-byte rows
    assert gather(ld=0) == EINVAL
    assert gather(dst_ptr=dst.data_ptr() + 2) == EINVAL and b"unaligned" in lib.mmrag_last_error()
    assert gather(src_ptr=rows16.data_ptr() + 8) == EINVAL and b"unaligned" in lib.mmrag_last_error()
    assert gather(dst_ptr=0) == EINVAL

    out = torch.full((2, 70), 5.0, dtype=torch.float32, device=DEV)

    def fetch(ld=128, dtype=F16, d=70, corpus=None):
        return lib.mmrag_fetch_rows_f32(rows16.data_ptr() if corpus is None else corpus, ld, dtype, keep.data_ptr(), 2, d,
                                        out.data_ptr(), stream)

    assert fetch(dtype=BAD) == EINVAL and b"bad dtype" in lib.mmrag_last_error()
    assert fetch(ld=64) == EINVAL and fetch(d=0) == EINVAL and fetch(corpus=0) == EINVAL
    torch.cuda.synchronize()
    assert bool((dst.view(torch.uint8) == POISON).all())                # no refused call wrote a byte
    assert bool((out == 5.0).all())
    assert fetch() == 0 and F32 == 0
    torch.cuda.synchronize()
    assert not bool(out.any())
