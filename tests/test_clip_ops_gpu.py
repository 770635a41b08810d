"""The CLIP towers' own kernels on the GPU against float64 references (tests/clip_ref.py) computed from the exact uint8 /
fp16 / fp32 values each kernel reads.  Every bound below comes from the kernel's arithmetic, not from its output; where
the arithmetic allows it the comparison is bit for bit.  These per-kernel bounds are the deciding ones for the front end
and the head; the whole towers are bounded in tests/test_clip_gpu.py (a multiple of the error fp16 storage alone causes).

  patchify_kernel, fp16 CHW ..... pure data movement: equal BITS (16-bit patterns, so NaN patterns count too).  The planes
                                  hold pattern (40503 * (c, y, x index) + 977 * b) mod 2^16: distinct within an image up to
                                  65536 elements (image 64, 96), and at 224 distinct for any two elements closer than
                                  65536 in (c, y, x) order -- no swap of (c, ph, pw), grid row / column or image survives.
  patchify_kernel, uint8 HWC .... (v / 255 - mean_c) / std_c: two fp32 divisions and a subtraction, one rounding to fp16:
                                  |got - ref| <= 2^-11 |ref| + 1e-6 (half an fp16 ulp; the fp32 error is at most about
                                  3 * 2^-24 / std = 7e-7 after the cancellation).  All 256 values x 3 channels + random tiles.
  vit_assemble_ln_kernel ........ LN(concat(cls, emb) + pos): test_encoder_ops_gpu.ln_row_limit (one fp16 rounding plus fp32
                                  statistics within MEAN_TOL / STAT_TOL), rows with a mean of 20 row-sigmas among them.
                                  Worst observed ratio against that limit on the MI355X: see LN_WORST below.
  embed_ln_kernel, g == nullptr . fp16(tok[id] + pos[p]), fp32 sum of two fp16 values and one rounding:
                                  |got - ref| <= (2^-11 + 2^-23) |ref|; integer tables: equal bits; ids / positions outside
                                  the tables are clamped (id >= vocab -> vocab - 1, negative -> 0).
  pool_norm_kernel<_Float16> .... modes 1 (first) and 2 (sel[b]) without normalisation copy a row: equal bits.
  mmrag_pool_normalize_f16 ...... pool = 2, normalised fp32: test_pool_normalize's bound, |got - ref| <= 1e-5.
  normalize_rows_kernel ......... x / max(||x||, 1e-12) in fp32: |got - ref| <= R_NORM * 2^-24 |ref| + 1e-30.

Each test records the worst observed ratio against its bound (`record_property`, visible with --junitxml)."""
import numpy as np
import pytest
import torch

from tests import clip_ref as R
from tests.test_encoder_ops_gpu import ln_ratio, ln_ref64, ln_row_limit

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11
U32 = 2.0 ** -24
# normalize_rows: worst |got - ref| / (2^-24 |ref|) observed on the MI355X over every case below: R_NORM_OBSERVED;
# the constant is twice that, rounded up to a power of two
R_NORM_OBSERVED = 3.0
R_NORM = 8.0
# vit_assemble_ln: worst ratio against ln_row_limit observed on the MI355X.  The limit is derived, not tuned to this: it is
# dominated by the half fp16 ulp of the output rounding, which some element of 100 000 always nearly reaches
LN_WORST = 0.985


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def dev16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).cuda().half().contiguous()


def dev32(x):
    return torch.from_numpy(np.asarray(x, np.float32)).cuda().contiguous()


def devi(x):
    return torch.from_numpy(np.asarray(x, np.int32)).cuda()


def bits(t):
    return t.view(torch.int16).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# patchify
# ---------------------------------------------------------------------------------------------------------------------
FRONT_SHAPES = [(64, 32), (224, 32), (224, 16), (64, 8), (96, 16)]


def pattern_planes(B, image):
    """int16 bit patterns [B, 3, image, image], see the module header"""
    idx = np.arange(3 * image * image, dtype=np.int64).reshape(1, 3, image, image)
    b = np.arange(B, dtype=np.int64).reshape(B, 1, 1, 1)
    return ((idx * 40503 + b * 977) % 65536).astype(np.uint16).view(np.int16)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("image,patch", FRONT_SHAPES)
def test_patchify_f16_bit_exact(N, image, patch, B):
    planes = pattern_planes(B, image)
    if 3 * image * image <= 65536:
        assert all(np.unique(p).size == p.size for p in planes)
    got = bits(N.patchify(torch.from_numpy(planes).cuda().view(torch.float16), image, patch))
    want = R.patchify(planes, patch)
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("(image, patch, element)", bad[:5].tolist())


def test_patchify_f16_bit_exact_large_batch(N):
    """305 images of 96 / 16: 1 054 080 chunks of 8 elements, above 2^20 and not a multiple of the 256-thread workgroup
    (the last workgroup is half empty)"""
    image, patch, B = 96, 16, 305
    chunks = B * (image // patch) ** 2 * (3 * patch * patch // 8)
    assert chunks > 2 ** 20 and chunks % 256 != 0
    planes = pattern_planes(B, image)
    got = bits(N.patchify(torch.from_numpy(planes).cuda().view(torch.float16), image, patch))
    assert np.array_equal(got, R.patchify(planes, patch))


def u8_ratio(got, tiles, patch):
    ref = R.patchify(R.normalize_u8(tiles), patch)
    r = np.abs(got - ref) / (U16 * np.abs(ref) + 1e-6)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), i, ref


def test_patchify_u8_all_values_every_channel(N, record_property):
    """one 64 x 64 image whose channel c holds (pixel index + 85 c) mod 256: all 768 (value, channel) cases, 16 times"""
    image, patch = 64, 8
    p = np.arange(image * image).reshape(image, image, 1)
    tiles = ((p + 85 * np.arange(3)) % 256).astype(np.uint8)[None]
    assert all(np.unique(tiles[0, :, :, c]).size == 256 for c in range(3))
    got = N.patchify(torch.from_numpy(tiles).cuda(), image, patch).cpu().numpy().astype(np.float64)
    r, i, ref = u8_ratio(got, tiles, patch)
    record_property("worst ratio", round(r, 3))
    assert r <= 1, ("(image, patch, element)", i, got[i], ref[i], r)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("image,patch", FRONT_SHAPES)
def test_patchify_u8_random_tiles(N, record_property, image, patch, B):
    """random tiles: neighbouring uint8 values are 1 / (255 std) = 0.014 apart after normalisation, 30 to 3000 times
    the bound, so a misplaced pixel fails as surely as a wrong constant"""
    tiles = np.random.default_rng(image + patch + B).integers(0, 256, (B, image, image, 3), dtype=np.uint8)
    got = N.patchify(torch.from_numpy(tiles).cuda(), image, patch).cpu().numpy().astype(np.float64)
    r, i, ref = u8_ratio(got, tiles, patch)
    record_property("worst ratio", round(r, 3))
    assert r <= 1, ("(image, patch, element)", i, got[i], ref[i], r)


def test_patchify_rejects_patch_not_multiple_of_8(N):
    with pytest.raises(N.MMRagNativeError):
        N.patchify(torch.zeros((1, 3, 224, 224), dtype=torch.float16, device="cuda"), 224, 14)


# ---------------------------------------------------------------------------------------------------------------------
# vit_assemble_ln
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 7])
@pytest.mark.parametrize("S", [5, 50, 197])
@pytest.mark.parametrize("H", [128, 768, 1024])
def test_vit_assemble_ln(N, record_property, H, S, B):
    """independent random rows: emb of spread 0.5, pos of spread 2, cls of spread 1, so the row of a neighbouring patch,
    position or image is O(1) away after the LayerNorm, thousands of times the limit.  Odd images carry a mean of 20
    row-sigmas (the case that broke the one-pass variance of the folded LayerNorm)"""
    g = np.random.default_rng(H + 7 * S + B)
    emb = g.standard_normal((B, S - 1, H)) * 0.5
    emb[1::2] += 20.0 * np.sqrt(0.25 + 4.0)
    emb, pos, cls = R.r16(emb), R.r16(g.standard_normal((S, H)) * 2.0), R.r16(g.standard_normal(H))
    gamma = (1.0 + 0.3 * g.standard_normal(H)).astype(np.float32)
    beta = (0.2 * g.standard_normal(H)).astype(np.float32)
    eps = 1e-5
    x = R.vit_assemble(emb, cls, pos)
    ref, _, rstd, z = ln_ref64(x, gamma.astype(np.float64), beta.astype(np.float64), eps)
    lim = ln_row_limit(x, ref, z, rstd, gamma, beta)
    got = N.vit_assemble_ln(dev16(emb), dev16(cls), dev16(pos), dev32(gamma), dev32(beta), eps)
    assert tuple(got.shape) == (B * S, H)
    got = got.cpu().numpy().astype(np.float64)
    r_cls, i_cls = ln_ratio(got[::S], ref[::S], lim[::S])
    r, i = ln_ratio(got, ref, lim)
    record_property("worst ratio", round(r, 3))
    assert r_cls <= 1, ("class-token row of image / column", i_cls, r_cls)
    assert r <= 1, ("row (image * S + token) / column", i, got[i], ref[i], r)


def test_vit_assemble_ln_uses_eps(N):
    """constant rows (variance 0): the output is beta exactly only if eps keeps rstd finite; (x - mean) = 0 either way,
    so this pins the absence of NaN; rows of spread 1e-3 (variance 1e-6 < eps = 1e-5) pin the value of eps"""
    H, S, B = 128, 5, 2
    g = np.random.default_rng(0)
    emb = R.r16(g.standard_normal((B, S - 1, H)) * 1e-3)
    emb[0, 0] = 0.25
    pos = np.zeros((S, H))
    cls = np.full(H, 0.5)
    gamma = np.ones(H, np.float32)
    beta = (0.2 * g.standard_normal(H)).astype(np.float32)
    x = R.vit_assemble(emb, cls, pos)
    ref, _, rstd, z = ln_ref64(x, 1.0, beta.astype(np.float64), 1e-5)
    lim = ln_row_limit(x, ref, z, rstd, gamma, beta)
    got = N.vit_assemble_ln(dev16(emb), dev16(cls), dev16(pos), dev32(gamma), dev32(beta), 1e-5).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert np.array_equal(got[0], R.r16(beta)) and np.array_equal(got[1], R.r16(beta))     # class row, constant row
    r, i = ln_ratio(got, ref, lim)
    assert r <= 1, (i, got[i], ref[i], r)


# ---------------------------------------------------------------------------------------------------------------------
# embed_ln without LayerNorm (CLIP text)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [128, 512, 192])
def test_embed_sum_without_layernorm(N, record_property, H):
    g = np.random.default_rng(H)
    V, P, T = 300, 77, 333
    tok, pos = R.r16(g.standard_normal((V, H)) * 0.1), R.r16(g.standard_normal((P, H)) * 0.1)
    tok[5] = R.r16(tok[5] * 2.0 ** -10)     # a row of fp16 subnormals and near-subnormals
    pos[3] = -tok[5]                        # row 2 of the output cancels to exact zeros
    ids, pid = g.integers(0, V, T), g.integers(0, P, T)
    ids[:4], pid[:4] = (0, V - 1, 5, 5), (P - 1, 0, 3, 4)
    got = N.embed_ln_f16(devi(ids), devi(pid), dev16(tok), dev16(pos), None, None, None, 1e-5)
    assert tuple(got.shape) == (T, H)
    got = got.cpu().numpy().astype(np.float64)
    ref = tok[ids] + pos[pid]
    assert np.all(got[2] == 0)
    lim = (U16 + 2.0 ** -23) * np.abs(ref)
    r = np.abs(got - ref) / np.where(lim > 0, lim, 1.0)
    record_property("worst ratio", round(float(r.max()), 3))
    assert np.all(np.abs(got - ref) <= lim), np.argwhere(np.abs(got - ref) > lim)[:5].tolist()


@pytest.mark.parametrize("H", [128, 512, 192])
def test_embed_sum_exact_integers_and_clamped_indices(N, H):
    """integer tables whose sums are exact in fp16; every (id, position) pair identifies itself.  Ids and positions
    outside the tables are clamped by the kernel before it forms an address (embed_ln_kernel: id >= vocab -> vocab - 1,
    negative -> 0), so every access stays inside the tables"""
    V, P = 40, 16
    tok = (np.arange(V)[:, None] * 16 + (np.arange(H)[None, :] % 7)).astype(np.float64)
    pos = -(np.arange(P)[:, None] + 3 * (np.arange(H)[None, :] % 5)).astype(np.float64)
    ids = np.array([0, 1, V - 1, V, V + 5, -1, -7, 2 ** 31 - 1, -2 ** 31, 17, 3], np.int64)
    pid = np.array([P - 1, P, 0, -1, 2 ** 31 - 1, 3, -2 ** 31, 5, P + 1, -3, 15], np.int64)
    got = N.embed_ln_f16(devi(ids), devi(pid), dev16(tok), dev16(pos), None, None, None, 1e-5).cpu().numpy()
    want = tok[R.clamp_index(ids, V)] + pos[R.clamp_index(pid, P)]
    assert np.array_equal(got.astype(np.float64), want)


# ---------------------------------------------------------------------------------------------------------------------
# pooling of the pre-LN head
# ---------------------------------------------------------------------------------------------------------------------
POOL_LENS = [1, 2, 77, 77, 2, 1, 77]
POOL_SEL = [0, 1, 0, 76, 0, 0, 40]      # 0, len - 1 and in between


@pytest.mark.parametrize("pool", [1, 2], ids=["first", "select"])
@pytest.mark.parametrize("H", [128, 512, 768, 1024])
def test_pool_f16_copies_the_row(N, H, pool):
    g = np.random.default_rng(H + pool)
    cu = np.concatenate([[0], np.cumsum(POOL_LENS)]).astype(np.int32)
    x = dev16(g.standard_normal((cu[-1], H)))
    got = bits(N.pool_f16(x, devi(cu), pool, sel=devi(POOL_SEL) if pool == 2 else None))
    rows = cu[:-1] + (np.array(POOL_SEL) if pool == 2 else 0)
    assert np.array_equal(got, bits(x)[rows])


@pytest.mark.parametrize("H", [128, 512, 768, 1024])
def test_pool_normalize_f16_select(N, H):
    g = np.random.default_rng(H)
    cu = np.concatenate([[0], np.cumsum(POOL_LENS)]).astype(np.int32)
    x = R.r16(g.standard_normal((cu[-1], H)))
    got = N.pool_normalize_f16(dev16(x), devi(cu), 2, sel=devi(POOL_SEL)).cpu().numpy().astype(np.float64)
    ref = R.normalize_rows(x[cu[:-1] + np.array(POOL_SEL)])
    assert np.abs(got - ref).max() <= 1e-5, float(np.abs(got - ref).max())
    raw = N.pool_normalize_f16(dev16(x), devi(cu), 2, normalize=False, sel=devi(POOL_SEL)).cpu().numpy()
    assert np.array_equal(raw.astype(np.float64), x[cu[:-1] + np.array(POOL_SEL)])


# ---------------------------------------------------------------------------------------------------------------------
# normalize_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 1000])
@pytest.mark.parametrize("D", [64, 512, 768, 100])
def test_normalize_rows(N, record_property, D, B):
    """random rows; with B = 5 also an all-zero row (exact zeros, no NaN), a row of 6e4 everywhere and a row of the
    smallest fp16 subnormal everywhere (the sum of squares stays inside fp32 for both)"""
    g = np.random.default_rng(D + B)
    x = R.r16(g.standard_normal((B, D)) * 0.7)
    if B == 5:
        x[1], x[2], x[3] = 0.0, 6e4, 2.0 ** -24
        assert np.all(R.r16(x[2]) == 6e4) and np.all(R.r16(x[3]) == 2.0 ** -24)
    got = N.normalize_rows(dev16(x)).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    if B == 5:
        assert np.all(got[1] == 0)
    ref = R.normalize_rows(x)
    need = (np.abs(got - ref) - 1e-30) / np.where(ref != 0, U32 * np.abs(ref), 1.0)
    record_property("worst ratio", round(float(need.max()) / R_NORM, 3))
    record_property("worst R", round(float(need.max()), 3))
    i = np.unravel_index(int(np.argmax(need)), need.shape)
    assert need[i] <= R_NORM, ("row / column", i, got[i], ref[i], float(need[i]))
