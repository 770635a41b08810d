"""Encoder ops on the GPU against float64 references computed from the exact fp16 / fp32 values the kernels read.

  A. mmrag_attention_f16: all five instantiations (`attention_kernel_name` quotes the dispatch rule), every seam length
     of the 64-key tiles, causal and not, packed batches that mix one long sequence with short ones, the streamed
     kernel forced by DBG_ATTENTION_STREAMED, exact Q = 0 probes, softmax extremes, launch-to-launch determinism.
     Bound from the arithmetic: P is rounded to fp16 before P.V and the output is rounded to fp16, so
     |got - ref| <= C_ATT * 2^-11 * (P.|V|) + 1e-6 elementwise, P and P.|V| in float64.
  B. the single-query forward's GEMM with the LayerNorm folded into its input (linear_small16_kernel<.., LN_IN>) and
     the normalised residual, through mmrag_internal_linear_f16_norms, on rows whose mean is far from 0 and rows with
     outlier channels; mmrag_layernorm_f16 on the same rows is the two-pass control.
  C. the fp32 encoder mode's attention, LayerNorm and pooling kernels on their own.

Each test records the worst observed ratio against its bound (`record_property`, visible with --junitxml)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11            # fp16 unit roundoff
DBG_ATTENTION_STREAMED = 4096

# attention_f16 bound constant.  Worst c observed on the MI355X, random cases (dispatch matrix) / softmax extremes:
#   <32,3> 1.56 / 1.62   <32,2,true,8> 1.48 / 1.59   <64,3> 1.69 / 2.35   <64,2,true,8> 1.54 / 2.14
#   <64,1,true,16,8> 1.52 / 2.35
C_ATT = 3.0
# fp32 attention: |got - ref| <= A32 * (P.|V|) + 1e-7 (worst observed 8.1e-7 * P.|V|)
A32 = 1e-6
# fp32 LayerNorm: |got - ref| <= L32 * max|ref| per row (worst observed 2.7e-7)
L32 = 5e-7
# (mean, rstd) of a LayerNorm with fp32 statistics vs float64: |d mean| <= MEAN_TOL * mean|x| (a sum of K fp32 terms:
# grows with the row's mean) and |d rstd| / rstd <= STAT_TOL (two passes: independent of the mean).  Worst observed
# 0.02 MEAN_TOL and 0.12 STAT_TOL; the one-pass variance this replaced was 8-40 STAT_TOL off at a mean of 20 sigma,
# 360 at 100 sigma.
MEAN_TOL = 64 * 2.0 ** -24
STAT_TOL = 32 * 2.0 ** -24

SEAM_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512]
# (H, heads): MiniLM 12x32, 4x32, bge / ViT 12x64, CLIP text 8x64
LAYOUTS = [(384, 12), (128, 4), (768, 12), (512, 8)]
LAYOUT_IDS = ["12x32", "4x32", "12x64", "8x64"]


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def _set_debug(N, flags):
    L = N.lib()
    L.mmrag_internal_set_debug.argtypes = [ctypes.c_uint]
    L.mmrag_internal_set_debug(flags)


def attention_kernel_name(dh, max_len, streamed):
    """which kernel mmrag_attention_f16 (csrc/encoder.hip) launches:
         dh 64, 128 < max_len <= 256 -> attention_kernel<64, 2, true, 8>     K / V^T resident, 8 waves
         dh 64, 256 < max_len <= 512 -> attention_kernel<64, 1, true, 16, 8> resident, 16 waves
         dh 64, otherwise            -> attention_kernel<64, 3>              key tiles streamed through LDS
         dh 32, 128 < max_len <= 256 -> attention_kernel<32, 2, true, 8>
         dh 32, otherwise            -> attention_kernel<32, 3>
       DBG_ATTENTION_STREAMED: the streamed kernel of the head dimension for every max_len"""
    if not streamed and 128 < max_len <= 256:
        return f"<{dh},2,true,8>"
    if not streamed and dh == 64 and 256 < max_len <= 512:
        return "<64,1,true,16,8>"
    return f"<{dh},3>"


def r16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def dev16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).cuda().half().contiguous()


def dev32(x):
    return torch.from_numpy(np.asarray(x, np.float32)).cuda().contiguous()


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def mixed_lens(L):
    """one sequence of L keys packed between shorter ones (which then run inside L's kernel)"""
    shorts = [s for s in (1, 33, 2, 65, 129, 31, 257) if s < L][:3]
    return shorts[:1] + [L] + shorts[1:]


def attention_ref64(qkv, lens, heads, causal):
    """softmax(Q K^T / sqrt(dh) + mask) V and P |V|, float64, per (sequence, head)"""
    qkv = np.asarray(qkv, np.float64)
    H = qkv.shape[1] // 3
    dh = H // heads
    out = np.zeros((qkv.shape[0], H))
    pav = np.zeros((qkv.shape[0], H))
    for a, b in zip(cu_of(lens)[:-1], cu_of(lens)[1:]):
        S = b - a
        q, k, v = (qkv[a:b, i * H:(i + 1) * H].reshape(S, heads, dh).transpose(1, 0, 2) for i in range(3))
        s = q @ k.transpose(0, 2, 1) / np.sqrt(dh)
        if causal:
            s = np.where(np.tril(np.ones((S, S), bool)), s, -np.inf)
        p = np.exp(s - s.max(axis=2, keepdims=True))
        p /= p.sum(axis=2, keepdims=True)
        out[a:b] = (p @ v).transpose(1, 0, 2).reshape(S, H)
        pav[a:b] = (p @ np.abs(v)).transpose(1, 0, 2).reshape(S, H)
    return out, pav


def run_attention(N, qkv, lens, heads, causal, streamed):
    cu = torch.from_numpy(cu_of(lens)).cuda()
    _set_debug(N, DBG_ATTENTION_STREAMED if streamed else 0)
    try:
        got = N.attention_f16(dev16(qkv), cu, max(lens), heads, causal)
    finally:
        _set_debug(N, 0)
    torch.cuda.synchronize()
    return got.cpu().numpy().astype(np.float64)


def attention_c(got, ref, pav):
    """the c each element needs in |got - ref| <= c * 2^-11 * P|V| + 1e-6 (worst element, its index)"""
    need = np.abs(got - ref) / (U16 * pav + 1e-6 / C_ATT)
    i = np.unravel_index(int(np.argmax(need)), need.shape)
    return float(need[i]), i


def attention_all_kernels(N, qkv, lens, heads, causal, record_property, ref=None):
    """default dispatch and the forced streamed kernel (once if they are the same kernel), each launched twice: equal
    bits, within the bound"""
    H = qkv.shape[1] // 3
    ref, pav = attention_ref64(qkv, lens, heads, causal) if ref is None else ref
    runs = {}
    for streamed in (False, True):
        name = attention_kernel_name(H // heads, max(lens), streamed)
        if name in runs:        # the dispatch already picked the streamed kernel
            continue
        got = run_attention(N, qkv, lens, heads, causal, streamed)
        again = run_attention(N, qkv, lens, heads, causal, streamed)
        c, i = attention_c(got, ref, pav)
        record_property("c " + name, round(c, 3))
        runs[name] = (got, again, c, i)
    for name, (got, again, c, i) in runs.items():
        assert np.array_equal(got, again), (name, "two launches differ")
        assert c <= C_ATT, (name, "token/col", i, "got", got[i], "ref", ref[i], "P|V|", pav[i], "c", c)


# ---------------------------------------------------------------------------------------------------------------------
# A. attention, fp16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["bidir", "causal"])
@pytest.mark.parametrize("L", SEAM_LENS)
@pytest.mark.parametrize("H,heads", LAYOUTS, ids=LAYOUT_IDS)
def test_attention_f16_dispatch_matrix(N, record_property, H, heads, L, causal):
    """random fp16 Q, K, V (unit scores); L is max_len and picks the instantiation; worst c observed on the MI355X
    per instantiation: see C_ATT"""
    lens = mixed_lens(L)
    g = np.random.default_rng(L * 7 + H + int(causal))
    qkv = r16(g.standard_normal((sum(lens), 3 * H)))
    attention_all_kernels(N, qkv, lens, heads, causal, record_property)


def plant_probe(L, H, heads, causal):
    """Q = 0: every visible key has p = 1 exactly.  V = 0 except 1024 at planted (key, head, channel) slots: every key
    position 0..L-1 of an L-key sequence is planted once, in a channel that depends on the head, spread over as many
    copies of the sequence as the H slots of a key row need; after every copy a short sequence whose first key is
    planted in every slot (a read across cu_seqlens lights up a channel that must be 0).  Returns qkv, lens, expected."""
    dh = H // heads
    n_copies = (L + H - 1) // H
    lens, plants = [2], [[(0, c) for c in range(H)]]          # (key, column)
    for c in range(n_copies):
        lens.append(L)
        pl = []
        for j in range(c * H, min(L, (c + 1) * H)):
            h = j % heads
            ch = (j // heads - c * dh + 7 * h) % dh
            pl.append((j, h * dh + ch))
        plants.append(pl)
        lens.append(3 if c % 2 == 0 else 1)
        plants.append([(0, col) for col in range(H)])
    cu = cu_of(lens)
    qkv = np.zeros((cu[-1], 3 * H))
    want = np.zeros((cu[-1], H))
    for s0, n, pl in zip(cu[:-1], lens, plants):
        q = np.arange(n)
        n_vis = (q + 1) if causal else np.full(n, n)
        for key, col in pl:
            qkv[s0 + key, 2 * H + col] = 1024.0
            vis = key <= q if causal else np.ones(n, bool)
            want[s0 + q[vis], col] = 1024.0 / n_vis[vis]
    return qkv, lens, want


@pytest.mark.parametrize("streamed", [False, True], ids=["dispatch", "streamed"])
@pytest.mark.parametrize("causal", [False, True], ids=["bidir", "causal"])
@pytest.mark.parametrize("L", [64, 65, 256, 257, 512])
@pytest.mark.parametrize("H,heads", LAYOUTS, ids=LAYOUT_IDS)
def test_attention_f16_exact_key_coverage(N, H, heads, L, causal, streamed):
    """integer-exact: 1024 / (visible keys) where the planted key is visible, exactly 0 everywhere else.  A dropped or
    doubled key, a tile-edge or causal off-by-one, a head offset or a leak across sequences changes a value by far
    more than the one fp16 rounding (plus the fp32 reciprocal) allowed"""
    qkv, lens, want = plant_probe(L, H, heads, causal)
    got = run_attention(N, qkv, lens, heads, causal, streamed)
    zero = want == 0
    bad = np.argwhere(zero & (got != 0))
    assert bad.size == 0, ("nonzero where 0 expected", attention_kernel_name(H // heads, L, streamed), bad[:5].tolist())
    err = np.abs(got - want)
    lim = (U16 + 2.0 ** -22) * want
    bad = np.argwhere(~zero & (err > lim))
    assert bad.size == 0, ("planted value off", attention_kernel_name(H // heads, L, streamed), bad[:5].tolist(),
                           [(got[tuple(i)], want[tuple(i)]) for i in bad[:5]])


def extreme_case(kind, lens, H, heads, g):
    """Q, K, V of one softmax extreme"""
    dh = H // heads
    T = sum(lens)
    qkv = g.standard_normal((T, 3 * H))
    if kind == "spread80":          # scaled scores with a standard deviation of 30: most p underflow
        qkv[:, :H] *= 30.0
    elif kind in ("max_first_tile", "max_last_tile"):
        # one key per sequence has a scaled score 16 (dh 64) / 22.6 (dh 32) above the rest: in the first key tile
        # (alpha stays 1 later) or in the last (alpha rescales everything accumulated before)
        qkv[:, :H] *= 0.5
        qkv[:, np.arange(heads) * dh] = 8.0
        for a, b in zip(cu_of(lens)[:-1], cu_of(lens)[1:]):
            key = a if kind == "max_first_tile" else b - 1
            qkv[key, H + np.arange(heads) * dh] = 16.0
    elif kind == "all_equal":       # Q = 0: P is uniform over the visible keys
        qkv[:, :H] = 0.0
    return r16(qkv)


@pytest.mark.parametrize("kind", ["spread80", "max_first_tile", "max_last_tile", "all_equal"])
@pytest.mark.parametrize("causal", [False, True], ids=["bidir", "causal"])
@pytest.mark.parametrize("L", [1, 65, 200, 300, 512])
@pytest.mark.parametrize("H,heads", [(384, 12), (768, 12)], ids=["12x32", "12x64"])
def test_attention_f16_softmax_extremes(N, record_property, H, heads, L, causal, kind):
    lens = mixed_lens(L)
    g = np.random.default_rng(L + H)
    attention_all_kernels(N, extreme_case(kind, lens, H, heads, g), lens, heads, causal, record_property)


# ---------------------------------------------------------------------------------------------------------------------
# B. the folded-LayerNorm GEMM of the single-query forward
# ---------------------------------------------------------------------------------------------------------------------
ROW_KINDS = ["offset0", "offset20", "offset100", "offset300", "outliers"]


def make_rows(kind, M, K, g, sigma=0.5):
    """fp16 rows of spread sigma around a mean of 0 / 20 / 100 / 300 sigma, or with a few large channels (BERT's outlier
    dimensions; channel 0 among them, so a pivot taken from it would not help)"""
    x = g.standard_normal((M, K)) * sigma
    if kind.startswith("offset"):
        x += float(kind[6:]) * sigma * np.where(g.random((M, 1)) < 0.5, -1.0, 1.0)
    else:
        for c, v in ((0, 60.0), (7, -120.0), (K // 3, 250.0), (K - 1, -200.0)):
            x[:, c] = v * sigma * (1 + 0.1 * g.standard_normal(M))
    return r16(x)


def ln_ref64(x, gamma, beta, eps):
    """LayerNorm in float64, two passes: (normalised rows, mean, rstd, z = (x - mean) * rstd)"""
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    z = (x - mean) * rstd
    return z * gamma + beta, mean[:, 0], rstd[:, 0], z


def ln_params(K, g):
    return (1.0 + 0.3 * g.standard_normal(K)).astype(np.float32), (0.2 * g.standard_normal(K)).astype(np.float32)


def ln_row_limit(x, ref, z, rstd, gamma, beta):
    """one fp16 rounding of the float64 LayerNorm plus twice what fp32 statistics within MEAN_TOL / STAT_TOL and the
    fp32 (x - mean) * rstd * gamma + beta may add before it"""
    pre = np.abs(gamma) * (MEAN_TOL * np.abs(x).mean(axis=1, keepdims=True) * rstd[:, None] + STAT_TOL * np.abs(z))
    pre += 2.0 ** -22 * (np.abs(gamma * z) + np.abs(beta))
    return U16 * np.abs(ref) + 2 * pre + 1e-7


def ln_ratio(got, ref, limit):
    r = np.abs(got - ref) / limit
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), i


@pytest.mark.parametrize("M", [1, 7, 16, 17, 64])
@pytest.mark.parametrize("K", [384, 512, 768, 1024])
def test_folded_layernorm_identity_rows_and_stats(N, record_property, K, M):
    """W = I: the GEMM hands back the fp16 rows it normalised on load, elementwise; (mean, rstd) in ln_stats_out against
    float64; mmrag_layernorm_f16 (two-pass ln_row) on the same rows as the control"""
    g = np.random.default_rng(K + M)
    gamma, beta = ln_params(K, g)
    eye = dev16(np.eye(K))
    worst = 0.0
    for kind in ROW_KINDS:
        x = make_rows(kind, M, K, g)
        ref, mean, rstd, z = ln_ref64(x, gamma.astype(np.float64), beta.astype(np.float64), 1e-12)
        stats = torch.zeros((M, 2), dtype=torch.float32, device="cuda")
        got = N.linear_f16_norms(dev16(x), eye, ln_gamma=dev32(gamma), ln_beta=dev32(beta), ln_eps=1e-12,
                                 ln_stats_out=stats)
        ctl = N.layernorm_f16(dev16(x), dev32(gamma), dev32(beta), 1e-12)
        torch.cuda.synchronize()
        st = stats.cpu().numpy().astype(np.float64)
        dmean = float((np.abs(st[:, 0] - mean) / (MEAN_TOL * np.abs(x).mean(axis=1))).max())
        drstd = float((np.abs(st[:, 1] / rstd - 1) / STAT_TOL).max())
        lim = ln_row_limit(x, ref, z, rstd, gamma, beta)
        r_ctl, i_ctl = ln_ratio(ctl.cpu().numpy().astype(np.float64), ref, lim)
        r_fold, i_fold = ln_ratio(got.cpu().numpy().astype(np.float64), ref, lim)
        record_property(kind, "mean %.3g rstd %.3g control %.3g folded %.3g" % (dmean, drstd, r_ctl, r_fold))
        assert r_ctl <= 1, (kind, "mmrag_layernorm_f16", i_ctl, r_ctl)
        assert dmean <= 1 and drstd <= 1, (kind, "ln_stats_out: |d mean| / (MEAN_TOL mean|x|), |d rstd| / (STAT_TOL rstd)",
                                           dmean, drstd)
        assert r_fold <= 1, (kind, "folded", i_fold, r_fold)
        worst = max(worst, dmean, drstd, r_fold)
    record_property("worst ratio", round(worst, 3))


VARIANTS = {  # (bias, act, input LayerNorm, normalised residual): the four GEMMs of a single-query layer and both together
    "qkv": (True, 0, True, False),
    "ffn1_gelu": (True, 1, True, False),
    "oproj_resid": (True, 0, False, True),
    "ln_quickgelu_resid": (True, 2, True, True),
    "ln_nobias": (False, 0, True, False),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("M", [1, 7, 16, 17, 64])
@pytest.mark.parametrize("K", [384, 512, 768, 1024])
def test_folded_layernorm_gemm(N, record_property, K, M, variant):
    """float64 reference: LayerNorm of the fp16 rows, rounded to fp16 (what the kernel feeds the MFMA), GEMM + bias,
    activation, rounded to fp16, plus the fp16-rounded normalised residual, rounded to fp16.  test_linear's bound."""
    from scipy.special import erf

    with_bias, act, ln_in, with_res = VARIANTS[variant]
    g = np.random.default_rng(K * 3 + M + act)
    Nf = 3 * K if variant == "qkv" else K
    w = r16(g.standard_normal((Nf, K)) * 0.05)
    b = (0.1 * g.standard_normal(Nf)).astype(np.float32) if with_bias else None
    gamma, beta = ln_params(K, g)
    rgamma, rbeta = ln_params(Nf, g)
    worst = 0.0
    for kind in ROW_KINDS:
        x = make_rows(kind, M, K, g)
        a = r16(ln_ref64(x, gamma.astype(np.float64), beta.astype(np.float64), 1e-12)[0]) if ln_in else x
        y = a @ w.T + (b if with_bias else 0.0)
        if act == 1:
            y = 0.5 * y * (1.0 + erf(y / np.sqrt(2.0)))
        elif act == 2:
            y = y / (1.0 + np.exp(-1.702 * y))
        y = r16(y)
        kw = {}
        if ln_in:
            kw.update(ln_gamma=dev32(gamma), ln_beta=dev32(beta), ln_eps=1e-12)
        if with_res:
            r = make_rows(kind, M, Nf, g)
            _, rm, rr, _ = ln_ref64(r, 1.0, 0.0, 1e-12)
            st = np.stack([rm, rr], 1).astype(np.float32)
            y = r16(y + r16((r - st[:, :1].astype(np.float64)) * st[:, 1:].astype(np.float64) * rgamma + rbeta))
            kw.update(resid=dev16(r), res_stats=dev32(st), res_gamma=dev32(rgamma), res_beta=dev32(rbeta))
        out = N.linear_f16_norms(dev16(x), dev16(w), dev32(b) if with_bias else None, act, **kw)
        torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.float64)
        lim = 2e-3 * max(1.0, float(np.abs(y).max()))
        err = float(np.abs(got - y).max())
        record_property(kind, round(err / lim, 3))
        assert err <= lim, (kind, err, lim)
        worst = max(worst, err / lim)
    record_property("worst ratio", round(worst, 3))


@pytest.mark.parametrize("M", [1, 17, 64])
@pytest.mark.parametrize("K,I", [(384, 1536), (768, 3072)])
def test_folded_layernorm_stats_feed_residual(N, record_property, K, I, M):
    """the single-query forward's chain: FFN1 normalises the un-normalised rows x on load and leaves their (mean, rstd)
    in ln_stats_out; FFN2 takes those as res_stats and adds LN(x), normalised again from them, to its output.  float64
    reference: r16(r16(gelu(r16(LN(x)) W1^T + b1)) W2^T + b2) + r16(LN(x)), rounded to fp16; test_linear's bound on
    both outputs"""
    from scipy.special import erf

    g = np.random.default_rng(K + I + M)
    w1, w2 = r16(g.standard_normal((I, K)) * 0.05), r16(g.standard_normal((K, I)) * 0.05)
    b1, b2 = (0.1 * g.standard_normal(I)).astype(np.float32), (0.1 * g.standard_normal(K)).astype(np.float32)
    gamma, beta = ln_params(K, g)
    worst = 0.0
    for kind in ROW_KINDS:
        x = make_rows(kind, M, K, g)
        ln = r16(ln_ref64(x, gamma.astype(np.float64), beta.astype(np.float64), 1e-12)[0])
        h = ln @ w1.T + b1
        h = r16(0.5 * h * (1.0 + erf(h / np.sqrt(2.0))))
        y = r16(r16(h @ w2.T + b2) + ln)
        stats = torch.zeros((M, 2), dtype=torch.float32, device="cuda")
        xd = dev16(x)
        hd = N.linear_f16_norms(xd, dev16(w1), dev32(b1), 1, ln_gamma=dev32(gamma), ln_beta=dev32(beta), ln_eps=1e-12,
                                ln_stats_out=stats)
        yd = N.linear_f16_norms(hd, dev16(w2), dev32(b2), 0, resid=xd, res_stats=stats, res_gamma=dev32(gamma),
                                res_beta=dev32(beta))
        torch.cuda.synchronize()
        r = []
        for got, ref in ((hd, h), (yd, y)):
            lim = 2e-3 * max(1.0, float(np.abs(ref).max()))
            r.append(float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()) / lim)
        record_property(kind, [round(v, 3) for v in r])
        assert max(r) <= 1, (kind, r)
        worst = max(worst, *r)
    record_property("worst ratio", round(worst, 3))


def test_folded_layernorm_rejects_unsupported_shapes(N):
    """the folded LayerNorm exists only in the 16-feature single-query kernel: M <= 64, K in {384, 512, 768, 1024}"""
    g = np.random.default_rng(0)
    gamma, beta = ln_params(640, g)
    with pytest.raises(N.MMRagNativeError):
        N.linear_f16_norms(dev16(np.zeros((4, 640))), dev16(np.zeros((64, 640))), ln_gamma=dev32(gamma),
                           ln_beta=dev32(beta))
    gamma, beta = ln_params(384, g)
    with pytest.raises(N.MMRagNativeError):
        N.linear_f16_norms(dev16(np.zeros((65, 384))), dev16(np.zeros((64, 384))), ln_gamma=dev32(gamma),
                           ln_beta=dev32(beta))


# ---------------------------------------------------------------------------------------------------------------------
# C. the fp32 mode's ops
# ---------------------------------------------------------------------------------------------------------------------
def run_attention_f32(N, qkv, lens, heads):
    cu = torch.from_numpy(cu_of(lens)).cuda()
    got = N.attention_f32(dev32(qkv), cu, max(lens), heads)
    torch.cuda.synchronize()
    return got.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("L", SEAM_LENS)
@pytest.mark.parametrize("H,heads", LAYOUTS, ids=LAYOUT_IDS)
def test_attention_f32_seams(N, record_property, H, heads, L):
    """32-key blocks, 128-query tiles; |got - ref| <= A32 * P|V| + 1e-7 against float64 on the same float32 values"""
    lens = mixed_lens(L)
    g = np.random.default_rng(L + 5 * H)
    qkv = g.standard_normal((sum(lens), 3 * H)).astype(np.float32).astype(np.float64)
    ref, pav = attention_ref64(qkv, lens, heads, False)
    got = run_attention_f32(N, qkv, lens, heads)
    again = run_attention_f32(N, qkv, lens, heads)
    need = np.abs(got - ref) / (pav + 1e-7 / A32)
    i = np.unravel_index(int(np.argmax(need)), need.shape)
    record_property("worst ratio", round(float(need[i]) / A32, 3))
    assert np.array_equal(got, again)
    assert need[i] <= A32, ("token/col", i, got[i], ref[i], pav[i], float(need[i]))


@pytest.mark.parametrize("L", [31, 32, 33, 64, 65, 128, 129, 256, 257, 512])
@pytest.mark.parametrize("H,heads", [(384, 12), (768, 12)], ids=["12x32", "12x64"])
def test_attention_f32_exact_key_coverage(N, H, heads, L):
    """the Q = 0 probe of the fp16 test: 1024 / (keys) where planted, exactly 0 elsewhere (one fp32 rounding each of the
    reciprocal and the product)"""
    qkv, lens, want = plant_probe(L, H, heads, False)
    got = run_attention_f32(N, qkv, lens, heads)
    zero = want == 0
    assert np.all(got[zero] == 0), np.argwhere(zero & (got != 0))[:5].tolist()
    assert np.all(np.abs(got - want)[~zero] <= 2.0 ** -22 * want[~zero])


@pytest.mark.parametrize("H", [128, 384, 768, 1024])
@pytest.mark.parametrize("T", [1, 5, 333])
def test_layernorm_f32(N, record_property, T, H):
    """float32 rows of spread 1 around means of 0 and 3; per row |got - ref| <= L32 * max|ref| against float64"""
    g = np.random.default_rng(T + H)
    x = g.standard_normal((T, H)) + np.where(np.arange(T) % 2 == 0, 0.0, 3.0)[:, None]
    x = x.astype(np.float32).astype(np.float64)
    gamma, beta = ln_params(H, g)
    ref = ln_ref64(x, gamma.astype(np.float64), beta.astype(np.float64), 1e-12)[0]
    got = N.layernorm_f32(dev32(x), dev32(gamma), dev32(beta), 1e-12).cpu().numpy().astype(np.float64)
    ratio = np.abs(got - ref).max(axis=1) / (L32 * np.abs(ref).max(axis=1))
    record_property("worst ratio", round(float(ratio.max()), 3))
    assert ratio.max() <= 1.0, float(ratio.max())


@pytest.mark.parametrize("pool", [0, 1, 2], ids=["mean", "first", "select"])
def test_pool_norm_f32(N, pool):
    g = np.random.default_rng(pool)
    lens = [1, 9, 256, 40, 513]
    H = 768
    x = g.standard_normal((sum(lens), H)).astype(np.float32).astype(np.float64)
    cu = cu_of(lens)
    sel = np.array([0, 8, 100, 39, 512], np.int32)
    got = N.pool_norm_f32(dev32(x), torch.from_numpy(cu).cuda(), pool,
                          sel=torch.from_numpy(sel).cuda() if pool == 2 else None).cpu().numpy()
    rows = [x[a:b].mean(0) if pool == 0 else x[a + (s if pool == 2 else 0)] for a, b, s in zip(cu[:-1], cu[1:], sel)]
    ref = np.stack(rows)
    ref /= np.linalg.norm(ref, axis=1, keepdims=True)
    assert np.abs(got - ref).max() <= 1e-6, float(np.abs(got - ref).max())
