"""Reference for FP8 (E4M3) collections: numpy float64, no torch kernels.

The storage format of include/mmrag.h MMRAG_F8E4M3: a stored element is the OCP E4M3 code of x * 256 rounded to nearest
even (subnormals kept, magnitudes above 448 saturate to 448, NaN stores +0); a score is the dot product of the decoded
values times 2^-16."""
import numpy as np

SCALE = 256.0


def _table():
    t = np.zeros(256, np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        v = m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)
        if (c & 0x7F) == 0x7F:
            v = np.nan
        t[c] = -v if c & 0x80 else v
    return t


TABLE = _table()
# the 127 non-negative finite values in code order (code == index)
_POS = TABLE[:127]


def encode_scaled(y):
    """E4M3 codes (uint8) of the values y (already scaled), explicit round to nearest even"""
    y = np.asarray(y, np.float64)
    a = np.abs(y)
    a = np.where(np.isnan(a), 0.0, np.minimum(a, 448.0))
    hi = np.searchsorted(_POS, a, side="left")          # first code with value >= a
    hi = np.minimum(hi, 126)
    lo = np.maximum(hi - 1, 0)
    d_lo, d_hi = a - _POS[lo], _POS[hi] - a
    take_hi = (d_hi < d_lo) | ((d_hi == d_lo) & (hi % 2 == 0))   # tie: even mantissa == even code
    code = np.where(take_hi, hi, lo).astype(np.uint8)
    sign = (np.signbit(y) & ~np.isnan(y)).astype(np.uint8) << 7
    return code | sign


def encode(x):
    """codes of float32 values x as stored: x * 256 is exact in float32 (a power of two)"""
    return encode_scaled(np.asarray(x, np.float32).astype(np.float64) * SCALE)


def decode(code):
    return TABLE[np.asarray(code, np.uint8)]


def scores(q_codes, c_codes):
    """float64 [B, n] scores of code matrices (pad columns are code 0)"""
    return decode(q_codes) @ decode(c_codes).T * 2.0 ** -16


def topk(s, k, alive=None):
    """rows [B, k] and scores [B, k] by (score desc, row asc); -1 / -inf padded"""
    s = np.array(s, np.float64)
    if alive is not None:
        s[:, ~alive] = -np.inf
    B, n = s.shape
    rows = np.full((B, k), -1, np.int64)
    vals = np.full((B, k), -np.inf)
    for b in range(B):
        order = np.lexsort((np.arange(n), -s[b]))[:k]
        order = order[np.isfinite(s[b][order])]
        rows[b, :order.size] = order
        vals[b, :order.size] = s[b][order]
    return rows, vals


def rescore(q, c, cand_rows, k):
    """float64 re-scoring of candidate lists: q [B, d], c [n, d] full precision, cand_rows [B, C] (-1 ends a list)"""
    B = cand_rows.shape[0]
    rows = np.full((B, k), -1, np.int64)
    vals = np.full((B, k), -np.inf)
    for b in range(B):
        cr = cand_rows[b]
        neg = np.nonzero(cr < 0)[0]
        cr = cr[: neg[0]] if neg.size else cr
        s = np.asarray(c, np.float64)[cr] @ np.asarray(q[b], np.float64)
        order = np.lexsort((cr, -s))[:k]
        rows[b, :order.size] = cr[order]
        vals[b, :order.size] = s[order]
    return rows, vals


def sweep():
    """float32 values x whose x * 256 holds every representable magnitude, every midpoint between neighbours, points
    just either side of them, the subnormal range, +-0 and values up to 1.01 * 256 (x * 256 stays at or below 448: see
    saturating() for what lies above, where torch's cast yields NaN and the storage format saturates)"""
    pos = _POS
    mids = (pos[:-1] + pos[1:]) / 2
    pts = np.concatenate([pos, mids, np.nextafter(mids.astype(np.float32), np.float32(0)).astype(np.float64),
                          np.nextafter(mids.astype(np.float32), np.float32(1e9)).astype(np.float64),
                          np.linspace(0, 2.0 ** -6, 257), np.linspace(0, 1.01 * 256, 1001)])
    y = np.concatenate([pts, -pts]).astype(np.float32)
    return (y / np.float32(256.0)).astype(np.float32)     # exact: a power of two


def saturating():
    """float32 x with |x * 256| above 448 (stored as +-448 = 0x7e / 0xfe), and NaN (stored as +0)"""
    y = np.array([449.0, 463.9, 464.0, 465.0, 500.0, 1e6, np.inf], np.float32)
    return np.concatenate([y, -y, [np.nan]]).astype(np.float32) / np.float32(256.0)


def clustered(n=20000, d=768, n_q=128, seed=1):
    import torch

    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(200, d, generator=g)
    rows = centres[torch.randint(0, 200, (n,), generator=g)] + 0.35 * torch.randn(n, d, generator=g)
    qs = centres[torch.randint(0, 200, (n_q,), generator=g)] + 0.35 * torch.randn(n_q, d, generator=g)
    rows = torch.nn.functional.normalize(rows, dim=1)
    qs = torch.nn.functional.normalize(qs, dim=1)
    return rows.numpy().astype(np.float32), qs.numpy().astype(np.float32)
