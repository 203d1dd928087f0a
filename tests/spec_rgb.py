"""RGB output: the definition of include/ovvc_hip.h ("RGB output on the device") restated in numpy, whole planes at a time, with the
coefficients from exact rationals (fractions).  Integer only, so the host twin and the kernel are compared with it for equality.
Written from the definition, not from the C: the C walks pixels, this builds index and weight vectors per axis."""
from fractions import Fraction as F

import numpy as np

U8, U16, F16, F32 = 0, 1, 2, 3
PLANAR, PACKED = 0, 1
NP_DTYPE = {U8: np.uint8, U16: np.uint16, F16: np.float16, F32: np.float32}
MATRICES = (1, 5, 6, 9)
# H.273 MatrixCoefficients -> (Kr, Kb)
KR_KB = {1: (F(2126, 10000), F(722, 10000)), 5: (F(299, 1000), F(114, 1000)), 6: (F(299, 1000), F(114, 1000)), 9: (F(2627, 10000), F(593, 10000))}
S = 14


def n_bits(dtype: int) -> int:
    return 8 if dtype == U8 else 10


def real_factors(matrix: int, full_range: int, nbits: int):
    """(cy, rv, gu, gv, bu) as exact rationals, and yoff"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    peak = F(2 ** nbits - 1)
    sy, sc, yoff = (peak / 1023, peak / 1023, 0) if full_range else (peak / 876, peak / 896, 64)
    rv = 2 * sc * (1 - kr)
    bu = 2 * sc * (1 - kb)
    return (sy, rv, bu * kb / kg, rv * kr / kg, bu), yoff


def coefs(matrix: int, full_range: int, nbits: int):
    """the integer coefficients: each factor times 2^14 rounded to nearest on the exact rational; asserts that none is a tie"""
    fac, yoff = real_factors(matrix, full_range, nbits)
    out = []
    for f in fac:
        v = f * 2 ** S
        lo = v.numerator // v.denominator
        frac = v - lo
        assert frac != F(1, 2), (matrix, full_range, nbits, f)
        out.append(lo + (1 if frac > F(1, 2) else 0))
    return tuple(out), yoff


def _axis(n_luma: int, n_chroma: int, off: int):
    """per luma coordinate: the two clamped chroma indices and the weight of the second, in quarters"""
    p = 2 * np.arange(n_luma, dtype=np.int64) - off
    k0, f = p >> 2, p & 3
    return np.clip(k0, 0, n_chroma - 1), np.clip(k0 + 1, 0, n_chroma - 1), f


def chroma16(c: np.ndarray, loc: int, w: int, h: int) -> np.ndarray:
    """16 times the bilinear chroma value at every luma position of the w x h picture (int64, not rounded)"""
    a = loc & 1
    b = {0: 1, 1: 1, 2: 0, 3: 0, 4: 2, 5: 2}[loc]
    c = c.astype(np.int64)
    i0, i1, fx = _axis(w, c.shape[1], a)
    j0, j1, fy = _axis(h, c.shape[0], b)
    top = (4 - fx)[None, :] * c[j0][:, i0] + fx[None, :] * c[j0][:, i1]
    bot = (4 - fx)[None, :] * c[j1][:, i0] + fx[None, :] * c[j1][:, i1]
    return (4 - fy)[:, None] * top + fy[:, None] * bot


def crop(p: np.ndarray, window) -> np.ndarray:
    l, r, a, b = window
    return p[2 * a:p.shape[0] - 2 * b, 2 * l:p.shape[1] - 2 * r]


def rgb_int(y, cb, cr, matrix: int, full_range: int, loc: int, nbits: int, window=(0, 0, 0, 0)) -> np.ndarray:
    """(3, H, W) int64: the clipped integers"""
    (cy, rv, gu, gv, bu), yoff = coefs(matrix, full_range, nbits)
    h, w = y.shape
    L = 16 * cy * (y.astype(np.int64) - yoff)
    u = chroma16(cb, loc, w, h) - 8192
    v = chroma16(cr, loc, w, h) - 8192
    acc = np.stack([L + rv * v, L - gu * u - gv * v, L + bu * u])
    assert np.abs(acc).max() < 2 ** 31 - 2 ** 17
    out = np.clip((acc + 2 ** 17) >> 18, 0, 2 ** nbits - 1)
    return np.stack([crop(p, window) for p in out])


def store(v: np.ndarray, dtype: int, layout: int, window=(0, 0, 0, 0)) -> np.ndarray:
    """(3, h, w) clipped integers of the whole picture -> the RGB picture of the window as the library stores it: (3, H, W) or (H, W, 3)
    in the format's dtype"""
    v = np.stack([crop(p, window) for p in v])
    if dtype in (U8, U16):
        out = v.astype(NP_DTYPE[dtype])
    else:
        out = v.astype(np.float32) * np.float32(1.0 / 1023)
        assert out.dtype == np.float32
        if dtype == F16:
            out = out.astype(np.float16)               # round to nearest even
    return np.ascontiguousarray(out if layout == PLANAR else out.transpose(1, 2, 0))


def convert(y, cb, cr, matrix: int, full_range: int, loc: int, dtype: int, layout: int, window=(0, 0, 0, 0)) -> np.ndarray:
    return store(rgb_int(y, cb, cr, matrix, full_range, loc, n_bits(dtype)), dtype, layout, window)


def rgb_real(y, cb, cr, matrix: int, full_range: int, loc: int, nbits: int) -> np.ndarray:
    """the real-valued model: the same c16, double arithmetic, the exact factors, before the clip -> (3, h, w) float64"""
    fac, yoff = real_factors(matrix, full_range, nbits)
    cy, rv, gu, gv, bu = (float(f) for f in fac)
    h, w = y.shape
    L = cy * (y.astype(np.float64) - yoff)
    u = chroma16(cb, loc, w, h).astype(np.float64) / 16 - 512
    v = chroma16(cr, loc, w, h).astype(np.float64) / 16 - 512
    return np.stack([L + rv * v, L - gu * u - gv * v, L + bu * u])


def rgb_unclipped(y, cb, cr, matrix: int, full_range: int, loc: int, nbits: int) -> np.ndarray:
    """the integer pipeline before its clip (for the comparison with rgb_real)"""
    (cy, rv, gu, gv, bu), yoff = coefs(matrix, full_range, nbits)
    h, w = y.shape
    L = 16 * cy * (y.astype(np.int64) - yoff)
    u = chroma16(cb, loc, w, h) - 8192
    v = chroma16(cr, loc, w, h) - 8192
    return (np.stack([L + rv * v, L - gu * u - gv * v, L + bu * u]) + 2 ** 17) >> 18


def random_planes(w: int, h: int, seed: int):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1024, (h, w), dtype=np.uint16), rng.integers(0, 1024, (h // 2, w // 2), dtype=np.uint16),
            rng.integers(0, 1024, (h // 2, w // 2), dtype=np.uint16))
