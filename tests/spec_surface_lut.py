"""Surface output through a colour table: the definition of include/ovvc_hip.h ("Surface output through a colour table") restated in
numpy, whole planes at a time.  It composes the restatements of its parts -- spec_rgb_lut.rgb10 and interpolate for the table's output,
spec_surface.surface for the store -- around parts 3 to 6 written here from the header's text: the normalising division, the forward
matrix with coefficients from exact rationals (fractions), the luma plane and the 4:2:0 filters.  Integer only, so the host twin and the
kernel are compared with it for equality.  Written from the definition, not from the C: the C walks chroma samples and their nine
taps, this builds clamped index vectors per axis and adds shifted planes."""
from fractions import Fraction as F

import numpy as np

import spec_rgb as sr
import spec_rgb_lut as sl
import spec_surface as ss

S = 14
DST_MATRICES = (1, 5, 6, 9)
DST_LOCS = (0, 1, 2, 3)


def rnd(v: F) -> int:
    """to nearest; asserts that it is no tie"""
    lo = v.numerator // v.denominator                    # floor, also below zero
    frac = v - lo
    assert frac != F(1, 2), v
    return lo + (1 if frac > F(1, 2) else 0)


def real_rows(matrix: int, full_range: int):
    """the three rows of the forward matrix as exact rationals (on R'G'B' in 0..1 -> 10-bit units without the offsets), and yoff"""
    kr, kb = sr.KR_KB[matrix]
    kg = 1 - kr - kb
    sy, sc, yoff = (F(1), F(1), 0) if full_range else (F(876, 1023), F(896, 1023), 64)
    return ((sy * kr, sy * kg, sy * kb),
            (-sc * kr / (2 * (1 - kb)), -sc * kg / (2 * (1 - kb)), sc / 2),
            (sc / 2, -sc * kg / (2 * (1 - kr)), -sc * kb / (2 * (1 - kr)))), yoff


def coefs(matrix: int, full_range: int):
    """(y_r, y_g, y_b, b_r, b_g, b_b, r_r, r_g, r_b) and yoff, as the header derives them"""
    (yr, yg, yb), (br, bg, bb), (rr, rg, rb) = real_rows(matrix, full_range)[0]
    yoff = real_rows(matrix, full_range)[1]
    k = 2 ** S
    T = rnd((yr + yg + yb) * k)
    y_r, y_b = rnd(yr * k), rnd(yb * k)
    b_r, b_g = rnd(br * k), rnd(bg * k)
    r_g, r_b = rnd(rg * k), rnd(rb * k)
    return (y_r, T - y_r - y_b, y_b, b_r, b_g, -b_r - b_g, -r_g - r_b, r_g, r_b), yoff


def bound14(matrix: int, full_range: int):
    """the largest distance, in units of 2^-4 of a 10-bit step, between (Y14, Cb14, Cr14) and the real-valued model on the same table
    output, derived and not measured: 1/2 for the row's own rounding shift, plus the row's absolute coefficients times the 1/2 a
    normalised value can be off, plus each coefficient's own distance from its exact rational times the largest q, 16368"""
    rows = real_rows(matrix, full_range)[0]
    c = coefs(matrix, full_range)[0]
    out = []
    for k, row in enumerate(rows):
        ints = c[3 * k:3 * k + 3]
        q_part = F(sum(abs(v) for v in ints), 2 * 2 ** S)
        c_part = sum(abs(F(v) - e * 2 ** S) for v, e in zip(ints, row)) * F(16368, 2 ** S)
        out.append(float(F(1, 2) + q_part + c_part))
    return tuple(out)


def normalise(o: np.ndarray, peak: int) -> np.ndarray:
    return (16368 * o.astype(np.int64) + peak // 2) // peak


def forward14(o: np.ndarray, peak: int, matrix: int, full_range: int) -> np.ndarray:
    """o: (3, ...) the table's output in 0..peak -> (3, ...) int64 (Y14, Cb14, Cr14)"""
    c, yoff = coefs(matrix, full_range)
    q = normalise(o, peak)
    assert q.min() >= 0 and q.max() <= 16368
    rows = [c[3 * k] * q[0] + c[3 * k + 1] * q[1] + c[3 * k + 2] * q[2] for k in range(3)]
    assert max(np.abs(r).max() for r in rows) < 2 ** 31 - 2 ** 13
    return np.stack([16 * yoff + ((rows[0] + 2 ** 13) >> S), 8192 + ((rows[1] + 2 ** 13) >> S), 8192 + ((rows[2] + 2 ** 13) >> S)])


def model14(o: np.ndarray, peak: int, matrix: int, full_range: int) -> np.ndarray:
    """the real-valued model of the same step in float64, in the units of forward14"""
    rows, yoff = real_rows(matrix, full_range)
    x = o.astype(np.float64) / peak * 16368.0
    out = [sum(float(e) * x[k] for k, e in enumerate(row)) for row in rows]
    return np.stack([16.0 * yoff + out[0], 8192.0 + out[1], 8192.0 + out[2]])


def taps(n_out: int, n_in: int, three: bool, first: int = 0):
    """[(clamped positions (n_out,), weight)]: 2k-1, 2k, 2k+1 with 1 2 1, or 2k, 2k+1 with 2 2; positions count from `first` of an axis
    of n_in samples they are clamped to"""
    k = np.arange(n_out, dtype=np.int64)
    offs = ((-1, 1), (0, 2), (1, 1)) if three else ((0, 2), (1, 2))
    return [(np.clip(first + 2 * k + d, 0, n_in - 1), w) for d, w in offs]


def subsample(c14: np.ndarray, dst_loc: int, rect=None) -> np.ndarray:
    """c14: (H, W) -> (H/2, W/2) clip((sum + 128) >> 8).  rect = (x0, y0, W, H): the window inside a larger plane whose edges the taps
    clamp to -- NOT the definition, which clamps to the window (rect None: c14 is the window)"""
    x0, y0, W, H = rect if rect is not None else (0, 0, c14.shape[1], c14.shape[0])
    acc = np.zeros((H // 2, W // 2), np.int64)
    for rows, wy in taps(H // 2, c14.shape[0], dst_loc >= 2, y0):
        for cols, wx in taps(W // 2, c14.shape[1], (dst_loc & 1) == 0, x0):
            acc += wy * wx * c14[rows][:, cols]
    return acc


def converted(planes, conv, table: np.ndarray, peak: int, window=(0, 0, 0, 0), clamp_to_picture: bool = False, census: "dict | None" = None):
    """the converted picture (y, cb, cr) of the window, uint16; conv = (src_matrix, src_full, src_loc, dst_matrix, dst_full, dst_loc).
    census: filled with what the inputs exercised"""
    sm, sf, sloc, dm, df, dloc = conv
    assert int(table.max()) <= peak and dloc in DST_LOCS
    y, cb, cr = planes
    h, w = y.shape
    l, r, a, b = window
    rect = (2 * l, 2 * a, w - 2 * (l + r), h - 2 * (a + b))
    rgb = sl.rgb10(y, cb, cr, sm, sf, sloc, (0, 0, 0, 0) if clamp_to_picture else window)
    v14 = forward14(sl.interpolate(rgb, table), peak, dm, df)
    y14 = v14[0] if not clamp_to_picture else sr.crop(v14[0], window)
    y_pre = (y14 + 8) >> 4
    accs = [subsample(v14[k], dloc, rect if clamp_to_picture else None) for k in (1, 2)]
    c_pre = [(acc + 128) >> 8 for acc in accs]
    if census is not None:
        census.setdefault("y_pre", []).append((int(y_pre.min()), int(y_pre.max())))
        census.setdefault("c_pre", []).append((min(int(c.min()) for c in c_pre), max(int(c.max()) for c in c_pre)))
        census.setdefault("rgb", []).append(rgb.reshape(3, -1))
    return tuple(np.clip(p, 0, 1023).astype(np.uint16) for p in (y_pre, c_pre[0], c_pre[1]))


def surface(planes, conv, table, peak, fmt, rounding=ss.ROUND, window=(0, 0, 0, 0), clamp_to_picture: bool = False, census=None, **layout):
    """(bytes of the surface, its size): spec_surface.surface of the converted picture"""
    return ss.surface(converted(planes, conv, table, peak, window, clamp_to_picture, census), fmt, rounding, **layout)
