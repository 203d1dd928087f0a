"""Colour tables for the RGB output through a colour table (include/ovvc_hip.h, "RGB output through a colour table"; engine.RgbLut).

A table is a numpy array of shape (S, S, S, 3) and dtype uint16 in the index order [b][g][r][c]: red is fastest, c = 0, 1, 2 are the
output's R, G, B, every entry is in 0..peak.  This module builds such tables in float64 with numpy alone.  It is not on the hot path and
nothing here is pinned bit for bit: the exact step is the library's, the colour science is the caller's.  pq_bt2020_to_bt709 is one
worked example of such science, not this project's opinion on tone mapping."""
from __future__ import annotations

import numpy as np

SIZES = (17, 33, 65)

# SMPTE ST 2084 (PQ)
_M1, _M2 = 2610 / 16384, 2523 / 4096 * 128
_C1, _C2, _C3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
# CIE xy of the primaries (R, G, B) and of D65
BT2020_XY = ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046))
BT709_XY = ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060))
D65_XY = (0.3127, 0.3290)


def _check(size: int, peak: int) -> None:
    if size not in SIZES:
        raise ValueError(f"table size {size}: one of {SIZES}")
    if not 1 <= peak <= 65535:
        raise ValueError(f"table peak {peak}: 1..65535")


def _quantise(v: np.ndarray, peak: int) -> np.ndarray:
    """floor(v * peak + 0.5), clipped to the table's range"""
    return np.clip(np.floor(np.asarray(v, np.float64) * peak + 0.5), 0, peak).astype(np.uint16)


def lattice(size: int) -> np.ndarray:
    """T[b][g][r] = (1023 r, 1023 g, 1023 b): with peak 65535 the interpolated output is exactly (size - 1) * (R, G, B)"""
    _check(size, 65535)
    k = 1023 * np.arange(size, dtype=np.uint16)
    t = np.empty((size, size, size, 3), np.uint16)
    t[..., 0] = k[None, None, :]
    t[..., 1] = k[None, :, None]
    t[..., 2] = k[:, None, None]
    return t


def from_function(f, size: int, peak: int) -> np.ndarray:
    """the table of f, which maps an (..., 3) array of R'G'B' in 0..1 to RGB in 0..1: lattice point k of a channel is k / (size - 1),
    an entry is floor(v * peak + 0.5) clipped to 0..peak"""
    _check(size, peak)
    k = np.arange(size, dtype=np.float64) / (size - 1)
    grid = np.empty((size, size, size, 3), np.float64)
    grid[..., 0] = k[None, None, :]
    grid[..., 1] = k[None, :, None]
    grid[..., 2] = k[:, None, None]
    out = np.asarray(f(grid), np.float64)
    if out.shape != grid.shape:
        raise ValueError(f"the function returned shape {out.shape}, not {grid.shape}")
    return _quantise(out, peak)


def write_cube(path, table: np.ndarray, peak: int, title: "str | None" = None) -> None:
    """the table as a .cube text file: entries divided by peak, red fastest (this table's own order)"""
    size = table.shape[0]
    if table.shape != (size, size, size, 3) or table.dtype != np.uint16:
        raise ValueError("a table has shape (S, S, S, 3) and dtype uint16")
    _check(size, peak)
    if int(table.max()) > peak:
        raise ValueError("an entry is above the peak")
    with open(path, "w") as fh:
        if title is not None:
            fh.write(f'TITLE "{title}"\n')
        fh.write(f"LUT_3D_SIZE {size}\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 1 1\n")
        for r, g, b in table.reshape(-1, 3).astype(np.float64) / peak:
            fh.write(f"{r:.10f} {g:.10f} {b:.10f}\n")


def read_cube(path, peak: int) -> np.ndarray:
    """a .cube text file as a table of that peak: LUT_3D_SIZE, an optional TITLE, DOMAIN_MIN / DOMAIN_MAX (only 0 0 0 / 1 1 1), lines
    starting with # are comments; values are quantised as from_function's"""
    size, rows = None, []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            word = line.split()
            if word[0] == "TITLE":
                continue
            if word[0] == "LUT_3D_SIZE":
                size = int(word[1])
            elif word[0] in ("DOMAIN_MIN", "DOMAIN_MAX"):
                want = 0.0 if word[0] == "DOMAIN_MIN" else 1.0
                if len(word) != 4 or any(float(x) != want for x in word[1:]):
                    raise ValueError(f"{path}:{n}: only the domain 0 0 0 .. 1 1 1 is read")
            elif word[0][0].isalpha():
                raise ValueError(f"{path}:{n}: keyword {word[0]} is not read")
            else:
                if len(word) != 3:
                    raise ValueError(f"{path}:{n}: three values expected")
                rows.append([float(x) for x in word])
    if size is None:
        raise ValueError(f"{path}: no LUT_3D_SIZE")
    _check(size, peak)
    if len(rows) != size ** 3:
        raise ValueError(f"{path}: {len(rows)} entries, {size ** 3} expected")
    return _quantise(np.array(rows, np.float64).reshape(size, size, size, 3), peak)


def pq_inverse_eotf(nits) -> np.ndarray:
    """ST 2084: luminance in cd/m^2 (0..10000) -> the non-linear signal 0..1"""
    y = np.power(np.clip(np.asarray(nits, np.float64) / 10000.0, 0.0, None), _M1)
    return np.power((_C1 + _C2 * y) / (1.0 + _C3 * y), _M2)


def pq_eotf(signal) -> np.ndarray:
    """ST 2084: the non-linear signal 0..1 -> luminance in cd/m^2"""
    p = np.power(np.clip(np.asarray(signal, np.float64), 0.0, None), 1.0 / _M2)
    return 10000.0 * np.power(np.maximum(p - _C1, 0.0) / (_C2 - _C3 * p), 1.0 / _M1)


def rgb_to_xyz(primaries_xy, white_xy=D65_XY) -> np.ndarray:
    """the 3 x 3 matrix from linear RGB of these primaries to CIE XYZ, white (1, 1, 1) at white_xy with Y = 1"""
    xyz = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in primaries_xy], np.float64).T
    xw, yw = white_xy
    s = np.linalg.solve(xyz, np.array([xw / yw, 1.0, (1.0 - xw - yw) / yw], np.float64))
    return xyz * s[None, :]


def bt2020_to_bt709_matrix() -> np.ndarray:
    """linear BT.2020 RGB -> linear BT.709 RGB, from the two sets of primaries and D65; each row sums to 1"""
    m = np.linalg.solve(rgb_to_xyz(BT709_XY), rgb_to_xyz(BT2020_XY))
    assert np.abs(m.sum(axis=1) - 1.0).max() < 1e-12
    return m


def bt2390_eetf(e1: np.ndarray, max_lum: float) -> np.ndarray:
    """BT.2390 EETF with black at 0, on the PQ signal normalised to the source's range: the identity below the knee KS = 1.5 maxLum -
    0.5, above it the Hermite spline that ends at maxLum"""
    ks = 1.5 * max_lum - 0.5
    t = np.clip((e1 - ks) / (1.0 - ks), 0.0, 1.0)
    spline = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1.0 - ks) + (-2 * t ** 3 + 3 * t ** 2) * max_lum
    return np.where(e1 < ks, e1, spline)


def pq_bt2020_to_bt709(size: int, peak: int, src_nits: float = 1000.0, dst_nits: float = 100.0) -> np.ndarray:
    """One worked conversion: PQ-coded BT.2020 R'G'B' mastered at src_nits -> gamma 2.4 BT.709 R'G'B' for a display of dst_nits.

    The ST 2084 EOTF per channel; m = max(R, G, B) in nits; the BT.2390 EETF on m in the PQ domain; all three channels scaled by
    m' / m (the hue is kept); divided by dst_nits; the BT.2020 -> BT.709 matrix; clipped to 0..1; the power 1 / 2.4."""
    pq_src, pq_dst = float(pq_inverse_eotf(src_nits)), float(pq_inverse_eotf(dst_nits))
    matrix = bt2020_to_bt709_matrix()

    def f(rgb):
        lin = pq_eotf(rgb)
        m = lin.max(axis=-1, keepdims=True)
        e1 = np.minimum(pq_inverse_eotf(m) / pq_src, 1.0)
        m2 = pq_eotf(bt2390_eetf(e1, pq_dst / pq_src) * pq_src)
        scale = np.divide(m2, m, out=np.zeros_like(m), where=m > 0)
        out = (lin * scale / dst_nits) @ matrix.T
        return np.power(np.clip(out, 0.0, 1.0), 1.0 / 2.4)

    return from_function(f, size, peak)
