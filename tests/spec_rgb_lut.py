"""RGB output through a colour table: the definition of include/ovvc_hip.h ("RGB output through a colour table") restated in numpy on
top of spec_rgb.rgb_int(..., nbits=10), whole planes at a time.  Integer only, so the host twin and the kernel are compared with it for
equality.  Written from the definition, not from the C: the C sorts three channels with compare-and-swap per pixel, this picks the
order of a whole picture with argsort (or, under tie_break=1, with the channels reversed first: another order wherever two fractions are
equal)."""
import numpy as np

import spec_rgb as sr

SIZES = (17, 33, 65)


def cells(v: np.ndarray, size: int):
    """channel values 0..1023 -> (cell index, fraction 0..1023)"""
    n = size - 1
    t = v.astype(np.int64) * n
    i = t // 1023
    f = t - 1023 * i
    top = i == n
    return np.where(top, n - 1, i), np.where(top, 1023, f)


def order(f: np.ndarray, tie_break: int = 0) -> np.ndarray:
    """f: (3, ...) fractions of (r, g, b) -> (3, ...) the channels by fraction descending; tie_break 0: the lower channel first among
    equals, 1: the higher one"""
    if tie_break == 0:
        return np.argsort(-f, axis=0, kind="stable")
    return 2 - np.argsort(-f[::-1], axis=0, kind="stable")


def interpolate(rgb: np.ndarray, table: np.ndarray, tie_break: int = 0) -> np.ndarray:
    """rgb: (3, ...) int in 0..1023; table: (S, S, S, 3) in the order [b][g][r][c] -> (3, ...) int64 o"""
    size = table.shape[0]
    assert table.shape == (size, size, size, 3) and size in SIZES
    assert rgb.min() >= 0 and rgb.max() <= 1023
    i, f = cells(rgb, size)
    ch = order(f, tie_break)
    fs = np.take_along_axis(f, ch, axis=0)                                # f1 >= f2 >= f3
    assert (fs[0] >= fs[1]).all() and (fs[1] >= fs[2]).all()
    w = [1023 - fs[0], fs[0] - fs[1], fs[1] - fs[2], fs[2]]
    assert (sum(w) == 1023).all()
    t = table.astype(np.int64)
    idx = i.copy()                                                        # (r, g, b) of the vertex
    acc = np.full(rgb.shape, 511, np.int64)
    for k in range(4):
        if k:
            np.put_along_axis(idx, ch[k - 1:k], np.take_along_axis(idx, ch[k - 1:k], axis=0) + 1, axis=0)
        acc += w[k][None] * np.moveaxis(t[idx[2], idx[1], idx[0]], -1, 0)
    assert acc.max() < 2 ** 26
    return acc // 1023


def store(o: np.ndarray, peak: int, dtype: int, layout: int) -> np.ndarray:
    """(3, H, W) interpolated integers -> the picture as the library stores it"""
    if dtype in (sr.U8, sr.U16):
        assert dtype != sr.U8 or peak <= 255
        out = o.astype(sr.NP_DTYPE[dtype])
    else:
        out = o.astype(np.float32) * np.float32(1.0 / peak)
        assert out.dtype == np.float32
        if dtype == sr.F16:
            out = out.astype(np.float16)               # round to nearest even, subnormals included
    return np.ascontiguousarray(out if layout == sr.PLANAR else out.transpose(1, 2, 0))


def rgb10(y, cb, cr, matrix: int, full_range: int, loc: int, window=(0, 0, 0, 0)) -> np.ndarray:
    """the table's input: the clipped integers of the RGB output at N = 10, whatever the dtype, of the window"""
    return sr.rgb_int(y, cb, cr, matrix, full_range, loc, 10, window)


def convert(y, cb, cr, matrix: int, full_range: int, loc: int, dtype: int, layout: int, table: np.ndarray, peak: int, window=(0, 0, 0, 0),
            tie_break: int = 0) -> np.ndarray:
    assert int(table.max()) <= peak
    return store(interpolate(rgb10(y, cb, cr, matrix, full_range, loc, window), table, tie_break), peak, dtype, layout)


def random_table(size: int, peak: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, peak + 1, (size, size, size, 3), dtype=np.uint16)
