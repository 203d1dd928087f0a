"""What tests/test_surface_lut_cpu.py and tests/test_gpu_surface_lut.py share: the pictures and tables of the census, the conversions, and
the host twin's call.  The reference of a case is tests/spec_surface_lut.py, computed once per case (cached) and never changed."""
import ctypes as C
import functools

import numpy as np

import spec_rgb as sr
import spec_rgb_lut as sl
import spec_surface as ss
import spec_surface_lut as sx
from openvvc_amd import capi, engine

EINVAL, EUNSUP = -3, -5
TAIL = 80                                                     # bytes behind the surface that must stay as they were
TABLE_SIZES = sl.SIZES
PEAKS = (255, 1023, 4000, 65535)
WINDOWS = [(0, 0, 0, 0), (1, 0, 0, 1), (1, 1, 1, 1)]
PICTURES = [(72, 40), (20, 12)]
SRC_LOCS = (0, 1, 2)
# (source matrix, source range, destination matrix, destination range): BT.2020 limited to BT.709 limited and full, BT.601 to BT.2020
CONVS = [(9, 0, 1, 0), (9, 0, 1, 1), (5, 0, 9, 1)]
PATCH = 8                                                     # luma samples of a flat patch's side
# flat patches of the 72 x 40 census picture, inside every window: (first luma column, luma value); all on luma rows 8..15, chroma 512
PATCHES = ((8, 0), (24, 1023), (40, 300), (56, 800))


def conv_of(k: int, src_loc: int, dst_loc: int):
    sm, sf, dm, df = CONVS[k]
    return (sm, sf, src_loc, dm, df, dst_loc)


def c_conv(conv) -> capi.SurfaceConv:
    return engine.surface_conv(*conv)


@functools.lru_cache(maxsize=None)
def _planes(w: int, h: int, seed: int):
    y, cb, cr = sr.random_planes(w, h, seed)
    if (w, h) == (72, 40):
        for x, v in PATCHES:
            y[8:8 + PATCH, x:x + PATCH] = v
            cb[4:4 + PATCH // 2, x // 2:(x + PATCH) // 2] = 512
            cr[4:4 + PATCH // 2, x // 2:(x + PATCH) // 2] = 512
    for p in (y, cb, cr):
        p.setflags(write=False)
    return y, cb, cr


def census_planes(w: int, h: int, seed: int = 0):
    """random planes (read-only: shared); 72 x 40 carries the four flat grey patches: black, white and two greys between"""
    return _planes(w, h, seed)


@functools.lru_cache(maxsize=None)
def _table(size: int, peak: int, seed: int):
    t = sl.random_table(size, peak, seed)
    n = size - 1
    # the diagonal, which greys interpolate along: black and white to the two chroma extremes, the lower greys to white, the upper to black
    t[0, 0, 0] = (0, 0, peak)
    t[n, n, n] = (peak, peak, 0)
    for k in range(1, n):
        t[k, k, k] = (peak, peak, peak) if k <= n // 2 else (0, 0, 0)
    t.setflags(write=False)
    return t


def census_table(size: int, peak: int, seed: int = 0) -> np.ndarray:
    """a random table whose diagonal sends the census picture's patches to the ends of the output range (read-only: shared)"""
    return _table(size, peak, 1000 * size + peak % 97 + seed)


def loose(fmt: int, W: int, H: int) -> dict:
    return ss.loose_layout(fmt, W, H)


def window_size(w, h, window):
    return w - 2 * (window[0] + window[1]), h - 2 * (window[2] + window[3])


def strided(planes, strides):
    """the planes in arrays of the given strides (samples), 0xA5A5 behind every row"""
    held = []
    for p, s in zip(planes, (strides[0], strides[1], strides[1])):
        a = np.full((p.shape[0], s), 0xA5A5, np.uint16)
        a[:, :p.shape[1]] = p
        held.append(a)
    return held


def host_twin(lib, planes, conv, fmt, rounding, table, peak, window=(0, 0, 0, 0), strides=None, **lay):
    """ovhip_surface_lut_host of strided planes (default: 5 and 3 samples above the widths) into a buffer that held 0xA5 -> (the buffer:
    the surface and TAIL bytes behind it, the surface's size by ovhip_surface_bytes)"""
    h, w = planes[0].shape
    sy, sc = strides or (w + 5, w // 2 + 3)
    held = strided(planes, (sy, sc))
    win, cf, cc = capi.Window(*window), engine.surface_format(fmt, rounding, **lay), c_conv(conv)
    need = lib.ovhip_surface_bytes(w, h, C.byref(win), C.byref(cf))
    assert need, (w, h, fmt, window, lay)
    out = np.full(need + TAIL, ss.FILL, np.uint8)
    table = np.ascontiguousarray(table)
    r = lib.ovhip_surface_lut_host(held[0].ctypes.data, held[1].ctypes.data, held[2].ctypes.data, w, h, sy, sc, C.byref(win), C.byref(cc), C.byref(cf),
                                   table.shape[0], peak, table.ctypes.data, out.ctypes.data, need)
    assert r == 0, r
    return out, need


@functools.lru_cache(maxsize=None)
def _converted(w, h, seed, conv, size, peak, window):
    census = {}
    planes = sx.converted(census_planes(w, h, seed), conv, census_table(size, peak), peak, window, census=census)
    for p in planes:
        p.setflags(write=False)
    return planes, census


def reference(w, h, conv, size, peak, window, fmt, rounding, total=None, seed=0, **lay):
    """(bytes, size) of the restatement for a census picture and table; the converted picture is computed once per case"""
    planes, _ = _converted(w, h, seed, tuple(conv), size, peak, tuple(window))
    return ss.surface(planes, fmt, rounding, total=total, **lay)


def census_of(w, h, conv, size, peak, window, seed=0) -> dict:
    return _converted(w, h, seed, tuple(conv), size, peak, tuple(window))[1]
