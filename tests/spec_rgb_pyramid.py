"""Numpy restatement of "RGB pyramid on the device" (include/ovvc_hip.h): level r of a pyramid is, by definition, the RGB output -- with a
table: the RGB output through the table -- of the reduced picture: spec_rgb.convert or spec_rgb_lut.convert of
spec_reduce.reduce_picture(...).  So there is nothing here but that composition, the census of pyramids the tests run, and the
conditions the census must meet, asserted on import on the restatement alone.  Integer only up to the one float multiplication of a
float element: what it gives is compared for equality with ovhip_rgb_pyramid_host and k_rgb_pyramid.

The sizes go by k_rgb_pyramid's tile of 120 x 12 pixels (its chroma: 60 x 6 with one column and row of halo on each side)."""
import functools

import numpy as np

import spec_reduce as sd
import spec_rgb as sr
import spec_rgb_lut as st
from spec_ladder_lut import ramp_planes

MAX_LEVELS = 8
TILE_W, TILE_H = 120, 12
U8, U16, F16, F32, CHW, HWC = sr.U8, sr.U16, sr.F16, sr.F32, sr.PLANAR, sr.PACKED
ES = {U8: 1, U16: 2, F16: 2, F32: 4}


def level(w, h, dtype=U8, layout=CHW):
    """one level's description: size, dtype, layout"""
    return (w, h, dtype, layout)


def level_bytes(lv):
    w, h, dtype, _layout = lv
    return 3 * w * h * ES[dtype]


def pyramid(planes, levels, matrix, full_range, loc, table=None, peak=0, window=(0, 0, 0, 0), reduced=None):
    """[level r as the library stores it: (3, H, W) or (H, W, 3) in the level's dtype]; reduced: the levels' reduced pictures where the
    caller holds them already"""
    out = []
    for k, (w, h, dtype, layout) in enumerate(levels):
        red = reduced[k] if reduced is not None else sd.reduce_picture(*planes, w, h, window, loc)
        if table is None:
            out.append(np.ascontiguousarray(sr.convert(*red, matrix, full_range, loc, dtype, layout)))
        else:
            out.append(np.ascontiguousarray(st.convert(*red, matrix, full_range, loc, dtype, layout, table, peak)))
    return out


_ALL = [(d, l) for d in (F16, U8, U16, F32) for l in (CHW, HWC)]                      # every dtype in both layouts: 8 formats
# on 544 x 96: 1:1, 4/3, 2:1 twice, 4:1, 8/3 (width 4 mod 8), 8:1 (width 4 mod 8), 68/9 by 6 (narrower than a tile, lower than two)
_SIZES8 = [(544, 96), (408, 72), (272, 48), (272, 48), (136, 24), (204, 36), (68, 12), (72, 16)]
_EIGHT = [level(w, h, d, l) for (w, h), (d, l) in zip(_SIZES8, _ALL)]

# name -> (source, window, levels, (matrix, full_range), (table size, peak) or None, chroma locations)
CENSUS = {
    # 4.5 x 8, 3.4 x 6 and 2.3 x 4 tiles at 1:1, 4/3 and 2:1: the chroma halo crosses tile seams on both axes; a level narrower than a
    # tile and lower than two; widths that are 4 mod 8; eight levels; every dtype in both layouts, so a U8 and a U16 level -- the 8-bit
    # and the 10-bit coefficient set -- in one launch; every chroma location
    "A": ((544, 96), (0, 0, 0, 0), _EIGHT, (1, 0), None, tuple(range(6))),
    # the same through a table whose peak a U8 level can take; full range
    "T": ((544, 96), (0, 0, 0, 0), _EIGHT, (9, 1), (17, 255), (0, 3)),
    # full range without a table: two coefficient sets again
    "F": ((136, 24), (0, 0, 0, 0), [level(136, 24, U8, HWC), level(68, 12, U16, CHW), level(136, 24, F32, CHW)], (9, 1), None, (1, 4)),
    # the 8:1 ceiling across tile seams (2.3 x 4 tiles), and 4:1 (4.5 x 8)
    "B": ((2176, 384), (0, 0, 0, 0), [level(272, 48, F16, CHW), level(544, 96, U16, HWC)], (9, 0), (33, 4095), (2,)),
    # a window: region 144 x 56 at luma (6, 4) of 160 x 64; 1:1 (1.2 x 4.7 tiles), 2:1, 4:1 by 2:1
    "W": ((160, 64), (3, 5, 2, 2), [level(144, 56, U16, CHW), level(72, 28, F32, HWC), level(36, 28, F16, CHW)], (9, 0), (65, 65535), (0,)),
    "WN": ((160, 64), (3, 5, 2, 2), [level(144, 56, U8, HWC), level(72, 28, F16, CHW), level(36, 28, U16, HWC)], (5, 0), None, (5,)),
    # the remaining peak; a single tile column
    "S": ((136, 24), (0, 0, 0, 0), [level(136, 24, F16, HWC), level(68, 12, U16, CHW)], (6, 0), (33, 1023), (1, 4, 5)),
}
WINDOW_CASES = ("W", "WN")
assert len(CENSUS["A"][2]) == MAX_LEVELS and {(lv[2], lv[3]) for lv in _EIGHT} == set(_ALL)
assert all(sd.check(w, h, lv[0], lv[1], win)[0] and lv[0] % 4 == 0 and lv[1] % 4 == 0 for (w, h), win, levels, _m, _t, _l in CENSUS.values() for lv in levels)
assert any(lv[0] % 8 == 4 for lv in _EIGHT) and any(lv[0] < TILE_W and lv[1] < 2 * TILE_H for lv in _EIGHT)
assert all(any(lv[0] > 2 * TILE_W and lv[1] > 2 * TILE_H and sd.check(544, 96, lv[0], lv[1])[1] == r for lv in _EIGHT) for r in ((1, 1, 1, 1), (4, 3, 4, 3), (2, 1, 2, 1)))
assert sd.check(2176, 384, 272, 48)[1] == (8, 1, 8, 1)
assert {t for *_x, t, _l in CENSUS.values() if t} == {(17, 255), (33, 4095), (65, 65535), (33, 1023)}


@functools.lru_cache(maxsize=None)
def window_planes(case):
    """a window case's picture: 1023 everywhere outside the window over a ramp of at most 511 inside -> (planes, inner)"""
    (w, h), (l, r, a, b), _levels, _m, _t, _locs = CENSUS[case]
    inner = ramp_planes(w - 2 * (l + r), h - 2 * (a + b), 3, top=512)
    planes = [np.full((h, w), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16)]
    planes[0][2 * a:h - 2 * b, 2 * l:w - 2 * r] = inner[0]
    planes[1][a:h // 2 - b, l:w // 2 - r] = inner[1]
    planes[2][a:h // 2 - b, l:w // 2 - r] = inner[2]
    return planes, inner


@functools.lru_cache(maxsize=None)
def census_planes(case):
    """the seeded picture of a census case (read only: shared)"""
    (w, h), _win, _levels, _m, _t, _locs = CENSUS[case]
    planes = window_planes(case)[0] if case in WINDOW_CASES else ramp_planes(w, h, 900 + sorted(CENSUS).index(case))
    for p in planes:
        p.setflags(write=False)
    return tuple(planes)


@functools.lru_cache(maxsize=None)
def census_table(case):
    """(table, peak) of a census case, or (None, 0)"""
    if CENSUS[case][4] is None:
        return None, 0
    size, peak = CENSUS[case][4]
    t = st.random_table(size, peak, 60 + sorted(CENSUS).index(case))
    t.setflags(write=False)
    return t, peak


@functools.lru_cache(maxsize=None)
def census_want(case, loc):
    """pyramid() of a census case at chroma location loc, computed once and shared (read only)"""
    _size, win, levels, (matrix, full_range), _t, _locs = CENSUS[case]
    table, peak = census_table(case)
    want = pyramid(census_planes(case), levels, matrix, full_range, loc, table, peak, win)
    for a in want:
        a.setflags(write=False)
    return want


def _conditions():
    """what the census must exercise, on the restatement alone"""
    # a level of the region's own size is the RGB output of the region
    _size, _win, levels, (matrix, full_range), _t, _locs = CENSUS["A"]
    w, h, dtype, layout = levels[0]
    assert (w, h) == CENSUS["A"][0]
    assert census_want("A", 2)[0].tobytes() == np.ascontiguousarray(sr.convert(*census_planes("A"), matrix, full_range, 2, dtype, layout)).tobytes()
    # a window case is the pyramid of the inner picture alone: one sample read from outside would show
    for case in WINDOW_CASES:
        _size, _win, levels, (matrix, full_range), _t, locs = CENSUS[case]
        table, peak = census_table(case)
        inner = pyramid(window_planes(case)[1], levels, matrix, full_range, locs[0], table, peak)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(census_want(case, locs[0]), inner)), "nothing outside the window is read"
    # the two coefficient sets of one launch differ in more than scale: both clips are reached in the U8 and in the U16 level
    for a, top in ((census_want("A", 0)[2], 255), (census_want("A", 0)[4], 1023)):
        assert a.min() == 0 and a.max() == top


_conditions()
