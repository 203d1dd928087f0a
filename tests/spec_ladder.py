"""Numpy restatement of "Output ladder on the device" (include/ovvc_hip.h): rung r of a ladder is, by definition, the surface of the
reduced picture -- spec_surface.surface(spec_reduce.reduce_picture(...)) -- so there is nothing here but that composition, and the
census of ladders the tests run.  Integer only: what it gives is compared for equality with ovhip_ladder_host and k_output_ladder."""
import functools

import spec_reduce as sd
import spec_surface as ss

MAX_RUNGS = 8
NV12, P010, I420, I010, ROUND, DITHER = ss.NV12, ss.P010, ss.I420, ss.I010, ss.ROUND, ss.DITHER


def rung(w, h, fmt=NV12, rounding=ROUND, loose=False):
    """one rung's description: size, format, rounding and the layout's keywords (tight, or spec_surface.loose_layout)"""
    return (w, h, fmt, rounding, ss.loose_layout(fmt, w, h) if loose else {})


def loosened(rungs):
    return [rung(w, h, fmt, rounding, True) for (w, h, fmt, rounding, _lay) in rungs]


def ladder(planes, rungs, window=(0, 0, 0, 0), loc=0, guard=0):
    """[(the bytes of rung r's surface in a buffer of its size + guard that held spec_surface.FILL before, its size)]"""
    out = []
    for (w, h, fmt, rounding, lay) in rungs:
        red = sd.reduce_picture(*planes, w, h, window, loc)
        _buf, size = ss.surface(red, fmt, rounding, **lay)
        out.append((ss.surface(red, fmt, rounding, total=size + guard, **lay)[0], size))
    return out


# (source, window, rungs, chroma locations to run): every size the smallest that reaches its case
CENSUS = [
    # the identity rung; equal sizes with two formats; 26/7 by 7/1; chroma 26 wide, narrower than a tile
    ((104, 56), (0, 0, 0, 0), [rung(104, 56, I010), rung(52, 28, NV12), rung(52, 28, NV12, DITHER), rung(28, 8, I420)], range(6)),
    # 3/2 by 5/3; a copy along x only; loose pitches and offset_c
    ((72, 40), (0, 0, 0, 0), [rung(48, 24, P010, loose=True), rung(36, 20, I420, DITHER, True), rung(24, 8, NV12, loose=True), rung(72, 20, I010, loose=True)], range(6)),
    # more than two column tiles; 6, 2 and 1 chroma rows; 50/7
    ((200, 20), (0, 0, 0, 0), [rung(200, 20, I420), rung(136, 12, NV12), rung(100, 12, P010), rung(28, 4, NV12, DITHER)], (0,)),
    # the 8:1 ceiling; a 4x4 chroma plane interleaved into 8-byte rows
    ((64, 64), (0, 0, 0, 0), [rung(32, 32, NV12, DITHER), rung(16, 16, NV12, DITHER), rung(8, 8, NV12, DITHER), rung(64, 8, NV12, DITHER)], (0,)),
    # the int32 ceiling beside a cheap rung
    ((1024, 1024), (0, 0, 0, 0), [rung(132, 132, NV12), rung(512, 512, P010)], (0,)),
    # the region's rows only 4- and 2-byte aligned
    ((80, 48), (1, 3, 2, 2), [rung(72, 40, NV12), rung(48, 24, I010), rung(36, 20, P010)], (0,)),
    # a single rung
    ((72, 40), (0, 0, 0, 0), [rung(36, 20, NV12)], (0,)),
    # OVHIP_LADDER_MAX_RUNGS rungs, all four formats
    ((72, 40), (0, 0, 0, 0), [rung(72, 40, I010), rung(48, 24, NV12), rung(36, 20, P010), rung(24, 8, I420, DITHER), rung(72, 20, NV12, DITHER), rung(36, 40, I420),
                              rung(48, 24, P010, loose=True), rung(36, 20, I010, loose=True)], (0,)),
]
WINDOW_CASE = 5
assert len(CENSUS[-1][2]) == MAX_RUNGS
assert all(sd.check(w, h, g[0], g[1], win)[0] for (w, h), win, rungs, _locs in CENSUS for g in rungs)


def window_planes(case=WINDOW_CASE, seed=3):
    """the window case's picture: 1023 everywhere outside the window over random content of at most 511 inside -> (planes, inner)"""
    import numpy as np
    (w, h), (l, r, a, b), _rungs, _locs = CENSUS[case]
    inner = sd.random_planes(w - 2 * (l + r), h - 2 * (a + b), seed, top=512)
    planes = [np.full((h, w), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16)]
    planes[0][2 * a:h - 2 * b, 2 * l:w - 2 * r] = inner[0]
    planes[1][a:h // 2 - b, l:w // 2 - r] = inner[1]
    planes[2][a:h // 2 - b, l:w // 2 - r] = inner[2]
    return planes, inner


def census_planes(case):
    """the seeded picture of a census case (the window case: window_planes)"""
    (w, h), _win, _rungs, _locs = CENSUS[case]
    return window_planes(case)[0] if case == WINDOW_CASE else list(sd.random_planes(w, h, 300 + case))


@functools.lru_cache(maxsize=None)
def census_want(case, loc, guard, loose=False):
    """ladder() of a census case's picture, computed once and shared (read only): with `loose` every rung in the loose layout"""
    _size, win, rungs, _locs = CENSUS[case]
    return ladder(census_planes(case), loosened(rungs) if loose else rungs, win, loc, guard)
