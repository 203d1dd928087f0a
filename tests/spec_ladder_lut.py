"""Numpy restatement of "Output ladder through a colour table" (include/ovvc_hip.h): rung r of such a ladder is, by definition, the
surface through the table of the reduced picture -- spec_surface_lut.surface(spec_reduce.reduce_picture(...)) -- so there is nothing
here but that composition, the census of ladders the tests run, and the conditions the census must meet, asserted on import on the
restatement alone.  Integer only: what it gives is compared for equality with ovhip_ladder_lut_host and k_ladder_lut.

The sizes go by k_ladder_lut's tile of 120 x 12 luma samples: cases A and B hold at least two tiles and a partial one on each axis at
their seam-crossing rungs."""
import functools

import numpy as np

import spec_ladder as sl
import spec_reduce as sd
import spec_rgb_lut as st
import spec_surface as ss
import spec_surface_lut as sx

MAX_RUNGS = sl.MAX_RUNGS
NV12, P010, I420, I010, ROUND, DITHER = sl.NV12, sl.P010, sl.I420, sl.I010, sl.ROUND, sl.DITHER
rung, loosened = sl.rung, sl.loosened
MATRICES = (9, 0, 1, 0)                                      # BT.2020 limited to BT.709 limited


def conv_of(src_loc, dst_loc):
    sm, sf, dm, df = MATRICES
    return (sm, sf, src_loc, dm, df, dst_loc)


def ramp_planes(w, h, seed, top=1024):
    """a seeded smooth ramp plus noise: luma rises along x, Cb along y, Cr along the diagonal, each over the whole of 0 .. top - 1, with
    noise of +- top / 16 on it.  (Plain noise averages to grey under a reduction and visits few cells of a table.)"""
    rng = np.random.default_rng(seed)

    def plane(hh, ww, fx, fy):
        x, y = np.meshgrid(np.arange(ww, dtype=np.float64) / max(ww - 1, 1), np.arange(hh, dtype=np.float64) / max(hh - 1, 1))
        v = (fx * x + fy * y) * (top - 1) + rng.integers(-(top // 16), top // 16 + 1, (hh, ww))
        return np.clip(np.rint(v), 0, top - 1).astype(np.uint16)

    return plane(h, w, 1.0, 0.0), plane(h // 2, w // 2, 0.0, 1.0), plane(h // 2, w // 2, 0.5, 0.5)


def ladder(planes, rungs, conv, table, peak, window=(0, 0, 0, 0), guard=0, reduced=None):
    """[(the bytes of rung r's surface in a buffer of its size + guard that held spec_surface.FILL before, its size)]; reduced: the
    rungs' reduced pictures where the caller holds them already"""
    out = []
    for k, (w, h, fmt, rounding, lay) in enumerate(rungs):
        red = reduced[k] if reduced is not None else sd.reduce_picture(*planes, w, h, window, conv[2])
        conv_pic = sx.converted(red, conv, table, peak)
        _buf, size = ss.surface(conv_pic, fmt, rounding, **lay)
        out.append((ss.surface(conv_pic, fmt, rounding, total=size + guard, **lay)[0], size))
    return out


def _ladder_case(k):
    (w, h), win, rungs, _locs = sl.CENSUS[k]
    return (w, h), win, rungs


# name -> (source, window, rungs, (table size, peak), [(source location, destination location)])
CENSUS = {
    # more than two column tiles and row tiles at 1:1, 4/3 and 2:1, so the halo crosses tile seams on both axes; a rung narrower than a
    # tile and lower than two (68/9 by 6)
    "A": ((544, 96), (0, 0, 0, 0),
          [rung(544, 96, I010), rung(272, 48, NV12), rung(408, 72, P010), rung(136, 24, I420, DITHER), rung(72, 16, NV12, DITHER)],
          (17, 1023), [(s, d) for s in (0, 2) for d in range(4)] + [(s, 0) for s in (1, 3, 4, 5)]),
    # the 8:1 ceiling across tile seams
    "B": ((2176, 384), (0, 0, 0, 0), [rung(272, 48, NV12), rung(544, 96, P010)], (33, 4095), [(0, 0), (0, 3)]),
    # spec_ladder's cases: loose pitches and offset_c; the 8:1 ceiling with a 4x4 interleaved chroma plane; the window; eight rungs
    "C1": _ladder_case(1) + ((65, 255), [(0, 1)]),
    "C3": _ladder_case(3) + ((65, 255), [(0, 3)]),
    "C5": _ladder_case(5) + ((65, 255), [(0, 1)]),
    "C7": _ladder_case(7) + ((65, 255), [(0, 3)]),
    # the int32 ceiling
    "D": _ladder_case(4) + ((17, 1023), [(0, 2)]),
}
WINDOW_CASE = "C5"
QUICK = [k for k in CENSUS if k != "D"]
assert len(CENSUS["C7"][2]) == MAX_RUNGS
assert all(sd.check(w, h, g[0], g[1], win)[0] and g[0] % 4 == 0 and g[1] % 4 == 0 for (w, h), win, rungs, _t, _c in CENSUS.values() for g in rungs)


@functools.lru_cache(maxsize=None)
def window_planes(case=WINDOW_CASE):
    """the window case's picture: 1023 everywhere outside the window over a ramp of at most 511 inside -> (planes, inner)"""
    (w, h), (l, r, a, b), _rungs, _t, _c = CENSUS[case]
    inner = ramp_planes(w - 2 * (l + r), h - 2 * (a + b), 3, top=512)
    planes = [np.full((h, w), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16)]
    planes[0][2 * a:h - 2 * b, 2 * l:w - 2 * r] = inner[0]
    planes[1][a:h // 2 - b, l:w // 2 - r] = inner[1]
    planes[2][a:h // 2 - b, l:w // 2 - r] = inner[2]
    return planes, inner


@functools.lru_cache(maxsize=None)
def census_planes(case):
    """the seeded picture of a census case (read only: shared)"""
    (w, h), _win, _rungs, _t, _c = CENSUS[case]
    planes = window_planes(case)[0] if case == WINDOW_CASE else ramp_planes(w, h, 700 + sorted(CENSUS).index(case))
    for p in planes:
        p.setflags(write=False)
    return tuple(planes)


@functools.lru_cache(maxsize=None)
def census_table(case):
    size, peak = CENSUS[case][3]
    t = st.random_table(size, peak, 40 + sorted(CENSUS).index(case))
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def census_reduced(case, src_loc):
    """the rungs' reduced pictures of a census case, computed once per source location and shared (read only)"""
    _size, win, rungs, _t, _c = CENSUS[case]
    return [sd.reduce_picture(*census_planes(case), w, h, win, src_loc) for (w, h, _f, _r, _l) in rungs]


@functools.lru_cache(maxsize=None)
def census_want(case, combo, guard, loose=False):
    """ladder() of a census case under its combo-th pair of locations, computed once and shared (read only)"""
    _size, win, rungs, (_s, peak), combos = CENSUS[case]
    conv = conv_of(*combos[combo])
    return ladder(census_planes(case), loosened(rungs) if loose else rungs, conv, census_table(case), peak, win, guard, census_reduced(case, conv[2]))


def tetrahedra(rgb, size):
    """the set of the six orders of the fractions that the pixels of rgb (3, N) fall into"""
    _i, f = st.cells(rgb, size)
    ch = st.order(f)
    return set(np.unique(ch[0] * 3 + ch[1]).tolist())


def _conditions():
    """what the census must exercise, on the restatement alone"""
    for case, (_size, win, rungs, (size, peak), combos) in CENSUS.items():
        planes, table, conv = census_planes(case), census_table(case), conv_of(*combos[0])
        reds = census_reduced(case, conv[2])
        rgb = np.concatenate([st.rgb10(*red, conv[0], conv[1], conv[2]).reshape(3, -1) for red in reds], axis=1)
        assert len(tetrahedra(rgb, size)) == 6, (case, "the reduced pictures' R'G'B' reaches all six tetrahedra")
        if case in ("A", "B"):
            assert rgb.min() == 0 and rgb.max() == 1023, (case, "both clips are reached")
    # the 1:1 rung is surface_lut of the source
    _size, win, rungs, (size, peak), combos = CENSUS["A"]
    for combo in (0, len(combos) - 1):
        w, h, fmt, rounding, lay = rungs[0]
        assert (w, h) == CENSUS["A"][0]
        want = sx.surface(census_planes("A"), conv_of(*combos[combo]), census_table("A"), peak, fmt, rounding, **lay)[0]
        assert census_want("A", combo, 0)[0][0].tobytes() == want.tobytes(), "a rung of the region's own size is surface_lut of the region"
    # the window case is the ladder of the inner picture alone
    _size, win, rungs, (size, peak), combos = CENSUS[WINDOW_CASE]
    inner = ladder(window_planes()[1], rungs, conv_of(*combos[0]), census_table(WINDOW_CASE), peak)
    assert all(a.tobytes() == b.tobytes() for (a, _n), (b, _m) in zip(census_want(WINDOW_CASE, 0, 0), inner)), "nothing outside the window is read"


_conditions()
