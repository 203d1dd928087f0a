"""The reference's intra slot cases (tests/golden/intra.ovg and intra_cells_*.ovg) laid out for the GPU tests: every case on its own
band of a tall picture, NB cases per launch.  Shared by test_gpu_intra.py, test_gpu_ctu_sizes.py and test_gpu_intra_flow.py."""
import functools

import numpy as np

import golden_io
from openvvc_amd import capi

BAND = 384            # a multiple of 128: a band's first row is a CTU row at every CTU size
NB = 160              # cases per launch (ovhip_itask.y is 16 bits)
FIXTURES = ("intra.ovg", "cells")


def cell_files():
    """the files gen_intra_cells wrote, in the order it wrote them"""
    return sorted(p.name for p in golden_io.GOLDEN.glob("intra_cells_*.ovg"))


@functools.lru_cache(maxsize=None)
def load(fixture):
    """fixture: "intra.ovg", or "cells" = all intra_cells_*.ovg in one list (they predict on intra.ovg's picture and hold none).
    -> (tasks, exp_off [n, 2], exp, (pic_y, pic_cb, pic_cr)); read-only, shared between the tests"""
    g = golden_io.load("intra.ovg")
    pic = (g["pic_y"], g["pic_cb"], g["pic_cr"])
    if fixture != "cells":
        assert fixture == "intra.ovg"
        parts = [g]
    else:
        parts = [golden_io.load(n) for n in cell_files()]
        assert parts, "no intra_cells_*.ovg under tests/golden"
    tasks, offs, exps, base = [], [], [], 0
    for p in parts:
        tasks.append(np.frombuffer(p["task"].tobytes(), dtype=capi.ITASK_DTYPE))
        offs.append(p["exp_off"].astype(np.int64) + base)
        exps.append(p["exp"])
        base += len(p["exp"])
    out = (np.concatenate(tasks), np.concatenate(offs), np.concatenate(exps), pic)
    for a in out[:3] + pic:
        a.setflags(write=False)
    return out


def band_planes(pic, S=0):
    """one band: the fixture's picture S luma rows below the band's first row"""
    H, W = pic[0].shape
    base = [np.zeros((BAND, W), np.uint16), np.zeros((BAND // 2, W // 2), np.uint16), np.zeros((BAND // 2, W // 2), np.uint16)]
    base[0][S:S + H] = pic[0]; base[1][S // 2:(S + H) // 2] = pic[1]; base[2][S // 2:(S + H) // 2] = pic[2]
    return base


@functools.lru_cache(maxsize=None)
def tall_planes(S=0):
    """NB bands of band_planes(intra.ovg's picture, S): the start picture of a launch; read-only, shared between the tests"""
    out = tuple(np.tile(p, (NB, 1)) for p in band_planes(load("intra.ovg")[3], S))
    for a in out:
        a.setflags(write=False)
    return out


def small_ctu(S, fixture="intra.ovg"):
    """The fixture placed S luma rows lower in each band.  The reference's prediction slots depend on the CTU size only through CCLM's
    ctu_first_line = !y0 (y0 relative to the fixture's 128-CTU at luma row 128): a block is on the first line of a CTU of size S iff its
    row relative to that CTU is a multiple of S.  LM / MDLM cases for which the two differ are left out; those at y0 = 0 stay, and are
    on a first line (row 128 + S) ONLY for a CTU of size S -- a kernel that ignores log2_ctu takes the two-row path there.
    -> (tasks with y moved, exp_off, exp, base planes of one band, number left out, number of LM cases on such a first line)"""
    tasks, exp_off, exp, pic = load(fixture)
    tasks = tasks.copy()
    lm = (tasks["kind"] == capi.IT_CHROMA) & (tasks["mode"] >= 67)
    y0 = 2 * tasks["y"].astype(np.int64) - 128                      # luma row relative to the fixture's CTU
    keep = ~(lm & ((y0 == 0) != (y0 % S == 0)))
    n_first = int((lm & (y0 == 0))[keep].sum())
    tasks["y"] += np.where(tasks["kind"] == capi.IT_LUMA, S, S // 2).astype(np.uint16)
    return tasks[keep], exp_off[keep], exp, band_planes(pic, S), int((~keep).sum()), n_first


def in_bands(t):
    t = t.copy()
    k = np.arange(len(t))
    t["y"] += np.where(t["kind"] == capi.IT_LUMA, k * BAND, k * (BAND // 2)).astype(np.uint16)
    return t


def case_ok(tt, planes, eo, exp):
    w, h, x, yy = 1 << int(tt["log2_w"]), 1 << int(tt["log2_h"]), int(tt["x"]), int(tt["y"])
    if tt["kind"] == capi.IT_LUMA:
        return np.array_equal(planes[0][yy:yy + h, x:x + w], exp[eo[0]:eo[0] + w * h].reshape(h, w))
    return (np.array_equal(planes[1][yy:yy + h, x:x + w], exp[eo[0]:eo[0] + w * h].reshape(h, w))
            and np.array_equal(planes[2][yy:yy + h, x:x + w], exp[eo[1]:eo[1] + w * h].reshape(h, w)))


def describe(i, tt):
    return (i, int(tt["kind"]), int(tt["mode"]), 1 << int(tt["log2_w"]), 1 << int(tt["log2_h"]), int(tt["x"]), int(tt["y"]) % BAND,
            int(tt["flags"]), int(tt["avl_lft"]), int(tt["avl_abv"]), int(tt["mrl_idx"]))


def restore_blocks(planes, start, t):
    """the blocks of the tasks t (already in their bands) of `planes` set back to what `start` holds there (planes modified in place)"""
    for tt in t:
        w, h, x, yy = 1 << int(tt["log2_w"]), 1 << int(tt["log2_h"]), int(tt["x"]), int(tt["y"])
        for k in ((0,) if tt["kind"] == capi.IT_LUMA else (1, 2)):
            planes[k][yy:yy + h, x:x + w] = start[k][yy:yy + h, x:x + w]
