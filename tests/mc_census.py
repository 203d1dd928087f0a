"""What the inter prediction slot fixtures (tests/golden/mc.ovg, mcx.ovg, mc_cells_*.ovg, mcx_cells_*.ovg) reach: every unit the recorder
cuts out of a fixture's PUs labelled with what the kernels decide from it, and the counting test_oracle_golden.py asserts.

Plain units (k_mc2, kernels_mc.hip; the window staging stage_unit_windows, mc_common.hip.h).  label_plain() restates, per unit:
  shape, lists, the luma (NOUT 1 / 2 / 4) and chroma (NOUT 1 / 2) finish bodies; per list the luma tap row (regular rows 0..15, the half-pel
  row 16, the table of 4x4 blocks) and the chroma phases of 32; the combine (uni L0 / L1, the weight pair of a bi-prediction, GPM, the
  fused CIIP weight with or without the luma-only bit); the planes; LMCS; per window (list x luma / chroma) the staging path (interior,
  clamped, slow) and its geometry against the picture (sides crossed, wholly outside, offset within the aligned group of 4).
The units always come from Recorder.pu(); units_of_pu() restates the recorder's cut (clip_mv, the identical-motion shortcut, the weights,
the flags) and is asserted against it on every PU (check_cut).  final_before_clip() restates the interpolation and the combine in numpy:
which cases clip at 0 and at 1023 comes from there, and it is asserted against the reference's samples on the combine family.

Refined units (k_mcx, kernels_mcx.hip): label_refined() restates what follows from the unit and the reference's recorded vectors alone --
shape, flags, where clip_mv (clip_mv_dev) moves an initial vector, whether the refined vector differs, whether it ends at a +-2^17 limit.
DMVR's outcome (label_dmvr) comes from the 25 costs the oracle's trace entry point returns (oracle_mcx_trace): the early exit, the arg-min
index and its tie kind, the sub-pel branch per axis, the final clip, BDOF switched off by the cost -- all restated here from the costs,
and the vector they predict is asserted against the reference's recorded exp_mv on every DMVR unit of every fixture (refined_fixture).
refined_reads() restates from the unit and the refined vector the whole-sample displacements (ldx, ldy, cdx, cdy) and which sides of the
replicated apron the unit reads in a way that shows: with the reference PICTURE's samples there, the average of the two 14-bit predictions
or a sample of BDOF's ring comes out another one -- a kernel reading the picture would compute another block.  label_bdof() takes BDOF's per-block
labels (zero gradient sums, weights at +-15, x_off) and the output clips from the same trace; the oracle that produces it equals the
reference's samples on every case."""
import functools

import numpy as np

import golden_cases
import spec_rpr
import spec_rpr_affine
from openvvc_amd import capi

SIZES = (4, 8, 16)
SHAPES = [(w, h) for w in SIZES for h in SIZES]
IN, LO, HI, OUT_LO, OUT_HI = range(5)                     # one axis of a window against the picture
SET_NAMES = {(LO, IN): "L", (HI, IN): "R", (IN, LO): "T", (IN, HI): "B", (LO, LO): "LT", (HI, LO): "RT", (LO, HI): "LB", (HI, HI): "RB"}
SIDE_SETS = ("L", "R", "T", "B", "LT", "RT", "LB", "RB", "out L", "out R", "out T", "out B")
BCW_PAIRS = ((10, -2), (5, 3), (4, 4), (3, 5), (-2, 10))   # (w0, w1) of bcw_idx_plus1 = 1..5; index 3 is the plain average
MV_LIMIT = 1 << 17


# ------------------------------------------------------------------------------------------------ the recorder's cut, restated
def clip_mv(pic_w, pic_h, px, py, pw, ph, mvx, mvy):
    """clip_mv (ovvc_record_inter.c; clip_mv_dev in kernels_mcx.hip): the window stays within reach of the picture"""
    return (min(max(mvx, -((pw + 3 + px) << 4)), (pic_w + 2 - px) << 4), min(max(mvy, -((ph + 3 + py) << 4)), (pic_h + 2 - py) << 4))


def units_of_pu(d, pic_w, pic_h):
    """ovhip_rec_pu for a plain PU (no refine, no GPM, no scaled reference) -> MC_UNIT_DTYPE array"""
    pw, ph = 1 << d.log2_w, 1 << d.log2_h
    dirn = d.inter_dir & 3
    if dirn == 3 and d.poc0 == d.poc1 and (d.mv0x, d.mv0y) == (d.mv1x, d.mv1y):
        dirn = 2                                           # identical motion: uni-prediction from list 1
    mv0 = clip_mv(pic_w, pic_h, d.x0, d.y0, pw, ph, d.mv0x, d.mv0y)
    mv1 = clip_mv(pic_w, pic_h, d.x0, d.y0, pw, ph, d.mv1x, d.mv1y)
    ref0, ref1 = d.ref0, d.ref1
    if not dirn & 1:
        mv0, ref0 = (0, 0), 0
    if not dirn & 2:
        mv1, ref1 = (0, 0), 0
    w0 = w1 = 4
    if dirn == 3 and d.bcw_idx_plus1 not in (0, 3):
        w0, w1 = BCW_PAIRS[d.bcw_idx_plus1 - 1]
    flags = ((capi.MC_HPEL_FILT if d.prec_amvr_half else 0) | (capi.MC_FILT_4x4 if (pw, ph) == (4, 4) else 0) |
             (0 if d.planes & 1 else capi.MC_NO_LUMA) | (0 if d.planes & 2 else capi.MC_NO_CHROMA) | (capi.MC_LMCS if d.lmcs else 0))
    aux = (d.ciip_wt & 7) | (0x100 if d.log2_w <= 2 else 0) if d.ciip_wt else 0
    uw, uh = min(pw, 16), min(ph, 16)
    out = np.zeros((pw // uw) * (ph // uh), capi.MC_UNIT_DTYPE)
    k = 0
    for uy in range(0, ph, uh):
        for ux in range(0, pw, uw):
            out[k] = (d.x0 + ux, d.y0 + uy, uw, uh, dirn, flags, ref0, ref1, w0, w1, mv0[0], mv0[1], mv1[0], mv1[1], aux)
            k += 1
    return out


def recorded(descs, pic_w, pic_h, check_cut=True):
    """the units Recorder.pu() cuts out of every PU -> [(case, plain units, refined units)]; the restated cut is asserted against the
    recorder's for the plain PUs"""
    rec = capi.Recorder(pic_w, pic_h)
    out = []
    for i, d in enumerate(descs):
        rec.reset()
        rec.pu(d)
        mc, mcx = rec.mc_units().copy(), rec.mcx_units().copy()
        if check_cut and not d.refine:
            assert units_of_pu(d, pic_w, pic_h).tobytes() == mc.tobytes(), f"case {i}: the census restates another cut than the recorder's"
        out.append((i, mc, mcx))
    return out


# ------------------------------------------------------------------------------------------------ plain units
def axis_class(s0, length, pic):
    return OUT_LO if s0 + length <= 0 else OUT_HI if s0 >= pic else LO if s0 < 0 else HI if s0 + length > pic else IN


def side_set(xc, yc):
    """the side set of a window that is not inside the picture; wholly outside along x names the unit before its rows do"""
    if xc in (OUT_LO, OUT_HI):
        return "out L" if xc == OUT_LO else "out R"
    if yc in (OUT_LO, OUT_HI):
        return "out T" if yc == OUT_LO else "out B"
    return SET_NAMES[(xc, yc)]


def windows(u, pic_w, pic_h, stride_y=None, stride_c=None):
    """the reference windows stage_unit_windows loads for unit u -> [(list, chroma?, path, side set or None, offset)]"""
    stride_y, stride_c = pic_w if stride_y is None else stride_y, pic_w >> 1 if stride_c is None else stride_c
    aligned = not ((stride_y | stride_c | pic_w | (pic_w >> 1)) & 3)
    do = ((u["flags"] & capi.MC_NO_LUMA) == 0, (u["flags"] & capi.MC_NO_CHROMA) == 0)
    out = []
    for l in (0, 1):
        if not (int(u["dir"]) >> l) & 1:
            continue
        mvx, mvy = int(u["mv1x" if l else "mv0x"]), int(u["mv1y" if l else "mv0y"])
        for c in (0, 1):
            if not do[c]:
                continue
            if c:
                sx, sy, ww, wh, rw, rh = (int(u["x"]) >> 1) + (mvx >> 5) - 1, (int(u["y"]) >> 1) + (mvy >> 5) - 1, (int(u["w"]) >> 1) + 3, (int(u["h"]) >> 1) + 3, pic_w >> 1, pic_h >> 1
            else:
                sx, sy, ww, wh, rw, rh = int(u["x"]) + (mvx >> 4) - 3, int(u["y"]) + (mvy >> 4) - 3, int(u["w"]) + 7, int(u["h"]) + 7, pic_w, pic_h
            xc, yc = axis_class(sx, ww, rw), axis_class(sy, wh, rh)
            out.append([l, c, None, None if (xc, yc) == (IN, IN) else side_set(xc, yc), sx & 3])
    inside = all(w[3] is None for w in out)
    for w in out:
        w[2] = "slow" if not aligned else "interior" if inside else "clamped"       # the path is chosen once per unit
    return [tuple(w) for w in out]


def combine_of(u):
    if u["flags"] & capi.MC_GPM:
        return ("gpm",)
    base = ("uni", 0) if u["dir"] == 1 else ("uni", 1) if u["dir"] == 2 else ("bi", int(u["w0"]), int(u["w1"]))
    return ("ciip", int(u["aux"]) & 7, bool(int(u["aux"]) & 0x100)) + base if u["aux"] else base


def label_plain(u, pic_w, pic_h, stride_y=None, stride_c=None):
    """one plain unit -> dict"""
    w, h, fl = int(u["w"]), int(u["h"]), int(u["flags"])
    table = "4x4" if fl & capi.MC_FILT_4x4 else "regular"
    hpel = table == "regular" and bool(fl & capi.MC_HPEL_FILT)
    lists = {}
    for l in (0, 1):
        if (int(u["dir"]) >> l) & 1:
            mvx, mvy = int(u["mv1x" if l else "mv0x"]), int(u["mv1y" if l else "mv0y"])
            row = lambda f: 16 if hpel and f == 8 else f
            lists[l] = dict(fx=row(mvx & 15), fy=row(mvy & 15), cfx=mvx & 31, cfy=mvy & 31)
    return dict(shape=(w, h), lists={1: "L0", 2: "L1", 3: "BI"}[int(u["dir"])], table=table, phases=lists,
                nout_l=4 if w * h >= 256 else 2 if w * h >= 128 else 1, nout_c=2 if (w >> 1) * (h >> 1) >= 64 else 1,
                combine=combine_of(u), planes="no luma" if fl & capi.MC_NO_LUMA else "no chroma" if fl & capi.MC_NO_CHROMA else "both",
                lmcs=bool(fl & capi.MC_LMCS), windows=windows(u, pic_w, pic_h, stride_y, stride_c))


# ---- cells that exist
def phase_cells_that_exist():
    """H and V passes, luma and chroma, keyed by how k_mc2 deals its lanes: (axis, plane, shape, lists, list, phase); the luma phase is
    the tap row.  Struck: the half-pel row 16 on a 4x4 PU -- its units carry OVHIP_MC_FILT_4x4, and the table of 4x4 blocks has no such
    row (rcn_mcp_b_l(2, 2): put_vvc_qpel of 4x4 blocks, the AMVR precision is not looked at; k_mc2: hpel = !FILT_4x4 && HPEL_FILT)."""
    out = set()
    for s in SHAPES:
        for lists, ls in (("L0", (0,)), ("L1", (1,)), ("BI", (0, 1))):
            for l in ls:
                for axis in "HV":
                    out |= {(axis, "luma", s, lists, l, f) for f in range(16 if s == (4, 4) else 17)}
                    out |= {(axis, "chroma", s, lists, l, f) for f in range(32)}
    return out


def combine_cells_that_exist():
    """(shape, combine).  Struck: GPM on a unit with a side of 4 (rcn_gpm_b runs for coding units of log2 sides > 2 only,
    vcl_coding_unit.c gpm_enabled; the recorder refuses the others); a CIIP weight on 4x4, 4x8 and 8x4 (ciip_enabled needs
    log2_cb_w + log2_cb_h >= 6); the luma-only bit is set exactly for the units 4 wide (rcn_ciip_b leaves the chroma of such a coding
    unit to the inter prediction)."""
    out = set()
    for s in SHAPES:
        out |= {(s, ("uni", 0)), (s, ("uni", 1))} | {(s, ("bi",) + p) for p in BCW_PAIRS}
        if min(s) >= 8:
            out.add((s, ("gpm",)))
        if s[0] * s[1] >= 64:
            out |= {(s, ("ciip", wt, s[0] == 4)) for wt in (1, 2, 3)}
    return out


def plane_cells_that_exist():
    return {(s, lists, p) for s in SHAPES for lists in ("L0", "L1", "BI") for p in ("both", "no luma", "no chroma")}


@functools.lru_cache(maxsize=None)
def _axis_reach(pic, chroma):
    """{unit length: {(class, offset)}} of one axis: every PU length 4..128 at every multiple of 4 inside the picture and its CTU, every
    vector clip_mv lets through, every unit of the PU -- what the recorder can emit, by enumeration"""
    out = {n: set() for n in SIZES}
    for l2 in range(2, 8):
        pu = 1 << l2
        unit = min(pu, 16)
        for pos in range(0, pic - pu + 1, 4):
            if pos >> 7 != (pos + pu - 1) >> 7:
                continue
            v = np.arange(-((pu + 3 + pos) << 4), ((pic + 2 - pos) << 4) + 1, 16)
            for u in range(0, pu, unit):
                s0 = ((pos + u) >> 1) + (v >> 5) - 1 if chroma else pos + u + (v >> 4) - 3
                length, lim = ((unit >> 1) + 3, pic >> 1) if chroma else (unit + 7, pic)
                cls = np.where(s0 + length <= 0, OUT_LO, np.where(s0 >= lim, OUT_HI, np.where(s0 < 0, LO, np.where(s0 + length > lim, HI, IN))))
                out[unit] |= set(zip(cls.tolist(), (s0 & 3).tolist()))
    return out


def border_cells_that_exist(pic_w, pic_h):
    """(plane, shape, side set, offset) of the windows that are not inside the picture.  Nothing is struck by hand: a cell exists if some
    PU, position and vector that clip_mv lets through produces it (_axis_reach).  What that leaves out: clip_mv keeps a PU's window
    within 3 samples of the picture, so a luma window wholly outside is that of a unit further out in a larger PU (sides of 16 only),
    and the chroma windows of narrow units are wholly outside at the one offset the clip limit gives."""
    out = set()
    for c, plane in ((0, "luma"), (1, "chroma")):
        rx, ry = _axis_reach(pic_w, c), _axis_reach(pic_h, c)
        for w, h in SHAPES:
            for xc, off in rx[w]:
                for yc in {k for k, _ in ry[h]}:
                    if (xc, yc) != (IN, IN):
                        out.add((plane, (w, h), side_set(xc, yc), off))
    return out


def reach_plain(labels):
    """-> dict of cell sets over the labelled plain units"""
    out = dict(phase=set(), combine=set(), planes=set(), border=set(), path=set(), nout=set(), lmcs=set(), corners={})
    for lb in labels:
        s = lb["shape"]
        for l, p in lb["phases"].items():
            if lb["planes"] != "no luma":
                out["phase"] |= {("H", "luma", s, lb["lists"], l, p["fx"]), ("V", "luma", s, lb["lists"], l, p["fy"])}
            if lb["planes"] != "no chroma":
                out["phase"] |= {("H", "chroma", s, lb["lists"], l, p["cfx"]), ("V", "chroma", s, lb["lists"], l, p["cfy"])}
        out["combine"].add((s, lb["combine"][:3] if lb["combine"][0] == "ciip" else lb["combine"]))
        out["planes"].add((s, lb["lists"], lb["planes"]))
        out["nout"].add((lb["nout_l"], lb["nout_c"], lb["lists"]))
        out["lmcs"].add(lb["lmcs"])
        for l, c, path, sides, off in lb["windows"]:
            out["path"].add(path)
            if sides is not None:
                out["border"].add(("chroma" if c else "luma", s, sides, off))
    return out


# ---- the interpolation and the combine in numpy (the reference's put_vvc_{qpel,epel}_* and put_vvc_{uni,bi}(_w)_*, as k_mc2 runs them)
def _predict14(plane, x, y, w, h, fh, fv):
    t = len(fh)
    o = t // 2 - 1
    xs = np.clip(np.arange(x - o, x - o + w + t - 1), 0, plane.shape[1] - 1)
    ys = np.clip(np.arange(y - o, y - o + h + t - 1), 0, plane.shape[0] - 1)
    win = plane[np.ix_(ys, xs)].astype(np.int64)
    hp = sum(int(fh[k]) * win[:, k:k + w] for k in range(t)) >> 2
    return sum(int(fv[k]) * hp[k:k + h, :] for k in range(t)) >> 6


def final_before_clip(u, refs):
    """-> [Y, Cb, Cr] (None for a plane the unit does not write): the combined prediction before ov_clip_bd (for a CIIP unit: before the
    clip of the inter prediction, the blend of two clipped values cannot leave the range)"""
    lb = label_plain(u, refs[0].w, refs[0].h)
    out = []
    for p in range(3):
        c = p != 0
        if lb["planes"] == ("no chroma" if c else "no luma"):
            out.append(None)
            continue
        w, h, x, y = int(u["w"]) >> c, int(u["h"]) >> c, int(u["x"]) >> c, int(u["y"]) >> c
        pred = {}
        for l, ph in lb["phases"].items():
            mvx, mvy = int(u["mv1x" if l else "mv0x"]), int(u["mv1y" if l else "mv0y"])
            plane = refs[int(u["ref1" if l else "ref0"])].planes()[p]
            if c:
                pred[l] = _predict14(plane, x + (mvx >> 5), y + (mvy >> 5), w, h, spec_rpr.MC_CHROMA[ph["cfx"]], spec_rpr.MC_CHROMA[ph["cfy"]])
            else:
                tab = spec_rpr_affine.MC_LUMA4 if lb["table"] == "4x4" else spec_rpr.MC_LUMA
                pred[l] = _predict14(plane, x + (mvx >> 4), y + (mvy >> 4), w, h, tab[ph["fx"]], tab[ph["fy"]])
        cmb = lb["combine"][3:] if lb["combine"][0] == "ciip" else lb["combine"]
        if cmb[0] == "gpm":
            aux = int(u["aux"])
            sx = lambda v, bits: v - (1 << bits) if v >> (bits - 1) else v
            k, a, b = sx(aux & 0xffff, 16), sx((aux >> 16) & 0xff, 8), sx(aux >> 24, 8)
            yy, xx = np.mgrid[0:h, 0:w] << c
            wgt = np.clip((k + a * xx + b * yy) >> 3, 0, 8)
            out.append((pred[1] * (8 - wgt) + pred[0] * wgt + 64) >> 7)
        elif cmb[0] == "uni":
            out.append((pred[cmb[1]] + 8) >> 4)
        elif cmb[1:] == (4, 4):
            out.append((pred[0] + pred[1] + 16) >> 5)
        else:
            out.append((pred[1] * cmb[2] + pred[0] * cmb[1] + 64) >> 7)
    return out


def final_samples(u, refs, intra=None):
    """the unit's samples [Y, Cb, Cr] from final_before_clip: clip, then the fused CIIP blend (no LMCS)"""
    out = []
    for p, v in enumerate(final_before_clip(u, refs)):
        if v is None:
            out.append(None)
            continue
        v = np.clip(v, 0, 1023)
        aux, c = int(u["aux"]), p != 0
        if aux and not u["flags"] & capi.MC_GPM and not (c and aux & 0x100):
            x, y = int(u["x"]) >> c, int(u["y"]) >> c
            ip = intra.planes()[p][y:y + v.shape[0], x:x + v.shape[1]].astype(np.int64)
            v = np.clip((ip * (aux & 7) + v * (4 - (aux & 7)) + 2) >> 2, 0, 1023)
        out.append(v.astype(np.uint16))
    return out


# ------------------------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def plain_fixture(name):
    """-> (refs, intra, descs, exp_off, exp, [(case, unit, label)]) of mc.ovg or one of the mc_cells files"""
    if name == "mc.ovg":
        refs, descs, exp_off, exp = golden_cases.mc_cases()
        intra = None
    else:
        refs, intra, descs, exp_off, exp = golden_cases.mc_cell_cases(name)
    units = [(i, u, label_plain(u, refs[0].w, refs[0].h)) for i, mc, _ in recorded(descs, refs[0].w, refs[0].h) for u in mc]
    return refs, intra, descs, exp_off, exp, units


def expected_picture(descs, exp_off, exp, w, h, cases=None, fill=0xABAB):
    """the picture the reference leaves when the cases run into one filled with `fill`: the PUs' rectangles, everything else untouched"""
    from oracle_lib import HostPic
    pic = HostPic(w, h)
    pic.y[:] = fill; pic.cb[:] = fill; pic.cr[:] = fill
    for i in range(len(descs)) if cases is None else cases:
        d = descs[i]
        pw, ph = 1 << d.log2_w, 1 << d.log2_h
        for p, plane in enumerate(pic.planes()):
            c = p != 0
            if d.planes & (2 if c else 1):
                o = int(exp_off[i, p])
                plane[d.y0 >> c:(d.y0 + ph) >> c, d.x0 >> c:(d.x0 + pw) >> c] = exp[o:o + (pw >> c) * (ph >> c)].reshape(ph >> c, pw >> c)
    return pic


def sheets(descs):
    """the cases dealt greedily to sheets: the PUs of a sheet do not overlap, so that one picture (one launch) takes them all"""
    out = []
    for i, d in enumerate(descs):
        r = (d.x0, d.y0, d.x0 + (1 << d.log2_w), d.y0 + (1 << d.log2_h))
        for sh in out:
            if all(r[2] <= q[0] or q[2] <= r[0] or r[3] <= q[1] or q[3] <= r[1] for _, q in sh):
                sh.append((i, r))
                break
        else:
            out.append([(i, r)])
    return [[i for i, _ in sh] for sh in out]


# ------------------------------------------------------------------------------------------------ refined units
def label_refined(u, pic_w, pic_h, exp_mv):
    """one refined unit and the reference's refined vector for it -> dict.  clip: the (list, side) at which clip_mv moves the initial
    vector before DMVR anchors its windows (never for a BDOF-only unit: the recorder has clipped those already)"""
    w, h, fl = int(u["w"]), int(u["h"]), int(u["flags"])
    ini = [(int(u["mv0x"]), int(u["mv0y"])), (int(u["mv1x"]), int(u["mv1y"]))]
    clip = set()
    if fl & capi.MC_DMVR:
        for l, (mx, my) in enumerate(ini):
            cx, cy = clip_mv(pic_w, pic_h, int(u["x"]), int(u["y"]), w, h, mx, my)
            clip |= {(l, s) for s, on in (("L", cx > mx), ("R", cx < mx), ("T", cy > my), ("B", cy < my)) if on}
    got = [int(v) for v in exp_mv]
    flat = [v for mv in ini for v in mv]
    return dict(shape=(w, h), bdof=bool(fl & capi.MC_BDOF), dmvr=bool(fl & capi.MC_DMVR), hpel=bool(fl & capi.MC_HPEL_FILT), clip=clip,
                moved=got != flat, at_limit={(k, v > 0) for k, v in enumerate(got) if v in (-MV_LIMIT, MV_LIMIT - 1)},
                ini_at_limit={(k, v > 0) for k, v in enumerate(flat) if v in (-MV_LIMIT, MV_LIMIT - 1)},
                symmetric=got[0] - flat[0] == flat[2] - got[2] and got[1] - flat[1] == flat[3] - got[3])


def _div_for_maxq7(num, den):
    sign, q = num < 0, 0
    num, den = abs(num), den << 3
    for _ in range(2):
        if num >= den:
            num -= den
            q += 1
        q <<= 1
        den >>= 1
    if num >= den:            # the last bit: no subtraction, the remainder is not needed
        q += 1
    return -q if sign else q


def _subpel(lo, s0, hi):
    """refine_mv along one axis from the costs beside the minimum -> (branch, sixteenths)"""
    den = lo + hi - 2 * s0
    if den == 0:
        return "den 0", 0
    if lo == s0:
        return "-8", -8
    if hi == s0:
        return "+8", 8
    q = _div_for_maxq7((lo - hi) << 4, den)
    return ("q<0" if q < 0 else "q>0" if q > 0 else "q=0"), q


DMVR_BRANCHES = ("ring", "den 0", "-8", "+8", "q<0", "q=0", "q>0")


def label_dmvr(u, trace):
    """the outcome of DMVR for unit u from the oracle's trace -> dict, with the refined vector the labels predict.  Restated: the early
    exit (three quarters of the centre SAD below w * h), the arg-min (lowest cost, the centre wins a tie, then the lowest index), the
    ring skip and the parametric sub-pel step, the +-2^17 clip, BDOF switched off below a cost of 2 * w * h."""
    w, h = int(u["w"]), int(u["h"])
    ini = [int(u["mv0x"]), int(u["mv0y"]), int(u["mv1x"]), int(u["mv1y"])]
    sad_c = int(trace[6])
    cost = sad_c - (sad_c >> 2)
    out = dict(searched=cost >= w * h, idx=12, tie="none", x=None, y=None, q7=set(), clip_binds=set())
    dh = dv = 0
    if out["searched"]:
        sad = [int(v) for v in trace[7:32]]
        assert sad[12] == cost
        cost = min(sad)
        at_min = [k for k in range(25) if sad[k] == cost]
        idx = 12 if 12 in at_min else at_min[0]
        out.update(idx=idx, tie="none" if len(at_min) == 1 else "centre" if idx == 12 else "index")
        dh, dv = (idx % 5 - 2) << 4, (idx // 5 - 2) << 4
        if abs(dh) == 32 or abs(dv) == 32:
            out["x"] = out["y"] = "ring"
        else:
            out["x"], ax = _subpel(sad[idx - 1], sad[idx], sad[idx + 1])
            out["y"], ay = _subpel(sad[idx - 5], sad[idx], sad[idx + 5])
            out["q7"] = {a for a, v in (("x", ax), ("y", ay)) if abs(v) == 7}
            dh, dv = dh + ax, dv + ay
        assert (int(trace[0]), int(trace[1]), int(trace[2]), int(trace[3])) == (1, idx, dh, dv), "the census restates another search than the oracle's"
        free = [ini[0] + dh, ini[1] + dv, ini[2] - dh, ini[3] - dv]
        out["clip_binds"] = {(k, v > 0) for k, v in enumerate(free) if not -MV_LIMIT <= v < MV_LIMIT}
        out["predicted"] = [min(max(v, -MV_LIMIT), MV_LIMIT - 1) for v in free]
    else:
        assert int(trace[0]) == 0
        out["predicted"] = ini
    out["dh"], out["dv"] = dh, dv
    out["bdof_off"] = bool(u["flags"] & capi.MC_BDOF) and cost < 2 * w * h
    assert int(trace[4]) == cost and int(trace[5]) == out["bdof_off"]
    return out


REFINED_SHAPES = ((8, 16), (16, 8), (16, 16))


def _window14(win, fh, fv, n):
    """the 14-bit prediction of an n = (w, h) block from its (h + taps - 1) x (w + taps - 1) window of samples"""
    t = len(fh)
    hp = sum(int(fh[k]) * win[:, k:k + n[0]] for k in range(t)) >> 2
    return sum(int(fv[k]) * hp[k:k + n[1], :] for k in range(t)) >> 6


def refined_reads(u, got, bdof_ran, refs, pic_w, pic_h):
    """What steps 3 and 4 of k_mcx read for unit u once its vectors are refined to `got` -> dict:
      disp   per list (ldx, ldy, cdx, cdy): the whole-sample displacement of the luma and of the chroma block against the windows,
             which stay anchored at clip_mv(initial vector) -- taken from the UNCLIPPED initial vector, as rcn_dmvr_mv_refine does;
      apron  {(plane "luma" / "chroma", side "L" / "R" / "T" / "B")}: the side of the 2-sample apron pad_sides / pad_rows replicate that
             the unit reads in a way that shows -- with the reference PICTURE's samples in place of the replicated ones on that side of
             one list's window, the average of the two 14-bit predictions (restated here) comes out another sample somewhere, or a
             whole sample of BDOF's ring is another one.  A difference that the interpolation's or the average's rounding swallows does
             not count: a kernel reading the picture there would compute the same block.
    A unit without DMVR has no displacement and no apron."""
    out = dict(disp={}, apron=set())
    if not u["flags"] & capi.MC_DMVR:
        return out
    w, h, x, y = int(u["w"]), int(u["h"]), int(u["x"]), int(u["y"])
    hpel = bool(u["flags"] & capi.MC_HPEL_FILT)
    todo = {}                                                          # (plane name, picture plane index) -> per list what to filter
    for l in (0, 1):
        ix, iy = int(u["mv1x" if l else "mv0x"]), int(u["mv1y" if l else "mv0y"])
        gx, gy = int(got[2 * l]), int(got[2 * l + 1])
        cx, cy = clip_mv(pic_w, pic_h, x, y, w, h, ix, iy)
        out["disp"][l] = ((gx >> 4) - (ix >> 4), (gy >> 4) - (iy >> 4), (gx >> 5) - (ix >> 5), (gy >> 5) - (iy >> 5))
        ref = refs[int(u["ref1" if l else "ref0"])]
        for plane, pls, ax, ay, d, n, lo, taps, fr in (
                ("luma", (ref.y,), x + (cx >> 4), y + (cy >> 4), out["disp"][l][:2], (w, h), -3, 8, (gx & 15, gy & 15)),
                ("chroma", (ref.cb, ref.cr), (x >> 1) + (cx >> 5), (y >> 1) + (cy >> 5), out["disp"][l][2:], (w >> 1, h >> 1), -1, 4, (gx & 31, gy & 31))):
            tabs, phases = (spec_rpr.MC_LUMA, [16 if hpel and f == 8 else f for f in fr]) if plane == "luma" else (spec_rpr.MC_CHROMA, list(fr))
            o = taps // 2 - 1
            cols, rows = np.arange(d[0] - o, d[0] + n[0] + taps - 1 - o), np.arange(d[1] - o, d[1] + n[1] + taps - 1 - o)
            hi = (n[0] - lo, n[1] - lo)                                # window offsets lo .. n + |lo| along each axis
            wc_, wr_ = np.clip(cols, lo, hi[0]), np.clip(rows, lo, hi[1])
            shape = (len(rows), len(cols))
            sides = (("L", np.broadcast_to(cols < lo, shape)), ("R", np.broadcast_to(cols > hi[0], shape)),
                     ("T", np.broadcast_to((rows < lo)[:, None], shape)), ("B", np.broadcast_to((rows > hi[1])[:, None], shape)))
            # BDOF's ring (extend_bdof_buff): the whole samples one around the block, one further on the side the phase leans to
            ring = np.zeros(shape, bool)
            if plane == "luma" and bdof_ran:
                ex, ey = int(phases[0] >= 8), int(phases[1] >= 8)
                ring[o - 1 + ey:o + n[1] + 1 + ey, o - 1 + ex:o + n[0] + 1 + ex] = True
                ring[o + ey:o + n[1] + ey, o + ex:o + n[0] + ex] = False
            for k, p in enumerate(pls):
                H, W = p.shape
                true = p[np.ix_(np.clip(ay + rows, 0, H - 1), np.clip(ax + cols, 0, W - 1))].astype(np.int64)
                rep = p[np.ix_(np.clip(ay + wr_, 0, H - 1), np.clip(ax + wc_, 0, W - 1))].astype(np.int64)
                todo.setdefault((plane, k), {})[l] = (true, rep, sides, ring, tabs[phases[0]], tabs[phases[1]], n)
    for (plane, _), lists in todo.items():
        base = {l: _window14(v[1], v[4], v[5], v[6]) for l, v in lists.items()}
        avg = lambda p0, p1: np.clip((p0 + p1 + 16) >> 5, 0, 1023)
        for l, (true, rep, sides, ring, fh, fv, n) in lists.items():
            for side, mask in sides:
                mixed = _window14(np.where(mask, true, rep), fh, fv, n)
                pair = (mixed, base[1]) if l == 0 else (base[0], mixed)
                if (avg(*pair) != avg(base[0], base[1])).any() or (ring & mask & (true != rep)).any():
                    out["apron"].add((plane, side))
    return out


def label_bdof(u, trace):
    """BDOF's labels for one unit from the oracle's trace -> None if BDOF did not run (not asked for, or switched off by DMVR's cost),
    else the set of what some 4x4 block of the unit shows (s_ax == 0, s_ay == 0, wx / wy at -15 / +15, x_off != 0) and what the unit's
    output shows (a sample clipped at 0, at 1023)"""
    if not int(trace[32]):
        return None
    nb = (int(u["w"]) >> 2) * (int(u["h"]) >> 2)
    b = np.asarray(trace[33:33 + 5 * nb]).reshape(nb, 5)
    out = set()
    for name, on in (("s_ax == 0", b[:, 0] != 0), ("s_ay == 0", b[:, 1] != 0), ("wx == -15", b[:, 2] == -15), ("wx == 15", b[:, 2] == 15),
                     ("wy == -15", b[:, 3] == -15), ("wy == 15", b[:, 3] == 15), ("x_off != 0", b[:, 4] != 0),
                     ("x_off == 0 with wx != 0", (b[:, 4] == 0) & (b[:, 2] != 0) & (b[:, 1] == 0))):
        if on.any():
            out.add(name)
    assert not ((b[:, 0] != 0) & (b[:, 2] != 0)).any() and not ((b[:, 1] != 0) & (b[:, 3] != 0)).any(), "a weight without its gradient sum"
    out |= ({"clip at 0"} if trace[33 + 80] else set()) | ({"clip at 1023"} if trace[33 + 81] else set())
    return out


BDOF_CELLS = {"s_ax == 0", "s_ay == 0", "wx == -15", "wx == 15", "wy == -15", "wy == 15", "x_off != 0", "x_off == 0 with wx != 0", "clip at 0", "clip at 1023"}


def refined_cells_that_exist():
    """flags (shape, BDOF / DMVR / both, half-pel), disp_l (ldx, ldy) and disp_c (cdx, cdy) of list 0 (list 1 mirrors it unless the
    final clip stops one of them), apron (plane, side), bdof (shape, label).  Nothing struck.  The displacements are those of the 25
    search points: a sub-pel step that carries into the next whole sample stays within them on the fixtures (reach_refined's disp_all
    is asserted to)."""
    return dict(flags={(s, k, hp) for s in REFINED_SHAPES for k in ("bdof", "dmvr", "both") for hp in (False, True)},
                disp_l={(a, b) for a in range(-2, 3) for b in range(-2, 3)},
                disp_c={(a, b) for a in range(-1, 2) for b in range(-1, 2)},
                apron={(p, sd) for p in ("luma", "chroma") for sd in "LRTB"}, bdof={(s, c) for s in REFINED_SHAPES for c in BDOF_CELLS})


def reach_refined(labels):
    out = dict(flags=set(), disp_l=set(), disp_c=set(), apron=set(), bdof=set(), disp_all=set())
    for lb in labels:
        out["flags"].add((lb["shape"], "both" if lb["bdof"] and lb["dmvr"] else "bdof" if lb["bdof"] else "dmvr", lb["hpel"]))
        if lb["reads"]["disp"]:
            d = lb["reads"]["disp"][0]
            out["disp_l"].add(d[:2]); out["disp_c"].add(d[2:]); out["disp_all"] |= {lb["reads"]["disp"][0][:2], lb["reads"]["disp"][1][:2]}
        out["apron"] |= lb["reads"]["apron"]
        if lb["bdof_labels"] is not None:
            out["bdof"] |= {(lb["shape"], c) for c in lb["bdof_labels"]}
    return out


def dmvr_cells_that_exist():
    """the sets reach_dmvr() fills.  Struck: BDOF kept after an early exit -- the exit takes a cost below w * h, and BDOF is switched off
    below 2 * w * h (rcn_dmvr_mv_refine: disable_bdof = min_cost < 2 * pu_w * pu_h)."""
    return dict(exit={(s, e) for s in REFINED_SHAPES for e in (False, True)}, idx=set(range(25)), tie={"none", "centre", "index"},
                branch={(a, b) for a in "xy" for b in DMVR_BRANCHES}, q7={(a, pos) for a in "xy" for pos in (False, True)},
                clip={(k, hi) for k in range(4) for hi in (False, True)},
                bdof_off={(s, searched, off) for s in REFINED_SHAPES for searched in (False, True) for off in (False, True)} - {(s, False, False) for s in REFINED_SHAPES})


def reach_dmvr(labels):
    """-> dict of sets over label_refined dicts that carry a DMVR outcome: exit (shape, early exit?), idx, tie, branch (axis, sub-pel
    branch), q7 (axis, +7 rather than -7), clip (component of the refined vector, upper limit?), bdof_off (shape, searched?, off?)"""
    out = dict(exit=set(), idx=set(), tie=set(), branch=set(), q7=set(), clip=set(), bdof_off=set())
    for lb in labels:
        o = lb.get("outcome")
        if o is None:
            continue
        out["exit"].add((lb["shape"], not o["searched"]))
        if o["searched"]:
            out["idx"].add(o["idx"])
            out["tie"].add(o["tie"])
            out["branch"] |= {("x", o["x"]), ("y", o["y"])}
            out["q7"] |= {(a, (o["dh"] if a == "x" else o["dv"]) % 16 == 7) for a in o["q7"]}
            out["clip"] |= o["clip_binds"]
        if lb["bdof"]:
            out["bdof_off"].add((lb["shape"], o["searched"], o["bdof_off"]))
    return out


@functools.lru_cache(maxsize=None)
def refined_fixture(name):
    """-> (refs, descs, exp_off, exp, exp_mv, [(case, unit, label)]) of mcx.ovg or one of the mcx_cells files (DMVR and BDOF units)"""
    refs, descs, exp_off, exp, exp_mv = golden_cases.mcx_cases(name)
    import oracle_lib
    units = []
    scratch = oracle_lib.HostPic(refs[0].w, refs[0].h)
    for i, _, mcx in recorded(descs, refs[0].w, refs[0].h):
        o = int(exp_off[i, 3]) // 4
        for k, u in enumerate(mcx):
            lb = label_refined(u, refs[0].w, refs[0].h, exp_mv[o + k])
            trace, _ = oracle_lib.dmvr_trace(scratch, refs, u)
            lb["bdof_labels"] = label_bdof(u, trace)
            lb["reads"] = refined_reads(u, exp_mv[o + k], lb["bdof_labels"] is not None, refs, refs[0].w, refs[0].h)
            if lb["dmvr"]:
                lb["outcome"] = label_dmvr(u, trace)
                assert lb["outcome"]["predicted"] == exp_mv[o + k].tolist(), f"{name} case {i} unit {k}: the census predicts {lb['outcome']['predicted']}, the reference refined to {exp_mv[o + k].tolist()}"
            units.append((i, u, lb))
    return refs, descs, exp_off, exp, exp_mv, units
