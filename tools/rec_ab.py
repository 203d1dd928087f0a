#!/usr/bin/env python
"""Differential check of the host recorder between two builds of the library (CPU only, no GPU needed).

The tests pin the recorder to the reference where fixtures exist; this tool pins it to another build of itself everywhere
else.  One run drives a fixed list of workloads through the recorder of ONE library -- the one OVVC_HIP_LIB_NAME names under
openvvc_amd/ (default libovvc_hip.so) -- and prints one JSON object per workload: the number of calls, a digest of every
call's return code, a digest of ovhip_rec_refusal() after every call (and the distinct texts after the refused ones), the
SHA-256 of every recorder array the workload fills, and of the call log the recorder wrote.  Two builds agree when their
outputs are equal:

    python tools/rec_ab.py --ab libovvc_hip_parent.so      # both builds, each in a child process of its own, then the diff
    OVVC_HIP_LIB_NAME=libovvc_hip_parent.so python tools/rec_ab.py > parent.jsonl ; python tools/rec_ab.py > new.jsonl

Loading a library through OVVC_HIP_LIB_NAME skips the ABI check of capi.load(); that is acceptable here only because both
builds are the same ABI version (the tool refuses a library whose ovhip_abi_version() is not capi.OVHIP_ABI_VERSION).

Workloads:
  calllog_4k   the call log of the synthetic 3840x2160 B picture with every tool (what tools/micro/rec_throughput.c replays),
               replayed with ovhip_calllog_replay
  rpr_ovg      the PUs of tests/golden/rpr/rpr.ovg with the scale table the RPR tests set, as stored and with far vectors,
               under both collocation settings, without and with ovhip_rec_set_rpr_tools
  rpr_affine_ovg  the same for the affine CUs of rpr_affine.ovg
  sweep/<k>    seeded random ovhip_pu_desc / ovhip_affine_desc (SWEEP_N of each per scale table and opt-in mask) on recorders
               with 0, 1 and 2 scaled slots, malformed and refused calls included
"""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

SWEEP_N = 700            # per (scale table, opt-in mask): 8 x 4 x 700 = 22 400 PUs and as many affine CUs
UNSCALED = 1 << 14


class Run:
    """One recorder and what was observed of the calls made on it."""

    def __init__(self, capi, lib, w, h, log=True):
        self.capi, self.lib = capi, lib
        self.rec = lib.ovhip_rec_create(w, h)
        assert self.rec
        self.log = lib.ovhip_calllog_create() if log else None
        if self.log:
            lib.ovhip_rec_set_calllog(self.rec, self.log)
        self.codes, self.refusals, self.refused = [], hashlib.sha256(), set()

    def seen(self, rc):
        self.codes.append(int(rc))
        text = self.lib.ovhip_rec_refusal(self.rec) or b""
        self.refusals.update(text + b"\0")
        if rc == self.capi.OVHIP_EUNSUP:
            self.refused.add(text.decode())
        return rc

    def scale(self, slot, s):
        self.seen(self.capi.set_ref_scale(self.lib, self.rec, slot, s["scale_hor"], s["scale_ver"], s["ref_w"], s["ref_h"],
                                          s["col_hor"], s["col_ver"]))

    def arrays(self, more=False):
        capi, lib = self.capi, self.lib
        kinds = [("mc", lib.ovhip_rec_mc_units, C.sizeof(capi.McUnit)), ("mcx", lib.ovhip_rec_mcx_units, C.sizeof(capi.McUnit)),
                 ("aff", lib.ovhip_rec_aff_units, capi.AFF_UNIT_DTYPE.itemsize), ("aff_rpr", lib.ovhip_rec_aff_rpr_units, C.sizeof(capi.AffRprUnit)),
                 ("rpr", lib.ovhip_rec_rpr_units, C.sizeof(capi.RprUnit)), ("aff_side", lib.ovhip_rec_aff_side, 4)]
        if more:
            kinds += [("tb", lib.ovhip_rec_tb_cmds, C.sizeof(capi.TbCmd)), ("coef", lib.ovhip_rec_coefs, 2),
                      ("regions", lib.ovhip_rec_lmcs_regions, capi.LMCS_REGION_DTYPE.itemsize),
                      ("ciip", lib.ovhip_rec_ciip_units, capi.CIIP_UNIT_DTYPE.itemsize), ("itasks", lib.ovhip_rec_itasks, capi.ITASK_DTYPE.itemsize)]
        out = {}
        for name, fn, elem in kinds:
            n = C.c_size_t(0)
            p = fn(self.rec, C.byref(n))
            out[name] = (C.string_at(p, n.value * elem) if n.value else b"", n.value)
        if more:
            for d, name in ((0, "edge_v"), (1, "edge_h")):
                n, offs = C.c_size_t(0), capi.DbfOffsets()
                p = lib.ovhip_rec_dbf_edges(self.rec, d, C.byref(n), C.byref(offs))
                out[name] = ((C.string_at(p, n.value * capi.DBF_EDGE_DTYPE.itemsize) if n.value else b"") + bytes(offs), n.value)
        return out

    def log_bytes(self):
        if not self.log:
            return b""
        n = C.c_size_t(0)
        p = self.lib.ovhip_calllog_data(self.log, C.byref(n))
        return C.string_at(p, n.value) if n.value else b""

    def close(self):
        if self.log:
            self.lib.ovhip_rec_set_calllog(self.rec, None)
            self.lib.ovhip_calllog_destroy(self.log)
        self.lib.ovhip_rec_destroy(self.rec)


class Digest:
    """What one workload prints: the observations of all its recorders, in order."""

    def __init__(self, name):
        self.name, self.calls, self.codes, self.refusals, self.refused = name, 0, hashlib.sha256(), hashlib.sha256(), set()
        self.hist, self.arr, self.count, self.log = {}, {}, {}, hashlib.sha256()

    def take(self, run, more=False):
        self.calls += len(run.codes)
        self.codes.update(b"".join(int(c).to_bytes(4, "little", signed=True) for c in run.codes))
        for c in run.codes:
            k = str(c) if c < 0 else "ok"
            self.hist[k] = self.hist.get(k, 0) + 1
        self.refusals.update(run.refusals.digest())
        self.refused |= run.refused
        for name, (data, n) in run.arrays(more).items():
            self.arr.setdefault(name, hashlib.sha256()).update(len(data).to_bytes(8, "little") + data)
            self.count[name] = self.count.get(name, 0) + n
        self.log.update(run.log_bytes())
        run.close()

    def emit(self):
        print(json.dumps(dict(workload=self.name, calls=self.calls, return_codes=self.codes.hexdigest(), return_code_counts=self.hist,
                              refusal_after_each_call=self.refusals.hexdigest(), refusal_texts=sorted(self.refused),
                              elements=self.count, arrays={k: v.hexdigest() for k, v in self.arr.items()},
                              calllog=self.log.hexdigest()), sort_keys=True), flush=True)


# ---------------------------------------------------------------- workloads
def wl_calllog_4k(capi, lib):
    from openvvc_amd import synth
    log = synth.make_workload(3840, 2160, 0x266, tools=synth.INTRA_TOOLS, intra_frac=0.12, calllog=True).calllog
    d = Digest("calllog_4k")
    run = Run(capi, lib, 3840, 2160, log=False)
    n = lib.ovhip_calllog_replay(log.ctypes.data, log.nbytes, run.rec)
    run.seen(min(n, 0))
    d.log.update(log.tobytes())            # the log this build's recorder wrote while the picture was generated
    d.take(run, more=True)
    d.calls = int(n)
    d.emit()


FAR = (37 << 11, -(29 << 11))              # added to the stored vectors: far outside the picture, 1/16 sample


def _fixture_runs(capi, lib, d, pic, sizes, cases, scales, feed):
    for tools in (0, capi.RPR_TOOL_AFFINE | capi.RPR_TOOL_PU4x4):
        for col in ((0, 0), (1, 1), (0, 1)):
            for far in (0, 1):
                run = Run(capi, lib, *pic)
                run.seen(lib.ovhip_rec_set_rpr_tools(run.rec, tools))
                for slot, s in scales(pic[0], pic[1], sizes, col).items():
                    run.scale(slot, s)
                for c in cases:
                    feed(run, c, far)
                d.take(run)


def wl_rpr_ovg(capi, lib):
    import rpr_golden
    from rpr_cases import pu_desc
    pic_w, pic_h, sizes, _, cases = rpr_golden.load()
    d = Digest("rpr_ovg")

    def feed(run, c, far):
        pu = dict(c["pu"])
        if far:
            pu.update(mv0x=pu["mv0x"] + FAR[0], mv0y=pu["mv0y"] + FAR[1], mv1x=pu["mv1x"] - FAR[0], mv1y=pu["mv1y"] + FAR[1])
        desc = pu_desc(capi, pu)                   # (as the tests feed it: luma and chroma)
        run.seen(lib.ovhip_rec_pu(run.rec, C.byref(desc)))
        if c["pu"]["planes"] != desc.planes:       # ... and with the planes the generator stored
            desc.planes = c["pu"]["planes"]
            run.seen(lib.ovhip_rec_pu(run.rec, C.byref(desc)))

    _fixture_runs(capi, lib, d, (pic_w, pic_h), sizes, cases, rpr_golden.scales, feed)
    d.emit()


def wl_rpr_affine_ovg(capi, lib):
    import numpy as np
    import rpr_golden
    import rpr_affine_golden
    pic_w, pic_h, sizes, _, cases, _ = rpr_affine_golden.load()
    d = Digest("rpr_affine_ovg")

    def feed(run, c, far):
        cu, keep = dict(c["cu"]), []
        if far:
            cu["mv0"] = cu["mv0"] + np.array(FAR, dtype=np.int32)
            cu["mv1"] = cu["mv1"] - np.array(FAR, dtype=np.int32)
        desc = rpr_affine_golden.affine_desc(capi, cu, keep)
        run.seen(lib.ovhip_rec_affine_cu(run.rec, C.byref(desc)))
        run.seen(lib.ovhip_rec_cu_inter(run.rec, None, C.byref(desc)))

    _fixture_runs(capi, lib, d, (pic_w, pic_h), sizes, cases, rpr_golden.scales, feed)
    d.emit()


def _scale(pic, num, den, col=(0, 0), size=True, ver=None):
    """A slot whose reference is num / den of the picture (ver: another ratio vertically); size=False: no size given."""
    vn, vd = ver or (num, den)
    rw, rh = pic[0] * num // den, pic[1] * vn // vd
    return dict(scale_hor=((rw << 14) + pic[0] // 2) // pic[0], scale_ver=((rh << 14) + pic[1] // 2) // pic[1],
                ref_w=rw if size else 0, ref_h=rh if size else 0, col_hor=col[0], col_ver=col[1])


def _other_size(pic):
    return dict(scale_hor=UNSCALED, scale_ver=UNSCALED, ref_w=pic[0] - 64, ref_h=pic[1], col_hor=0, col_ver=0)


def sweep_tables():
    a, b = (1920, 1080), (3840, 2160)
    return [("none", a, {}), ("2to1", b, {0: _scale(b, 2, 1)}), ("3to2", a, {0: _scale(a, 3, 2, (1, 0))}), ("1to1_other_size", a, {0: _other_size(a)}),
            ("2to1_3to2", a, {0: _scale(a, 2, 1, (0, 1)), 1: _scale(a, 3, 2)}), ("3to2_1to1_other_size", b, {0: _scale(b, 3, 2), 1: _other_size(b)}),
            ("2to1_no_size_and_half", a, {0: _scale(a, 2, 1, (1, 1), size=False), 1: _scale(a, 1, 2)}),
            ("anisotropic_and_eighth", a, {0: _scale(a, 2, 1, ver=(1, 1)), 1: _scale(a, 1, 8, (1, 1))})]


def _pos(rnd, pic_len, block):
    """Interior, at and near both borders, and beyond the far one (multiples of 4, never negative: the fields are uint16)."""
    k = rnd.randrange(6)
    if k == 0:
        return rnd.choice((0, 4, 8))
    if k == 1:
        return max(0, pic_len - block + rnd.choice((-8, -4, 0)))
    if k == 2:
        return max(0, pic_len + rnd.choice((-4, 0, 4, 8, 64, 256)))
    return rnd.randrange(0, pic_len - block + 1, 4) if pic_len > block else 0


def _mv(rnd, cap):
    span = rnd.choice((1 << 6, 1 << 10, 1 << 15, 1 << 17, 1 << 20, cap))
    return rnd.randrange(-span, span + 1)


def random_pu(capi, rnd, pic):
    d = capi.PuDesc()
    d.log2_w, d.log2_h = rnd.choice((2, 2, 3, 3, 4, 4, 5, 6, 7)), rnd.choice((2, 2, 3, 3, 4, 4, 5, 6, 7))
    if rnd.random() < 0.15:
        d.log2_h = d.log2_w
    d.x0, d.y0 = _pos(rnd, pic[0], 1 << d.log2_w), _pos(rnd, pic[1], 1 << d.log2_h)
    d.inter_dir = rnd.choice((1, 1, 2, 2, 2, 3, 3, 3, 3, 3, 7)) if rnd.random() > 0.03 else 0
    d.bcw_idx_plus1 = rnd.choice((0, 0, 0, 0, 1, 2, 3, 4, 5)) if rnd.random() > 0.03 else 6
    d.prec_amvr_half, d.lmcs = int(rnd.random() < 0.2), int(rnd.random() < 0.3)
    d.planes = rnd.choice((3, 3, 3, 1, 1, 2, 0))
    d.refine = rnd.choice((0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 4, 5))
    d.ciip_wt = rnd.choice((0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4))
    d.gpm_split_dir = rnd.randrange(64) if rnd.random() > 0.04 else rnd.choice((64, 200))
    d.mv0x, d.mv0y, d.mv1x, d.mv1y = (_mv(rnd, 1 << 30) for _ in range(4))
    d.ref0, d.ref1 = rnd.randrange(4), rnd.randrange(4)
    d.ref_idx0, d.ref_idx1 = d.ref0, d.ref1
    d.poc0, d.poc1 = 10 + d.ref0, 20 + d.ref1
    k = rnd.random()
    if k < 0.12:                                   # identical motion
        d.mv1x, d.mv1y, d.poc1 = d.mv0x, d.mv0y, d.poc0
    elif k < 0.16:                                 # same picture, other vector; same vector, other picture
        d.poc1 = d.poc0
    elif k < 0.20:
        d.mv1x, d.mv1y = d.mv0x, d.mv0y
    return d


def random_affine(capi, rnd, pic, keep):
    d = capi.AffineDesc()
    d.log2_w, d.log2_h = rnd.choice((3, 3, 4, 4, 4, 5, 5, 6, 7)), rnd.choice((3, 3, 4, 4, 4, 5, 5, 6, 7))
    if rnd.random() < 0.03:
        d.log2_w = 2                                            # no affine CU below 8x8: malformed
    w, h = 1 << d.log2_w, 1 << d.log2_h
    d.x0, d.y0 = _pos(rnd, pic[0], w), _pos(rnd, pic[1], h)
    d.inter_dir = rnd.choice((1, 1, 2, 2, 2, 3, 3, 3, 3, 3, 7)) if rnd.random() > 0.03 else 0
    d.bcw_idx_plus1 = rnd.choice((0, 0, 0, 0, 1, 2, 3, 4, 5)) if rnd.random() > 0.03 else 6
    d.prof_dir = rnd.choice((0, 0, 0, 1, 2, 3, 3, 4, 7))
    d.lmcs = int(rnd.random() < 0.3)
    d.ref0, d.ref1 = rnd.randrange(4), rnd.randrange(4)
    d.poc0, d.poc1 = 10 + d.ref0, 20 + d.ref1
    nsx, nsy = max(w >> 2, 1), max(h >> 2, 1)
    stride = nsx + rnd.choice((0, 0, 0, 0, 0, 2, 2, 30, 30, -1))            # the reference's 34-wide context; too narrow: malformed
    rows = max(stride, 1)
    fields = []
    for _ in range(2):                                          # both lists always hold something, used or not
        bx, by = _mv(rnd, 1 << 28), _mv(rnd, 1 << 28)
        ax, ay, cx, cy = (rnd.randrange(-24, 25) for _ in range(4))
        m = (C.c_int32 * (2 * rows * nsy))()
        for j in range(nsy):
            for i in range(rows):
                m[2 * (j * rows + i)] = bx + ((ax * i + cx * j) >> 1)
                m[2 * (j * rows + i) + 1] = by + ((ay * i + cy * j) >> 1)
        fields.append(m)
    k = rnd.random()
    if k < 0.12:                                   # identical motion (every sub-block, luma and chroma)
        fields[1], d.poc1 = fields[0], d.poc0
    elif k < 0.16:
        d.poc1 = d.poc0
    elif k < 0.20:
        fields[1] = fields[0]
    keep[:] = fields
    d.mv_stride = stride
    d.mv0, d.mv1 = C.cast(fields[0], C.c_void_p), C.cast(fields[1], C.c_void_p)
    for t in range(4):
        for i in range(16):
            d.dmv_scale[t][i] = rnd.randrange(-(1 << 15), 1 << 15)
    return d


def wl_sweep(capi, lib):
    for k, (name, pic, table) in enumerate(sweep_tables()):
        d = Digest(f"sweep/{name}")
        for tools in range(4):
            rnd = random.Random(0x5eed00 + 16 * k + tools)
            run = Run(capi, lib, *pic)
            run.seen(lib.ovhip_rec_set_rpr_tools(run.rec, tools))
            for slot, s in table.items():
                run.scale(slot, s)
            keep = []
            for _ in range(SWEEP_N):
                run.seen(lib.ovhip_rec_pu(run.rec, C.byref(random_pu(capi, rnd, pic))))
                run.seen(lib.ovhip_rec_affine_cu(run.rec, C.byref(random_affine(capi, rnd, pic, keep))))
            d.take(run)
        d.emit()


def child():
    from openvvc_amd import capi
    lib = capi.load()
    if lib.ovhip_abi_version() != capi.OVHIP_ABI_VERSION:
        sys.exit(f"{capi.LIB_PATH}: ABI {lib.ovhip_abi_version()}, this tool compares builds of ABI {capi.OVHIP_ABI_VERSION}")
    # (the 4K picture first: the log's padding bytes are whatever the heap held, and a fresh process has a clean one)
    for wl in (wl_calllog_4k, wl_rpr_ovg, wl_rpr_affine_ovg, wl_sweep):
        wl(capi, lib)


def ab(other):
    outs = []
    for name in ("libovvc_hip.so", other):
        env = dict(os.environ, OVVC_HIP_LIB_NAME=name)
        outs.append(subprocess.run([sys.executable, __file__], env=env, check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    bad = 0
    for a, b in zip(*outs):
        a, b = json.loads(a), json.loads(b)
        keys = [k for k in a if a[k] != b.get(k)] + [f"arrays.{k}" for k in a["arrays"] if a["arrays"][k] != b["arrays"].get(k)]
        print(f"{a['workload']:40s} {a['calls']:8d} calls  {a['return_code_counts']}  " + ("identical" if not keys else "DIFFERS in " + ", ".join(keys)))
        bad += bool(keys)
    if bad or len(outs[0]) != len(outs[1]):
        sys.exit("libovvc_hip.so and %s record differently" % other)
    print("libovvc_hip.so and %s record the same bytes, return codes and refusals in all %d workloads" % (other, len(outs[0])))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--ab":
        ab(sys.argv[2])
    elif len(sys.argv) == 1:
        child()
    else:
        sys.exit(__doc__)
