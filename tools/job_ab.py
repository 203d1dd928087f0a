#!/usr/bin/env python
"""Differential check of the picture job (ovhip_job_flush / ovhip_job_band) between two builds of the library, on the GPU.

The tests pin the job to the oracle; this tool pins it to another build of itself, launch counts included.  One run drives a fixed
list of pictures through the job of ONE library -- the one OVVC_HIP_LIB_NAME names under openvvc_amd/ (default libovvc_hip.so) --
and prints one line per (picture, way of submitting it): the MD5 of the three planes, of the refined vectors and of the TMVP cells,
and every field of ovhip_job_stats except the four host_us_* (wall time).  A submission the library refuses ends the run.
Two builds agree when their outputs are equal text:

    python tools/job_ab.py --ab libovvc_hip_parent.so      # both builds, each in a child process of its own, then the diff

(the other build: the library of another checkout, copied to openvvc_amd/ under that name.  As in tools/rec_ab.py, loading through
OVVC_HIP_LIB_NAME skips capi.load()'s ABI check; the tool refuses another ABI version.  For the worker counts of the flow launches,
which are not in the stats, run each library once under `rocprofv3 --kernel-trace -- python tools/job_ab.py` and compare the grid
sizes of the k_intra_flow dispatches.)

Pictures (seeded synth workloads at the smallest sizes the tests use, and one picture of the RPR fixture):
  i_416x240      416x240 I picture (intra_frac 1.0)
  b_832x480      832x480 B picture with the intra tools, intra_frac 0.2, with LMCS; b_832x480_nolmcs: without
  default_832    832x480 default workload: CIIP and DMVR units, the picture with the CIIP units' intra prediction
  rpr            the first batch of scaled-reference PUs of tests/golden/rpr/rpr.ovg plus the regular PUs beside them (prediction only)
Ways: a full flush; the stages MC / ITX / DBF / SAO / ALF off one at a time; the ordered pass per level and per CTU; 64 and 4096
flow workers; a resident replay; after ovhip_job_test_abort_next_flow (n_ordered_retries 1); with TMVP cells; with the eager DMVR
rows in two halves, the rest recorded behind them and the flush while the second half is pending; in bands of 1, 2 and all CTU rows.
"""
import copy
import ctypes as C
import hashlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

HOST_TIMES = ("host_us_prepare", "host_us_upload", "host_us_wait", "host_us_launch")


def md5(*arrays):
    h = hashlib.md5()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


class Picture:
    """One recorded picture: how to load it into a job, its references, and whether it can go in bands."""

    def __init__(self, name, w, h, load, refs, intra=None, wl=None, stages=0):
        self.name, self.w, self.h, self.load, self.refs, self.intra, self.wl, self.stages = name, w, h, load, refs, intra, wl, stages


def synth_picture(ctx, name, w, h, seed, **kw):
    from openvvc_amd import capi, synth
    wl = synth.make_workload(w, h, seed, **kw)
    if wl.ciip_units is None or not len(wl.ciip_units):
        # a band is a slice of the lists in decoding order (tests/test_gpu_bands.py): the coefficient offsets give it back
        tb = np.asarray(wl.tb_cmds).view(capi.TB_CMD_DTYPE).reshape(-1)
        wl = copy.copy(wl)
        wl.tb_cmds = np.ascontiguousarray(tb[np.argsort(tb["coef_off"], kind="stable")])
    intra = ctx.upload_pic(*wl.intra) if wl.intra is not None else None
    return Picture(name, w, h, lambda job: job.load_workload(wl), [ctx.upload_pic(*r) for r in wl.refs], intra, wl)


def rpr_picture(ctx):
    import rpr_golden
    from openvvc_amd import capi
    from rpr_cases import pu_desc
    pic_w, pic_h, sizes, refs, cases = rpr_golden.load()
    is_rpr = [rpr_golden.is_rpr(c, pic_w, pic_h, sizes) for c in cases]
    rpr_idx = [i for i, r in enumerate(is_rpr) if r]
    idx = [rpr_idx[i] for i in next(rpr_golden.batches([cases[i] for i in rpr_idx]))]
    box = lambda p: (p["x0"], p["y0"], p["x0"] + (1 << p["log2_w"]), p["y0"] + (1 << p["log2_h"]))
    occ = [box(cases[i]["pu"]) for i in idx]
    for i, r in enumerate(is_rpr):                       # the regular PUs that overlap nothing taken so far (k_mc2 beside k_mc_rpr)
        b = box(cases[i]["pu"])
        if not r and all(b[2] <= o[0] or o[2] <= b[0] or b[3] <= o[1] or o[3] <= b[1] for o in occ):
            idx.append(i); occ.append(b)

    def load(job):
        job.begin()
        rec = job.lib.ovhip_job_recorder(job.j)
        for slot, s in rpr_golden.scales(pic_w, pic_h, sizes, cases[idx[0]]["col"]).items():
            assert capi.set_ref_scale(job.lib, rec, slot, s["scale_hor"], s["scale_ver"], s["ref_w"], s["ref_h"], s["col_hor"], s["col_ver"]) == 0
        for i in idx:
            assert job.lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, cases[i]["pu"]))) > 0
        job.params = capi.JobParams()
        job.params.log2_ctu_s, job.params.stages = 7, capi.STAGE_MC

    return Picture("rpr", pic_w, pic_h, load, [ctx.upload_pic(*r) for r in refs], stages=capi.STAGE_MC)


def ways(capi, pic):
    """(name, what to do between load and flush / instead of the flush)"""
    base = pic.stages or capi.STAGE_ALL

    def stages(s):
        return lambda job, dst: (setattr(job.params, "stages", s), job.flush(dst, pic.refs, pic.intra))

    def workers(n):
        return lambda job, dst: (setattr(job.params, "flow_workers", n), job.flush(dst, pic.refs, pic.intra))

    def resident(job, dst):
        job.flush(dst, pic.refs, pic.intra)
        job.wait()
        job.params.stages = base | capi.STAGE_RESIDENT
        job.flush(dst, pic.refs, pic.intra)

    def aborted(job, dst):
        job.test_abort_next_flow()
        job.flush(dst, pic.refs, pic.intra)

    def tmvp(job, dst):
        job.params.tmvp_cells = 1
        job.flush(dst, pic.refs, pic.intra)

    def eager(job, dst):
        # the shim's order: refined units recorded and searched row by row, the rest of the picture recorded behind them WITHOUT a new
        # begin, the flush while the second pass is still pending (the flush collects it; its units are searched, not searched again)
        wl, ux = pic.wl, pic.wl.mcx_units
        job.begin()
        for a, b in ((0, len(ux) // 2), (len(ux) // 2, len(ux))):
            job.rec.append_raw(capi.REC_MCX, ux[a:b])
            job.dmvr_rows_begin(pic.refs, 7)
        for which, arr in ((capi.REC_COEF, wl.coefs), (capi.REC_TB, wl.tb_cmds), (capi.REC_MC, wl.mc_units), (capi.REC_AFF, wl.aff_units),
                           (capi.REC_SIDE, wl.aff_side), (capi.REC_REGION, wl.lmcs_regions), (capi.REC_CIIP, wl.ciip_units),
                           (capi.REC_ITASK, wl.itasks), (capi.REC_EDGE_V, wl.dbf_edges[0]), (capi.REC_EDGE_H, wl.dbf_edges[1])):
            if arr is not None and len(arr):
                job.rec.append_raw(which, arr)
        offs = capi.DbfOffsets()
        for i in range(8):
            offs.beta[i], offs.tc[i] = wl.dbf_planes["beta_offset"], wl.dbf_planes["tc_offset"]
        assert job.lib.ovhip_rec_set_dbf_offsets(job.rec.h, C.byref(offs), 1) == 0
        job.flush(dst, pic.refs, pic.intra)                    # (job.params: the load before this way made them)

    def bands(per_band):
        return lambda job, dst: job.flush_in_bands(pic.wl, dst, pic.refs, per_band)

    out = [("flush", lambda job, dst: job.flush(dst, pic.refs, pic.intra))]
    out += [(f"no_{n}", stages(base & ~getattr(capi, "STAGE_" + n.upper()))) for n in ("mc", "itx", "dbf", "sao", "alf")]
    out += [("intra_levels", stages(base | capi.STAGE_INTRA_LEVELS)), ("intra_ctu", stages(base | capi.STAGE_INTRA_CTU)),
            ("workers_64", workers(64)), ("workers_4096", workers(4096)), ("resident", resident), ("aborted", aborted), ("tmvp_cells", tmvp)]
    if pic.wl is not None:
        if pic.wl.mcx_units is not None and len(pic.wl.mcx_units) > 1:
            out.append(("eager_rows", eager))
        out += [(f"bands_{k}", bands(k)) for k in (1, 2, (pic.h + 127) // 128)]
    return out


def child():
    from openvvc_amd import capi, engine, synth
    lib = capi.load()
    if lib.ovhip_abi_version() != capi.OVHIP_ABI_VERSION:
        sys.exit(f"{capi.LIB_PATH}: ABI {lib.ovhip_abi_version()}, this tool compares builds of ABI {capi.OVHIP_ABI_VERSION}")
    ctx = engine.Context(0)
    no_lmcs = tuple(t for t in synth.INTRA_TOOLS if t != "lmcs")
    pictures = [synth_picture(ctx, "i_416x240", 416, 240, 5, tools=synth.INTRA_TOOLS, intra_frac=1.0),
                synth_picture(ctx, "b_832x480", 832, 480, 0x266, tools=synth.INTRA_TOOLS, intra_frac=0.2),
                synth_picture(ctx, "b_832x480_nolmcs", 832, 480, 11, tools=no_lmcs, intra_frac=0.2),
                synth_picture(ctx, "default_832", 832, 480, 3), rpr_picture(ctx)]
    for pic in pictures:
        job = engine.Job(ctx, pic.w, pic.h)
        dst = ctx.new_pic(pic.w, pic.h)
        for name, submit in ways(capi, pic):
            dst.upload(*[np.full_like(p, 0x155) for p in dst.download()])          # nothing of the previous way may survive unnoticed
            pic.load(job)
            submit(job, dst)                                    # (a refusal ends the run: every way listed is one both builds must take)
            job.wait()
            st = job.stats()
            stats = " ".join(f"{f}={getattr(st, f)}" for f, _ in capi.JobStats._fields_ if f not in HOST_TIMES)
            print(f"{pic.name:18s} {name:22s} yuv {md5(*dst.download())} mv {md5(job.refined_mvs())} tmvp {md5(job.tmvp_cells())} {stats}", flush=True)
        job.close()
    ctx.close()


def ab(other):
    outs = []
    for name in ("libovvc_hip.so", other):
        env = dict(os.environ, OVVC_HIP_LIB_NAME=name)
        outs.append(subprocess.run([sys.executable, __file__], env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=180).stdout.splitlines())
    bad = [(a, b) for a, b in zip(*outs) if a != b]
    for a, b in bad:
        print(f"libovvc_hip.so: {a}\n{other}: {b}")
    if bad or len(outs[0]) != len(outs[1]) or not outs[0]:
        sys.exit(f"libovvc_hip.so and {other} differ in {len(bad)} of {len(outs[0])} / {len(outs[1])} lines")
    print("\n".join(outs[0]))
    print(f"libovvc_hip.so and {other}: identical text in all {len(outs[0])} lines")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--ab":
        ab(sys.argv[2])
    elif len(sys.argv) == 1:
        child()
    else:
        sys.exit(__doc__)
