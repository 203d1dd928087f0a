"""GPU: prediction from scaled references against the REFERENCE's own slots (tests/golden/rpr/rpr.ovg, written by
tools/rpr_golden/gen_rpr.c from rcn_mcp_b / rcn_gpm_b): the recorder + ovhip_mc_rpr_launch, and the recorder + the picture job
(ovhip_job_flush, which launches k_mc_rpr beside k_mc2 only on pictures that hold RPR units), bit-exact; GPM units (rcn_gpm_b)
included; the fused CIIP blend against put_weighted_ciip_pixels applied to the reference's inter prediction."""
import ctypes as C

import numpy as np
import pytest

from openvvc_amd import capi, engine
import rpr_golden
from rpr_cases import pu_desc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return rpr_golden.load()


def _record(lib, rec, golden, idx, ciip=0):
    pic_w, pic_h, sizes, refs, cases = golden
    for slot, s in rpr_golden.scales(pic_w, pic_h, sizes, cases[idx[0]]["col"]).items():
        assert capi.set_ref_scale(lib, rec, slot, s["scale_hor"], s["scale_ver"], s["ref_w"], s["ref_h"], s["col_hor"], s["col_ver"]) == 0
    for i in idx:
        pu = dict(cases[i]["pu"])
        if ciip and not pu["refine"]:
            pu["ciip_wt"] = ciip
        assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu))) > 0, lib.ovhip_rec_refusal(rec)


def _check(golden, idx, y, cb, cr, intra=None, wt=0):
    cases = golden[4]
    for i in idx:
        pu = cases[i]["pu"]
        x0, y0, pw, ph = pu["x0"], pu["y0"], 1 << pu["log2_w"], 1 << pu["log2_h"]
        exp = [e.astype(np.int64) for e in cases[i]["exp"]]
        if intra is not None and not pu["refine"]:
            # put_weighted_ciip_pixels (rcn_mc.c:1611-1628) on the reference's inter prediction
            iy, icb, icr = (p.astype(np.int64) for p in intra)
            sl = [(slice(y0, y0 + ph), slice(x0, x0 + pw)), (slice(y0 // 2, (y0 + ph) // 2), slice(x0 // 2, (x0 + pw) // 2))]
            exp = [np.clip((ip[sl[k > 0]] * wt + e * (4 - wt) + 2) >> 2, 0, 1023) for k, (e, ip) in enumerate(zip(exp, (iy, icb, icr)))]
        assert np.array_equal(y[y0:y0 + ph, x0:x0 + pw], exp[0]), pu
        assert np.array_equal(cb[y0 // 2:(y0 + ph) // 2, x0 // 2:(x0 + pw) // 2], exp[1]), pu
        assert np.array_equal(cr[y0 // 2:(y0 + ph) // 2, x0 // 2:(x0 + pw) // 2], exp[2]), pu


def _upload_refs(ctx, refs):
    return [ctx.upload_pic(*r) for r in refs]


def _free(ctx, pics):
    for p in pics:
        ctx.lib.ovhip_pic_free(ctx.h, C.byref(p.s))


@pytest.mark.parametrize("ciip", [0, 2])
def test_launch_equals_reference(ctx, golden, ciip):
    pic_w, pic_h, sizes, refs, cases = golden
    lib = capi.load()
    rng = np.random.default_rng(3)
    intra_np = (rng.integers(0, 1024, (pic_h, pic_w)).astype(np.uint16), rng.integers(0, 1024, (pic_h // 2, pic_w // 2)).astype(np.uint16),
                rng.integers(0, 1024, (pic_h // 2, pic_w // 2)).astype(np.uint16))
    d_refs = _upload_refs(ctx, refs)
    intra = ctx.upload_pic(*intra_np) if ciip else None
    n_checked = 0
    try:
        rpr_idx = [i for i, c in enumerate(cases) if rpr_golden.is_rpr(c, pic_w, pic_h, sizes)]
        for idx in rpr_golden.batches([cases[i] for i in rpr_idx]):
            idx = [rpr_idx[i] for i in idx]
            rec = lib.ovhip_rec_create(pic_w, pic_h)
            try:
                _record(lib, rec, golden, idx, ciip)
                units = capi.rpr_units(lib, rec)
            finally:
                lib.ovhip_rec_destroy(rec)
            d_units = ctx.upload(np.frombuffer(bytes((capi.RprUnit * len(units))(*units)), dtype=np.uint8))
            d_units.count = len(units)
            dst = ctx.new_pic(pic_w, pic_h)
            ctx.mc_rpr(dst, d_refs, d_units, None, intra=intra)
            ctx.sync()
            _check(golden, idx, *dst.download(), intra=intra_np if ciip else None, wt=ciip)
            n_checked += len(idx)
            _free(ctx, [dst])
            d_units.free()
    finally:
        _free(ctx, d_refs + ([intra] if intra else []))
    assert n_checked > 100


def _stats(lib, job):
    st = capi.JobStats()
    assert lib.ovhip_job_last_stats(job.j, C.byref(st)) == 0
    return st


def test_job_flush_equals_reference_and_adds_one_launch(ctx, golden):
    pic_w, pic_h, sizes, refs, cases = golden
    lib = capi.load()
    d_refs = _upload_refs(ctx, refs)
    job = engine.Job(ctx, pic_w, pic_h)
    try:
        params = capi.JobParams()
        params.log2_ctu_s, params.stages = 7, capi.STAGE_MC
        rpr_idx = [i for i, c in enumerate(cases) if rpr_golden.is_rpr(c, pic_w, pic_h, sizes)]
        reg_idx = [i for i, c in enumerate(cases) if not rpr_golden.is_rpr(c, pic_w, pic_h, sizes)]
        assert reg_idx
        # a picture without RPR units: the fixture's cases that only read the unscaled reference (k_mc2 alone, other slots of the
        # table are pictures of other sizes: stand-ins for k_mc2)
        reg = [reg_idx[i] for i in next(rpr_golden.batches([cases[i] for i in reg_idx]))]
        job.begin()
        _record(lib, lib.ovhip_job_recorder(job.j), golden, reg)
        dst = ctx.new_pic(pic_w, pic_h)
        job.flush(dst, d_refs, params=params)
        job.wait()
        base = _stats(lib, job).n_launches
        _check(golden, reg, *dst.download())
        _free(ctx, [dst])
        assert base == 1
        n_checked = 0
        for idx in rpr_golden.batches([cases[i] for i in rpr_idx]):
            idx = [rpr_idx[i] for i in idx]
            # the same picture plus the regular cases that do not overlap it
            occ = [(cases[i]["pu"]["x0"], cases[i]["pu"]["y0"], cases[i]["pu"]["x0"] + (1 << cases[i]["pu"]["log2_w"]),
                    cases[i]["pu"]["y0"] + (1 << cases[i]["pu"]["log2_h"])) for i in idx]
            extra = []
            for i in reg:
                p = cases[i]["pu"]
                r = (p["x0"], p["y0"], p["x0"] + (1 << p["log2_w"]), p["y0"] + (1 << p["log2_h"]))
                if all(r[2] <= o[0] or o[2] <= r[0] or r[3] <= o[1] or o[3] <= r[1] for o in occ):
                    extra.append(i); occ.append(r)
            job.begin()
            _record(lib, lib.ovhip_job_recorder(job.j), golden, idx + extra)
            dst = ctx.new_pic(pic_w, pic_h)
            job.flush(dst, d_refs, params=params)
            job.wait()
            assert _stats(lib, job).n_launches == (base if extra else 0) + 1
            _check(golden, idx + extra, *dst.download())
            n_checked += len(idx)
            _free(ctx, [dst])
        assert n_checked > 100
    finally:
        job.close()
        _free(ctx, d_refs)
