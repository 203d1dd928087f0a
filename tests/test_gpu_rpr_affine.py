"""GPU: affine coding units on scaled references (reference picture resampling) -- the recorder + ovhip_mca_rpr_launch and the
recorder + the picture job against the REFERENCE's own slots (tests/golden/rpr/rpr_affine.ovg, written by
tools/rpr_golden/gen_rpr_affine.c), the fixture's no-PROF cases once more as lone 4x4 luma PUs, and a 1920x1080 B picture
against the numpy restatement (tests/spec_rpr_affine.py), alone and mixed with regular, GPM and plain RPR units."""
import ctypes as C

import numpy as np
import pytest

from openvvc_amd import capi, engine
import rpr_affine_golden as G
import rpr_golden
import spec_rpr as S
import spec_rpr_affine as A
from rpr_affine_cases import random_affine_cus, reads_scaled
from rpr_cases import lmcs_lut, pu_desc, random_pus, ref_planes, scales_for

pytestmark = pytest.mark.gpu
BOTH = capi.RPR_TOOL_AFFINE | capi.RPR_TOOL_PU4x4


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return G.load()


def _set_scales(lib, rec, scales):
    for slot, s in scales.items():
        assert capi.set_ref_scale(lib, rec, slot, s["scale_hor"], s["scale_ver"], s["ref_w"], s["ref_h"], s["col_hor"], s["col_ver"]) == 0


def _free(ctx, pics):
    for p in pics:
        ctx.lib.ovhip_pic_free(ctx.h, C.byref(p.s))


def _dev_array(ctx, lib, rec, fn, elem):
    n = C.c_size_t(0)
    p = getattr(lib, fn)(rec, C.byref(n))
    raw = C.string_at(p, n.value * elem) if n.value else b""
    d = ctx.upload(np.frombuffer(raw, dtype=np.uint8) if raw else np.zeros(16, np.uint8))
    d.count = n.value
    return d


def _launch_recorded(ctx, lib, rec, dst, d_refs, d_lut):
    """What a caller of the stage launches does with an opted-in recorder's RPR arrays."""
    d_aff = _dev_array(ctx, lib, rec, "ovhip_rec_aff_rpr_units", C.sizeof(capi.AffRprUnit))
    d_side = _dev_array(ctx, lib, rec, "ovhip_rec_aff_side", 4)
    d_rpr = _dev_array(ctx, lib, rec, "ovhip_rec_rpr_units", C.sizeof(capi.RprUnit))
    if d_rpr.count:
        ctx.mc_rpr(dst, d_refs, d_rpr, d_lut)
    if d_aff.count:
        ctx.mca_rpr(dst, d_refs, d_aff, d_side, d_lut)
    ctx.sync()
    counts = (d_aff.count, d_rpr.count)
    for d in (d_aff, d_side, d_rpr):
        d.free()
    return counts


def _check_cases(cases, idx, y, cb, cr, lut=None, luma_only=False):
    for i in idx:
        cu = cases[i]["cu"]
        x0, y0, w, h = cu["x0"], cu["y0"], 1 << cu["log2_w"], 1 << cu["log2_h"]
        ey, ecb, ecr = cases[i]["exp"]
        if lut is not None:
            ey = lut[ey]                               # lmcs_reshape_forward runs on every clipped luma block
        info = {k: v for k, v in cu.items() if k not in ("mv0", "mv1", "dmv_scale")}
        assert np.array_equal(y[y0:y0 + h, x0:x0 + w], ey), info
        if not luma_only:
            assert np.array_equal(cb[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], ecb), info
            assert np.array_equal(cr[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], ecr), info


@pytest.mark.parametrize("lmcs", [0, 1])
def test_launch_equals_reference(ctx, golden, lmcs):
    pic_w, pic_h, sizes, refs, cases, _ = golden
    lib = capi.load()
    lut = lmcs_lut()
    d_refs = [ctx.upload_pic(*r) for r in refs]
    d_lut = ctx.upload(lut)
    keep = []
    n_checked = 0
    try:
        for idx in G.batches(cases):
            rec = lib.ovhip_rec_create(pic_w, pic_h)
            dst = ctx.new_pic(pic_w, pic_h)
            try:
                assert lib.ovhip_rec_set_rpr_tools(rec, capi.RPR_TOOL_AFFINE) == 0
                _set_scales(lib, rec, rpr_golden.scales(pic_w, pic_h, sizes, cases[idx[0]]["col"]))
                for i in idx:
                    assert lib.ovhip_rec_affine_cu(rec, C.byref(G.affine_desc(capi, dict(cases[i]["cu"], lmcs=lmcs), keep))) > 0
                n_aff, n_rpr = _launch_recorded(ctx, lib, rec, dst, d_refs, d_lut)
                assert n_aff and not n_rpr
                _check_cases(cases, idx, *dst.download(), lut=lut if lmcs else None)
                n_checked += len(idx)
            finally:
                lib.ovhip_rec_destroy(rec)
                _free(ctx, [dst])
    finally:
        _free(ctx, d_refs)
        d_lut.free()
    assert n_checked == len(cases)


def _stats(lib, job):
    st = capi.JobStats()
    assert lib.ovhip_job_last_stats(job.j, C.byref(st)) == 0
    return st


def test_job_flush_equals_reference_and_adds_one_launch(ctx, golden):
    pic_w, pic_h, sizes, refs, cases, _ = golden
    pu_cases = rpr_golden.load()[4]
    lib = capi.load()
    d_refs = [ctx.upload_pic(*r) for r in refs]
    job = engine.Job(ctx, pic_w, pic_h)
    keep = []
    try:
        params = capi.JobParams()
        params.log2_ctu_s, params.stages = 7, capi.STAGE_MC
        rec = lib.ovhip_job_recorder(job.j)
        assert lib.ovhip_rec_set_rpr_tools(rec, BOTH) == 0            # once: the setting survives every job.begin()
        reg_idx = [i for i, c in enumerate(pu_cases) if not rpr_golden.is_rpr(c, pic_w, pic_h, sizes)]
        reg = [reg_idx[i] for i in next(rpr_golden.batches([pu_cases[i] for i in reg_idx]))]

        def check_reg(idx, y, cb, cr):
            for i in idx:
                pu = pu_cases[i]["pu"]
                x0, y0, pw, ph = pu["x0"], pu["y0"], 1 << pu["log2_w"], 1 << pu["log2_h"]
                assert np.array_equal(y[y0:y0 + ph, x0:x0 + pw], pu_cases[i]["exp"][0]), pu
                assert np.array_equal(cb[y0 // 2:(y0 + ph) // 2, x0 // 2:(x0 + pw) // 2], pu_cases[i]["exp"][1]), pu
                assert np.array_equal(cr[y0 // 2:(y0 + ph) // 2, x0 // 2:(x0 + pw) // 2], pu_cases[i]["exp"][2]), pu

        # a picture without such units: exactly the launches of before (k_mc2 alone)
        job.begin()
        for i in reg:
            assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu_cases[i]["pu"]))) > 0
        dst = ctx.new_pic(pic_w, pic_h)
        job.flush(dst, d_refs, params=params)
        job.wait()
        base = _stats(lib, job).n_launches
        check_reg(reg, *dst.download())
        _free(ctx, [dst])
        assert base == 1
        n_checked = 0
        for idx in G.batches(cases):
            occ = [(cases[i]["cu"]["x0"], cases[i]["cu"]["y0"], cases[i]["cu"]["x0"] + (1 << cases[i]["cu"]["log2_w"]),
                    cases[i]["cu"]["y0"] + (1 << cases[i]["cu"]["log2_h"])) for i in idx]
            extra = []                                      # (PUs on the unscaled reference read no collocation flag)
            for i in reg:
                p = pu_cases[i]["pu"]
                r = (p["x0"], p["y0"], p["x0"] + (1 << p["log2_w"]), p["y0"] + (1 << p["log2_h"]))
                if all(r[2] <= o[0] or o[2] <= r[0] or r[3] <= o[1] or o[3] <= r[1] for o in occ):
                    extra.append(i); occ.append(r)
            job.begin()
            _set_scales(lib, rec, rpr_golden.scales(pic_w, pic_h, sizes, cases[idx[0]]["col"]))
            for i in idx:
                assert lib.ovhip_rec_cu_inter(rec, None, C.byref(G.affine_desc(capi, cases[i]["cu"], keep))) > 0
            for i in extra:
                assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu_cases[i]["pu"]))) > 0
            dst = ctx.new_pic(pic_w, pic_h)
            job.flush(dst, d_refs, params=params)
            job.wait()
            assert _stats(lib, job).n_launches == (base if extra else 0) + 1
            y, cb, cr = dst.download()
            _check_cases(cases, idx, y, cb, cr)
            check_reg(extra, y, cb, cr)
            n_checked += len(idx)
            _free(ctx, [dst])
        assert n_checked == len(cases)
    finally:
        job.close()
        _free(ctx, d_refs)


def test_no_prof_cases_as_lone_4x4_luma_pus(ctx, golden):
    """What the unpatched caller's fallback records: every sub-block one rcn_mcp_b_l(2,2) call, planes = 1."""
    pic_w, pic_h, sizes, refs, cases, _ = golden
    lib = capi.load()
    d_refs = [ctx.upload_pic(*r) for r in refs]
    n_checked = n_mixed = n_plain = 0
    try:
        sel = [i for i, c in enumerate(cases) if not c["cu"]["prof_dir"]]
        for idx in G.batches([cases[i] for i in sel]):
            idx = [sel[i] for i in idx]
            rec = lib.ovhip_rec_create(pic_w, pic_h)
            dst = ctx.new_pic(pic_w, pic_h)
            try:
                assert lib.ovhip_rec_set_rpr_tools(rec, capi.RPR_TOOL_PU4x4) == 0
                _set_scales(lib, rec, rpr_golden.scales(pic_w, pic_h, sizes, cases[idx[0]]["col"]))
                for i in idx:
                    cu = cases[i]["cu"]
                    for sy in range((1 << cu["log2_h"]) >> 2):
                        for sx in range((1 << cu["log2_w"]) >> 2):
                            pu = dict(x0=cu["x0"] + 4 * sx, y0=cu["y0"] + 4 * sy, log2_w=2, log2_h=2, inter_dir=cu["inter_dir"],
                                      ref0=cu["ref0"], ref1=cu["ref1"], mv0x=int(cu["mv0"][sy, sx, 0]), mv0y=int(cu["mv0"][sy, sx, 1]),
                                      mv1x=int(cu["mv1"][sy, sx, 0]), mv1y=int(cu["mv1"][sy, sx, 1]), bcw_idx_plus1=cu["bcw_idx_plus1"],
                                      poc0=cu["poc0"], poc1=cu["poc1"])
                            d = pu_desc(capi, pu)
                            d.planes = 1
                            assert lib.ovhip_rec_pu(rec, C.byref(d)) == 1, lib.ovhip_rec_refusal(rec)
                n = C.c_size_t(0)
                lib.ovhip_rec_mc_units(rec, C.byref(n))
                assert n.value == 0                        # every block of these cases reads a scaled list
                n_aff, n_rpr = _launch_recorded(ctx, lib, rec, dst, d_refs, None)
                assert n_aff + n_rpr
                n_mixed += n_aff
                n_plain += n_rpr
                _check_cases(cases, idx, *dst.download(), luma_only=True)
                n_checked += len(idx)
            finally:
                lib.ovhip_rec_destroy(rec)
                _free(ctx, [dst])
    finally:
        _free(ctx, d_refs)
    assert n_checked == len(sel) and n_checked > 60 and n_mixed > 0 and n_plain > n_mixed


PIC_W, PIC_H = 1920, 1080
SIZES = [(3840, 2160), (2880, 1620), (1280, 720), (960, 540), (1920, 1080)]


def _picture(seed, far, cols, n_cus, n_pus):
    """Affine CUs on one half of the 64x64 cells, regular / GPM / plain RPR PUs on the other."""
    scales = scales_for(PIC_W, PIC_H, SIZES, cols)
    cells = [(x, y) for y in range(0, PIC_H - 63, 64) for x in range(0, PIC_W - 63, 64)]
    rng = np.random.default_rng(seed)
    rng.shuffle(cells)
    cells = [tuple(int(v) for v in c) for c in cells]
    cus = [cu for cu in random_affine_cus(PIC_W, PIC_H, len(SIZES), n_cus, seed=seed, far=far, cells=cells[:n_cus]) if reads_scaled(cu, scales)]
    taken = set(cells[:n_cus])
    pus = [pu for pu in random_pus(PIC_W, PIC_H, len(SIZES), 10 ** 6, seed=seed + 1, far=far)
           if (pu["x0"] & ~63, pu["y0"] & ~63) not in taken][:n_pus]
    for k, pu in enumerate(pus):
        if k % 5 == 0 and pu["log2_w"] >= 3 and pu["log2_h"] >= 3:
            pu.update(refine=4, inter_dir=3, gpm_split_dir=(7 * k) % 64, bcw_idx_plus1=0, prec_amvr_half=0)     # GPM
    return scales, cus, pus


def _record_picture(lib, rec, scales, cus, pus, keep):
    _set_scales(lib, rec, scales)
    for pu in pus:
        assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu))) > 0, lib.ovhip_rec_refusal(rec)
    for cu in cus:
        assert lib.ovhip_rec_affine_cu(rec, C.byref(G.affine_desc(capi, cu, keep))) > 0, lib.ovhip_rec_refusal(rec)


@pytest.fixture(scope="module")
def refs_1080():
    return [ref_planes(w, h, 11 + i) for i, (w, h) in enumerate(SIZES)]


@pytest.mark.parametrize("far,cols", [(False, (0, 0)), (True, (1, 1))])
def test_b_picture_from_four_sizes(ctx, refs_1080, far, cols):
    """Affine CUs of a 1920x1080 B picture that read 3840x2160, 2880x1620, 1280x720 and 960x540 references (and the picture's own
    size on the other list), far vectors included, both collocation settings: bit-exact with the restatement, CU by CU."""
    lib = capi.load()
    lut = lmcs_lut()
    scales, cus, _ = _picture(41 + far, far, cols, 200, 0)
    assert len(cus) > 120
    rec = lib.ovhip_rec_create(PIC_W, PIC_H)
    d_refs = [ctx.upload_pic(*r) for r in refs_1080]
    d_lut = ctx.upload(lut)
    dst = ctx.new_pic(PIC_W, PIC_H)
    keep = []
    try:
        assert lib.ovhip_rec_set_rpr_tools(rec, capi.RPR_TOOL_AFFINE) == 0
        _record_picture(lib, rec, scales, cus, [], keep)
        n_aff, _ = _launch_recorded(ctx, lib, rec, dst, d_refs, d_lut)
        assert n_aff > 200
        y, cb, cr = dst.download()
        slots = set()
        for cu in cus:
            ey, ecb, ecr = A.predict_affine_cu(refs_1080, scales, PIC_W, PIC_H, cu, lut)
            x0, y0, w, h = cu["x0"], cu["y0"], 1 << cu["log2_w"], 1 << cu["log2_h"]
            info = {k: v for k, v in cu.items() if k not in ("mv0", "mv1", "dmv_scale")}
            assert np.array_equal(y[y0:y0 + h, x0:x0 + w], ey), info
            assert np.array_equal(cb[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], ecb), info
            assert np.array_equal(cr[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], ecr), info
            slots |= {cu["ref0"], cu["ref1"]}
        assert slots >= {0, 1, 2, 3}
    finally:
        lib.ovhip_rec_destroy(rec)
        _free(ctx, d_refs + [dst])
        d_lut.free()


def test_other_units_of_the_picture_are_untouched(ctx, refs_1080):
    """The same kind of picture with regular, GPM and plain RPR units beside the affine ones, through the picture job: those units'
    samples are what the job leaves without the affine CUs (the path of before: k_mc2 + k_mc_rpr), the affine CUs' samples the
    restatement's, and the affine units cost exactly one launch."""
    lib = capi.load()
    scales, cus, pus = _picture(77, True, (0, 1), 150, 160)
    assert len(cus) > 80 and len(pus) > 120 and any(pu.get("refine") == 4 for pu in pus)
    d_refs = [ctx.upload_pic(*r) for r in refs_1080]
    job = engine.Job(ctx, PIC_W, PIC_H)
    keep = []
    try:
        params = capi.JobParams()
        params.log2_ctu_s, params.stages = 7, capi.STAGE_MC
        rec = lib.ovhip_job_recorder(job.j)
        out, launches, counts = [], [], []
        for with_affine in (False, True):
            assert lib.ovhip_rec_set_rpr_tools(rec, BOTH if with_affine else 0) == 0
            job.begin()
            _record_picture(lib, rec, scales, cus if with_affine else [], pus, keep)
            counts.append((len(capi.rpr_units(lib, rec)), len(capi.aff_rpr_units(lib, rec))))
            dst = ctx.new_pic(PIC_W, PIC_H)
            job.flush(dst, d_refs, params=params)
            job.wait()
            launches.append(_stats(lib, job).n_launches)
            out.append(dst.download())
            _free(ctx, [dst])
        assert counts[0][0] > 20 and counts[0][1] == 0 and counts[1][0] == counts[0][0] and counts[1][1] > 80
        assert launches == [2, 3]
        for pu in pus:
            x0, y0, pw, ph = pu["x0"], pu["y0"], 1 << pu["log2_w"], 1 << pu["log2_h"]
            for a, b, s in ((out[0][0], out[1][0], 1), (out[0][1], out[1][1], 2), (out[0][2], out[1][2], 2)):
                assert np.array_equal(a[y0 // s:(y0 + ph) // s, x0 // s:(x0 + pw) // s], b[y0 // s:(y0 + ph) // s, x0 // s:(x0 + pw) // s]), pu
        y, cb, cr = out[1]
        for cu in cus:
            ey, ecb, ecr = A.predict_affine_cu(refs_1080, scales, PIC_W, PIC_H, cu, None)
            x0, y0, w, h = cu["x0"], cu["y0"], 1 << cu["log2_w"], 1 << cu["log2_h"]
            assert np.array_equal(y[y0:y0 + h, x0:x0 + w], ey) and np.array_equal(cb[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], ecb)
            assert np.array_equal(cr[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], ecr)
        # and outside every unit nothing was written
        mask = np.ones((PIC_H, PIC_W), bool)
        for b in pus + cus:
            mask[b["y0"]:b["y0"] + (1 << b["log2_h"]), b["x0"]:b["x0"] + (1 << b["log2_w"])] = False
        assert not y[mask].any()
    finally:
        job.close()
        _free(ctx, d_refs)
