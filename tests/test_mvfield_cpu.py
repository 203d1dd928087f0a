"""CPU: motion field output on the host (openvvc_amd/csrc/ovvc_mvfield.c): ovhip_mvfield_host and ovhip_mvfield_bytes against the numpy
restatement tests/spec_mvfield.py -- the recorder's own arrays of two synthetic pictures with the oracle's refined vectors, directed
lists at 72x40, recorder-made units on scaled references, empty lists --, and the refusals, each with its destinations proven
unwritten.  The definition is exact: every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import oracle_pipeline
import rpr_affine_golden as G
import rpr_golden
import spec_mvfield as sm
from openvvc_amd import capi, engine, synth
from rpr_affine_cases import random_affine_cus
from rpr_cases import pu_desc, random_pus, scales_for

EINVAL = -3
TAIL = 48                                                     # bytes behind a destination that must stay as they were


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def c_src(L, refined=True):
    """(ovhip_mvfield_src over the arrays of a spec_mvfield.lists() dict, in host memory; what keeps them alive)"""
    s = capi.MvfieldSrc()
    keep = {k: np.ascontiguousarray(L[k]) for k in ("mc", "mcx", "aff", "rpr", "affr", "side")}
    for k in ("mc", "mcx", "aff", "rpr", "affr"):
        setattr(s, k, keep[k].ctypes.data if len(keep[k]) else None)
        setattr(s, "n_" + k, len(keep[k]))
    s.side = keep["side"].ctypes.data if len(keep["side"]) else None
    if refined and L["refined"] is not None and len(L["refined"]):
        keep["refined"] = np.ascontiguousarray(L["refined"], dtype=np.int32)
        s.refined = keep["refined"].ctypes.data
    return s, keep


def host_field(lib, w, h, L, dtype, layout, vectors, want=(True, True), lead=(0, 0)):
    """ovhip_mvfield_host into buffers that held 0xA5 -> (vectors buffer or None, info buffer or None, sizes): each buffer is its
    `lead` bytes, the destination, TAIL bytes"""
    fmt = engine.mvfield_format(dtype, layout, vectors)
    ib = C.c_size_t()
    vb = lib.ovhip_mvfield_bytes(w, h, C.byref(fmt), C.byref(ib))
    assert (vb, ib.value) == sm.sizes(w, h, dtype)
    src, keep = c_src(L)
    vec = np.full(lead[0] + vb + TAIL, sm.FILL, np.uint8) if want[0] else None
    info = np.full(lead[1] + ib.value + TAIL, sm.FILL, np.uint8) if want[1] else None
    r = lib.ovhip_mvfield_host(w, h, C.byref(src), C.byref(fmt), vec.ctypes.data + lead[0] if want[0] else None, vb,
                               info.ctypes.data + lead[1] if want[1] else None, ib.value)
    assert r == 0, r
    return vec, info, (vb, ib.value)


def check_against_spec(lib, w, h, L, dtype, layout, vectors, want=(True, True), lead=(0, 0)):
    what = (w, h, dtype, layout, vectors, want, lead)
    vec, info, (vb, ib) = host_field(lib, w, h, L, dtype, layout, vectors, want, lead)
    sv, si = sm.field(w, h, L, dtype, layout, vectors)
    assert (sv.nbytes, si.nbytes) == (vb, ib), what
    for got, spec, n, ld in ((vec, sv, vb, lead[0]), (info, si, ib, lead[1])):
        if got is None:
            continue
        assert (got[:ld] == sm.FILL).all() and (got[ld + n:] == sm.FILL).all(), what
        assert got[ld:ld + n].tobytes() == spec.tobytes(), what


def workload_lists(wl, refined=None):
    return sm.lists(wl.mc_units, wl.mcx_units, wl.aff_units, None, None, wl.aff_side, refined)


@pytest.fixture(scope="module")
def pictures():
    """the two 416x240 pictures with the oracle's refined vectors (computed once, shared, left unchanged)"""
    out = []
    for seed, kw in ((3, dict(tools=synth.ALL_TOOLS)), (9, dict(tools=synth.INTRA_TOOLS, intra_frac=0.3))):
        wl = synth.make_workload(416, 240, seed, **kw)
        _, mvs = oracle_pipeline.decode(wl, stages=("mc",), want_mvs=True)
        out.append((seed, wl, np.asarray(mvs, np.int32).reshape(-1, 4)))
    return out


def test_struct_layout_enums_and_names():
    assert C.sizeof(capi.MvfieldFormat) == 4
    assert C.sizeof(capi.MvfieldSrc) == 7 * 8 + 5 * 4 + 4
    assert (capi.MVF_I32, capi.MVF_F32, capi.MVF_F16) == sm.DTYPES == (0, 1, 2)
    assert (capi.MVF_PLANAR, capi.MVF_CELLS, capi.MVF_UNIT, capi.MVF_REFINED) == (sm.PLANAR, sm.CELLS, sm.UNIT, sm.REFINED) == (0, 1, 0, 1)
    assert (capi.MVF_INTER, capi.MVF_AFFINE, capi.MVF_GPM, capi.MVF_DMVR, capi.MVF_BDOF, capi.MVF_BCW, capi.MVF_PROF) == (1, 2, 4, 8, 16, 32, 64)
    assert capi.MVF_EMPTY == sm.EMPTY == 0x0000FFFF
    assert capi.OVHIP_ABI_VERSION == 9
    for name in ("ovhip_mvfield_bytes", "ovhip_mvfield_host", "ovhip_mvfield_launch", "ovhip_job_mvfield", "ovhip_frame_set_mvfield_output",
                 "ovhip_stream_set_mvfield_output"):
        assert name in capi.EXPORTED_SYMBOLS, name
    assert (sm.MC_UNIT.itemsize, sm.RPR_UNIT.itemsize, sm.AFFR_UNIT.itemsize) == (C.sizeof(capi.McUnit), C.sizeof(capi.RprUnit), C.sizeof(capi.AffRprUnit))
    assert sm.MC_UNIT == capi.MC_UNIT_DTYPE and sm.AFF_UNIT == capi.AFF_UNIT_DTYPE
    assert engine.mvfield_shape(engine.mvfield_format(layout=capi.MVF_PLANAR), 72, 40) == ((4, 10, 18), (10, 18))
    assert engine.mvfield_shape(engine.mvfield_format(layout=capi.MVF_CELLS), 70, 38) == ((10, 18, 4), (10, 18))


@pytest.mark.parametrize("w,h", [(4, 4), (5, 3), (72, 40), (416, 240), (3840, 2160), (16384, 16384)])
def test_bytes_is_the_formula(lib, w, h):
    for dtype in sm.DTYPES:
        fmt = engine.mvfield_format(dtype)
        ib = C.c_size_t(77)
        w4, h4 = (w + 3) >> 2, (h + 3) >> 2
        assert lib.ovhip_mvfield_bytes(w, h, C.byref(fmt), C.byref(ib)) == 4 * w4 * h4 * (2 if dtype == sm.F16 else 4)
        assert ib.value == 4 * w4 * h4
        assert lib.ovhip_mvfield_bytes(w, h, C.byref(fmt), None) == 4 * w4 * h4 * (2 if dtype == sm.F16 else 4)
    for bad in ((0, 8), (8, 0), (-4, 8), (16385, 8), (8, 16385)):
        ib = C.c_size_t(77)
        assert lib.ovhip_mvfield_bytes(bad[0], bad[1], C.byref(engine.mvfield_format()), C.byref(ib)) == 0 and ib.value == 0
    assert lib.ovhip_mvfield_bytes(8, 8, None, None) == 0
    assert lib.ovhip_mvfield_bytes(8, 8, C.byref(engine.mvfield_format(3)), None) == 0


def test_the_pictures_hold_what_the_field_is_about(pictures):
    """what was measured when the test was written: the tools' shares, the chroma-only unit, the empty cells"""
    (_, wl3, mv3), (_, wl9, mv9) = pictures
    for wl, mvs, covered, min_moved in ((wl3, mv3, 6240, 25), (wl9, mv9, 4340, 14)):
        L = workload_lists(wl, mvs)
        _, info, cov = sm.dense(416, 240, L)
        assert cov.size == 6240 and int(cov.sum()) == covered
        assert ((info == sm.EMPTY) == ~cov).all()
        ux = L["mcx"]
        is_dmvr = (ux["flags"] & sm.MC_DMVR) != 0
        own = np.stack([ux["mv0x"], ux["mv0y"], ux["mv1x"], ux["mv1y"]], axis=1)
        moved = int((mvs[is_dmvr] != own[is_dmvr]).any(axis=1).sum())
        assert moved >= 10, moved                              # otherwise vectors 0 and 1 could not be told apart
        assert moved == min_moved, moved                       # (25 of 36 and 14 of 14 DMVR units when the test was written)
    mc, ux, ua = wl3.mc_units, wl3.mcx_units, wl3.aff_units
    gpm, bi = (mc["flags"] & sm.MC_GPM) != 0, mc["dir"] == 3
    luma = (mc["flags"] & sm.MC_NO_LUMA) == 0
    bcw = luma & bi & ~gpm & ((mc["w0"] != 4) | (mc["w1"] != 4))
    assert (int(luma.sum()), int(gpm.sum()), int(bcw.sum()), int((~luma).sum())) == (577, 17, 20, 1)
    assert (int(((ux["flags"] & sm.MC_DMVR) != 0).sum()), int(((ux["flags"] & (sm.MC_DMVR | sm.MC_BDOF)) == sm.MC_BDOF).sum())) == (36, 41)
    assert (len(ua), int(((ua["flags"] & sm.AFF_PROF) != 0).sum())) == (30, 26)


@pytest.mark.parametrize("which", [0, 1])
def test_twin_equals_restatement_on_the_recorders_arrays(lib, pictures, which):
    _, wl, mvs = pictures[which]
    L = workload_lists(wl, mvs)
    for dtype in sm.DTYPES:
        for layout in sm.LAYOUTS:
            for vectors in sm.VECTORS:
                for want in ((True, True), (True, False), (False, True)):
                    check_against_spec(lib, 416, 240, L, dtype, layout, vectors, want)
    # the two settings of `vectors` differ, and only in cells of DMVR units
    a, ia = sm.field(416, 240, L, sm.I32, sm.CELLS, sm.UNIT)
    b, ib = sm.field(416, 240, L, sm.I32, sm.CELLS, sm.REFINED)
    differ = (a != b).any(axis=2)
    assert differ.any() and ((ia[differ] >> 16) & sm.DMVR).all() and np.array_equal(ia, ib)


def test_directed_lists(lib):
    w, h = sm.DIRECTED_SIZE
    L = sm.directed_lists()
    for dtype in sm.DTYPES:
        for layout in sm.LAYOUTS:
            for vectors in sm.VECTORS:
                for want in ((True, True), (True, False), (False, True)):
                    check_against_spec(lib, w, h, L, dtype, layout, vectors, want)
                check_against_spec(lib, w, h, L, dtype, layout, vectors, lead=(sm.ELEM[dtype], 4))
    # the rules, read off the restatement's cells
    V, info, cov = sm.dense(w, h, L, sm.REFINED)
    assert info[0, 0] == 0xFF | 1 << 8 | sm.INTER << 16 and tuple(V[:, 0, 0]) == (0, 0, sm.ODD, -sm.ODD)            # uni on list 1
    assert info[0, 2] == 1 | 0xFF << 8 | sm.INTER << 16 and tuple(V[:, 1, 2]) == (sm.BIG, -sm.BIG, 0, 0)
    assert (info[1, 3] >> 16) == sm.INTER | sm.BCW and (info[0, 5] >> 16) == sm.INTER | sm.GPM
    assert (info[2, 11] >> 16) == sm.INTER, "DMVR / BDOF are flags of the refined list only"
    assert (info[3, 10] >> 16) == sm.INTER | sm.DMVR | sm.BDOF and tuple(V[:, 3, 10]) == (172, -148, -172, 148)
    assert (info[1, 12] >> 16) == sm.INTER | sm.BDOF and tuple(V[:, 1, 12]) == (33, 34, 35, 36)
    assert (info[9, 17] & 0xFFFF) == 7 | 9 << 8 and cov[6:10, 14:18].all()                                          # the corner
    assert cov[2:4, 16:18].all() and cov[8:10, 8:10].all()                                                           # the clipped units
    assert (info[2, 0] >> 16) == sm.INTER | sm.AFFINE | sm.PROF | sm.BCW and tuple(V[:, 2, 0]) == (sm.BIG, -sm.BIG, sm.ODD, -sm.ODD)
    assert tuple(V[:, 5, 7]) == tuple(int(q) for q in L["side"][96 + 28:96 + 30]) + (0, 0)
    assert [int(info[6, cx] >> 24) for cx in (0, 2, 4, 6, 8)] == [1, 2, 3, 0, 1]
    assert tuple(V[:, 6, 0]) == (0, 0, 0, 0) and tuple(V[:, 6, 2]) == (sm.BIG, -sm.ODD, 0, 0) and tuple(V[:, 6, 6]) == (0, 0, -sm.ODD, sm.BIG)
    assert (info[6, 0] & 0xFFFF) == 2 | 0xFF << 8 and (info[6, 8] >> 16) & 0xFF == sm.INTER | sm.GPM
    assert info[8, 0] == 4 | 5 << 8 | (sm.INTER | sm.AFFINE | sm.PROF) << 16 | 2 << 24
    assert tuple(V[:, 9, 3]) == tuple(int(q) for q in L["side"][160 + 28:160 + 30]) + (0, 0)
    assert info[8, 5] == 4 | 0xFF << 8 | (sm.INTER | sm.AFFINE) << 16 | 1 << 24 and not V[:, 8, 5].any()
    assert info[8, 4] == sm.EMPTY and not cov[8, 4]
    # 2049 / 16: F32 keeps it, F16 rounds it (to even: 128.0625 -> 128.0)
    f32, _ = sm.field(w, h, L, sm.F32)
    f16, _ = sm.field(w, h, L, sm.F16)
    assert f32[2, 0, 0] == np.float32(128.0625) and f16[2, 0, 0] == np.float16(128.0) and f16[3, 0, 0] == np.float16(-128.0)
    assert f32[0, 1, 2] == np.float32(sm.BIG / 16) and f16[0, 1, 2] == np.float16(8192.0)


def test_empty_lists_give_an_all_empty_field(lib):
    for w, h in ((72, 40), (5, 3)):
        L = sm.lists()
        for dtype in sm.DTYPES:
            for layout in sm.LAYOUTS:
                check_against_spec(lib, w, h, L, dtype, layout, sm.REFINED)
        vec, info, (vb, ib) = host_field(lib, w, h, L, sm.I32, sm.PLANAR, sm.UNIT)
        assert not vec[:vb].any() and (info[:ib].view(np.uint32) == sm.EMPTY).all()


def _recorded(lib, rec):
    """the five lists and the side arena of a recorder, as a spec_mvfield.lists() dict (copies)"""
    def arr(fn, dt):
        n = C.c_size_t(0)
        p = getattr(lib, fn)(rec, C.byref(n))
        return np.frombuffer(C.string_at(p, n.value * dt.itemsize), dtype=dt).copy() if n.value else np.zeros(0, dt)
    return sm.lists(arr("ovhip_rec_mc_units", sm.MC_UNIT), arr("ovhip_rec_mcx_units", sm.MC_UNIT), arr("ovhip_rec_aff_units", sm.AFF_UNIT),
                    arr("ovhip_rec_rpr_units", sm.RPR_UNIT), arr("ovhip_rec_aff_rpr_units", sm.AFFR_UNIT),
                    arr("ovhip_rec_aff_side", np.dtype("<i4")))


def _set_scales(lib, rec, scales):
    for slot, s in scales.items():
        assert capi.set_ref_scale(lib, rec, slot, s["scale_hor"], s["scale_ver"], s["ref_w"], s["ref_h"], s["col_hor"], s["col_ver"]) == 0


def test_recorder_made_units_on_scaled_references(lib):
    """prediction units and affine coding units recorded against a table with scaled slots, as tests/test_rpr_cpu.py and
    tests/test_rpr_affine_cpu.py record theirs (non-overlapping blocks on a 64x64 grid): rpr and affr units of every mix of scaled
    and unscaled lists, beside the mc and aff units of the blocks that read no scaled slot"""
    pic_w, pic_h = 1920, 1080
    sizes = [(3840, 2160), (1280, 720), (960, 540), (1920, 1080)]
    scales = scales_for(pic_w, pic_h, sizes)
    keep = []
    for kind in ("pu", "affine"):
        rec = lib.ovhip_rec_create(pic_w, pic_h)
        assert rec
        try:
            assert lib.ovhip_rec_set_rpr_tools(rec, capi.RPR_TOOL_AFFINE | capi.RPR_TOOL_PU4x4) == 0
            _set_scales(lib, rec, scales)
            if kind == "pu":
                for pu in random_pus(pic_w, pic_h, len(sizes), 200, seed=7):
                    assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu))) > 0, lib.ovhip_rec_refusal(rec)
            else:
                for cu in random_affine_cus(pic_w, pic_h, len(sizes), 220, seed=31):
                    assert lib.ovhip_rec_affine_cu(rec, C.byref(G.affine_desc(capi, cu, keep))) > 0, lib.ovhip_rec_refusal(rec)
            L = _recorded(lib, rec)
        finally:
            lib.ovhip_rec_destroy(rec)
        if kind == "pu":
            assert len(L["rpr"]) > 100 and len(L["mc"]) > 10
            assert {int(f) & 3 for f in L["rpr"]["flags"]} == {1, 2, 3}
        else:
            assert len(L["affr"]) > 100 and len(L["aff"]) > 10 and len(L["side"])
            assert {int(f) & 3 for f in L["affr"]["flags"]} == {1, 2, 3}
        _, info, cov = sm.dense(pic_w, pic_h, L)
        assert {int(s) for s in np.unique(info[cov] >> 24)} == {0, 1, 2, 3}
        for dtype, layout in ((sm.I32, sm.CELLS), (sm.F16, sm.PLANAR), (sm.F32, sm.PLANAR)):
            check_against_spec(lib, pic_w, pic_h, L, dtype, layout, sm.UNIT)


def test_recorder_made_units_of_the_committed_cases(lib):
    """the reference's own cases (tests/golden/rpr): each coding unit recorded alone, as the tests of the recorder do"""
    pic_w, pic_h, sizes, _refs, cases, _ = G.load()
    keep, n_affr, n_rpr = [], 0, 0
    for c in cases[:40]:
        rec = lib.ovhip_rec_create(pic_w, pic_h)
        try:
            assert lib.ovhip_rec_set_rpr_tools(rec, capi.RPR_TOOL_AFFINE | capi.RPR_TOOL_PU4x4) == 0
            _set_scales(lib, rec, rpr_golden.scales(pic_w, pic_h, sizes, c["col"]))
            assert lib.ovhip_rec_affine_cu(rec, C.byref(G.affine_desc(capi, c["cu"], keep))) > 0, lib.ovhip_rec_refusal(rec)
            L = _recorded(lib, rec)
        finally:
            lib.ovhip_rec_destroy(rec)
        n_affr += len(L["affr"])
        check_against_spec(lib, pic_w, pic_h, L, sm.I32, sm.CELLS, sm.UNIT)
    pic_w, pic_h, sizes, _refs, cases = rpr_golden.load()
    for c in [c for c in cases if rpr_golden.is_rpr(c, pic_w, pic_h, sizes) and not c["pu"].get("refine")][:40]:
        rec = lib.ovhip_rec_create(pic_w, pic_h)
        try:
            _set_scales(lib, rec, rpr_golden.scales(pic_w, pic_h, sizes, c["col"]))
            assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, c["pu"]))) > 0, lib.ovhip_rec_refusal(rec)
            L = _recorded(lib, rec)
        finally:
            lib.ovhip_rec_destroy(rec)
        n_rpr += len(L["rpr"])
        check_against_spec(lib, pic_w, pic_h, L, sm.F32, sm.PLANAR, sm.UNIT)
    assert n_affr > 20 and n_rpr > 20


def test_refusals_write_nothing(lib):
    w, h = sm.DIRECTED_SIZE
    L = sm.directed_lists()
    ok = engine.mvfield_format(sm.F16, sm.CELLS, sm.REFINED)
    vb, ib = sm.sizes(w, h, sm.F16)
    vec = np.full(vb + TAIL, sm.FILL, np.uint8)
    info = np.full(ib + TAIL, sm.FILL, np.uint8)
    both = np.full(vb + ib, sm.FILL, np.uint8)
    src, keep = c_src(L)
    V, I = vec.ctypes.data, info.ctypes.data

    def fmt(dtype=sm.F16, layout=sm.CELLS, vectors=sm.REFINED, rsv=0):
        f = engine.mvfield_format(dtype, layout, vectors)
        f.rsv = rsv
        return f

    def altered(**kw):
        s, _ = c_src(L)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def shifted(field, **kw):
        """the directed lists with the first unit of one list changed"""
        M = dict(L)
        M[field] = L[field].copy()
        for k, v in kw.items():
            M[field][k][0] = v
        return c_src(M)

    unaligned, k1 = shifted("mc", x=2)
    unaligned_h, k2 = shifted("rpr", h=6)
    twice, k3 = shifted("mcx", x=0, y=0)                       # onto the first mc unit's cells
    twice_aff, k4 = shifted("affr", x=28, y=4)                 # onto a refined unit's
    cases = [
        ("null format", w, h, src, None, V, vb, I, ib),
        ("both NULL", w, h, src, ok, None, vb, None, ib),
        ("null source", w, h, None, ok, V, vb, I, ib),
        ("size", 0, h, src, ok, V, vb, I, ib), ("size", w, -8, src, ok, V, vb, I, ib),
        ("size", 16385, h, src, ok, V, 1 << 40, I, 1 << 40), ("size", w, 16388, src, ok, V, 1 << 40, I, 1 << 40),
        ("dtype", w, h, src, fmt(dtype=3), V, 2 * vb, I, ib), ("layout", w, h, src, fmt(layout=2), V, vb, I, ib),
        ("vectors", w, h, src, fmt(vectors=2), V, vb, I, ib), ("rsv", w, h, src, fmt(rsv=1), V, vb, I, ib),
        ("alignment", w, h, src, ok, V + 1, vb, I, ib), ("alignment", w, h, src, fmt(dtype=sm.I32), V + 2, 2 * vb, I, ib),
        ("alignment", w, h, src, ok, V, vb, I + 2, ib),
        ("too small", w, h, src, ok, V, vb - 1, I, ib), ("too small", w, h, src, ok, V, vb, I, ib - 1),
        ("too small", w, h, src, fmt(dtype=sm.F32), V, vb, I, ib),
        ("overlap", w, h, src, ok, both.ctypes.data, vb, both.ctypes.data + vb - 4, ib),
        ("overlap", w, h, src, ok, both.ctypes.data + ib - 2, vb, both.ctypes.data, ib),
        ("count without array", w, h, altered(mc=None), ok, V, vb, I, ib), ("count without array", w, h, altered(mcx=None), ok, V, vb, I, ib),
        ("count without array", w, h, altered(aff=None), ok, V, vb, I, ib), ("count without array", w, h, altered(rpr=None), ok, V, vb, I, ib),
        ("count without array", w, h, altered(affr=None), ok, V, vb, I, ib), ("count without array", w, h, altered(side=None), ok, V, vb, I, ib),
        ("refined without array", w, h, altered(refined=None), ok, V, vb, I, ib),
        ("not 4-aligned", w, h, unaligned, ok, V, vb, I, ib), ("not 4-aligned", w, h, unaligned_h, ok, V, vb, I, ib),
        ("covered twice", w, h, twice, ok, V, vb, I, ib), ("covered twice", w, h, twice_aff, ok, V, vb, I, ib),
    ]
    for what, ww, hh, s, f, pv, nv, pi, ni in cases:
        r = lib.ovhip_mvfield_host(ww, hh, C.byref(s) if s is not None else None, C.byref(f) if f is not None else None, pv, nv, pi, ni)
        assert r == EINVAL, (what, r)
        assert (vec == sm.FILL).all() and (info == sm.FILL).all() and (both == sm.FILL).all(), what
    # what is refused above is accepted once it is put right: no refined array is needed without REFINED, or without mcx units
    assert lib.ovhip_mvfield_host(w, h, C.byref(altered(refined=None)), C.byref(fmt(vectors=sm.UNIT)), V, vb, I, ib) == 0
    assert lib.ovhip_mvfield_host(w, h, C.byref(altered(refined=None, mcx=None, n_mcx=0)), C.byref(ok), V, vb, I, ib) == 0
    # adjacent destinations do not overlap
    assert lib.ovhip_mvfield_host(w, h, C.byref(src), C.byref(ok), both.ctypes.data, vb, both.ctypes.data + vb, ib) == 0
    assert not (both == sm.FILL).all()
    del keep, k1, k2, k3, k4


def test_dry_frame_accepts_the_setter_and_writes_nothing(built_lib):
    """a DPB on a counting memory back-end (no device): the setting is taken, the picture is submitted and published as before; the
    setter's own refusals come back from a dry frame too; a null frame or stream is refused"""
    from test_dpb_cpu import FakeMem
    lib = built_lib
    mem, h, f = FakeMem(), C.c_void_p(), C.c_void_p()
    assert lib.ovhip_dpb_create_ex(C.byref(h), 1, C.byref(mem.ops)) == 0
    assert lib.ovhip_frame_create(h, 0, 64, 64, C.byref(f)) == 0
    fmt = engine.mvfield_format(sm.F32, sm.CELLS, sm.REFINED)
    vb, ib = sm.sizes(64, 64, sm.F32)
    vec, info = np.full(vb, sm.FILL, np.uint8), np.full(ib, sm.FILL, np.uint8)
    assert lib.ovhip_frame_set_mvfield_output(f, C.byref(fmt), vec.ctypes.data, vb, info.ctypes.data, ib) == 0
    assert lib.ovhip_frame_set_mvfield_output(f, C.byref(fmt), None, 0, info.ctypes.data, ib) == 0
    assert lib.ovhip_frame_set_mvfield_output(f, C.byref(fmt), None, 0, None, 0) == EINVAL
    assert lib.ovhip_frame_set_mvfield_output(f, C.byref(engine.mvfield_format(3)), vec.ctypes.data, vb, info.ctypes.data, ib) == EINVAL
    assert lib.ovhip_frame_set_mvfield_output(f, C.byref(fmt), vec.ctypes.data + 1, vb, info.ctypes.data, ib) == EINVAL
    assert lib.ovhip_frame_set_mvfield_output(f, C.byref(fmt), vec.ctypes.data, vb, vec.ctypes.data + 8, ib) == EINVAL
    assert lib.ovhip_frame_begin_tag(f, C.c_void_p(0x10), 1) == 0
    p = capi.JobParams()
    assert lib.ovhip_frame_submit(f, None, None, C.byref(p), None) == 0
    assert (vec == sm.FILL).all() and (info == sm.FILL).all()
    dev, pic = C.c_int(-1), capi.Pic()
    assert lib.ovhip_dpb_lookup(h, C.c_void_p(0x10), C.byref(dev), C.byref(pic)) == 0 and (pic.w, pic.h) == (64, 64)
    assert lib.ovhip_frame_set_mvfield_output(f, None, None, 0, None, 0) == 0                   # off
    assert lib.ovhip_frame_set_mvfield_output(None, C.byref(fmt), vec.ctypes.data, vb, info.ctypes.data, ib) == EINVAL
    assert lib.ovhip_stream_set_mvfield_output(None, C.byref(fmt), vec.ctypes.data, vb, info.ctypes.data, ib, 1) == EINVAL
    assert lib.ovhip_job_mvfield(None, C.byref(fmt), vec.ctypes.data, vb, info.ctypes.data, ib) == EINVAL
    lib.ovhip_frame_destroy(f)
    lib.ovhip_dpb_destroy(h)
