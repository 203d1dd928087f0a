"""CPU: reference picture resampling in the recorder -- the per-slot scale table, the ovhip_rpr_unit tiles it emits
(anchors, steps and filter sets equal to the numpy restatement of the reference, tests/spec_rpr.py), the cases that stay
refused, the call log, the unchanged output without a scale table, and the generated filter tables."""
import ctypes as C

import numpy as np
import pytest

from openvvc_amd import capi
import spec_rpr as S
from rpr_cases import pu_desc, random_pus, scales_for

PIC_W, PIC_H = 1920, 1080
SIZES = [(3840, 2160), (2880, 1620), (1280, 720), (960, 540), (1920, 1080), (3232, 1818), (2160, 1215)]


@pytest.fixture
def lib():
    return capi.load()


def _rec(lib, w=PIC_W, h=PIC_H):
    r = lib.ovhip_rec_create(w, h)
    assert r
    return r


def _set_scales(lib, rec, scales):
    for slot, s in scales.items():
        assert capi.set_ref_scale(lib, rec, slot, s["scale_hor"], s["scale_ver"], s["ref_w"], s["ref_h"],
                                  s["col_hor"], s["col_ver"]) == 0


def _mc_bytes(lib, rec):
    n = C.c_size_t(0)
    p = lib.ovhip_rec_mc_units(rec, C.byref(n))
    return C.string_at(p, n.value * C.sizeof(capi.McUnit)) if n.value else b""


def _rpr_bytes(lib, rec):
    n = C.c_size_t(0)
    p = lib.ovhip_rec_rpr_units(rec, C.byref(n))
    return C.string_at(p, n.value * C.sizeof(capi.RprUnit)) if n.value else b""


def test_struct_sizes():
    assert C.sizeof(capi.RprUnit) == 64 and C.sizeof(capi.RprSide) == 24 and C.sizeof(capi.RefScale) == 20
    assert capi.OVHIP_ABI_VERSION == 9


def test_filter_tables():
    assert (S.RPR_LUMA.sum(axis=2) == 64).all() and (S.RPR_CHROMA.sum(axis=2) == 64).all()
    # set 0 is the regular table; sets 3..5 are sets 0..2 with the outer taps folded in (6-tap, 4x4 blocks)
    assert (S.RPR_LUMA[0] == S.MC_LUMA[:16]).all() and (S.RPR_CHROMA[0] == S.MC_CHROMA).all()
    for s in range(3):
        f = S.RPR_LUMA[s].copy()
        f[:, 1] += f[:, 0]
        f[:, 6] += f[:, 7]
        f[:, 0] = f[:, 7] = 0
        assert (S.RPR_LUMA[s + 3] == f).all()
    # the set thresholds: up to 5/4, up to 7/4, above; +3 for 4x4
    assert [S.filter_idx(v, False) for v in (2048, 20480, 20481, 28672, 28673, 32768)] == [0, 0, 1, 1, 2, 2]
    assert S.filter_idx(32768, True) == 5


def test_no_scale_table_records_as_before(lib):
    pus = random_pus(PIC_W, PIC_H, len(SIZES), 120, seed=1)
    a, b = _rec(lib), _rec(lib)
    try:
        for pu in pus:
            assert lib.ovhip_rec_pu(a, C.byref(pu_desc(capi, pu))) > 0
        # b: a scale table that is set and then restored, then reset
        _set_scales(lib, b, scales_for(PIC_W, PIC_H, SIZES))
        for slot in range(len(SIZES)):
            assert capi.set_ref_scale(lib, b, slot) == 0
        lib.ovhip_rec_reset(b)
        for pu in pus:
            assert lib.ovhip_rec_pu(b, C.byref(pu_desc(capi, pu))) > 0
        assert _mc_bytes(lib, a) == _mc_bytes(lib, b) and _mc_bytes(lib, a)
        assert _rpr_bytes(lib, a) == b"" and _rpr_bytes(lib, b) == b""
        assert lib.ovhip_rec_refusal(a) == b""
    finally:
        lib.ovhip_rec_destroy(a)
        lib.ovhip_rec_destroy(b)


def _expected_side(pu, l, scales, pic_w, pic_h):
    slot = pu["ref1"] if l else pu["ref0"]
    mvx, mvy = (pu["mv1x"], pu["mv1y"]) if l else (pu["mv0x"], pu["mv0y"])
    pw, ph = 1 << pu["log2_w"], 1 << pu["log2_h"]
    s = scales.get(slot)
    if s is None:
        return dict(scaled=False, pos=S.clip_mv(pu["x0"], pu["y0"], pw, ph, pic_w, pic_h, mvx, mvy))
    ax, stx = S.anchor(pu["x0"], mvx, s["scale_hor"], 0, pw, s["ref_w"], 4, False)
    ay, sty = S.anchor(pu["y0"], mvy, s["scale_ver"], 0, ph, s["ref_h"], 4, True)
    add_x = (1 - s["col_hor"]) * 8 * (s["scale_hor"] - S.UNSCALED)
    add_y = (1 - s["col_ver"]) * 8 * (s["scale_ver"] - S.UNSCALED)
    cx, _ = S.anchor(pu["x0"] >> 1, mvx, s["scale_hor"], add_x, pw >> 1, s["ref_w"] >> 1, 5, False)
    cy, _ = S.anchor(pu["y0"] >> 1, mvy, s["scale_ver"], add_y, ph >> 1, s["ref_h"] >> 1, 5, True)
    filt = S.filter_idx(s["scale_hor"], False) | S.filter_idx(s["scale_ver"], False) << 4
    return dict(scaled=True, pos=(ax, ay), cpos=(cx, cy), step=(stx, sty), filt=filt)


@pytest.mark.parametrize("pic,far,cols", [((1920, 1080), False, (0, 0)), ((1920, 1080), True, (1, 1)),
                                          ((3840, 2160), True, (0, 1))])
def test_units_match_restatement(lib, pic, far, cols):
    pic_w, pic_h = pic
    sizes = [(pic_w * 2, pic_h * 2), (pic_w * 3 // 2, pic_h * 3 // 2), (pic_w * 2 // 3, pic_h * 2 // 3), (pic_w // 2, pic_h // 2),
             (pic_w, pic_h), (pic_w // 8, pic_h // 8), (pic_w * 5 // 4, pic_h * 5 // 4)]
    scales = scales_for(pic_w, pic_h, sizes, cols)
    pus = random_pus(pic_w, pic_h, len(sizes), 200, seed=7 + far, far=far)
    if far:   # vectors that make the int32 ref_pos wrap at 4K with a 2:1 reference
        pus.append(dict(x0=pic_w - 64, y0=pic_h - 64, log2_w=6, log2_h=6, inter_dir=1, ref0=0, ref1=0, mv0x=1 << 17,
                        mv0y=1 << 17, mv1x=0, mv1y=0, bcw_idx_plus1=0, poc0=1, poc1=2))
    rec = _rec(lib, pic_w, pic_h)
    try:
        _set_scales(lib, rec, scales)
        n_rpr = 0
        for pu in pus:
            before = len(capi.rpr_units(lib, rec))
            assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu))) > 0, lib.ovhip_rec_refusal(rec)
            units = capi.rpr_units(lib, rec)[before:]
            d = pu["inter_dir"]
            if d == 3 and pu["poc0"] == pu["poc1"] and pu["mv0x"] == pu["mv1x"] and pu["mv0y"] == pu["mv1y"]:
                d = 2
            used = [l for l in (0, 1) if d & (1 << l)]
            if not any((pu["ref1"] if l else pu["ref0"]) in scales for l in used):
                assert not units
                continue
            pw, ph = 1 << pu["log2_w"], 1 << pu["log2_h"]
            assert len(units) == (pw // min(pw, 16)) * (ph // min(ph, 16))
            n_rpr += len(units)
            for u in units:
                assert (u.x - u.ox, u.y - u.oy) == (pu["x0"], pu["y0"]) and u.dir == d
                for l in used:
                    e, s = _expected_side(pu, l, scales, pic_w, pic_h), u.s[l]
                    assert bool(u.flags & (1 << l)) == e["scaled"]
                    assert (s.pos_x, s.pos_y) == tuple(e["pos"])
                    if e["scaled"]:
                        assert (s.cpos_x, s.cpos_y) == e["cpos"] and (s.step_x, s.step_y) == e["step"]
                        assert s.filt == e["filt"] and s.filt_c == e["filt"]
        assert n_rpr > 50
    finally:
        lib.ovhip_rec_destroy(rec)


def test_anchor_wraps_like_int32(lib):
    # 4K picture, 2:1 reference, PU at (3776, 2096), mv = (2^17, 2^17):
    #   x: ((3776 << 4) + 2^17) * 32768 + 128 = 6274678912 -> 1979711616 in int32 (inside the clip range, kept)
    #   y: ((2096 << 4) + 2^17) * 32768 + 128 = 5393875072 -> 1098907776 in int32 (kept)
    # without the wrap both would exceed (ref + 3) << 18 and clip there instead
    assert ((3776 << 4) + (1 << 17)) * 32768 + 128 - (1 << 32) == 1979711616
    assert ((2096 << 4) + (1 << 17)) * 32768 + 128 - (1 << 32) == 1098907776
    assert S.anchor(3776, 1 << 17, 32768, 0, 64, 7680, 4, False) == (1979711616, 32768)
    assert S.anchor(2096, 1 << 17, 32768, 0, 64, 4320, 4, True) == (1098907776, 32768)
    rec = _rec(lib, 3840, 2160)
    try:
        assert capi.set_ref_scale(lib, rec, 0, 32768, 32768, 7680, 4320) == 0
        pu = dict(x0=3776, y0=2096, log2_w=6, log2_h=6, inter_dir=1, ref0=0, ref1=0, mv0x=1 << 17, mv0y=1 << 17, mv1x=0, mv1y=0,
                  bcw_idx_plus1=0, poc0=1, poc1=2)
        assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu))) > 0
        u = capi.rpr_units(lib, rec)[0]
        assert (u.s[0].pos_x, u.s[0].pos_y) == (1979711616, 1098907776)
    finally:
        lib.ovhip_rec_destroy(rec)


def test_restatement_equals_reference():
    """tests/golden/rpr/rpr.ovg: the reference's own rcn_mcp_b on scaled references (GPM cases: rcn_gpm_b, which the restatement
    does not model -- they are checked against the reference on the GPU)."""
    import rpr_golden
    pic_w, pic_h, sizes, refs, cases = rpr_golden.load()
    n = 0
    for c in cases:
        if c["pu"]["refine"] or not rpr_golden.is_rpr(c, pic_w, pic_h, sizes):
            continue
        got = S.predict_pu(refs, rpr_golden.scales(pic_w, pic_h, sizes, c["col"]), pic_w, pic_h, c["pu"])
        for a, b in zip(got, c["exp"]):
            assert np.array_equal(a, b), c["pu"]
        n += 1
    assert n > 80 and len(cases) - n > 5


def test_recorder_on_reference_cases(lib):
    """The recorder fed the fixture's descriptors with the scale table set: one unit per <=16x16 tile, anchors / steps / filter
    sets equal to the restatement's (which equals the reference's samples, test above)."""
    import rpr_golden
    pic_w, pic_h, sizes, refs, cases = rpr_golden.load()
    for c in (c for c in cases if rpr_golden.is_rpr(c, pic_w, pic_h, sizes)):
        sc = rpr_golden.scales(pic_w, pic_h, sizes, c["col"])
        rec = _rec(lib, pic_w, pic_h)
        try:
            _set_scales(lib, rec, sc)
            pu = c["pu"]
            assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu))) > 0, lib.ovhip_rec_refusal(rec)
            units = capi.rpr_units(lib, rec)
            pw, ph = 1 << pu["log2_w"], 1 << pu["log2_h"]
            assert len(units) == (pw // min(pw, 16)) * (ph // min(ph, 16)) and not _mc_bytes(lib, rec)
            for u in units:
                for l in (0, 1):
                    if not u.dir & (1 << l):
                        continue
                    e = _expected_side(pu, l, sc, pic_w, pic_h)
                    assert (u.s[l].pos_x, u.s[l].pos_y) == tuple(e["pos"])
                    if e["scaled"]:
                        assert (u.s[l].cpos_x, u.s[l].cpos_y) == e["cpos"] and u.s[l].filt == e["filt"]
        finally:
            lib.ovhip_rec_destroy(rec)


def test_rpr_taps_header_matches_the_reference_probe():
    """vvc_rpr_taps.h is what tools/rpr_golden/gen_rpr_taps.c prints; re-run the probe where the compiled reference exists."""
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    if not (root / "oracle" / "_ref" / "libovvcref.so").exists():
        pytest.skip("compiled reference not present")
    subprocess.check_call(["make", "-s", "-C", str(root / "tools" / "rpr_golden"), "_build/gen_rpr_taps"])
    out = subprocess.check_output([str(root / "tools" / "rpr_golden" / "_build" / "gen_rpr_taps")])
    assert out == (root / "openvvc_amd" / "csrc" / "vvc_rpr_taps.h").read_bytes()


def test_gpm_units_carry_the_gpm_plane(lib):
    base = dict(x0=64, y0=128, log2_w=5, log2_h=4, inter_dir=3, ref0=0, ref1=1, mv0x=37, mv0y=-21, mv1x=-90, mv1y=13,
                bcw_idx_plus1=0, poc0=5, poc1=6, refine=4)
    for split in (0, 7, 18, 33, 63):
        pu = dict(base, gpm_split_dir=split)
        a, b = _rec(lib), _rec(lib)
        try:
            assert lib.ovhip_rec_pu(a, C.byref(pu_desc(capi, pu))) > 0
            _set_scales(lib, b, scales_for(PIC_W, PIC_H, [(3840, 2160), (1920, 1080)]))
            assert lib.ovhip_rec_pu(b, C.byref(pu_desc(capi, pu))) > 0
            n = C.c_size_t(0)
            p = lib.ovhip_rec_mc_units(a, C.byref(n))
            mc = (capi.McUnit * n.value).from_address(p)
            rpr = capi.rpr_units(lib, b)
            assert len(rpr) == n.value and _mc_bytes(lib, b) == b""
            for m, u in zip(mc, rpr):
                assert (m.x, m.y, m.w, m.h, m.aux) == (u.x, u.y, u.w, u.h, u.aux)
                assert u.flags & capi.RPR_GPM and u.flags & capi.RPR_S0 and not u.flags & capi.RPR_S1
                assert (u.s[1].pos_x, u.s[1].pos_y) == (m.mv1x, m.mv1y)     # the unscaled side: clip_mv as the GPM path
        finally:
            lib.ovhip_rec_destroy(a)
            lib.ovhip_rec_destroy(b)


def _refused(lib, rec, call, reason):
    assert call() == -5
    assert reason in lib.ovhip_rec_refusal(rec).decode()


def test_refused_cases(lib):
    rec = _rec(lib)
    try:
        _set_scales(lib, rec, scales_for(PIC_W, PIC_H, [(3840, 2160), (1920, 1080)]))
        pu = dict(x0=64, y0=64, log2_w=4, log2_h=4, inter_dir=3, ref0=0, ref1=1, mv0x=3, mv0y=5, mv1x=-3, mv1y=-5, poc0=1, poc1=3)
        for refine in (1, 2, 3):
            _refused(lib, rec, lambda: lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, dict(pu, refine=refine)))), "DMVR / BDOF")
        # affine CUs: both entry points (the whole-CU call of a recorder-friendly caller and the sub-block collection)
        mv = (C.c_int32 * 128)(*([7, -9] * 64))
        aff = capi.AffineDesc(x0=32, y0=32, log2_w=4, log2_h=4, inter_dir=1, ref0=0, ref1=1, poc0=1, poc1=2, mv_stride=4,
                              mv0=C.cast(mv, C.c_void_p), mv1=C.cast(mv, C.c_void_p))
        _refused(lib, rec, lambda: lib.ovhip_rec_affine_cu(rec, C.byref(aff)), "affine")
        _refused(lib, rec, lambda: lib.ovhip_rec_cu_inter(rec, None, C.byref(aff)), "affine")
        for prof in (1, 3):
            aff.inter_dir, aff.prof_dir = 3, prof
            _refused(lib, rec, lambda: lib.ovhip_rec_cu_inter(rec, None, C.byref(aff)), "affine")
        # an affine CU on unscaled slots still records
        aff.ref0 = aff.ref1 = 1
        assert lib.ovhip_rec_affine_cu(rec, C.byref(aff)) > 0
        # scale 1 on a reference of another size
        assert capi.set_ref_scale(lib, rec, 2, S.UNSCALED, S.UNSCALED, 1280, 720) == 0
        _refused(lib, rec, lambda: lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, dict(pu, inter_dir=1, ref0=2)))), "scale 1")
        # scales outside 1/8 .. 2 are malformed
        assert capi.set_ref_scale(lib, rec, 3, 2 * S.UNSCALED + 1, S.UNSCALED, 3900, 1080) == -3
        assert capi.set_ref_scale(lib, rec, 3, S.UNSCALED // 8 - 1, S.UNSCALED, 200, 1080) == -3
        lib.ovhip_rec_reset(rec)
        assert lib.ovhip_rec_refusal(rec) == b""
        assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, dict(pu, refine=1)))) > 0     # reset: unscaled again
    finally:
        lib.ovhip_rec_destroy(rec)


def test_calllog_replays_byte_identically(lib):
    rec, rep = _rec(lib), _rec(lib)
    log = lib.ovhip_calllog_create()
    try:
        lib.ovhip_rec_set_calllog(rec, log)
        _set_scales(lib, rec, scales_for(PIC_W, PIC_H, SIZES, (1, 0)))
        assert capi.set_ref_scale(lib, rec, 1) == 0                       # a restored slot is logged too
        for pu in random_pus(PIC_W, PIC_H, len(SIZES), 80, seed=3):
            assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu))) > 0
        n = C.c_size_t(0)
        p = lib.ovhip_calllog_data(log, C.byref(n))
        assert lib.ovhip_calllog_replay(p, n.value, rep) > 0
        assert _rpr_bytes(lib, rec) == _rpr_bytes(lib, rep) and _rpr_bytes(lib, rec)
        assert _mc_bytes(lib, rec) == _mc_bytes(lib, rep)
    finally:
        lib.ovhip_rec_set_calllog(rec, None)
        lib.ovhip_calllog_destroy(log)
        lib.ovhip_rec_destroy(rec)
        lib.ovhip_rec_destroy(rep)


def test_rpr_fixture_regenerates_from_the_reference(tmp_path):
    """tests/golden/rpr/rpr.ovg is what tools/rpr_golden/gen_rpr.c writes (every case run twice over differently poisoned
    scratch buffers); re-run it where the compiled reference exists."""
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    if not (root / "oracle" / "_ref" / "libovvcref.so").exists():
        pytest.skip("compiled reference not present")
    subprocess.check_call(["make", "-s", "-C", str(root / "tools" / "rpr_golden"), "_build/gen_rpr"])
    subprocess.check_call([str(root / "tools" / "rpr_golden" / "_build" / "gen_rpr"), str(tmp_path)], stderr=subprocess.DEVNULL)
    assert (tmp_path / "rpr.ovg").read_bytes() == (root / "tests" / "golden" / "rpr" / "rpr.ovg").read_bytes()
