"""CPU: intra block copy -- the numpy restatement of the reference's ring against the reference-generated fixtures
(tests/golden/ibc, tools/ibc_golden/gen_ibc.c), the window in which the ring and the picture hold the same sample, and what the
recorder makes of IBC coding units: kinds, offsets, levels, residual marks, refusals, call log."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ibc_cases
import spec_ibc as S
from openvvc_amd import capi

ROOT = Path(__file__).resolve().parent.parent
RES_STORE = 16          # OVHIP_RES_STORE


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_restatement_equals_the_reference_frame(name):
    """spec_ibc.decode_ring (attach, wrap split, chroma floor, residual add + clip) == what rcn_ibc_l / rcn_ibc_c + tmp.rcn_transform_tree
    left in the frame, all three planes; c: CTU 64, ten CTUs, the ring of eight wraps."""
    sc = S.scenario(name)
    got, _ = S.decode_ring(sc)
    for p, plane in enumerate(("Y", "Cb", "Cr")):
        assert np.array_equal(got[p], sc.exp[p]), f"scenario {name}, plane {plane}: {int((got[p] != sc.exp[p]).sum())} samples differ"
    if name == "c":
        assert sc.log2_ctu == 6 and sc.w >> 6 == 10
        far = [int(cu[S.CU_X0] >> 6) - int((cu[S.CU_X0] + cu[S.CU_MVX]) >> 6) for cu in sc.cu]
        assert max(far) == 7, "a source seven CTUs left"
        assert any(int(cu[S.CU_X0] + cu[S.CU_MVX]) < 512 < int(cu[S.CU_X0] + cu[S.CU_MVX]) + (1 << int(cu[S.CU_L2W])) for cu in sc.cu), "a source across the ring's end"


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_ring_read_is_the_picture_read_and_the_check_accepts(built_lib, name):
    """For EVERY coding unit of the fixtures (none left out): the block the ring delivers is the block at (x0 + mv_x, y0 + mv_y) of the
    picture, luma and chroma (the vector halved, arithmetic), and ovhip_rec_ibc_check accepts the vector."""
    sc = S.scenario(name)
    ring, ring_reads = S.decode_ring(sc, poison=0x7e7e)
    pic, pic_reads = S.decode_picture(sc)
    rec = capi.Recorder(sc.w, sc.h)
    n = 0
    for i in range(len(sc.cu)):
        for p in range(3):
            a, b = ring_reads[i][p], pic_reads[i][p]
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), f"scenario {name}, CU {i}, plane {p}: the ring delivers another block"
        assert S.in_window(sc.cu[i], sc.log2_ctu, sc.w, sc.h)
        assert rec.ibc_check(ibc_cases.ibc_desc(sc, i)) == 0, f"scenario {name}, CU {i}: {rec.refusal()}"
        n += 1
    assert n == len(sc.cu) > 80
    for p in range(3):
        assert np.array_equal(ring[p], pic[p])
    rec.close()


def test_fixture_covers_what_it_is_for():
    sc = S.scenario("a")
    shapes = {(int(c[S.CU_L2W]), int(c[S.CU_L2H])) for c in sc.cu}
    assert {(2, 2), (2, 6), (6, 2), (3, 3), (4, 5), (6, 6)} <= shapes and sc.log2_max_tb == 5
    assert all(not c[S.CU_CHROMA] for c in sc.cu if c[S.CU_L2W] == 2 and c[S.CU_L2H] == 2)
    mv = sc.cu[:, S.CU_MVX:S.CU_MVY + 1]
    assert (mv[:, 0] & 1).any() and (mv[:, 1] & 1).any() and not (mv[:, 0] & 1).all()
    sx, x0, w = sc.cu[:, S.CU_X0] + sc.cu[:, S.CU_MVX], sc.cu[:, S.CU_X0], 1 << sc.cu[:, S.CU_L2W]
    left, cur = (sx + w - 1) >> 7 < x0 >> 7, sx >> 7 == x0 >> 7
    assert left.any() and cur.any() and (~left & ~cur).any(), "sources left of, inside and across the CTU boundary"
    assert any(c[S.CU_MVX] == -(1 << c[S.CU_L2W]) and c[S.CU_MVY] == 0 for c in sc.cu) and any(c[S.CU_MVX] == 0 and c[S.CU_MVY] == -(1 << c[S.CU_L2H]) for c in sc.cu)
    cbf = sc.tu[:, S.TU_CBF]
    assert (cbf == 0).any() and (cbf & 0x10).any() and (cbf & 0x3).any() and (sc.tu[:, S.TU_TS] != 0).any()
    b = S.scenario("b")
    assert b.h == 256 and (b.cu[:, S.CU_Y0] >= 128).any() and (b.cu[:, S.CU_Y0] < 128).any()


def _chain(sc):
    """scenario a's 32 CUs of 8x8 at row 104, each copying its left neighbour"""
    idx = [i for i in range(len(sc.cu)) if sc.cu[i][S.CU_Y0] == 104 and sc.cu[i][S.CU_L2W] == 3 and sc.cu[i][S.CU_MVX] == -8 and sc.cu[i][S.CU_MVY] == 0
           and 160 <= sc.cu[i][S.CU_X0] < 416]
    assert len(idx) == 32
    return sorted(idx, key=lambda i: int(sc.cu[i][S.CU_X0]))


def test_recorded_tasks_are_as_designed(built_lib):
    """One OVHIP_IT_IBC_L task per luma transform block and one OVHIP_IT_IBC_C per chroma pair, the CU's vector in pad[0..1] (chroma: halved,
    arithmetic), OVHIP_IF_RES_* exactly where the TU's cbf says, every transform block of the picture marked OVHIP_RES_STORE."""
    assert C.sizeof(capi.ITask) == 32 and capi.ITASK_DTYPE.itemsize == 32 and built_lib.ovhip_abi_version() == 9 == capi.OVHIP_ABI_VERSION
    sc = S.scenario("a")
    rec = capi.Recorder(sc.w, sc.h)
    n_cmd = ibc_cases.record(rec, sc)
    t = rec.itasks()
    dx, dy = capi.itask_ibc_offset(t)
    k = 0
    n_bits = 0
    for i in range(len(sc.cu)):
        cu = sc.cu[i]
        for u in sc.tus_of(i):
            tu = sc.tu[u]
            a = t[k]; k += 1
            assert (a["kind"], a["x"], a["y"], a["log2_w"], a["log2_h"]) == (capi.IT_IBC_L, tu[S.TU_X0], tu[S.TU_Y0], tu[S.TU_L2W], tu[S.TU_L2H])
            assert (dx[k - 1], dy[k - 1]) == (cu[S.CU_MVX], cu[S.CU_MVY]) and a["level"] >= 1
            assert bool(a["flags"] & capi.IF_RES_Y) == bool(tu[S.TU_CBF] & 0x10)
            n_bits += bin(int(tu[S.TU_CBF]) & 0x13).count("1")
            if cu[S.CU_CHROMA]:
                c = t[k]; k += 1
                assert (c["kind"], c["x"], c["y"], c["log2_w"], c["log2_h"]) == (capi.IT_IBC_C, tu[S.TU_X0] >> 1, tu[S.TU_Y0] >> 1, tu[S.TU_L2W] - 1, tu[S.TU_L2H] - 1)
                assert (dx[k - 1], dy[k - 1]) == (cu[S.CU_MVX] >> 1, cu[S.CU_MVY] >> 1)
                assert bool(c["flags"] & capi.IF_RES_CB) == bool(tu[S.TU_CBF] & 0x2) and bool(c["flags"] & capi.IF_RES_CR) == bool(tu[S.TU_CBF] & 0x1)
                assert not c["flags"] & capi.IF_RES_SCALE
    assert k == len(t) == rec.ibc_tasks()
    cmds = rec.tb_cmds()
    assert len(cmds) == n_cmd == n_bits and (cmds["res_mode"] & RES_STORE).all()
    # a CU wider than the maximum transform size: four tasks (and four chroma tasks) with the CU's vector
    big = [i for i in range(len(sc.cu)) if sc.cu[i][S.CU_L2W] == 6 and sc.cu[i][S.CU_L2H] == 6]
    assert big and all(len(sc.tus_of(i)) == 4 for i in big)
    # the flag of a task none of whose source units has an ordered writer: exactly the tasks of level 1
    ibc = t[t["kind"] >= capi.IT_IBC_L]
    assert np.array_equal((ibc["flags"] & capi.IF_IBC_FREE) != 0, ibc["level"] == 1) and (ibc["level"] == 1).any() and (ibc["level"] > 1).any()
    rec.close()


def test_chain_gets_strictly_rising_levels(built_lib):
    sc = S.scenario("a")
    rec = capi.Recorder(sc.w, sc.h)
    ibc_cases.record(rec, sc)
    t = rec.itasks()
    for kind, sh in ((capi.IT_IBC_L, 0), (capi.IT_IBC_C, 1)):
        lv = []
        for i in _chain(sc):
            m = (t["kind"] == kind) & (t["x"] == sc.cu[i][S.CU_X0] >> sh) & (t["y"] == 104 >> sh)
            assert m.sum() == 1
            lv.append(int(t[m][0]["level"]))
        assert all(b == a + 1 for a, b in zip(lv, lv[1:])), lv
    rec.close()


def _ibc_tu(rec, x0, y0, l2, mvx, mvy, chroma=1):
    st = capi.TuState()
    d = capi.TuDesc()
    d.x0, d.y0, d.log2_tb_w, d.log2_tb_h, d.tree, d.cu_flags = x0, y0, l2, l2, 0 if chroma else 1, S.FLG_IBC
    return rec.tu_ibc(st, d, capi.IbcDesc(x0, y0, l2, l2, 7, chroma, mvx, mvy, 0, 0))


def _intra_tu(rec, x0, y0, l2, avl_lft=0, avl_abv=0):
    st = capi.TuState()
    d = capi.TuDesc()
    d.x0, d.y0, d.log2_tb_w, d.log2_tb_h, d.tree, d.cu_flags = x0, y0, l2, l2, 1, 2
    tl = capi.ITask()
    tl.kind, tl.x, tl.y, tl.log2_w, tl.log2_h, tl.mode, tl.avl_lft, tl.avl_abv = capi.IT_LUMA, x0, y0, l2, l2, 1, avl_lft, avl_abv
    return rec.tu_intra(st, d, tl, None)


def test_levels_between_intra_and_ibc_tasks(built_lib):
    """An IBC task copying an intra task's block runs one level after it; an intra task whose reference arm touches an IBC block runs after
    that block."""
    rec = capi.Recorder(256, 128)
    _intra_tu(rec, 64, 0, 4)                                   # level 1
    _intra_tu(rec, 80, 0, 4, avl_lft=4)                        # its left arm is the first block: level 2
    assert _ibc_tu(rec, 128, 0, 4, -50, 3, chroma=0) == 0      # source (78..94, 3..19): both intra blocks -> level 3
    _intra_tu(rec, 144, 0, 4, avl_lft=4)                       # left arm = the IBC block's last column -> level 4
    assert _ibc_tu(rec, 160, 32, 4, -160, 0, chroma=0) == 0    # source: nothing ordered -> level 1
    t = rec.itasks()
    assert [int(v) for v in t["level"]] == [1, 2, 3, 4, 1]
    assert [int(v) for v in t["kind"]] == [capi.IT_LUMA, capi.IT_LUMA, capi.IT_IBC_L, capi.IT_LUMA, capi.IT_IBC_L]
    assert not t[2]["flags"] & capi.IF_IBC_FREE and t[4]["flags"] & capi.IF_IBC_FREE
    # the task of the left CTU is the IBC task's dependency for the CTU grouping (bit 0: left)
    assert t[2]["ctu_deps"] & 0x8001 == 0x8001
    rec.close()


REFUSED = [("other CTU row", 128, 128, 4, 0, -16), ("left of win_x0", 128, 0, 4, -100, 0), ("left of the ring", 384, 0, 4, -272, 0),
           ("right of the current CTU", 96, 32, 4, 24, -32), ("outside the picture", 128, 160, 4, -32, 32), ("overlapping the CU", 128, 32, 4, -8, 8)]


@pytest.mark.parametrize("rule,x0,y0,l2,mvx,mvy", REFUSED)
def test_vectors_outside_the_window_are_refused(built_lib, rule, x0, y0, l2, mvx, mvy):
    """One vector per rule of the window: OVHIP_EUNSUP, a reason, and the recorder as it was (no task, no command)."""
    rec = capi.Recorder(512, 200)
    assert _ibc_tu(rec, 0, 0, 3, 8, 0) == 0 and _ibc_tu(rec, 200, 0, 3, -8, 0) == 0
    n_task, n_cmd = len(rec.itasks()), len(rec.tb_cmds())
    cu = capi.IbcDesc(x0, y0, l2, l2, 7, 1, mvx, mvy, 64 if rule == "left of win_x0" else 0, 0)
    assert rec.ibc_check(cu) == capi.OVHIP_EUNSUP, rule
    why = rec.refusal()
    assert why.startswith("IBC: ")
    st, d = capi.TuState(), capi.TuDesc()
    d.x0, d.y0, d.log2_tb_w, d.log2_tb_h, d.cu_flags, d.cbf_mask = x0, y0, l2, l2, S.FLG_IBC, 0
    assert rec.tu_ibc(st, d, cu) == capi.OVHIP_EUNSUP and rec.refusal() == why
    assert len(rec.itasks()) == n_task == rec.ibc_tasks() and len(rec.tb_cmds()) == n_cmd
    # the same CU with a vector inside the window is taken
    ok = {"other CTU row": (-16, 0), "left of win_x0": (-64, 0), "left of the ring": (-128, 0), "right of the current CTU": (16, -32),
          "outside the picture": (-16, 0), "overlapping the CU": (-16, 8)}[rule]
    cu.mv_x, cu.mv_y = ok
    assert rec.ibc_check(cu) == 0, (rule, rec.refusal())
    rec.close()


def test_each_rule_has_its_own_reason(built_lib):
    rec = capi.Recorder(512, 200)
    seen = set()
    for rule, x0, y0, l2, mvx, mvy in REFUSED:
        assert rec.ibc_check(capi.IbcDesc(x0, y0, l2, l2, 7, 1, mvx, mvy, 64 if rule == "left of win_x0" else 0, 0)) == capi.OVHIP_EUNSUP
        seen.add(rec.refusal())
    assert len(seen) == len(REFUSED)
    rec.close()


def _records(log):
    out, o = [], 0
    while o < len(log):
        t, n = (int(v) for v in np.frombuffer(log[o:o + 8].tobytes(), np.uint32))
        out.append(t); o += 8 + n
    return out


def test_call_log_takes_a_record_kind_of_its_own(built_lib):
    """ovhip_rec_tu_ibc is serialised as record kind 11, which nothing else writes: a picture without IBC logs the kinds it always did
    (and replays to the same arrays); an IBC picture's log replays to the same tasks, commands and coefficients, byte for byte."""
    from openvvc_amd import synth
    wl = synth.make_workload(416, 240, 3, tools=synth.INTRA_TOOLS, intra_frac=0.5, calllog=True)
    assert set(_records(wl.calllog)) <= set(range(1, 11))
    rec = capi.Recorder(416, 240)
    rec.replay(wl.calllog)
    assert np.array_equal(rec.itasks(), wl.itasks) and np.array_equal(rec.coefs(), wl.coefs) and rec.ibc_tasks() == 0
    rec.close()
    sc = S.scenario("c")
    a = capi.Recorder(sc.w, sc.h)
    a.start_calllog()
    ibc_cases.record(a, sc)
    log = a.take_calllog()
    kinds = _records(log)
    assert kinds[0] == 1 and set(kinds[1:]) == {11} and len(kinds) == 1 + len(sc.tu)
    b = capi.Recorder(sc.w, sc.h)
    assert b.replay(log) == len(kinds)
    assert a.itasks().tobytes() == b.itasks().tobytes() and a.tb_cmds().tobytes() == b.tb_cmds().tobytes() and np.array_equal(a.coefs(), b.coefs())
    with pytest.raises(ValueError):
        b.reset(); b.replay(log[:len(log) - 8].copy())          # the last TU's coefficients cut short
    a.close(); b.close()


def _need_reference():
    if not (ROOT / "oracle" / "_ref" / "libovvcref.so").exists():
        pytest.skip("compiled reference not present")


def test_fixtures_regenerate_from_the_reference(tmp_path):
    """tests/golden/ibc/*.ovg are what tools/ibc_golden/gen_ibc.c writes; re-run it where the compiled reference exists."""
    _need_reference()
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "tools" / "ibc_golden"), "_build/gen_ibc"])
    subprocess.check_call([str(ROOT / "tools" / "ibc_golden" / "_build" / "gen_ibc"), str(tmp_path)], stderr=subprocess.DEVNULL)
    for f in ("ibc.ovg", "ibc_rows.ovg"):
        assert (tmp_path / f).read_bytes() == (ROOT / "tests" / "golden" / "ibc" / f).read_bytes()
        assert (ROOT / "tests" / "golden" / "ibc" / f).stat().st_size <= 1 << 20


def test_shim_slots_record_what_the_direct_call_records():
    """The generator's second mode: the fixtures' rcn_ibc_l / rcn_ibc_c / tmp.rcn_transform_tree calls through the shim's table bound to a
    recorder == direct ovhip_rec_tu_ibc calls, tasks, commands and coefficients byte for byte."""
    _need_reference()
    if not (ROOT / "shim" / "_build" / "librcn_hip.so").exists():
        pytest.skip("shim not built")
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "tools" / "ibc_golden"), "_build/gen_ibc_shim"])
    subprocess.check_call([str(ROOT / "tools" / "ibc_golden" / "_build" / "gen_ibc_shim")], stderr=subprocess.DEVNULL)
