"""The intra-block-copy scenarios of tests/golden/ibc (spec_ibc.Scenario) as recorder calls: shared by test_ibc_cpu.py and test_gpu_ibc.py."""
import ctypes as C

import numpy as np

import spec_ibc as S
from openvvc_amd import capi


def tu_state(sc: S.Scenario, chroma_scale=None) -> capi.TuState:
    st = capi.TuState.from_buffer_copy(sc.state)
    if chroma_scale is not None:          # LMCS chroma residual scaling with a constant scale (rcn_init_ict_functions type 1)
        st.ict_type, st.lmcs_scale_c, st.lmcs_chroma_scale = 1, 1, chroma_scale
    return st


def ibc_desc(sc: S.Scenario, i: int, win_x0: int = 0) -> capi.IbcDesc:
    cu = sc.cu[i]
    return capi.IbcDesc(int(cu[S.CU_X0]), int(cu[S.CU_Y0]), int(cu[S.CU_L2W]), int(cu[S.CU_L2H]), sc.log2_ctu, int(cu[S.CU_CHROMA]),
                        int(cu[S.CU_MVX]), int(cu[S.CU_MVY]), win_x0, 0)


def tu_desc(sc: S.Scenario, t: int) -> capi.TuDesc:
    """ovhip_tu_desc of transform unit t; the coefficient pointers go into sc.coef (which the scenario keeps alive)"""
    tu = sc.tu[t]
    d = capi.TuDesc()
    d.x0, d.y0, d.log2_tb_w, d.log2_tb_h, d.tree = int(tu[S.TU_X0]), int(tu[S.TU_Y0]), int(tu[S.TU_L2W]), int(tu[S.TU_L2H]), int(tu[S.TU_TREE])
    d.cbf_mask, d.tr_skip_mask, d.cu_flags = int(tu[S.TU_CBF]), int(tu[S.TU_TS]), S.FLG_IBC
    for k in range(3):
        d.last_pos[k], d.sig_sb_map[k] = int(tu[S.TU_LAST + k]), int(sc.map[t][k])
        off = int(tu[S.TU_COEF + k])
        d.coef[k] = sc.coef.ctypes.data + 2 * off if off >= 0 else None
    return d


def record(rec: capi.Recorder, sc: S.Scenario, cus=None, chroma_scale=None) -> int:
    """Every TU of the CUs (indices; default all, in decoding order) through ovhip_rec_tu_ibc; returns the commands appended."""
    st, n = tu_state(sc, chroma_scale), 0
    if sc.log2_ctu != 7:
        assert rec.lib.ovhip_rec_set_ctu_size(rec.h, sc.log2_ctu) == 0
    for i in (range(len(sc.cu)) if cus is None else cus):
        cu = ibc_desc(sc, i)
        for t in sc.tus_of(i):
            r = rec.tu_ibc(st, tu_desc(sc, t), cu)
            assert r >= 0, f"scenario {sc.name}: CU {i}, TU {t}: ovhip_rec_tu_ibc -> {r} ({rec.refusal()})"
            n += r
    return n


def n_tb_cmds(rec: capi.Recorder) -> int:
    n = C.c_size_t()
    rec.lib.ovhip_rec_tb_cmds(rec.h, C.byref(n))
    return n.value


def tb_cmds(rec: capi.Recorder) -> np.ndarray:
    n = C.c_size_t()
    p = rec.lib.ovhip_rec_tb_cmds(rec.h, C.byref(n))
    if not n.value:
        return np.zeros(0, capi.TB_CMD_DTYPE)
    return np.frombuffer((C.c_char * (n.value * 32)).from_address(p), dtype=capi.TB_CMD_DTYPE).copy()
