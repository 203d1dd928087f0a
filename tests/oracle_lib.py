"""TEST INFRASTRUCTURE: ctypes access to oracle/liboracle.so (the CPU restatement).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "oracle" / "liboracle.so"


class OPic(C.Structure):
    _fields_ = [("y", C.c_void_p), ("cb", C.c_void_p), ("cr", C.c_void_p),
                ("w", C.c_int32), ("h", C.c_int32), ("stride_y", C.c_int32), ("stride_c", C.c_int32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not LIB.exists():
            subprocess.check_call(["make", "-C", str(ROOT / "oracle"), "liboracle.so"])
        _lib = C.CDLL(str(LIB))
        vp = C.c_void_p
        _lib.oracle_itx.argtypes = [C.POINTER(OPic), vp, C.c_uint32, vp]
        _lib.oracle_itx.restype = None
        _lib.oracle_mc.argtypes = [C.POINTER(OPic), C.POINTER(OPic), C.c_uint32, vp, C.c_uint32, vp]
        _lib.oracle_mc.restype = None
        _lib.oracle_mc_full.argtypes = [C.POINTER(OPic), C.POINTER(OPic), C.c_uint32, vp, C.c_uint32, vp, vp, C.POINTER(OPic)]
        _lib.oracle_mc_full.restype = None
        _lib.oracle_mc_ex.argtypes = [C.POINTER(OPic), C.POINTER(OPic), C.c_uint32, vp, C.c_uint32, vp, vp]
        _lib.oracle_mc_ex.restype = None
        _lib.oracle_mcx_trace.argtypes = [C.POINTER(OPic), C.POINTER(OPic), C.c_uint32, vp, vp, vp, C.c_int]
        _lib.oracle_mcx_trace.restype = None
        _lib.oracle_tmvp_cells.argtypes = [vp, C.c_uint32, vp, C.c_int, C.c_int, vp]
        _lib.oracle_tmvp_cells.restype = None
        _lib.oracle_itx_ex.argtypes = [C.POINTER(OPic), vp, C.c_uint32, vp, vp]
        _lib.oracle_itx_ex.restype = None
        _lib.oracle_lmcs_scale.argtypes = [C.POINTER(OPic), vp, C.c_uint32, vp, vp]
        _lib.oracle_lmcs_scale.restype = None
        _lib.oracle_lmcs_inverse.argtypes = [C.POINTER(OPic), vp]
        _lib.oracle_lmcs_inverse.restype = None
        _lib.oracle_ciip.argtypes = [C.POINTER(OPic), C.POINTER(OPic), vp, C.c_uint32]
        _lib.oracle_ciip.restype = None
        _lib.oracle_mca.argtypes = [C.POINTER(OPic), C.POINTER(OPic), C.c_uint32, vp, C.c_uint32, vp, vp]
        _lib.oracle_mca.restype = None
        _lib.oracle_dbf.argtypes = [C.POINTER(OPic), vp]
        _lib.oracle_dbf.restype = None
        _lib.oracle_dbf_edges.argtypes = [C.POINTER(OPic), vp, C.c_uint32, vp, C.c_uint32, vp]
        _lib.oracle_dbf_edges.restype = None
        _lib.oracle_sao.argtypes = [C.POINTER(OPic), C.POINTER(OPic), vp, C.c_int]
        _lib.oracle_sao.restype = None
        _lib.oracle_alf_run.argtypes = [C.POINTER(OPic), C.POINTER(OPic), vp]
        _lib.oracle_alf_run.restype = None
        _lib.oracle_itx_res.argtypes = [C.POINTER(OPic), vp, C.c_uint32, vp, vp, C.POINTER(OPic)]
        _lib.oracle_itx_res.restype = None
        _lib.oracle_intra_tasks.argtypes = [C.POINTER(OPic), vp, vp, C.c_uint32, vp, vp, vp, C.c_int]
        _lib.oracle_intra_tasks.restype = None
    return _lib


class ORes(C.Structure):
    """int16 residual planes the transform stage STOREd for the ordered tasks (oracle_res)."""
    _fields_ = [("y", C.c_void_p), ("cb", C.c_void_p), ("cr", C.c_void_p), ("stride_y", C.c_int32), ("stride_c", C.c_int32)]


def intra_tasks(pic: "HostPic", tasks: np.ndarray, res=None, regions=None, luts=None, scales=None, log2_ctu: int = 7):
    """The ordered pass: tasks (capi.ITASK_DTYPE) in recording order; res = (y, cb, cr) int16 arrays or None."""
    s = pic.struct()
    r = None
    if res is not None:
        res = [np.ascontiguousarray(a, dtype=np.int16) for a in res]
        r = ORes(res[0].ctypes.data, res[1].ctypes.data, res[2].ctypes.data, res[0].shape[1], res[1].shape[1])
    tasks = np.ascontiguousarray(tasks)
    reg = np.ascontiguousarray(regions) if regions is not None and len(regions) else None
    lib().oracle_intra_tasks(C.byref(s), C.byref(r) if r is not None else None, tasks.ctypes.data, len(tasks),
                             reg.ctypes.data if reg is not None else None, C.byref(luts) if luts is not None else None,
                             scales.ctypes.data if scales is not None else None, log2_ctu)


class HostPic:
    """Three contiguous uint16 planes in host memory + the struct the oracle takes."""

    def __init__(self, w, h, y=None, cb=None, cr=None):
        self.w, self.h = w, h
        self.y = np.ascontiguousarray(y if y is not None else np.zeros((h, w), np.uint16), dtype=np.uint16)
        self.cb = np.ascontiguousarray(cb if cb is not None else np.zeros((h // 2, w // 2), np.uint16), dtype=np.uint16)
        self.cr = np.ascontiguousarray(cr if cr is not None else np.zeros((h // 2, w // 2), np.uint16), dtype=np.uint16)
        assert self.y.shape == (h, w) and self.cb.shape == (h // 2, w // 2) and self.cr.shape == (h // 2, w // 2)

    def struct(self):
        return OPic(self.y.ctypes.data, self.cb.ctypes.data, self.cr.ctypes.data, self.w, self.h, self.w, self.w // 2)

    def copy(self):
        return HostPic(self.w, self.h, self.y.copy(), self.cb.copy(), self.cr.copy())

    def planes(self):
        return [self.y, self.cb, self.cr]


def itx(pic: HostPic, cmds: np.ndarray, coefs: np.ndarray):
    s = pic.struct()
    cmds = np.ascontiguousarray(cmds)
    coefs = np.ascontiguousarray(coefs, dtype=np.int16)
    lib().oracle_itx(C.byref(s), cmds.ctypes.data, len(cmds), coefs.ctypes.data)


def itx_ex(pic: HostPic, cmds: np.ndarray, coefs: np.ndarray, lmcs_scales: np.ndarray):
    s = pic.struct()
    cmds = np.ascontiguousarray(cmds)
    coefs = np.ascontiguousarray(coefs, dtype=np.int16)
    lmcs_scales = np.ascontiguousarray(lmcs_scales, dtype=np.int16)
    lib().oracle_itx_ex(C.byref(s), cmds.ctypes.data, len(cmds), coefs.ctypes.data, lmcs_scales.ctypes.data)


def itx_res(pic: HostPic, cmds: np.ndarray, coefs: np.ndarray, lmcs_scales, respic: HostPic):
    """Transform blocks incl. those of ordered tasks (OVHIP_RES_STORE -> respic, whose uint16 planes hold int16 bits)."""
    if not len(cmds):
        return
    cmds, coefs = np.ascontiguousarray(cmds), np.ascontiguousarray(coefs)
    s, rs = pic.struct(), respic.struct()
    sc = np.ascontiguousarray(lmcs_scales, dtype=np.int16) if lmcs_scales is not None else None
    lib().oracle_itx_res(C.byref(s), cmds.ctypes.data, len(cmds), coefs.ctypes.data, sc.ctypes.data if sc is not None else None, C.byref(rs))


def lmcs_scale(pic: HostPic, regions: np.ndarray, luts) -> np.ndarray:
    """regions: capi.LMCS_REGION_DTYPE array; luts: capi.LmcsLuts.  Returns int16 scales."""
    s = pic.struct()
    regions = np.ascontiguousarray(regions)
    out = np.zeros(len(regions), np.int16)
    lib().oracle_lmcs_scale(C.byref(s), regions.ctypes.data, len(regions), C.addressof(luts), out.ctypes.data)
    return out


def lmcs_inverse(pic: HostPic, bwd_lut: np.ndarray):
    s = pic.struct()
    bwd_lut = np.ascontiguousarray(bwd_lut, dtype=np.uint16)
    lib().oracle_lmcs_inverse(C.byref(s), bwd_lut.ctypes.data)


def mc(dst: HostPic, refs, units: np.ndarray, lmcs_fwd=None, intra: "HostPic | None" = None):
    """intra: planar-prediction picture for units that carry a fused CIIP blend (aux != 0)."""
    s = dst.struct()
    arr = (OPic * len(refs))(*[r.struct() for r in refs])
    units = np.ascontiguousarray(units)
    lut = None
    if lmcs_fwd is not None:
        lmcs_fwd = np.ascontiguousarray(lmcs_fwd, dtype=np.uint16)
        lut = lmcs_fwd.ctypes.data
    ip = intra.struct() if intra is not None else None
    lib().oracle_mc_full(C.byref(s), arr, len(refs), units.ctypes.data, len(units), lut, None, C.byref(ip) if ip else None)


def ciip(dst: HostPic, intra: HostPic, units: np.ndarray):
    d, s = dst.struct(), intra.struct()
    units = np.ascontiguousarray(units)
    lib().oracle_ciip(C.byref(d), C.byref(s), units.ctypes.data, len(units))


def mca(dst: HostPic, refs, units: np.ndarray, side: np.ndarray, lmcs_fwd=None):
    """Affine (+PROF) units."""
    s = dst.struct()
    arr = (OPic * len(refs))(*[r.struct() for r in refs])
    units = np.ascontiguousarray(units)
    side = np.ascontiguousarray(side, dtype=np.int32)
    lut = None
    if lmcs_fwd is not None:
        lmcs_fwd = np.ascontiguousarray(lmcs_fwd, dtype=np.uint16)
        lut = lmcs_fwd.ctypes.data
    lib().oracle_mca(C.byref(s), arr, len(refs), units.ctypes.data, len(units), side.ctypes.data, lut)


def mc_ex(dst: HostPic, refs, units: np.ndarray, lmcs_fwd=None) -> np.ndarray:
    """Plain + BDOF / DMVR units; returns the int32 [n, 4] motion vectors finally used."""
    s = dst.struct()
    arr = (OPic * len(refs))(*[r.struct() for r in refs])
    units = np.ascontiguousarray(units)
    lut = None
    if lmcs_fwd is not None:
        lmcs_fwd = np.ascontiguousarray(lmcs_fwd, dtype=np.uint16)
        lut = lmcs_fwd.ctypes.data
    mv = np.zeros((len(units), 4), np.int32)
    lib().oracle_mc_ex(C.byref(s), arr, len(refs), units.ctypes.data, len(units), lut, mv.ctypes.data)
    return mv


def dmvr_trace(dst: HostPic, refs, unit, true_apron: bool = False) -> "tuple[np.ndarray, np.ndarray]":
    """One refined unit through the oracle with the trace of its search and of BDOF -> (int64[115] as mc_refined_unit documents it,
    refined vector).  true_apron: the edit that reads the reference picture in place of DMVR's replicated apron."""
    s = dst.struct()
    arr = (OPic * len(refs))(*[r.struct() for r in refs])
    u = np.ascontiguousarray(np.array([unit], dtype=unit.dtype))
    trace, mv = np.zeros(115, np.int64), np.zeros(4, np.int32)
    lib().oracle_mcx_trace(C.byref(s), arr, len(refs), u.ctypes.data, mv.ctypes.data, trace.ctypes.data, int(true_apron))
    return trace, mv


def dbf_planes_struct(planes: dict):
    """planes: dict from capi.Recorder.dbf_planes() / synth (numpy uint16 arrays). Returns (struct, keepalive)."""
    from openvvc_amd import capi
    keep = {k: np.ascontiguousarray(planes[k], dtype=np.uint16) for k in capi.DBF_PLANE_NAMES}
    s = capi.DbfPlanes(*[keep[k].ctypes.data for k in capi.DBF_PLANE_NAMES], planes["w4"], planes["h4"],
                       planes["beta_offset"], planes["tc_offset"])
    return s, keep


def dbf(pic: HostPic, planes: dict):
    s = pic.struct()
    pl, keep = dbf_planes_struct(planes)
    lib().oracle_dbf(C.byref(s), C.addressof(pl))


def dbf_edges(pic: HostPic, edges_v: np.ndarray, edges_h: np.ndarray, offsets):
    """edges_*: capi.DBF_EDGE_DTYPE in the order to filter; offsets: capi.DbfOffsets."""
    s = pic.struct()
    edges_v, edges_h = np.ascontiguousarray(edges_v), np.ascontiguousarray(edges_h)
    lib().oracle_dbf_edges(C.byref(s), edges_v.ctypes.data, len(edges_v), edges_h.ctypes.data, len(edges_h), C.addressof(offsets))


def sao(dst: HostPic, src: HostPic, params: np.ndarray, log2_ctu: int = 7):
    d, s_ = dst.struct(), src.struct()
    params = np.ascontiguousarray(params)
    lib().oracle_sao(C.byref(d), C.byref(s_), params.ctypes.data, log2_ctu)


def alf(dst: HostPic, src: HostPic, alf: dict, log2_ctu: int = 7):
    from openvvc_amd import capi
    keep = [np.ascontiguousarray(alf[k], dtype=dt) for k, dt in capi.ALF_TABLES]
    scratch = np.zeros(((src.w + 3) // 4) * ((src.h + 3) // 4), np.uint8)
    st = capi.AlfPic(*[a.ctypes.data for a in keep], scratch.ctypes.data, log2_ctu)
    d, s_ = dst.struct(), src.struct()
    lib().oracle_alf_run(C.byref(d), C.byref(s_), C.addressof(st))


def tmvp_cells(units: np.ndarray, refined: np.ndarray, log2_ctu: int, nb_ctb_w: int) -> np.ndarray:
    """oracle_tmvp_cells: the plane cells the refined vectors of the DMVR units go to (4 entries per unit)"""
    from openvvc_amd import capi
    units = np.ascontiguousarray(units)
    refined = np.ascontiguousarray(refined, dtype=np.int32)
    out = np.zeros(4 * len(units), capi.TMVP_CELL_DTYPE)
    lib().oracle_tmvp_cells(units.ctypes.data, len(units), refined.ctypes.data, log2_ctu, nb_ctb_w, out.ctypes.data)
    return out
