"""Python host harness over the device engine (ovhip_ctx_* / ovhip_*_launch).

Plumbing only: device buffers, picture upload/download and stage launches all go through the
C ABI in libovvc_hip.so.  There is no Python or CPU implementation of any stage here."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


class EngineError(RuntimeError):
    pass


def rgb_format(matrix: int = 1, full_range: int = 0, chroma_loc: int = 0, dtype: int = capi.RGB_U8, layout: int = capi.RGB_PLANAR) -> capi.RgbFormat:
    """an ovhip_rgb_format (include/ovvc_hip.h, "RGB output on the device")"""
    return capi.RgbFormat(matrix, full_range, chroma_loc, dtype, layout)


def rgb_shape(fmt: capi.RgbFormat, w: int, h: int, window=(0, 0, 0, 0)) -> tuple:
    """the array shape of the RGB picture of a w x h picture under `window`: (3, H, W) planar, (H, W, 3) packed"""
    W, H = w - 2 * (window[0] + window[1]), h - 2 * (window[2] + window[3])
    return (3, H, W) if fmt.layout == capi.RGB_PLANAR else (H, W, 3)


def _device_tensor(tensor, what: str, dtypes: tuple, shape: "tuple | None" = None, need: "int | None" = None, slots: bool = False) -> "tuple[int, int, int]":
    """(data_ptr, bytes of one slot, slots) of a torch tensor on the device that is to take `what` -- one, or with `slots` one per index of
    its first dimension -- after checking device, dtype (one of `dtypes`) and contiguity, then either the exact `shape` of a slot or at
    least `need` bytes in a slot.  The one place torch is more than a test import."""
    import torch
    if not isinstance(tensor, torch.Tensor) or not tensor.is_cuda:
        raise EngineError(f"{what}: the destination must be a torch tensor on the device")
    if tensor.dtype not in dtypes:
        raise EngineError(f"{what}: tensor dtype {tensor.dtype}, the format takes {dtypes}")
    if not tensor.is_contiguous():
        raise EngineError(f"{what}: the destination tensor must be contiguous")
    if slots and tensor.ndim < 2:
        raise EngineError(f"{what}: a tensor of slots has them as its first dimension")
    n = int(tensor.shape[0]) if slots else 1
    if shape is not None:
        if tuple(tensor.shape[1:] if slots else tensor.shape) != tuple(shape):
            raise EngineError(f"{what}: tensor shape {tuple(tensor.shape)}, the output is {'[slots] + ' if slots else ''}{tuple(shape)}")
        return tensor.data_ptr(), int(np.prod(shape, dtype=np.int64)) * tensor.element_size(), n
    per = tensor.numel() * tensor.element_size() // n if n else 0
    if not need or per < need:
        raise EngineError(f"{what}: {per} bytes per picture, the output needs {need}")
    return tensor.data_ptr(), per, n


def _rgb_tensor(tensor, fmt: capi.RgbFormat, shape: tuple, n: "int | None" = None) -> "tuple[int, int]":
    """(data_ptr, bytes per picture) of a torch tensor that is to take RGB pictures of `shape` (n of them, one after the other, with n given)"""
    import torch
    want = {capi.RGB_U8: torch.uint8, capi.RGB_U16: torch.uint16, capi.RGB_F16: torch.float16, capi.RGB_F32: torch.float32}.get(fmt.dtype)
    ptr, per, got = _device_tensor(tensor, "rgb output", (want,) if want is not None else (), shape=shape, slots=n is not None)
    if n is not None and got != n:
        raise EngineError(f"rgb output: {got} slots, {n} expected")
    return ptr, per


def surface_format(format: int = capi.SURF_NV12, rounding: int = capi.SURF_ROUND, pitch_y: int = 0, pitch_c: int = 0, offset_c=(0, 0)) -> capi.SurfaceFormat:
    """an ovhip_surface_format (include/ovvc_hip.h, "Surface output on the device"); pitches and offsets in bytes, 0: tight"""
    fmt = capi.SurfaceFormat(format, rounding)
    fmt.pitch_y, fmt.pitch_c = pitch_y, pitch_c
    fmt.offset_c[0], fmt.offset_c[1] = offset_c
    return fmt


def surface_conv(src_matrix: int = 9, src_full_range: int = 0, src_chroma_loc: int = 2, dst_matrix: int = 1, dst_full_range: int = 0,
                 dst_chroma_loc: int = 0) -> capi.SurfaceConv:
    """an ovhip_surface_conv (include/ovvc_hip.h, "Surface output through a colour table"): matrix, range and chroma location of the
    decoded picture and of the converted one.  The defaults: BT.2020 limited, chroma top-left, to BT.709 limited, chroma left"""
    return capi.SurfaceConv(src_matrix, src_full_range, src_chroma_loc, dst_matrix, dst_full_range, dst_chroma_loc)


def _surface_tensor(tensor, fmt: capi.SurfaceFormat, need: int, slots: bool = False) -> "tuple[int, int, int]":
    """(data_ptr, bytes of one slot, slots) of a torch tensor that is to take surfaces of `need` bytes"""
    import torch
    allowed = (torch.uint8,) if capi.SURF_ELEM_BYTES.get(fmt.format) == 1 else (torch.uint8, torch.int16, torch.uint16)
    return _device_tensor(tensor, "surface output", allowed, need=need, slots=slots)


def reduce_check(src_w: int, src_h: int, dst_w: int, dst_h: int, src_window=(0, 0, 0, 0), chroma_loc: int = 0) -> "tuple[int, tuple]":
    """(code, (p_x, q_x, p_y, q_y)) of ovhip_output_reduce_check: whether src_w x src_h under src_window reduces to dst_w x dst_h
    (include/ovvc_hip.h, "Reduced-size output on the device").  Host only."""
    ratio = (C.c_int32 * 4)()
    r = capi.load().ovhip_output_reduce_check(src_w, src_h, C.byref(capi.ReduceInfo(capi.Window(*src_window), chroma_loc)), dst_w, dst_h, ratio)
    return r, tuple(ratio)


def ladder_rung(out_w: int, out_h: int, fmt: "capi.SurfaceFormat | None" = None, dst=None, nbytes: "int | None" = None, slots: bool = False) -> capi.LadderRung:
    """an ovhip_ladder_rung (include/ovvc_hip.h, "Output ladder on the device"): out_w x out_h as a surface of `fmt` (default: tight
    NV12) at `dst` -- a contiguous torch tensor on the device (checked against the surface's bytes and kept alive by the rung; with
    `slots` its first dimension counts a stream's slots and the rung's bytes are one slot's), an address with `nbytes`, or None for a
    rung that only describes (ladder_check, DevPic.ladder)"""
    fmt = fmt if fmt is not None else surface_format()
    rung = capi.LadderRung(out_w, out_h, fmt)
    if dst is None or isinstance(dst, int):
        rung.dst, rung.dst_bytes = dst or None, nbytes or 0
    else:
        need = capi.load().ovhip_surface_bytes(out_w, out_h, None, C.byref(fmt))
        ptr, per, n = _surface_tensor(dst, fmt, need, slots=slots)
        rung.dst, rung.dst_bytes = ptr, per
        rung._keep, rung._slots = dst, n
    return rung


def _rung_array(rungs) -> "tuple":
    """(the C array, n) of a sequence of capi.LadderRung"""
    rungs = list(rungs)
    return (capi.LadderRung * max(len(rungs), 1))(*rungs), len(rungs)


def ladder_check(src_w: int, src_h: int, rungs, src_window=(0, 0, 0, 0), chroma_loc: int = 0) -> "tuple[int, list]":
    """(code, [(p_x, q_x, p_y, q_y) per rung]) of ovhip_ladder_check: whether src_w x src_h under src_window leaves as these rungs.
    Host only."""
    arr, n = _rung_array(rungs)
    ratio = ((C.c_int32 * 4) * capi.LADDER_MAX_RUNGS)()
    r = capi.load().ovhip_ladder_check(src_w, src_h, C.byref(capi.ReduceInfo(capi.Window(*src_window), chroma_loc)), arr, n, ratio)
    return r, [tuple(ratio[k]) for k in range(min(n, capi.LADDER_MAX_RUNGS))]


def ladder_lut_check(src_w: int, src_h: int, rungs, conv: "capi.SurfaceConv | None", size: int, peak: int, src_window=(0, 0, 0, 0),
                     chroma_loc: "int | None" = None) -> "tuple[int, list]":
    """(code, [(p_x, q_x, p_y, q_y) per rung]) of ovhip_ladder_lut_check: whether src_w x src_h under src_window leaves as these rungs
    converted by `conv` through a table of `size` points and peak `peak` (include/ovvc_hip.h, "Output ladder through a colour table").
    chroma_loc None: conv's src_chroma_loc.  Host only."""
    arr, n = _rung_array(rungs)
    ratio = ((C.c_int32 * 4) * capi.LADDER_MAX_RUNGS)()
    info = capi.ReduceInfo(capi.Window(*src_window), _ladder_loc(chroma_loc, conv))
    r = capi.load().ovhip_ladder_lut_check(src_w, src_h, C.byref(info), arr, n, C.byref(conv) if conv is not None else None, size, peak, ratio)
    return r, [tuple(ratio[k]) for k in range(min(n, capi.LADDER_MAX_RUNGS))]


def _ladder_loc(chroma_loc: "int | None", conv: "capi.SurfaceConv | None") -> int:
    """the ladder's chroma location: the one given, else the one the conversion reads (the reduced pictures keep it), else 0"""
    return chroma_loc if chroma_loc is not None else (conv.src_chroma_loc if conv is not None else 0)


def rgb_level(out_w: int, out_h: int, fmt: "capi.RgbFormat | None" = None, dst=None, slots: bool = False, nbytes: "int | None" = None) -> capi.RgbLevel:
    """an ovhip_rgb_level (include/ovvc_hip.h, "RGB pyramid on the device"): out_w x out_h as an RGB tensor of `fmt` (default:
    rgb_format()) at `dst` -- a contiguous torch tensor on the device of the format's dtype and the level's shape, such as one picture of
    a batch tensor (kept alive by the level; with `slots` its first dimension counts a stream's slots and the level's bytes are one
    slot's), an address with `nbytes`, or None for a level that only describes (rgb_pyramid_check, DevPic.rgb_pyramid)"""
    fmt = fmt if fmt is not None else rgb_format()
    level = capi.RgbLevel(out_w, out_h, fmt)
    if dst is None or isinstance(dst, int):
        level.dst, level.dst_bytes = dst or None, nbytes or 0
    else:
        ptr, per, n = _device_tensor(dst, "rgb pyramid output", _rgb_torch_dtypes(fmt), shape=rgb_shape(fmt, out_w, out_h), slots=slots)
        level.dst, level.dst_bytes = ptr, per
        level._keep, level._slots = dst, n
    return level


def _rgb_torch_dtypes(fmt: capi.RgbFormat) -> tuple:
    import torch
    want = {capi.RGB_U8: torch.uint8, capi.RGB_U16: torch.uint16, capi.RGB_F16: torch.float16, capi.RGB_F32: torch.float32}.get(fmt.dtype)
    return (want,) if want is not None else ()


def _level_array(levels) -> "tuple":
    """(the C array, n) of a sequence of capi.RgbLevel"""
    levels = list(levels)
    return (capi.RgbLevel * max(len(levels), 1))(*levels), len(levels)


def _pyramid_info(levels, src_window, chroma_loc: "int | None") -> capi.ReduceInfo:
    """the pyramid's ovhip_reduce_info; chroma_loc None: the one the first level's format names (the reduced pictures keep it), else 0"""
    levels = list(levels)
    loc = chroma_loc if chroma_loc is not None else (levels[0].fmt.chroma_loc if levels else 0)
    return capi.ReduceInfo(capi.Window(*src_window), loc)


def rgb_pyramid_check(src_w: int, src_h: int, levels, src_window=(0, 0, 0, 0), chroma_loc: "int | None" = None, lut_size: int = 0,
                      lut_peak: int = 0) -> "tuple[int, list]":
    """(code, [(p_x, q_x, p_y, q_y) per level]) of ovhip_rgb_pyramid_check: whether src_w x src_h under src_window leaves as these levels,
    through a table of lut_size points and peak lut_peak unless lut_size is 0.  chroma_loc None: the first level's.  Host only."""
    arr, n = _level_array(levels)
    ratio = ((C.c_int32 * 4) * capi.PYRAMID_MAX_LEVELS)()
    r = capi.load().ovhip_rgb_pyramid_check(src_w, src_h, C.byref(_pyramid_info(levels, src_window, chroma_loc)), arr, n, lut_size, lut_peak, ratio)
    return r, [tuple(ratio[k]) for k in range(min(n, capi.PYRAMID_MAX_LEVELS))]


def mvfield_format(dtype: int = capi.MVF_I32, layout: int = capi.MVF_PLANAR, vectors: int = capi.MVF_UNIT) -> capi.MvfieldFormat:
    """an ovhip_mvfield_format (include/ovvc_hip.h, "Motion field output on the device")"""
    return capi.MvfieldFormat(dtype, layout, vectors, 0)


def mvfield_shape(fmt: capi.MvfieldFormat, w: int, h: int) -> "tuple[tuple, tuple]":
    """(shape of the vectors, shape of the info) of a w x h picture's motion field: (4, H4, W4) or (H4, W4, 4), and (H4, W4)"""
    w4, h4 = (w + 3) >> 2, (h + 3) >> 2
    return ((h4, w4, 4) if fmt.layout == capi.MVF_CELLS else (4, h4, w4)), (h4, w4)


def _mvfield_dsts(vec, info, fmt: capi.MvfieldFormat, w: int, h: int, vec_bytes, info_bytes, slots: bool = False):
    """(vec ptr, vec bytes, info ptr, info bytes, slots) of a pair of destinations, each a torch tensor (checked against the field's
    shape), a device address with its byte count, or None"""
    vshape, ishape = mvfield_shape(fmt, w, h)
    n = None
    if vec is None or isinstance(vec, int):
        vp, vb = vec or 0, vec_bytes or 0
    else:
        import torch
        tdt = {capi.MVF_I32: (torch.int32,), capi.MVF_F32: (torch.float32,), capi.MVF_F16: (torch.float16,)}.get(fmt.dtype, ())
        vp, vb, n = _device_tensor(vec, "motion field vectors", tdt, shape=vshape, slots=slots)
    if info is None or isinstance(info, int):
        ip, ib = info or 0, info_bytes or 0
    else:
        import torch
        ip, ib, ni = _device_tensor(info, "motion field info", (torch.int32, torch.uint32), shape=ishape, slots=slots)
        if n is not None and ni != n:
            raise EngineError(f"motion field output: {n} slots of vectors, {ni} of info")
        n = ni
    return vp, vb, ip, ib, n


def _set_output(owner, kind: str, fmt, dsts: list, window=None, n_slots: "int | None" = None, check: bool = True) -> int:
    """The one flow behind Frame.set_*_output and Stream.set_*_output (kind: "rgb", "surface" or "mvfield").  dsts: the (destination,
    bytes) pairs the C setter takes, each destination a torch tensor on the device (checked against what the output needs at the size
    the owner outputs, and kept alive by the owner), a device address with its bytes, or -- the motion field's only -- None.  A
    stream's tensors carry the slots as their first dimension; with addresses n_slots counts.  fmt None: off."""
    stream = isinstance(owner, Stream)
    who = "stream" if stream else "frame"
    fn, handle = getattr(owner.lib, f"ovhip_{who}_set_{kind}_output"), owner.s if stream else owner.f
    if fmt is None:
        return fn(handle, None, *([None] if window is not None else []), *[a for _ in dsts for a in (None, 0)], *([0] if stream else []))
    w, h = (owner.cfg.w, owner.cfg.h) if stream else (owner.w, owner.h)
    win = capi.Window(*window) if window is not None else None
    n = None
    if kind == "mvfield":                                  # (the motion is the decoded picture's: no output scale)
        (vec, vb), (info, ib) = dsts
        vp, vb, ip, ib, n = _mvfield_dsts(vec, info, fmt, w, h, vb, ib, slots=stream)
        dsts, keep = [(vp, vb), (ip, ib)], (vec, info)
    elif not isinstance(dsts[0][0], int):
        keep = dsts[0][0]
        w, h = getattr(owner, "_out_size", None) or (w, h)
        if kind == "rgb":
            n = (int(keep.shape[0]) if getattr(keep, "ndim", 0) == 4 else 0) if stream else None
            dsts = [_rgb_tensor(keep, fmt, rgb_shape(fmt, w, h, window), n)]
        else:
            ptr, per, n = _surface_tensor(keep, fmt, owner.lib.ovhip_surface_bytes(w, h, C.byref(win), C.byref(fmt)), slots=stream)
            dsts = [(ptr, per)]
    else:
        keep = None
    if keep is not None and stream:
        owner._keep.append(keep)                           # (as long as the stream)
    elif keep is not None:
        setattr(owner, f"_{kind}_keep", keep)              # (until the frame's next setting of this kind)
    r = fn(handle, C.byref(fmt), *([C.byref(win)] if win is not None else []), *[a for p, b in dsts for a in (C.c_void_p(p) if p else None, b or 0)],
           *([n if n is not None else (n_slots or 0)] if stream else []))
    if check and r:
        raise EngineError(f"{who}_set_{kind}_output: {r}")
    return r


def _set_lut(owner, kind: str, lut_or_table, peak: int = 0, conv=None, check: bool = True) -> int:
    """The one flow behind Frame.set_*_lut and Stream.set_*_lut (kind: "rgb", "surface", "ladder" or "rgb_pyramid"; the surface's and the
    ladder's C setters take the conversion `conv`).  A frame takes an RgbLut and keeps it alive; a stream takes the table as a numpy
    array with its peak and uploads it itself.  None: off."""
    stream = isinstance(owner, Stream)
    who = "stream" if stream else "frame"
    fn, handle = getattr(owner.lib, f"ovhip_{who}_set_{kind}_lut"), owner.s if stream else owner.f
    off = lut_or_table is None
    cv = [C.byref(conv) if conv is not None and not (stream and off) else None] if kind in ("surface", "ladder") else []
    if stream:
        table, size = (None, 0) if off else _lut_table(lut_or_table, f"stream_set_{kind}_lut")
        r = fn(handle, *cv, size, 0 if off else int(peak), None if off else table.ctypes.data)
    else:
        r = fn(handle, None if off else lut_or_table.h, *cv)
    if check and r:
        raise EngineError(f"{who}_set_{kind}_lut: {r}")
    if r == 0 and not stream:
        setattr(owner, f"_{kind.replace('rgb_pyramid', 'pyramid')}_lut", lut_or_table)
    return r


def _set_levels(owner, kind: str, items, info, n_slots: "int | None" = None, check: bool = True) -> int:
    """The one flow behind set_ladder_output and set_rgb_pyramid_output of Frame and Stream (kind: "ladder" or "rgb_pyramid").  items:
    the rungs or the levels, kept alive by the owner; info: their capi.ReduceInfo.  A stream's items carry the slots they were made with
    (the same for all); with addresses n_slots counts.  None: off."""
    stream = isinstance(owner, Stream)
    who = "stream" if stream else "frame"
    fn, handle = getattr(owner.lib, f"ovhip_{who}_set_{kind}_output"), owner.s if stream else owner.f
    if items is None:
        return fn(handle, None, None, 0, *([0] if stream else []))
    items = list(items)
    slots = []
    if stream:
        name, noun = ("ladder", "rungs") if kind == "ladder" else ("rgb pyramid", "levels")
        counts = {g._slots for g in items if hasattr(g, "_slots")}
        if len(counts) > 1 or (counts and n_slots is not None and counts != {n_slots}):
            raise EngineError(f"{name} output: the {noun}' slots differ: {sorted(counts)}")
        slots = [counts.pop() if counts else (n_slots or 0)]
    arr, n = _rung_array(items) if kind == "ladder" else _level_array(items)
    r = fn(handle, C.byref(info), arr, n, *slots)
    if check and r:
        raise EngineError(f"{who}_set_{kind}_output: {r}")
    if r == 0 and stream:
        owner._keep.append(items)                              # (as long as the stream)
    elif r == 0:
        setattr(owner, f"_{kind.replace('rgb_pyramid', 'pyramid')}_keep", items)      # (until the frame's next setting of this kind)
    return r


class Context:
    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = capi.load()
        h = C.c_void_p()
        r = self.lib.ovhip_ctx_create(C.byref(h), device, C.c_void_p(stream) if stream else None)
        if r != 0:
            raise EngineError(f"ovhip_ctx_create(device={device}) failed: {r} (no HIP device? the engine has no CPU fallback)")
        self.h = h
        self._bufs = []

    def _chk(self, r, what):
        if r != 0:
            raise EngineError(f"{what}: {r}: {self.lib.ovhip_last_error(self.h).decode()}")

    def scratch_bytes(self) -> int:
        """bytes held by the context's grow-only scratch buffers (ovhip_ctx_scratch_bytes)"""
        return int(self.lib.ovhip_ctx_scratch_bytes(self.h))

    def sync(self):
        self._chk(self.lib.ovhip_ctx_sync(self.h), "sync")

    @property
    def stream(self) -> int:
        return self.lib.ovhip_ctx_stream(self.h) or 0

    def close(self):
        if self.h:
            self.lib.ovhip_ctx_destroy(self.h)
            self.h = None

    # ---- raw buffers ----
    def upload(self, arr: np.ndarray) -> "DevBuf":
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        self._chk(self.lib.ovhip_malloc(self.h, arr.nbytes, C.byref(p)), "malloc")
        if arr.nbytes:
            self._chk(self.lib.ovhip_h2d(self.h, p, arr.ctypes.data, arr.nbytes), "h2d")
            self.sync()
        return DevBuf(self, p, arr.nbytes, len(arr))

    # ---- pictures ----
    def new_pic(self, w: int, h: int) -> "DevPic":
        pic = capi.Pic()
        self._chk(self.lib.ovhip_pic_alloc(self.h, w, h, C.byref(pic)), "pic_alloc")
        return DevPic(self, pic, owns=True)

    def alloc(self, nbytes: int) -> "DevBuf":
        p = C.c_void_p()
        self._chk(self.lib.ovhip_malloc(self.h, max(int(nbytes), 16), C.byref(p)), "malloc")
        return DevBuf(self, p, int(nbytes), int(nbytes))

    def upload_pic(self, y, cb, cr) -> "DevPic":
        h, w = y.shape
        p = self.new_pic(w, h)
        p.upload(y, cb, cr)
        return p

    def fork(self, k: int):
        """Route the following launches to side stream k (1..3); 0 = back to the main stream."""
        self._chk(self.lib.ovhip_ctx_fork(self.h, k), "ctx_fork")

    def join(self):
        self._chk(self.lib.ovhip_ctx_join(self.h), "ctx_join")

    # ---- stages ----
    def itx(self, dst: "DevPic", cmds: "DevBuf", coefs: "DevBuf", n: int | None = None, first: int = 0,
            lmcs_scales: "DevBuf | None" = None):
        """n commands starting at command `first`; lmcs_scales: device-derived chroma scales (lmcs_scale)."""
        n = cmds.count - first if n is None else n
        ptr = C.c_void_p(cmds.ptr.value + first * capi.TB_CMD_DTYPE.itemsize) if first else cmds.ptr
        self._chk(self.lib.ovhip_itx_launch(self.h, C.byref(dst.s), ptr, n, coefs.ptr,
                                            lmcs_scales.ptr if lmcs_scales else None), "itx_launch")

    def itx_classes(self, dst: "DevPic", cmds: "DevBuf", coefs: "DevBuf", first: int, n_large: int, n_small: int,
                    lmcs_scales: "DevBuf | None" = None):
        """Commands [first, first + n_large) of any size, then n_small commands all <= 16x16 (recorder's split order)."""
        ptr = C.c_void_p(cmds.ptr.value + first * capi.TB_CMD_DTYPE.itemsize) if first else cmds.ptr
        self._chk(self.lib.ovhip_itx_launch_classes(self.h, C.byref(dst.s), ptr, n_large, n_small, coefs.ptr,
                                                    lmcs_scales.ptr if lmcs_scales else None), "itx_launch_classes")

    def itx_chroma_lmcs(self, dst: "DevPic", cmds: "DevBuf", coefs: "DevBuf", first: int, n_large: int, n_small: int,
                        lmcs_scales: "DevBuf | None", bwd_lut: "DevBuf"):
        """The chroma commands plus the inverse LMCS mapping of luma in the same launch (ovhip_itx_launch_chroma_lmcs)."""
        ptr = C.c_void_p(cmds.ptr.value + first * capi.TB_CMD_DTYPE.itemsize) if first else cmds.ptr
        self._chk(self.lib.ovhip_itx_launch_chroma_lmcs(self.h, C.byref(dst.s), ptr, n_large, n_small, coefs.ptr,
                                                        lmcs_scales.ptr if lmcs_scales else None, bwd_lut.ptr),
                  "itx_launch_chroma_lmcs")

    def lmcs_scale(self, pic: "DevPic", regions: "DevBuf", luts: "capi.LmcsLuts", scales: "DevBuf", n: int | None = None):
        n = regions.count if n is None else n
        self._chk(self.lib.ovhip_lmcs_scale_launch(self.h, C.byref(pic.s), regions.ptr, n, C.byref(luts), scales.ptr),
                  "lmcs_scale_launch")

    def lmcs_inverse(self, pic: "DevPic", bwd_lut: "DevBuf"):
        self._chk(self.lib.ovhip_lmcs_inverse_launch(self.h, C.byref(pic.s), bwd_lut.ptr), "lmcs_inverse_launch")

    def intra_level(self, pic: "DevPic", res: "DevPic", tasks: "DevBuf", first: int, n: int, regions: "DevBuf | None" = None,
                    luts=None, scales: "DevBuf | None" = None, log2_ctu: int = 7, geom: int = 0x12):
        """One level of the ordered pass: tasks [first, first + n) of the device task list."""
        ptr = C.c_void_p(tasks.ptr.value + first * 32)
        self._chk(self.lib.ovhip_intra_level_launch(self.h, C.byref(pic.s), C.byref(res.s), ptr, n, regions.ptr if regions else None,
                                                    C.byref(luts) if luts is not None else None, scales.ptr if scales else None, log2_ctu, geom),
                  "intra_level_launch")

    def intra_ctu(self, pic: "DevPic", res: "DevPic", tasks: "DevBuf", ctus: "DevBuf", n_ctus: int, sync: "DevBuf", epoch: int,
                  regions: "DevBuf | None" = None, luts=None, scales: "DevBuf | None" = None, log2_ctu: int = 7):
        """The whole ordered pass in one launch (tasks / ctus: device copies of Recorder.itasks_by_ctu()).  sync: a zeroed
        device buffer of ovhip_intra_sync_words() uint32; epoch: fresh and != 0 for every launch on the same sync."""
        self._chk(self.lib.ovhip_intra_ctu_launch(self.h, C.byref(pic.s), C.byref(res.s), tasks.ptr, ctus.ptr, n_ctus,
                                                  regions.ptr if regions else None, C.byref(luts) if luts is not None else None,
                                                  scales.ptr if scales else None, log2_ctu, sync.ptr, epoch, None), "intra_ctu_launch")

    def intra_flow_words(self, w: int, h: int) -> int:
        """uint32 words of the state block of intra_flow() for a w x h picture"""
        return int(self.lib.ovhip_intra_flow_words(w, h))

    def intra_flow_items(self, tasks: np.ndarray) -> np.ndarray:
        """Items of the flow launch (ovhip_intra_flow_items) of the LEVEL-SORTED host task list: one uint32 per (task, strip, plane).
        A list the flow path refuses is an error, never an empty launch."""
        tasks = np.ascontiguousarray(tasks)
        items = np.zeros(32 * len(tasks), np.uint32)                  # at most 16 strips x 2 planes per task
        n = int(self.lib.ovhip_intra_flow_items(tasks.ctypes.data, len(tasks), items.ctypes.data, len(items)))
        if len(tasks) and not n:
            raise EngineError("intra_flow_items: the flow launch cannot take this task list")
        return items[:n]

    def intra_flow(self, pic: "DevPic", res: "DevPic", tasks: "DevBuf", n_tasks: int, items: "DevBuf", n_items: int, state: "DevBuf",
                   epoch: int, regions: "DevBuf | None" = None, luts=None, scales: "DevBuf | None" = None, log2_ctu: int = 7,
                   prepare: int = 1, n_workers: int = 0):
        """The ordered pass as a flow launch (k_intra_flow).  tasks / items: device copies of the level-sorted list and of its
        intra_flow_items().  state: a zeroed device buffer of intra_flow_words() uint32 that the caller owns; epoch: fresh and
        != 0 for every launch on the same state.  n_workers: 0 = one workgroup per item.  Word 0 of `state` is the abort code:
        the owner looks at it after the launch (intra_flow_abort)."""
        self._chk(self.lib.ovhip_intra_flow_launch(self.h, C.byref(pic.s), C.byref(res.s), tasks.ptr, n_tasks, items.ptr, n_items,
                                                   regions.ptr if regions else None, C.byref(luts) if luts is not None else None,
                                                   scales.ptr if scales else None, log2_ctu, state.ptr, epoch, None, prepare, n_workers),
                  "intra_flow_launch")

    def intra_flow_abort(self, state: "DevBuf") -> int:
        """Word 0 of a flow launch's state block: 0, or the code of the wait that expired (the picture is then incomplete)."""
        self.sync()
        word = np.zeros(1, np.uint32)
        self._chk(self.lib.ovhip_d2h(self.h, word.ctypes.data, state.ptr, 4), "d2h")
        self.sync()
        return int(word[0])

    def intra_flow_untag(self, pic: "DevPic", tasks: "DevBuf", n: int, with_luma: int = 1):
        """Clears the hand-over bit (bit 15) in the blocks the n ordered tasks wrote (k_flow_untag): after the picture's flow
        launches, before anything else reads the picture.  with_luma = 0: chroma blocks only."""
        self._chk(self.lib.ovhip_intra_flow_untag_launch(self.h, C.byref(pic.s), tasks.ptr, n, with_luma), "intra_flow_untag_launch")

    def tmvp_cells(self, units: "DevBuf", n: int, refined: "DevBuf", log2_ctu: int, nb_ctb_w: int) -> np.ndarray:
        out = self.alloc(4 * n * capi.TMVP_CELL_DTYPE.itemsize)
        self._chk(self.lib.ovhip_tmvp_cells_launch(self.h, units.ptr, n, refined.ptr, log2_ctu, nb_ctb_w, out.ptr), "tmvp_cells")
        self.sync()
        r = out.download(np.uint8).view(capi.TMVP_CELL_DTYPE).copy()
        out.free()
        return r

    def dbf(self, pic: "DevPic", planes: "DevDbfPlanes"):
        self._chk(self.lib.ovhip_dbf_launch(self.h, C.byref(pic.s), C.byref(planes.s)), "dbf_launch")

    def dbf_edges(self, pic: "DevPic", edges_v: "DevBuf", edges_h: "DevBuf", beta_offset: int = 0, tc_offset: int = 0):
        """Deblocking driven by the compact edge lists (capi.dbf_compact)."""
        self._chk(self.lib.ovhip_dbf_launch_edges(self.h, C.byref(pic.s), edges_v.ptr, edges_v.count, edges_h.ptr,
                                                  edges_h.count, beta_offset, tc_offset), "dbf_launch_edges")

    def dbf_edges_ex(self, pic: "DevPic", edges_v: "DevBuf", edges_h: "DevBuf", offsets: "capi.DbfOffsets"):
        """The same with the per-slice offset table of the recorder (capi.Recorder.dbf_edges): edge.pad selects the pair."""
        self._chk(self.lib.ovhip_dbf_launch_edges_ex(self.h, C.byref(pic.s), edges_v.ptr, edges_v.count, edges_h.ptr,
                                                     edges_h.count, C.byref(offsets)), "dbf_launch_edges_ex")

    def sao(self, dst: "DevPic", src: "DevPic", params: "DevBuf", log2_ctu: int = 7):
        self._chk(self.lib.ovhip_sao_launch(self.h, C.byref(dst.s), C.byref(src.s), params.ptr, log2_ctu), "sao_launch")

    def alf(self, dst: "DevPic", src: "DevPic", alf: "DevAlf"):
        self._chk(self.lib.ovhip_alf_launch(self.h, C.byref(dst.s), C.byref(src.s), C.byref(alf.s)), "alf_launch")

    def mc(self, dst: "DevPic", refs: list, units: "DevBuf", lmcs_fwd: "DevBuf | None" = None, n: int | None = None,
           intra: "DevPic | None" = None):
        """intra: picture with the planar prediction of the CIIP CUs whose blend is fused into the units (aux != 0)."""
        n = units.count if n is None else n
        arr = (capi.Pic * len(refs))(*[r.s for r in refs])
        self._chk(self.lib.ovhip_mc_launch(self.h, C.byref(dst.s), arr, len(refs), units.ptr, n,
                                           lmcs_fwd.ptr if lmcs_fwd else None, C.byref(intra.s) if intra else None), "mc_launch")

    def mc_rpr(self, dst: "DevPic", refs: list, units: "DevBuf", lmcs_fwd: "DevBuf | None" = None, n: int | None = None,
               intra: "DevPic | None" = None):
        """Units that read references of another size (ovhip_rpr_unit); each reference keeps its own geometry."""
        n = units.count if n is None else n
        arr = (capi.Pic * len(refs))(*[r.s for r in refs])
        self._chk(self.lib.ovhip_mc_rpr_launch(self.h, C.byref(dst.s), arr, len(refs), units.ptr, n,
                                               lmcs_fwd.ptr if lmcs_fwd else None, C.byref(intra.s) if intra else None),
                  "mc_rpr_launch")

    def ciip(self, dst: "DevPic", intra: "DevPic", units: "DevBuf", n: int | None = None):
        n = units.count if n is None else n
        self._chk(self.lib.ovhip_ciip_launch(self.h, C.byref(dst.s), C.byref(intra.s), units.ptr, n), "ciip_launch")

    def mca(self, dst: "DevPic", refs: list, units: "DevBuf", side: "DevBuf", lmcs_fwd: "DevBuf | None" = None,
            n: int | None = None):
        """Affine (+PROF) units; side: device copy of the recorder's affine side arena."""
        n = units.count if n is None else n
        arr = (capi.Pic * len(refs))(*[r.s for r in refs])
        self._chk(self.lib.ovhip_mca_launch(self.h, C.byref(dst.s), arr, len(refs), units.ptr, n, side.ptr,
                                            lmcs_fwd.ptr if lmcs_fwd else None), "mca_launch")

    def mca_rpr(self, dst: "DevPic", refs: list, units: "DevBuf", side: "DevBuf", lmcs_fwd: "DevBuf | None" = None,
                n: int | None = None):
        """Affine units that read references of another size (ovhip_aff_rpr_unit); each reference keeps its own geometry."""
        n = units.count if n is None else n
        arr = (capi.Pic * len(refs))(*[r.s for r in refs])
        self._chk(self.lib.ovhip_mca_rpr_launch(self.h, C.byref(dst.s), arr, len(refs), units.ptr, n, side.ptr,
                                                lmcs_fwd.ptr if lmcs_fwd else None), "mca_rpr_launch")

    def mcxa(self, dst: "DevPic", refs: list, xunits: "DevBuf", aunits: "DevBuf", side: "DevBuf",
             lmcs_fwd: "DevBuf | None" = None, mv_out: "DevBuf | None" = None):
        """BDOF / DMVR units and affine units in one launch (ovhip_mcxa_launch)."""
        arr = (capi.Pic * len(refs))(*[r.s for r in refs])
        self._chk(self.lib.ovhip_mcxa_launch(self.h, C.byref(dst.s), arr, len(refs), xunits.ptr, xunits.count,
                                             mv_out.ptr if mv_out else None, aunits.ptr, aunits.count, side.ptr,
                                             lmcs_fwd.ptr if lmcs_fwd else None), "mcxa_launch")

    def mvfield(self, w: int, h: int, fmt: "capi.MvfieldFormat | None", vec=None, info=None, mc: "DevBuf | None" = None, mcx: "DevBuf | None" = None,
                aff: "DevBuf | None" = None, rpr: "DevBuf | None" = None, affr: "DevBuf | None" = None, side: "DevBuf | None" = None,
                refined: "DevBuf | None" = None, vec_bytes: "int | None" = None, info_bytes: "int | None" = None, check: bool = True) -> int:
        """ovhip_mvfield_launch: the motion field of a w x h picture from unit lists the caller uploaded (DevBufs whose count is the
        number of units) into `vec` and `info` -- torch tensors on the device of mvfield_shape(), device addresses with their byte
        counts, or None for a destination that is not wanted.  Asynchronous."""
        vp, vb, ip, ib, _n = _mvfield_dsts(vec, info, fmt, w, h, vec_bytes, info_bytes) if fmt is not None else (vec or 0, vec_bytes or 0, info or 0, info_bytes or 0, None)
        src = capi.MvfieldSrc()
        for name, b in (("mc", mc), ("mcx", mcx), ("aff", aff), ("rpr", rpr), ("affr", affr)):
            setattr(src, name, b.ptr if b is not None and b.count else None)
            setattr(src, "n_" + name, b.count if b is not None else 0)
        src.side = side.ptr if side is not None else None
        src.refined = refined.ptr if refined is not None else None
        r = self.lib.ovhip_mvfield_launch(self.h, w, h, C.byref(src), C.byref(fmt) if fmt is not None else None,
                                          C.c_void_p(vp) if vp else None, vb, C.c_void_p(ip) if ip else None, ib)
        if check:
            self._chk(r, "mvfield_launch")
        return r

    def mcx(self, dst: "DevPic", refs: list, units: "DevBuf", lmcs_fwd: "DevBuf | None" = None,
            mv_out: "DevBuf | None" = None, n: int | None = None):
        """BDOF / DMVR units; mv_out: device int32[n][4] receiving the refined motion vectors."""
        n = units.count if n is None else n
        arr = (capi.Pic * len(refs))(*[r.s for r in refs])
        self._chk(self.lib.ovhip_mcx_launch(self.h, C.byref(dst.s), arr, len(refs), units.ptr, n,
                                            lmcs_fwd.ptr if lmcs_fwd else None,
                                            mv_out.ptr if mv_out else None), "mcx_launch")

    def dmvr_search(self, geom: "DevPic", refs: list, units: "DevBuf", mv_out: "DevBuf", n: int | None = None):
        """The decoder-side MV refinement alone (ovhip_dmvr_search_launch) for the units that carry OVHIP_MC_DMVR: their refined
        vectors into mv_out (int32[n][4]; the entries of other units are left alone); geom gives the picture geometry, nothing is
        written to it."""
        n = units.count if n is None else n
        arr = (capi.Pic * len(refs))(*[r.s for r in refs])
        self._chk(self.lib.ovhip_dmvr_search_launch(self.h, C.byref(geom.s), arr, len(refs), units.ptr, n, mv_out.ptr), "dmvr_search_launch")


class DevDbfPlanes:
    """Deblocking edge planes resident on the device (ovhip_dbf_planes with device pointers)."""

    def __init__(self, ctx: "Context", planes: dict):
        self.bufs = {k: ctx.upload(np.ascontiguousarray(planes[k], dtype=np.uint16).ravel()) for k in capi.DBF_PLANE_NAMES}
        self.s = capi.DbfPlanes(*[self.bufs[k].ptr for k in capi.DBF_PLANE_NAMES], planes["w4"], planes["h4"],
                                planes["beta_offset"], planes["tc_offset"])
        self.nbytes = sum(b.nbytes for b in self.bufs.values())

    def free(self):
        for b in self.bufs.values():
            b.free()


class DevAlf:
    """ALF parameter tables resident on the device (ovhip_alf_pic with device pointers).
    `alf`: dict with ctus (ALF_CTU_DTYPE), luma_coeff/luma_clip [24,1300], chroma_coeff/chroma_clip [8,7], cc_coeff [2,4,8]."""

    def __init__(self, ctx: "Context", alf: dict, w: int, h: int, log2_ctu: int = 7):
        self.bufs = {k: ctx.upload(np.ascontiguousarray(alf[k], dtype=dt).ravel()) for k, dt in capi.ALF_TABLES}
        self.scratch = ctx.upload(np.zeros(((w + 3) // 4) * ((h + 3) // 4), np.uint8))
        self.s = capi.AlfPic(*[self.bufs[k].ptr for k, _ in capi.ALF_TABLES], self.scratch.ptr, log2_ctu)
        self.nbytes = sum(b.nbytes for b in self.bufs.values())

    def free(self):
        for b in list(self.bufs.values()) + [self.scratch]:
            b.free()


class DevBuf:
    def __init__(self, ctx: Context, ptr, nbytes: int, count: int):
        self.ctx, self.ptr, self.nbytes, self.count = ctx, ptr, nbytes, count

    def free(self):
        if self.ptr:
            self.ctx.lib.ovhip_free(self.ctx.h, self.ptr)
            self.ptr = None

    def download(self, dtype=np.uint8) -> np.ndarray:
        """Synchronous device -> host copy of the whole buffer."""
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype)
        if self.nbytes:
            self.ctx._chk(self.ctx.lib.ovhip_d2h(self.ctx.h, out.ctypes.data, self.ptr, self.nbytes), "d2h")
        return out


def _lut_table(table, what: str) -> "tuple[np.ndarray, int]":
    """a colour table as the C ABI takes it: contiguous uint16 of shape (S, S, S, 3), index order [b][g][r][c] -> (array, S)"""
    if not isinstance(table, np.ndarray) or table.dtype != np.uint16 or table.ndim != 4 or table.shape[3] != 3 or len(set(table.shape[:3])) != 1:
        raise EngineError(f"{what}: the table must be a numpy array of shape (S, S, S, 3) and dtype uint16")
    return np.ascontiguousarray(table), int(table.shape[0])


class RgbLut:
    """ovhip_rgb_lut: a 3D colour table on the device of `ctx` (include/ovvc_hip.h, "RGB output through a colour table"); table: numpy
    uint16 of shape (S, S, S, 3), S one of 17, 33, 65, index order [b][g][r][c], every entry <= peak.  Immutable; usable from every
    context of that device.  openvvc_amd.lut3d builds tables."""

    def __init__(self, ctx: Context, table: np.ndarray, peak: int):
        table, size = _lut_table(table, "RgbLut")
        self.lib, self.size, self.peak = ctx.lib, size, int(peak)
        h = C.c_void_p()
        ctx._chk(ctx.lib.ovhip_rgb_lut_create(ctx.h, size, self.peak, table.ctypes.data, C.byref(h)), "rgb_lut_create")
        self.h = h

    def close(self):
        if self.h:
            self.lib.ovhip_rgb_lut_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DevPic:
    def __init__(self, ctx: Context, s: capi.Pic, owns: bool):
        self.ctx, self.s, self.owns = ctx, s, owns

    @property
    def w(self):
        return self.s.w

    @property
    def h(self):
        return self.s.h

    def upload(self, y, cb, cr):
        y, cb, cr = (np.ascontiguousarray(a, dtype=np.uint16) for a in (y, cb, cr))
        self.ctx._chk(self.ctx.lib.ovhip_pic_upload(self.ctx.h, C.byref(self.s), y.ctypes.data, cb.ctypes.data,
                                                    cr.ctypes.data, y.shape[1], cb.shape[1]), "pic_upload")

    def download(self):
        y = np.empty((self.h, self.w), np.uint16)
        cb = np.empty((self.h // 2, self.w // 2), np.uint16)
        cr = np.empty_like(cb)
        self.ctx._chk(self.ctx.lib.ovhip_pic_download(self.ctx.h, C.byref(self.s), y.ctypes.data, cb.ctypes.data,
                                                      cr.ctypes.data, self.w, self.w // 2), "pic_download")
        return y, cb, cr

    def _packed(self, w: int, h: int, window, fn: str, *args) -> np.ndarray:
        """size the array for a w x h picture cropped by `window`, call lib.ovhip_<fn>(ctx, pic, *args, window, array), check"""
        win = capi.Window(*window)
        n = self.ctx.lib.ovhip_output_bytes(w, h, C.byref(win))
        if not n:
            raise EngineError("output window leaves nothing")
        out = np.empty(n // 2, np.uint16)
        self.ctx._chk(getattr(self.ctx.lib, "ovhip_" + fn)(self.ctx.h, C.byref(self.s), *args, C.byref(win), out.ctypes.data), fn)
        return out

    def _digest16(self, window, fn: str, *args) -> bytes:
        win, out = capi.Window(*window), (C.c_uint8 * 16)()
        self.ctx._chk(getattr(self.ctx.lib, "ovhip_" + fn)(self.ctx.h, C.byref(self.s), *args, C.byref(win), out), fn)
        return bytes(out)

    def output(self, window=(0, 0, 0, 0)) -> np.ndarray:
        """The cropped frame in the byte layout dectest.c:372-409 writes (uint16 LE: Y rows, Cb rows, Cr rows), packed on the
        device and fetched with one D2H.  window = (lft, rgt, abv, blw) in chroma sample units."""
        return self._packed(self.w, self.h, window, "pic_output")

    def digest(self, window=(0, 0, 0, 0)) -> bytes:
        """the picture's fingerprint: an MD5 tree over the cropped frame computed on the device (include/ovvc_hip.h, "Digest")"""
        return self._digest16(window, "pic_digest")

    def scale_into(self, dst: "DevPic", scale_window=(0, 0, 0, 0), col=(0, 0), check: bool = True) -> int:
        """Resample this picture into dst (its own size) as the reference's output resampler does (ovhip_output_scale_launch);
        scale_window = (left, right, top, bottom) in chroma sample units, col = the chroma collocation flags.  Asynchronous."""
        info = capi.ScaleInfo(*scale_window, *col)
        r = self.ctx.lib.ovhip_output_scale_launch(self.ctx.h, C.byref(self.s), C.byref(info), C.byref(dst.s))
        if check:
            self.ctx._chk(r, "output_scale")
        return r

    def output_scaled(self, out_w: int, out_h: int, scale_window=(0, 0, 0, 0), col=(0, 0), window=(0, 0, 0, 0)) -> np.ndarray:
        """output() of the picture resampled to out_w x out_h; `window` crops the resampled picture"""
        return self._packed(out_w, out_h, window, "pic_output_scaled", C.byref(capi.ScaleInfo(*scale_window, *col)), out_w, out_h)

    def digest_scaled(self, out_w: int, out_h: int, scale_window=(0, 0, 0, 0), col=(0, 0), window=(0, 0, 0, 0)) -> bytes:
        return self._digest16(window, "pic_digest_scaled", C.byref(capi.ScaleInfo(*scale_window, *col)), out_w, out_h)

    def reduce_into(self, dst: "DevPic", src_window=(0, 0, 0, 0), chroma_loc: int = 0, check: bool = True) -> int:
        """The exact area average of this picture's window (chroma sample units) into dst, its own smaller size
        (ovhip_output_reduce_launch; include/ovvc_hip.h, "Reduced-size output on the device").  Asynchronous."""
        info = capi.ReduceInfo(capi.Window(*src_window), chroma_loc)
        r = self.ctx.lib.ovhip_output_reduce_launch(self.ctx.h, C.byref(self.s), C.byref(info), C.byref(dst.s))
        if check:
            self.ctx._chk(r, "output_reduce")
        return r

    def output_reduced(self, out_w: int, out_h: int, src_window=(0, 0, 0, 0), chroma_loc: int = 0, window=(0, 0, 0, 0)) -> np.ndarray:
        """output() of the picture reduced to out_w x out_h; `window` crops the reduced picture"""
        info = capi.ReduceInfo(capi.Window(*src_window), chroma_loc)
        return self._packed(out_w, out_h, window, "pic_output_reduced", C.byref(info), out_w, out_h)

    def digest_reduced(self, out_w: int, out_h: int, src_window=(0, 0, 0, 0), chroma_loc: int = 0, window=(0, 0, 0, 0)) -> bytes:
        info = capi.ReduceInfo(capi.Window(*src_window), chroma_loc)
        return self._digest16(window, "pic_digest_reduced", C.byref(info), out_w, out_h)

    def _fg_model(self, params: capi.FgParams) -> capi.FgModel:
        r, model, _ = capi.fg_derive(self.ctx.lib, params)
        if r:
            raise EngineError(f"fg_derive: {r}")
        return model

    def grain_into(self, dst: "DevPic", params: capi.FgParams, poc: int, check: bool = True) -> int:
        """dst = this picture with the film grain `params` (the SEI's fields, derived once as for one picture) asks for at `poc`
        (ovhip_fg_derive + ovhip_film_grain_launch).  Asynchronous."""
        model = self._fg_model(params)
        r = self.ctx.lib.ovhip_film_grain_launch(self.ctx.h, C.byref(self.s), C.byref(model), poc, 0, C.byref(dst.s))
        if check:
            self.ctx._chk(r, "film_grain")
        return r

    def output_grain(self, params: capi.FgParams, poc: int, window=(0, 0, 0, 0)) -> np.ndarray:
        """output() of the picture with film grain"""
        return self._packed(self.w, self.h, window, "pic_output_grain", C.byref(self._fg_model(params)), poc)

    def digest_grain(self, params: capi.FgParams, poc: int, window=(0, 0, 0, 0)) -> bytes:
        return self._digest16(window, "pic_digest_grain", C.byref(self._fg_model(params)), poc)

    def hash(self, method: int, n_planes: int = 3, check: bool = True):
        """ovhip_pic_hash: the decoded picture hash SEI's value of this picture (CRC / checksum on the device, MD5 through the host) ->
        capi.PicHashValue, or the error code with check=False"""
        out = capi.PicHashValue()
        r = self.ctx.lib.ovhip_pic_hash(self.ctx.h, C.byref(self.s), method, n_planes, C.byref(out))
        if check:
            self.ctx._chk(r, "pic_hash")
        return out if r == 0 else r

    def hash_launch(self, method: int, n_planes: int, d_out: "DevBuf", offset: int = 0, check: bool = True) -> int:
        """ovhip_pic_hash_launch into d_out at byte `offset` (one uint32 per plane).  Asynchronous."""
        r = self.ctx.lib.ovhip_pic_hash_launch(self.ctx.h, C.byref(self.s), method, n_planes,
                                               C.c_void_p(d_out.ptr.value + offset) if d_out is not None else None)
        if check:
            self.ctx._chk(r, "pic_hash_launch")
        return r

    def rgb(self, fmt: capi.RgbFormat, window=(0, 0, 0, 0), lut: "RgbLut | None" = None) -> np.ndarray:
        """ovhip_pic_output_rgb: this picture as RGB (include/ovvc_hip.h, "RGB output on the device"), converted on the device and
        fetched with one D2H -> (3, H, W) or (H, W, 3) in the format's dtype.  lut: through that colour table
        (ovhip_pic_output_rgb_lut, "RGB output through a colour table")"""
        win = capi.Window(*window)
        n = self.ctx.lib.ovhip_rgb_bytes(self.w, self.h, C.byref(win), C.byref(fmt))
        if not n:
            raise EngineError("rgb: bad size / window / format")
        out = np.empty(rgb_shape(fmt, self.w, self.h, window), capi.RGB_NP_DTYPE[fmt.dtype])
        if lut is None:
            self.ctx._chk(self.ctx.lib.ovhip_pic_output_rgb(self.ctx.h, C.byref(self.s), C.byref(win), C.byref(fmt), out.ctypes.data, out.nbytes), "pic_output_rgb")
        else:
            self.ctx._chk(self.ctx.lib.ovhip_pic_output_rgb_lut(self.ctx.h, C.byref(self.s), C.byref(win), C.byref(fmt), lut.h, out.ctypes.data, out.nbytes),
                          "pic_output_rgb_lut")
        return out

    def rgb_into(self, ptr: int, nbytes: int, fmt: capi.RgbFormat, window=(0, 0, 0, 0), check: bool = True, lut: "RgbLut | None" = None) -> int:
        """ovhip_rgb_launch into device memory at `ptr` (a DevBuf's address plus an offset, a tensor's data_ptr()).  Asynchronous.
        lut: through that colour table (ovhip_rgb_lut_launch)"""
        win = capi.Window(*window)
        args = (self.ctx.h, C.byref(self.s), C.byref(win), C.byref(fmt) if fmt is not None else None)
        dst = (C.c_void_p(ptr) if ptr else None, nbytes)
        r = self.ctx.lib.ovhip_rgb_launch(*args, *dst) if lut is None else self.ctx.lib.ovhip_rgb_lut_launch(*args, lut.h, *dst)
        if check:
            self.ctx._chk(r, "rgb_launch" if lut is None else "rgb_lut_launch")
        return r

    def surface(self, fmt: capi.SurfaceFormat, window=(0, 0, 0, 0), lut: "RgbLut | None" = None, conv: "capi.SurfaceConv | None" = None) -> np.ndarray:
        """ovhip_pic_output_surface: this picture as a surface (include/ovvc_hip.h, "Surface output on the device"), written on the
        device and fetched -> the surface's bytes (bytes the layout leaves out are 0).  lut and conv (surface_conv()): the converted
        picture's surface (ovhip_pic_output_surface_lut, "Surface output through a colour table")"""
        if (lut is None) != (conv is None):
            raise EngineError("surface: lut and conv go together")
        win = capi.Window(*window)
        n = self.ctx.lib.ovhip_surface_bytes(self.w, self.h, C.byref(win), C.byref(fmt))
        if not n:
            raise EngineError("surface: bad size / window / format")
        out = np.zeros(n, np.uint8)
        if lut is None:
            self.ctx._chk(self.ctx.lib.ovhip_pic_output_surface(self.ctx.h, C.byref(self.s), C.byref(win), C.byref(fmt), out.ctypes.data, out.nbytes), "pic_output_surface")
        else:
            self.ctx._chk(self.ctx.lib.ovhip_pic_output_surface_lut(self.ctx.h, C.byref(self.s), C.byref(win), C.byref(conv), C.byref(fmt), lut.h, out.ctypes.data,
                                                                    out.nbytes), "pic_output_surface_lut")
        return out

    def surface_into(self, ptr: int, nbytes: int, fmt: capi.SurfaceFormat, window=(0, 0, 0, 0), check: bool = True, lut: "RgbLut | None" = None,
                     conv: "capi.SurfaceConv | None" = None) -> int:
        """ovhip_surface_launch into device memory at `ptr` (a DevBuf's address plus an offset, a tensor's data_ptr()).  Asynchronous.
        conv: ovhip_surface_lut_launch with that conversion through the colour table `lut` (which may be None only to see the refusal)"""
        win = capi.Window(*window)
        f, d = C.byref(fmt) if fmt is not None else None, C.c_void_p(ptr) if ptr else None
        if conv is None and lut is None:
            r = self.ctx.lib.ovhip_surface_launch(self.ctx.h, C.byref(self.s), C.byref(win), f, d, nbytes)
        else:
            r = self.ctx.lib.ovhip_surface_lut_launch(self.ctx.h, C.byref(self.s), C.byref(win), C.byref(conv) if conv is not None else None, f,
                                                      lut.h if lut is not None else None, d, nbytes)
        if check:
            self.ctx._chk(r, "surface_launch" if conv is None and lut is None else "surface_lut_launch")
        return r

    def ladder(self, rungs, src_window=(0, 0, 0, 0), chroma_loc: "int | None" = None, lut: "RgbLut | None" = None,
               conv: "capi.SurfaceConv | None" = None) -> "list[np.ndarray]":
        """ovhip_pic_output_ladder: this picture as the rungs of a ladder (include/ovvc_hip.h, "Output ladder on the device"; each
        rung a ladder_rung() without a destination), written on the device by one launch and fetched -> the surfaces' bytes, one
        array per rung (bytes a layout leaves out are 0).  lut and conv (surface_conv()): the rungs of the CONVERTED reduced pictures
        (ovhip_pic_output_ladder_lut, "Output ladder through a colour table"); chroma_loc None: conv's src_chroma_loc, else 0"""
        if (lut is None) != (conv is None):
            raise EngineError("ladder: lut and conv go together")
        outs, full = [], []
        for g in rungs:
            n = self.ctx.lib.ovhip_surface_bytes(g.out_w, g.out_h, None, C.byref(g.fmt))
            if not n:
                raise EngineError("ladder: bad size / format of a rung")
            outs.append(np.zeros(n, np.uint8))
            full.append(ladder_rung(g.out_w, g.out_h, g.fmt, outs[-1].ctypes.data, n))
        arr, n = _rung_array(full)
        info = capi.ReduceInfo(capi.Window(*src_window), _ladder_loc(chroma_loc, conv))
        if lut is None:
            self.ctx._chk(self.ctx.lib.ovhip_pic_output_ladder(self.ctx.h, C.byref(self.s), C.byref(info), arr, n), "pic_output_ladder")
        else:
            self.ctx._chk(self.ctx.lib.ovhip_pic_output_ladder_lut(self.ctx.h, C.byref(self.s), C.byref(info), arr, n, C.byref(conv), lut.h), "pic_output_ladder_lut")
        return outs

    def ladder_into(self, rungs, src_window=(0, 0, 0, 0), chroma_loc: "int | None" = None, check: bool = True, lut: "RgbLut | None" = None,
                    conv: "capi.SurfaceConv | None" = None) -> int:
        """ovhip_ladder_launch: every rung (ladder_rung() with a torch tensor or a device address) written by one launch.  Asynchronous.
        conv: ovhip_ladder_lut_launch with that conversion through the colour table `lut` (which may be None only to see the refusal);
        chroma_loc None: conv's src_chroma_loc, else 0"""
        arr, n = _rung_array(rungs)
        info = capi.ReduceInfo(capi.Window(*src_window), _ladder_loc(chroma_loc, conv))
        if conv is None and lut is None:
            r = self.ctx.lib.ovhip_ladder_launch(self.ctx.h, C.byref(self.s), C.byref(info), arr, n)
        else:
            r = self.ctx.lib.ovhip_ladder_lut_launch(self.ctx.h, C.byref(self.s), C.byref(info), arr, n, C.byref(conv) if conv is not None else None,
                                                     lut.h if lut is not None else None)
        if check:
            self.ctx._chk(r, "ladder_launch" if conv is None and lut is None else "ladder_lut_launch")
        return r

    def rgb_pyramid(self, levels, src_window=(0, 0, 0, 0), chroma_loc: "int | None" = None, lut: "RgbLut | None" = None) -> "list[np.ndarray]":
        """ovhip_pic_output_rgb_pyramid: this picture as the levels of an RGB pyramid (include/ovvc_hip.h, "RGB pyramid on the device";
        each level an rgb_level() without a destination), written on the device by one launch and fetched -> one array per level,
        (3, H, W) or (H, W, 3) in the level's dtype.  lut: through that colour table; chroma_loc None: the first level's"""
        outs, full = [], []
        for g in levels:
            if not self.ctx.lib.ovhip_rgb_bytes(g.out_w, g.out_h, None, C.byref(g.fmt)):
                raise EngineError("rgb_pyramid: bad size / format of a level")
            outs.append(np.empty(rgb_shape(g.fmt, g.out_w, g.out_h), capi.RGB_NP_DTYPE[g.fmt.dtype]))
            full.append(rgb_level(g.out_w, g.out_h, g.fmt, outs[-1].ctypes.data, nbytes=outs[-1].nbytes))
        arr, n = _level_array(full)
        info = _pyramid_info(full, src_window, chroma_loc)
        self.ctx._chk(self.ctx.lib.ovhip_pic_output_rgb_pyramid(self.ctx.h, C.byref(self.s), C.byref(info), arr, n, lut.h if lut is not None else None),
                      "pic_output_rgb_pyramid")
        return outs

    def rgb_pyramid_into(self, levels, src_window=(0, 0, 0, 0), chroma_loc: "int | None" = None, check: bool = True, lut: "RgbLut | None" = None) -> int:
        """ovhip_rgb_pyramid_launch: every level (rgb_level() with a torch tensor or a device address) written by one launch.
        Asynchronous.  lut: through that colour table; chroma_loc None: the first level's"""
        arr, n = _level_array(levels)
        r = self.ctx.lib.ovhip_rgb_pyramid_launch(self.ctx.h, C.byref(self.s), C.byref(_pyramid_info(levels, src_window, chroma_loc)), arr, n,
                                                  lut.h if lut is not None else None)
        if check:
            self.ctx._chk(r, "rgb_pyramid_launch")
        return r

    def row_digests(self, window=(0, 0, 0, 0)) -> np.ndarray:
        win = capi.Window(*window)
        rows = self.ctx.lib.ovhip_output_rows(self.w, self.h, C.byref(win))
        buf = self.ctx.alloc(rows * 16)
        self.ctx._chk(self.ctx.lib.ovhip_output_row_md5_launch(self.ctx.h, C.byref(self.s), C.byref(win), buf.ptr), "row_md5")
        self.ctx.sync()
        d = buf.download(np.uint8).reshape(rows, 16).copy()
        buf.free()
        return d

    def band(self, y0: int, h: int) -> "DevPic":
        """A view of rows [y0, y0+h) (luma) as its own picture (no copy)."""
        s = capi.Pic(self.s.y + y0 * self.s.stride_y * 2, self.s.cb + (y0 // 2) * self.s.stride_c * 2,
                     self.s.cr + (y0 // 2) * self.s.stride_c * 2, self.s.w, h, self.s.stride_y, self.s.stride_c)
        return DevPic(self.ctx, s, owns=False)

    def free(self):
        if self.owns and self.s.y:
            self.ctx.lib.ovhip_pic_free(self.ctx.h, C.byref(self.s))


class ResidentPicture:
    """A recorded picture resident in HBM: reference pictures, command buffers, coefficient arena,
    in-loop filter side information and two picture buffers.  `decode()` enqueues every stage of
    the rcn path in the order the reference executes them (prediction -> residual -> inverse luma
    mapping -> deblocking -> SAO -> ALF/CC-ALF), each as frame-wide launches on the context stream.
    The reconstructed / deblocked picture lives in `dst`, SAO writes `tmp`, ALF writes the final
    samples back to `dst`.

    Launch order inside the two composite stages:
      "mc"  = plain / GPM units, BDOF / DMVR units (+ refined-MV write-back), affine units, CIIP blend
      "itx" = luma TBs, LMCS chroma-scale derivation (reads the luma just reconstructed), chroma TBs,
              inverse luma mapping"""

    STAGES = ("mc", "itx", "dbf", "sao", "alf")
    SUBSTAGES = ("mcp", "mcx", "mca", "ciip", "itx_l", "lmcs_scale", "itx_c", "lmcs_inv", "dbf", "sao", "alf")
    _GROUPS = {"mc": ("mcp", "mcx", "mca", "ciip"), "itx": ("itx_l", "lmcs_scale", "itx_c", "lmcs_inv")}

    def __init__(self, ctx: Context, wl, log2_ctu: int = 7, overlap: bool = False):
        self.ctx, self.wl, self.log2_ctu, self.overlap = ctx, wl, log2_ctu, overlap
        self.refs = [ctx.upload_pic(*r) for r in wl.refs]
        self.dst = ctx.new_pic(wl.w, wl.h)
        self.tmp = ctx.new_pic(wl.w, wl.h)
        self.mc_units = ctx.upload(wl.mc_units)
        self.tb_cmds = ctx.upload(wl.tb_cmds)
        self.coefs = ctx.upload(wl.coefs)
        self.dbf_v = ctx.upload(wl.dbf_edges[0])              # the lists ovhip_rec_dbf_ctu emitted CTU by CTU
        self.dbf_h = ctx.upload(wl.dbf_edges[1])
        self.sao_params = ctx.upload(wl.sao_params)
        self.alf = DevAlf(ctx, wl.alf, wl.w, wl.h, log2_ctu)
        self.bufs = [self.mc_units, self.tb_cmds, self.coefs, self.sao_params, self.dbf_v, self.dbf_h]
        up = lambda a: self._keep(ctx.upload(a)) if a is not None and len(a) else None
        self.mcx_units = up(wl.mcx_units)
        self.mv_out = self._keep(ctx.alloc(16 * len(wl.mcx_units))) if self.mcx_units else None
        self.aff_units, self.aff_side = up(wl.aff_units), up(wl.aff_side)
        self.ciip_units = up(wl.ciip_units)
        self.intra = ctx.upload_pic(*wl.intra) if wl.intra is not None else None
        self.lmcs = wl.lmcs
        self.lmcs_fwd = up(wl.lmcs_fwd)
        self.lmcs_bwd = up(wl.lmcs_bwd)
        self.lmcs_regions = up(wl.lmcs_regions)
        self.lmcs_scales = self._keep(ctx.alloc(2 * len(wl.lmcs_regions))) if self.lmcs_regions else None
        self.n_luma = wl.n_luma_cmds

    def _keep(self, b):
        self.bufs.append(b)
        return b

    def run_stage(self, name: str, on_sub=None):
        """on_sub(sub_stage_name, "begin" | "end"): optional hook around every launch that goes to the main stream."""
        c = self.ctx
        if name == "mc" and self.overlap:
            # plain, refined and affine units write disjoint samples: the three kernels may share the GPU, the CIIP
            # blend follows once all of them are done.  Measured on MI355X: the two cross-stream event waits cost more
            # (frame 0.353 ms) than the overlap of ramp-up / tail gains (serial 0.324 ms), hence off by default.
            self._sub("mcp", on_sub)
            for k, sub in enumerate(("mcx", "mca"), start=1):
                c.fork(k)
                self._launch(sub)
            c.join()
            self._sub("ciip", on_sub)
            return
        if name in self._GROUPS:
            for sub in self._GROUPS[name]:
                self._sub(sub, on_sub)
            return
        self._sub(name, on_sub)

    def _sub(self, name, on_sub):
        if on_sub:
            on_sub(name, "begin")
        self._launch(name)
        if on_sub:
            on_sub(name, "end")

    def _launch(self, name: str):
        c = self.ctx
        if name == "mcp":
            c.mc(self.dst, self.refs, self.mc_units, self.lmcs_fwd, intra=self.intra)
        elif name == "mcx":
            if self.mcx_units and self.aff_units:       # both kinds: one launch (the "mca" sub-stage is then empty)
                c.mcxa(self.dst, self.refs, self.mcx_units, self.aff_units, self.aff_side, self.lmcs_fwd, self.mv_out)
            elif self.mcx_units:
                c.mcx(self.dst, self.refs, self.mcx_units, self.lmcs_fwd, self.mv_out)
        elif name == "mca":
            if self.aff_units and not self.mcx_units:
                c.mca(self.dst, self.refs, self.aff_units, self.aff_side, self.lmcs_fwd)
        elif name == "ciip":
            if self.ciip_units:
                c.ciip(self.dst, self.intra, self.ciip_units)
        elif name == "itx_l":
            k = self.wl.tb_classes
            c.itx_classes(self.dst, self.tb_cmds, self.coefs, 0, k[0], k[1])
        elif name == "lmcs_scale":
            if self.lmcs_regions:
                c.lmcs_scale(self.dst, self.lmcs_regions, self.lmcs, self.lmcs_scales)
        elif name == "itx_c":
            k = self.wl.tb_classes
            if self.lmcs is not None and k[3]:          # the inverse mapping rides in the chroma launch ("lmcs_inv" is then empty)
                c.itx_chroma_lmcs(self.dst, self.tb_cmds, self.coefs, k[0] + k[1], k[2], k[3], self.lmcs_scales, self.lmcs_bwd)
            elif k[2] + k[3]:
                c.itx_classes(self.dst, self.tb_cmds, self.coefs, k[0] + k[1], k[2], k[3], self.lmcs_scales)
        elif name == "lmcs_inv":
            if self.lmcs is not None and not self.wl.tb_classes[3]:
                c.lmcs_inverse(self.dst, self.lmcs_bwd)
        elif name == "dbf":
            c.dbf_edges(self.dst, self.dbf_v, self.dbf_h, self.wl.dbf_planes["beta_offset"], self.wl.dbf_planes["tc_offset"])
        elif name == "sao":
            c.sao(self.tmp, self.dst, self.sao_params, self.log2_ctu)
        elif name == "alf":
            c.alf(self.dst, self.tmp, self.alf)
        else:
            raise ValueError(name)

    def decode(self, stages=STAGES):
        for s in stages:
            self.run_stage(s)

    def result(self):
        self.ctx.sync()
        return self.dst.download()

    def refined_mvs(self) -> np.ndarray:
        """int32 [n_mcx_units, 4]: the motion vectors the BDOF / DMVR units finally used."""
        self.ctx.sync()
        return self.mv_out.download(np.int32).reshape(-1, 4) if self.mv_out else np.zeros((0, 4), np.int32)

    def free(self):
        for b in self.bufs + [self.alf]:
            b.free()
        for p in self.refs + [self.dst, self.tmp] + ([self.intra] if self.intra else []):
            p.free()


class Job:
    """One picture in flight through the C-side flush (ovhip_job_*): the recorder's arrays are page-locked, `flush`
    enqueues H2D + every stage launch + the D2H of the refined motion vectors and returns without waiting."""

    def __init__(self, ctx: Context, w: int, h: int):
        self.ctx, self.lib, self.w, self.h = ctx, ctx.lib, w, h
        j = C.c_void_p()
        ctx._chk(self.lib.ovhip_job_create(ctx.h, w, h, C.byref(j)), "job_create")
        self.j = j
        self.rec = capi.Recorder.__new__(capi.Recorder)          # a view of the job's recorder (not owned)
        self.rec.lib, self.rec.h, self.rec._keep = self.lib, self.lib.ovhip_job_recorder(j), []
        self._keep = {}

    def close(self):
        if self.j:
            self.rec.h = None
            self.lib.ovhip_job_destroy(self.j)
            self.j = None

    def begin(self):
        self.ctx._chk(self.lib.ovhip_job_begin(self.j), "job_begin")

    def load_workload(self, wl):
        """Replay a recorded picture (synth.Workload) into the job's recorder: commands, arena, edge lists."""
        self.begin()
        r = self.rec
        for which, arr in ((capi.REC_COEF, wl.coefs), (capi.REC_TB, wl.tb_cmds), (capi.REC_MC, wl.mc_units),
                           (capi.REC_MCX, wl.mcx_units), (capi.REC_AFF, wl.aff_units), (capi.REC_SIDE, wl.aff_side),
                           (capi.REC_REGION, wl.lmcs_regions), (capi.REC_CIIP, wl.ciip_units), (capi.REC_ITASK, wl.itasks),
                           (capi.REC_EDGE_V, wl.dbf_edges[0]), (capi.REC_EDGE_H, wl.dbf_edges[1])):
            if arr is not None and len(arr):
                r.append_raw(which, arr)
        offs = capi.DbfOffsets()
        for i in range(8):
            offs.beta[i], offs.tc[i] = wl.dbf_planes["beta_offset"], wl.dbf_planes["tc_offset"]
        self.ctx._chk(self.lib.ovhip_rec_set_dbf_offsets(r.h, C.byref(offs), 1), "set_dbf_offsets")
        self.params = self.make_params(wl)

    def make_params(self, wl, log2_ctu: int = 7, stages: int = 0) -> "capi.JobParams":
        keep = self._keep
        keep["sao"] = np.ascontiguousarray(wl.sao_params)
        keep["alf"] = {k: np.ascontiguousarray(wl.alf[k], dtype=dt) for k, dt in capi.ALF_TABLES}
        keep["lmcs"] = wl.lmcs
        a = keep["alf"]
        p = capi.JobParams()
        p.lmcs = C.addressof(wl.lmcs) if wl.lmcs is not None else None
        p.sao = keep["sao"].ctypes.data
        p.alf_ctus = a["ctus"].ctypes.data
        p.alf_luma_coeff, p.alf_luma_clip = a["luma_coeff"].ctypes.data, a["luma_clip"].ctypes.data
        p.alf_chroma_coeff, p.alf_chroma_clip = a["chroma_coeff"].ctypes.data, a["chroma_clip"].ctypes.data
        p.alf_cc_coeff = a["cc_coeff"].ctypes.data
        p.log2_ctu_s, p.stages = log2_ctu, stages
        return p

    def flush(self, dst: "DevPic", refs: list, intra: "DevPic | None" = None, params=None):
        arr = (capi.Pic * max(len(refs), 1))(*[r.s for r in refs])
        self.ctx._chk(self.lib.ovhip_job_flush(self.j, C.byref(dst.s), arr, len(refs), C.byref(intra.s) if intra else None,
                                               C.byref(params if params is not None else self.params)), "job_flush")

    def wait(self):
        self.ctx._chk(self.lib.ovhip_job_wait(self.j), "job_wait")

    def band(self, dst: "DevPic", refs: list, row_end: int, last: bool = False, upto: "capi.BandCounts | None" = None, params=None):
        """ovhip_job_band: what was recorded since the previous call (or up to `upto`) as one band of CTU rows ending at row_end"""
        arr = (capi.Pic * max(len(refs), 1))(*[r.s for r in refs])
        self.ctx._chk(self.lib.ovhip_job_band(self.j, C.byref(dst.s), arr, len(refs), C.byref(params if params is not None else self.params),
                                              C.byref(upto) if upto is not None else None, row_end, int(last)), "job_band")

    def band_progress(self) -> int:
        rows = C.c_int32()
        self.ctx._chk(self.lib.ovhip_job_band_progress(self.j, C.byref(rows), None, None), "job_band_progress")
        return rows.value

    def flush_in_bands(self, wl, dst: "DevPic", refs: list, ctu_rows_per_band: int = 1, log2_ctu: int = 7, params=None):
        """A recorded picture (load_workload(wl) before) submitted band by band, as the live decoder's row hooks do while the picture is
        parsed: the counts of every array at each band's last CTU row come from the commands' positions (the arrays are in decoding order)."""
        rows = list(range(ctu_rows_per_band << log2_ctu, self.h, ctu_rows_per_band << log2_ctu))
        cuts = band_counts(wl, rows, log2_ctu)
        for r, c in zip(rows, cuts):
            self.band(dst, refs, r, False, c, params)
        self.band(dst, refs, self.h, True, None, params)

    def bind(self, ctx: "Context"):
        """The next flushes go to ctx's stream (a free frame thread takes the picture over)."""
        self.ctx._chk(self.lib.ovhip_job_bind(self.j, ctx.h), "job_bind")
        self.ctx = ctx

    def dmvr_rows(self, refs: list) -> int:
        arr = (capi.Pic * max(len(refs), 1))(*[r.s for r in refs])
        n = self.lib.ovhip_job_dmvr_rows(self.j, arr, len(refs))
        if n < 0:
            self.ctx._chk(int(n), "job_dmvr_rows")
        return int(n)

    def dmvr_rows_begin(self, refs: list, log2_ctu: int = 0) -> int:
        """enqueue the eager pass over the refined units recorded since the last one (log2_ctu != 0: + their TMVP plane entries)"""
        arr = (capi.Pic * max(len(refs), 1))(*[r.s for r in refs])
        n = self.lib.ovhip_job_dmvr_rows_begin(self.j, arr, len(refs), log2_ctu)
        if n < 0:
            self.ctx._chk(int(n), "job_dmvr_rows_begin")
        return int(n)

    def dmvr_rows_collect(self) -> int:
        n = self.lib.ovhip_job_dmvr_rows_collect(self.j)
        if n < 0:
            self.ctx._chk(int(n), "job_dmvr_rows_collect")
        return int(n)

    def refined_mvs(self) -> np.ndarray:
        n = C.c_size_t()
        p = self.lib.ovhip_job_refined_mvs(self.j, C.byref(n))
        if not n.value:
            return np.zeros((0, 4), np.int32)
        return np.frombuffer((C.c_int32 * (4 * n.value)).from_address(p), dtype=np.int32).reshape(-1, 4).copy()

    def mvfield(self, fmt: "capi.MvfieldFormat | None", vec=None, info=None, vec_bytes: "int | None" = None, info_bytes: "int | None" = None,
                check: bool = True) -> int:
        """ovhip_job_mvfield after wait() of a whole-picture flush: the picture's motion field into `vec` and `info` (as
        Context.mvfield takes them), from the device copies the flush placed.  Asynchronous on the job's context."""
        vp, vb, ip, ib, _n = _mvfield_dsts(vec, info, fmt, self.w, self.h, vec_bytes, info_bytes) if fmt is not None else (vec or 0, vec_bytes or 0, info or 0, info_bytes or 0, None)
        r = self.lib.ovhip_job_mvfield(self.j, C.byref(fmt) if fmt is not None else None, C.c_void_p(vp) if vp else None, vb, C.c_void_p(ip) if ip else None, ib)
        if check:
            self.ctx._chk(r, "job_mvfield")
        return r

    def tmvp_cells(self) -> np.ndarray:
        """ovhip_job_tmvp_cells after wait(): capi.TMVP_CELL_DTYPE, 4 entries per refined unit (cell == capi.TMVP_NONE: unused)"""
        n = C.c_size_t()
        p = self.lib.ovhip_job_tmvp_cells(self.j, C.byref(n))
        if not n.value:
            return np.zeros(0, capi.TMVP_CELL_DTYPE)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n.value * capi.TMVP_CELL_DTYPE.itemsize,)).view(capi.TMVP_CELL_DTYPE).copy()

    def test_abort_next_flow(self):
        """test hook: the next flush's flow launch is abandoned for real (ovhip_job_test_abort_next_flow)"""
        self.ctx._chk(self.lib.ovhip_job_test_abort_next_flow(self.j), "job_test_abort_next_flow")

    def stats(self) -> "capi.JobStats":
        s = capi.JobStats()
        self.lib.ovhip_job_last_stats(self.j, C.byref(s))
        return s

    def time_stage(self, name: "str | None"):
        self.ctx._chk(self.lib.ovhip_job_time_stage(self.j, capi.TIME_STAGES.index(name) if name else -1), "job_time_stage")

    def stage_time(self):
        """(sum of the bracketed launch group's durations in seconds, number of flushes measured)"""
        s, n = C.c_double(), C.c_uint64()
        self.ctx._chk(self.lib.ovhip_job_stage_time(self.j, C.byref(s), C.byref(n)), "job_stage_time")
        return s.value * 1e-3, n.value


def band_counts(wl, rows, log2_ctu: int = 7) -> list:
    """capi.BandCounts of a recorded picture at each luma row of `rows` (CTU-row boundaries): how many entries of every array belong
    to the CTU rows above it.  The arrays must be in decoding order (CTU rows ascending) -- checked."""
    def cut(ctu_row, what):
        ctu_row = np.asarray(ctu_row, np.int64)
        if len(ctu_row) > 1 and (np.diff(ctu_row) < 0).any():
            raise EngineError(f"band_counts: {what} are not in CTU-row order")
        return [int(np.searchsorted(ctu_row, r >> log2_ctu, side="left")) for r in rows]

    def arr(a, dt):
        return np.zeros(0, dt) if a is None or not len(a) else np.asarray(a).view(dt).reshape(-1)

    tb, mc, mcx = arr(wl.tb_cmds, capi.TB_CMD_DTYPE), arr(wl.mc_units, capi.MC_UNIT_DTYPE), arr(wl.mcx_units, capi.MC_UNIT_DTYPE)
    aff, reg, it = arr(wl.aff_units, capi.AFF_UNIT_DTYPE), arr(wl.lmcs_regions, capi.LMCS_REGION_DTYPE), arr(wl.itasks, capi.ITASK_DTYPE)
    ev, eh = arr(wl.dbf_edges[0], capi.DBF_EDGE_DTYPE), arr(wl.dbf_edges[1], capi.DBF_EDGE_DTYPE)
    n_coef = 0 if wl.coefs is None else len(wl.coefs)
    n_side = 0 if wl.aff_side is None else len(wl.aff_side)
    tb_row = (tb["y"].astype(np.int64) << (tb["plane"] != 0)) >> log2_ctu
    it_chroma = (it["kind"] == capi.IT_CHROMA) | (it["kind"] == capi.IT_RES_C)
    it_row = (it["y"].astype(np.int64) << it_chroma) >> log2_ctu
    k_tb, k_mc, k_mcx = cut(tb_row, "transform blocks"), cut(mc["y"] >> log2_ctu, "MC units"), cut(mcx["y"] >> log2_ctu, "refined units")
    k_aff, k_reg, k_it = cut(aff["y"] >> log2_ctu, "affine units"), cut(reg["y"] >> log2_ctu, "regions"), cut(it_row, "ordered tasks")
    # an edge's uy counts units of 4 LUMA samples in every plane (the 4x4-luma grid of the deblocking maps)
    k_ev = cut((ev["uy"].astype(np.int64) << 2) >> log2_ctu, "vertical edges")
    k_eh = cut((eh["uy"].astype(np.int64) << 2) >> log2_ctu, "horizontal edges")
    out = []
    for i in range(len(rows)):
        c = capi.BandCounts()
        c.n_tb, c.n_mc, c.n_mcx, c.n_aff, c.n_reg, c.n_itask, c.n_edge_v, c.n_edge_h = k_tb[i], k_mc[i], k_mcx[i], k_aff[i], k_reg[i], k_it[i], k_ev[i], k_eh[i]
        # the arenas are appended with the commands that own their entries: a band's share ends where the next band's first owner starts
        later = tb["coef_off"][k_tb[i]:]
        c.n_coef = int(later.min()) if len(later) else n_coef
        la = aff[k_aff[i]:]
        c.n_side = int(min(la["side_off"].min(), la["prof_off"][(la["flags"] & 1) != 0].min(initial=0xffffffff))) if len(la) else n_side
        out.append(c)
    return out


class Dpb:
    """Device mirror of the decoded picture buffer (ovhip_dpb_*): `devices` = HIP ordinals of the logical devices."""

    def __init__(self, devices=(0,), ops: "capi.DpbOps | None" = None, n_devices: int | None = None):
        self.lib = capi.load()
        h = C.c_void_p()
        if ops is not None:
            self._ops = ops
            r = self.lib.ovhip_dpb_create_ex(C.byref(h), n_devices or 1, C.byref(ops))
        else:
            arr = (C.c_int * len(devices))(*devices)
            r = self.lib.ovhip_dpb_create(C.byref(h), arr, len(devices))
        if r != 0:
            raise EngineError(f"ovhip_dpb_create: {r} (no HIP device? the DPB has no CPU back-end outside the tests' own)")
        self.h = h

    def close(self):
        if self.h:
            self.lib.ovhip_dpb_destroy(self.h)
            self.h = None

    def stats(self) -> "capi.DpbStats":
        st = capi.DpbStats()
        self.lib.ovhip_dpb_get_stats(self.h, C.byref(st))
        return st

    def begin(self, key: int, dev: int, w: int, h: int, tag: int = 0) -> "capi.Pic":
        pic = capi.Pic()
        r = self.lib.ovhip_dpb_begin_tag(self.h, C.c_void_p(key), tag, dev, w, h, C.byref(pic))
        if r != 0:
            raise EngineError(f"ovhip_dpb_begin: {r}")
        return pic

    def lookup(self, key: int) -> "tuple[int, capi.Pic]":
        pic, dev = capi.Pic(), C.c_int()
        r = self.lib.ovhip_dpb_lookup(self.h, C.c_void_p(key), C.byref(dev), C.byref(pic))
        if r != 0:
            raise EngineError(f"ovhip_dpb_lookup: {r}")
        return dev.value, pic


class Frame:
    """One frame thread (ovhip_frame_*): context + job on a logical device of a DPB."""

    def __init__(self, dpb: Dpb, dev: int, w: int, h: int):
        self.lib, self.dpb, self.w, self.h = dpb.lib, dpb, w, h
        f = C.c_void_p()
        r = self.lib.ovhip_frame_create(dpb.h, dev, w, h, C.byref(f))
        if r != 0:
            raise EngineError(f"ovhip_frame_create: {r}")
        self.f = f

    def _chk(self, r, what):
        if r < 0:
            raise EngineError(f"{what}: {r}: {self.lib.ovhip_frame_last_error(self.f).decode()}")
        return r

    def close(self):
        if self.f:
            self.lib.ovhip_frame_destroy(self.f)
            self.f = None

    def begin(self, key: int, tag: int = 0):
        self._chk(self.lib.ovhip_frame_begin_tag(self.f, C.c_void_p(key), tag), "frame_begin")

    def ref(self, key: int, tag: int = 0) -> int:
        return self._chk(self.lib.ovhip_frame_ref_tag(self.f, C.c_void_p(key), tag), "frame_ref")

    def ref_at(self, slot: int, key: int) -> int:
        return self._chk(self.lib.ovhip_frame_ref_at(self.f, slot, C.c_void_p(key)), "frame_ref_at")

    def recorder(self) -> "capi.Recorder":
        r = capi.Recorder.__new__(capi.Recorder)
        r.lib, r.h, r._keep = self.lib, self.lib.ovhip_frame_recorder(self.f), []
        if not r.h:
            raise EngineError("ovhip_frame_recorder")
        r.close = lambda: None                                     # owned by the frame's job
        return r

    def dmvr_rows(self) -> int:
        return int(self._chk(self.lib.ovhip_frame_dmvr_rows(self.f), "frame_dmvr_rows"))

    def dmvr_rows_begin(self, log2_ctu: int = 7) -> int:
        return int(self._chk(self.lib.ovhip_frame_dmvr_rows_begin(self.f, log2_ctu), "frame_dmvr_rows_begin"))

    def dmvr_rows_collect(self) -> int:
        return int(self._chk(self.lib.ovhip_frame_dmvr_rows_collect(self.f), "frame_dmvr_rows_collect"))

    def submit(self, params: "capi.JobParams", job: "Job | None" = None, out: "capi.FrameOutput | None" = None, check: bool = True) -> int:
        r = self.lib.ovhip_frame_submit(self.f, job.j if job is not None else None, None, C.byref(params), C.byref(out) if out is not None else None)
        return self._chk(r, "frame_submit") if check else r

    def fail(self, status: int = -3):
        self.lib.ovhip_frame_fail(self.f, status)

    def set_film_grain(self, params, poc: int = 0, check: bool = True) -> int:
        """ovhip_frame_set_film_grain: the outputs deliver the picture with film grain at `poc`; params None switches it off"""
        r = self.lib.ovhip_frame_set_film_grain(self.f, C.byref(params) if params is not None else None, poc)
        if check and r:
            raise EngineError(f"frame_set_film_grain: {r}")
        return r

    def set_picture_hash(self, method: int, n_planes: int = 3, expected: "capi.PicHashValue | None" = None, check: bool = True) -> int:
        """ovhip_frame_set_picture_hash: every following picture is hashed after its decode (method < 0: off); expected: the SEI's value"""
        r = self.lib.ovhip_frame_set_picture_hash(self.f, method, n_planes, C.byref(expected) if expected is not None else None)
        if check and r:
            raise EngineError(f"frame_set_picture_hash: {r}")
        return r

    def picture_hash(self) -> "tuple[int, capi.PicHashValue]":
        """(1 equal or nothing expected / 0 differs / OVHIP_EINVAL nothing computed, the last picture's hash)"""
        out = capi.PicHashValue()
        return self.lib.ovhip_frame_picture_hash(self.f, C.byref(out)), out

    def set_output_scale(self, out_w: int, out_h: int, scale_window=(0, 0, 0, 0), col=(0, 0), check: bool = True) -> int:
        """the frame's outputs deliver the picture resampled to out_w x out_h; (0, 0) switches it off"""
        info = capi.ScaleInfo(*scale_window, *col)
        r = self.lib.ovhip_frame_set_output_scale(self.f, out_w, out_h, C.byref(info))
        if r < 0 and check:
            raise EngineError(f"frame_set_output_scale: {r}")
        if r >= 0:
            self._out_size = (out_w, out_h) if out_w or out_h else None
        return r

    def set_output_reduce(self, out_w: int, out_h: int, src_window=(0, 0, 0, 0), chroma_loc: int = 0, check: bool = True) -> int:
        """the frame's outputs (RGB, surface, PACKED / PLANES / DIGEST) read the picture reduced to out_w x out_h; (0, 0) switches it off"""
        info = capi.ReduceInfo(capi.Window(*src_window), chroma_loc)
        r = self.lib.ovhip_frame_set_output_reduce(self.f, out_w, out_h, C.byref(info))
        if r < 0 and check:
            raise EngineError(f"frame_set_output_reduce: {r}")
        if r >= 0:
            self._out_size = (out_w, out_h) if out_w or out_h else None
        return r

    def set_rgb_output(self, dst, fmt: "capi.RgbFormat | None", window=(0, 0, 0, 0), nbytes: "int | None" = None, check: bool = True) -> int:
        """ovhip_frame_set_rgb_output: the NEXT picture completed is also written as RGB into `dst` -- a torch tensor on the device of
        shape (3, H, W) / (H, W, 3) for the size the frame outputs (checked here), or a device address with `nbytes`; fmt None: off"""
        return _set_output(self, "rgb", fmt, [(dst, nbytes)], window, check=check)

    def set_rgb_lut(self, lut: "RgbLut | None", check: bool = True) -> int:
        """ovhip_frame_set_rgb_lut: while set, every RGB output of this frame goes through the colour table (sticky, unlike the
        destination; kept alive here); None: off"""
        return _set_lut(self, "rgb", lut, check=check)

    def set_surface_lut(self, lut: "RgbLut | None", conv: "capi.SurfaceConv | None" = None, check: bool = True) -> int:
        """ovhip_frame_set_surface_lut: while set, every surface output of this frame is that of the picture converted by `conv`
        (surface_conv()) through the colour table (sticky, unlike the destination; kept alive here; independent of set_rgb_lut);
        None: off"""
        return _set_lut(self, "surface", lut, conv=conv, check=check)

    def set_ladder_lut(self, lut: "RgbLut | None", conv: "capi.SurfaceConv | None" = None, check: bool = True) -> int:
        """ovhip_frame_set_ladder_lut: while set, the rungs of this frame's ladder output are those of the reduced pictures converted
        by `conv` (surface_conv()) through the colour table (sticky, unlike the rungs; kept alive here; independent of set_rgb_lut
        and set_surface_lut); None: off"""
        return _set_lut(self, "ladder", lut, conv=conv, check=check)

    def set_surface_output(self, dst, fmt: "capi.SurfaceFormat | None", window=(0, 0, 0, 0), nbytes: "int | None" = None, check: bool = True) -> int:
        """ovhip_frame_set_surface_output: the NEXT picture completed is also written as a surface into `dst` -- a contiguous torch
        tensor on the device (uint8, or int16 / uint16 for the 16-bit formats) of at least the surface's bytes for the size the frame
        outputs (checked here), or a device address with `nbytes`; fmt None: off"""
        return _set_output(self, "surface", fmt, [(dst, nbytes)], window, check=check)

    def set_ladder_output(self, rungs, src_window=(0, 0, 0, 0), chroma_loc: int = 0, check: bool = True) -> int:
        """ovhip_frame_set_ladder_output: the NEXT picture completed is also written as the rungs of a ladder (ladder_rung() with torch
        tensors on the device, kept alive here, or device addresses); None: off"""
        return _set_levels(self, "ladder", rungs, capi.ReduceInfo(capi.Window(*src_window), chroma_loc), check=check)

    def set_rgb_pyramid_output(self, levels, src_window=(0, 0, 0, 0), chroma_loc: "int | None" = None, check: bool = True) -> int:
        """ovhip_frame_set_rgb_pyramid_output: the NEXT picture completed is also written as the levels of an RGB pyramid (rgb_level()
        with torch tensors on the device, kept alive here, or device addresses); None: off.  chroma_loc None: the first level's"""
        levels = list(levels) if levels is not None else None
        return _set_levels(self, "rgb_pyramid", levels, None if levels is None else _pyramid_info(levels, src_window, chroma_loc), check=check)

    def set_rgb_pyramid_lut(self, lut: "RgbLut | None", check: bool = True) -> int:
        """ovhip_frame_set_rgb_pyramid_lut: while set, the levels of this frame's RGB pyramid output go through the colour table (sticky,
        unlike the levels; kept alive here; independent of the other outputs' tables); None: off"""
        return _set_lut(self, "rgb_pyramid", lut, check=check)

    def set_mvfield_output(self, fmt: "capi.MvfieldFormat | None", vec=None, info=None, vec_bytes: "int | None" = None, info_bytes: "int | None" = None,
                           check: bool = True) -> int:
        """ovhip_frame_set_mvfield_output: the motion field of the NEXT picture completed goes to `vec` and `info` -- torch tensors on
        the device of mvfield_shape() for the frame's size (checked here, kept alive here), device addresses with their byte counts,
        or None for a destination that is not wanted; fmt None: off"""
        return _set_output(self, "mvfield", fmt, [(vec, vec_bytes), (info, info_bytes)], check=check)

    def job(self) -> "Job":
        """the frame's own job as an engine.Job view (not owned)"""
        j = Job.__new__(Job)
        ctx = Context.__new__(Context)
        ctx.lib, ctx.h, ctx._bufs = self.lib, C.c_void_p(self.lib.ovhip_frame_ctx(self.f)), []
        j.ctx, j.lib, j.w, j.h, j.j, j._keep = ctx, self.lib, self.w, self.h, C.c_void_p(self.lib.ovhip_frame_job(self.f)), {}
        j.rec = self.recorder()
        return j


class Stream:
    """The C stream driver (ovhip_stream_*): frame threads per device decoding a list of pictures in decoding order.

    contents: list of dicts {"params": capi.JobParams, "calllog": np.ndarray | None, "n_ref_slots": int}; jobs: engine.Job list
    (pre-recorded pictures).  Everything referenced stays alive as long as this object."""

    def __init__(self, dpb: Dpb, w: int, h: int, contents: list, jobs: list = (), threads_per_device: int = 1, flags: int = 0,
                 output: int = 0, window=(0, 0, 0, 0), extra_stages: int = 0, rank: int = 0, xfer: "capi.StreamXfer | None" = None,
                 intra_lookahead: int = 0, ahead_own_queue: int = 0):
        self.lib, self.dpb = dpb.lib, dpb
        self._contents = (capi.StreamContent * len(contents))()
        self._keep = [contents, jobs, xfer]
        for i, c in enumerate(contents):
            sc = self._contents[i]
            log = c.get("calllog")
            sc.calllog = log.ctypes.data if log is not None else None
            sc.calllog_bytes = log.nbytes if log is not None else 0
            sc.params = c["params"]
            sc.n_ref_slots = c.get("n_ref_slots", 2)
        self._jobs = (C.c_void_p * max(1, len(jobs)))(*[j.j for j in jobs])
        cfg = capi.StreamCfg()
        cfg.w, cfg.h, cfg.flags, cfg.threads_per_device, cfg.output = w, h, flags, threads_per_device, output
        cfg.window = capi.Window(*window)
        cfg.extra_stages, cfg.rank = extra_stages, rank
        # a capi.StreamXfer of Python callbacks, or the address of a C one (RcclTransport.xfer: ovhip_rccl_xfer)
        cfg.xfer = (C.cast(C.c_void_p(xfer), C.POINTER(capi.StreamXfer)) if isinstance(xfer, int) else C.pointer(xfer)) if xfer is not None else None
        cfg.intra_lookahead, cfg.ahead_own_queue = intra_lookahead, ahead_own_queue
        self.cfg = cfg
        s = C.c_void_p()
        r = self.lib.ovhip_stream_create(C.byref(s), dpb.h, C.byref(cfg), self._contents, len(contents), self._jobs, len(jobs))
        if r != 0:
            raise EngineError(f"ovhip_stream_create: {r}")
        self.s = s

    def close(self):
        if self.s:
            self.lib.ovhip_stream_destroy(self.s)
            self.s = None

    def set_film_grain(self, params, check: bool = True) -> int:
        """ovhip_stream_set_film_grain: every picture of the following runs leaves with film grain at its own POC; None: off"""
        r = self.lib.ovhip_stream_set_film_grain(self.s, C.byref(params) if params is not None else None)
        if check and r:
            raise EngineError(f"stream_set_film_grain: {r}")
        return r

    def set_output_scale(self, out_w: int, out_h: int, scale_window=(0, 0, 0, 0), col=(0, 0), check: bool = True) -> int:
        """before a run: the PACKED frames / DIGEST fingerprints are those of the pictures resampled to out_w x out_h; (0, 0): off"""
        info = capi.ScaleInfo(*scale_window, *col)
        r = self.lib.ovhip_stream_set_output_scale(self.s, out_w, out_h, C.byref(info))
        if r < 0 and check:
            raise EngineError(f"stream_set_output_scale: {r}")
        if r >= 0:
            self._out_size = (out_w, out_h) if out_w or out_h else None
        return r

    def set_output_reduce(self, out_w: int, out_h: int, src_window=(0, 0, 0, 0), chroma_loc: int = 0, check: bool = True) -> int:
        """before a run and before the RGB / surface setters: every output that shows the picture reads it reduced to out_w x out_h;
        (0, 0): off"""
        info = capi.ReduceInfo(capi.Window(*src_window), chroma_loc)
        r = self.lib.ovhip_stream_set_output_reduce(self.s, out_w, out_h, C.byref(info))
        if r < 0 and check:
            raise EngineError(f"stream_set_output_reduce: {r}")
        if r >= 0:
            self._out_size = (out_w, out_h) if out_w or out_h else None
        return r

    def set_rgb_output(self, dst, fmt: "capi.RgbFormat | None", window=(0, 0, 0, 0), bytes_per_picture: "int | None" = None,
                       n_slots: "int | None" = None, check: bool = True) -> int:
        """ovhip_stream_set_rgb_output: picture idx of the following runs is also written as RGB into slot idx % n of `dst` -- a torch
        tensor on the device of shape (n, 3, H, W) / (n, H, W, 3) for the size the stream outputs (checked here, kept alive here), or
        a device address with bytes_per_picture and n_slots; fmt None: off"""
        return _set_output(self, "rgb", fmt, [(dst, bytes_per_picture)], window, n_slots, check)

    def set_rgb_lut(self, table: "np.ndarray | None", peak: int = 0, check: bool = True) -> int:
        """ovhip_stream_set_rgb_lut: the RGB output of the following runs goes through the colour table (numpy uint16 of shape
        (S, S, S, 3), uploaded once per device, owned by the stream); None: off"""
        return _set_lut(self, "rgb", table, peak, check=check)

    def set_surface_lut(self, table: "np.ndarray | None", peak: int = 0, conv: "capi.SurfaceConv | None" = None, check: bool = True) -> int:
        """ovhip_stream_set_surface_lut: the surface output of the following runs is that of the pictures converted by `conv`
        (surface_conv()) through the colour table (numpy uint16 of shape (S, S, S, 3), uploaded once per device, owned by the
        stream); None: off"""
        return _set_lut(self, "surface", table, peak, conv, check)

    def set_ladder_lut(self, table: "np.ndarray | None", peak: int = 0, conv: "capi.SurfaceConv | None" = None, check: bool = True) -> int:
        """ovhip_stream_set_ladder_lut: the ladder output of the following runs is that of the reduced pictures converted by `conv`
        (surface_conv()) through the colour table (numpy uint16 of shape (S, S, S, 3), uploaded once per device, owned by the
        stream); None: off"""
        return _set_lut(self, "ladder", table, peak, conv, check)

    def set_surface_output(self, dst, fmt: "capi.SurfaceFormat | None", window=(0, 0, 0, 0), bytes_per_picture: "int | None" = None,
                           n_slots: "int | None" = None, check: bool = True) -> int:
        """ovhip_stream_set_surface_output: picture idx of the following runs is also written as a surface into slot idx % n of `dst` --
        a contiguous torch tensor on the device whose first dimension is the slot count and whose slots hold at least the surface's
        bytes for the size the stream outputs (checked here, kept alive here), or a device address with bytes_per_picture and n_slots;
        fmt None: off"""
        return _set_output(self, "surface", fmt, [(dst, bytes_per_picture)], window, n_slots, check)

    def set_ladder_output(self, rungs, src_window=(0, 0, 0, 0), chroma_loc: int = 0, n_slots: "int | None" = None, check: bool = True) -> int:
        """ovhip_stream_set_ladder_output: picture idx of the following runs is also written as the rungs of a ladder, rung r into slot
        idx % n of its own destination -- ladder_rung(..., slots=True) with a contiguous torch tensor on the device whose first
        dimension is the slot count (the same for every rung; kept alive here), or device addresses with the bytes per picture and
        n_slots; None: off"""
        return _set_levels(self, "ladder", rungs, capi.ReduceInfo(capi.Window(*src_window), chroma_loc), n_slots, check)

    def set_rgb_pyramid_output(self, levels, src_window=(0, 0, 0, 0), chroma_loc: "int | None" = None, n_slots: "int | None" = None, check: bool = True) -> int:
        """ovhip_stream_set_rgb_pyramid_output: picture idx of the following runs is also written as the levels of an RGB pyramid, level r
        into slot idx % n of its own destination -- rgb_level(..., slots=True) with a contiguous torch tensor on the device whose first
        dimension is the slot count (the same for every level; kept alive here), or device addresses with the bytes per picture and
        n_slots; None: off.  chroma_loc None: the first level's"""
        levels = list(levels) if levels is not None else None
        return _set_levels(self, "rgb_pyramid", levels, None if levels is None else _pyramid_info(levels, src_window, chroma_loc), n_slots, check)

    def set_rgb_pyramid_lut(self, table: "np.ndarray | None", peak: int = 0, check: bool = True) -> int:
        """ovhip_stream_set_rgb_pyramid_lut: the RGB pyramid output of the following runs goes through the colour table (numpy uint16 of
        shape (S, S, S, 3), uploaded once per device, owned by the stream); None: off"""
        return _set_lut(self, "rgb_pyramid", table, peak, check=check)

    def set_mvfield_output(self, fmt: "capi.MvfieldFormat | None", vec=None, info=None, vec_bytes_per_picture: "int | None" = None,
                           info_bytes_per_picture: "int | None" = None, n_slots: "int | None" = None, check: bool = True) -> int:
        """ovhip_stream_set_mvfield_output: the motion field of picture idx of the following runs goes to slot idx % n of `vec` and
        `info` -- torch tensors on the device whose first dimension is the slot count and whose slots have mvfield_shape() for the
        stream's size (checked here, kept alive here), device addresses with bytes per picture and n_slots, or None; fmt None: off"""
        return _set_output(self, "mvfield", fmt, [(vec, vec_bytes_per_picture), (info, info_bytes_per_picture)], n_slots=n_slots, check=check)

    def set_picture_hashes(self, method: int, n_planes: int = 3, expected=None, check: bool = True) -> int:
        """ovhip_stream_set_picture_hashes; expected: a (capi.PicHashValue * n_total) array (kept alive here) or None"""
        self._keep.append(expected)
        r = self.lib.ovhip_stream_set_picture_hashes(self.s, method, n_planes, expected)
        if check and r:
            raise EngineError(f"stream_set_picture_hashes: {r}")
        return r

    def picture_hashes(self, n: int):
        """of the last run of n pictures -> (status, [capi.PicHashValue] * n, n_mismatch, first_mismatch)"""
        out = (capi.PicHashValue * max(1, n))()
        nm, fm = C.c_uint32(), C.c_int32()
        r = self.lib.ovhip_stream_picture_hashes(self.s, out, C.byref(nm), C.byref(fm))
        return r, list(out)[:n], nm.value, fm.value

    def queue_info(self):
        """(streams replaced to clear the look-ahead thread's hardware queue, in-order streams still sharing it)"""
        a, b = C.c_int(), C.c_int()
        self.lib.ovhip_stream_queue_info(self.s, C.byref(a), C.byref(b))
        return a.value, b.value

    def picture(self, idx: int, ctx: "Context") -> "DevPic":
        """the device picture of stream picture idx (kept by OVHIP_STREAM_KEEP), as a DevPic on ctx for download()"""
        key = self.lib.ovhip_stream_key(self.s, idx)
        _dev, pic = self.dpb.lookup(key)
        return DevPic(ctx, pic, owns=False)

    @staticmethod
    def pics_array(pics: list):
        """pics: list of dicts (content, job, poc, device, refs, owner, send_mask) -> (capi.StreamPic * n)"""
        arr = (capi.StreamPic * max(1, len(pics)))()
        for i, p in enumerate(pics):
            a = arr[i]
            a.content, a.job, a.poc, a.device = p.get("content", 0), p.get("job", 0), p.get("poc", i), p.get("device", 0)
            refs = list(p.get("refs", ()))
            assert len(refs) <= capi.STREAM_MAX_REFS
            a.n_refs = len(refs)
            for k, r in enumerate(refs):
                a.refs[k] = r
            a.owner, a.send_mask = p.get("owner", 0), p.get("send_mask", 0)
        return arr

    def run(self, arr, n_total: int, first: int, n: int, flags: int = 0, digests: bool = False, check: bool = True, trace=None):
        """-> (capi.StreamResult, digests uint8 [n, 16] | None); trace: float64 [n, 8] filled with (taken, submit, published, thread, references in hand, launches enqueued, submit returned, complete on the device)"""
        res = capi.StreamResult()
        if trace is not None:
            res.trace = trace.ctypes.data
        dg = np.zeros((n, 16), np.uint8) if digests else None
        r = self.lib.ovhip_stream_run(self.s, arr, n_total, first, n, flags | (capi.STREAM_DIGESTS if digests else 0),
                                      dg.ctypes.data if dg is not None else None, C.byref(res))
        if r != 0 and check:
            raise EngineError(f"ovhip_stream_run: {r}: {res.error.decode(errors='replace')}")
        return res, dg


class RcclTransport:
    """ovhip_rccl_*: the stream driver's multi-process exchange over RCCL point-to-point (one process per GPU)."""

    def __init__(self, unique_id: bytes, rank: int, world: int, hip_device: int):
        self.lib = capi.load()
        h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        r = self.lib.ovhip_rccl_create(C.byref(h), buf, rank, world, hip_device)
        if r != 0:
            raise EngineError(f"ovhip_rccl_create: {r}")
        self.h = h

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        r = capi.load().ovhip_rccl_unique_id(buf)
        if r != 0:
            raise EngineError(f"ovhip_rccl_unique_id: {r}")
        return bytes(buf)

    @property
    def xfer(self) -> int:
        return int(self.lib.ovhip_rccl_xfer(self.h))

    def stats(self) -> dict:
        out = (C.c_uint64 * 4)()
        self.lib.ovhip_rccl_stats(self.h, out)
        return {"pictures_sent": int(out[0]), "bytes_sent": int(out[1]), "pictures_received": int(out[2]), "bytes_received": int(out[3])}

    def self_exchange(self, src: "DevPic", dst: "DevPic"):
        r = self.lib.ovhip_rccl_self_exchange(self.h, C.byref(src.s), C.byref(dst.s))
        if r != 0:
            raise EngineError(f"ovhip_rccl_self_exchange: {r}: {self.lib.ovhip_rccl_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.lib.ovhip_rccl_destroy(self.h)
            self.h = None
