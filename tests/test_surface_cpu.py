"""CPU: surface output on the host (openvvc_amd/csrc/ovvc_surface.c): ovhip_surface_host and ovhip_surface_bytes against the numpy
restatement tests/spec_surface.py -- every format, rounding, size and window, strided pictures, layouts with gaps that must stay
unwritten --, the relations between the formats, the dither's property, and the refusals.  The definition is integer only: every
comparison is of bytes."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import spec_surface as ss
from openvvc_amd import capi, engine

ROOT = Path(__file__).resolve().parent.parent
EINVAL = -3
TAIL = 80                                                     # bytes behind the surface that must stay as they were


def c_format(fmt, rounding=0, pitch_y=0, pitch_c=0, offset_c=(0, 0)):
    return engine.surface_format(fmt, rounding, pitch_y, pitch_c, offset_c)


def host_surface(lib, planes, fmt, rounding=0, window=(0, 0, 0, 0), strides=None, **lay):
    """ovhip_surface_host of tight (or strided) planes into a buffer that held 0xA5 -> (the buffer: the surface and TAIL bytes behind
    it, the surface's size by ovhip_surface_bytes)"""
    h, w = planes[0].shape
    sy, sc = strides or (w, w // 2)
    held = []
    for p, s in zip(planes, (sy, sc, sc)):
        a = np.full((p.shape[0], s), 0xA5A5, np.uint16)
        a[:, :p.shape[1]] = p
        held.append(a)
    win, cf = capi.Window(*window), c_format(fmt, rounding, **lay)
    need = lib.ovhip_surface_bytes(w, h, C.byref(win), C.byref(cf))
    assert need, (w, h, fmt, window, lay)
    out = np.full(need + TAIL, ss.FILL, np.uint8)
    r = lib.ovhip_surface_host(held[0].ctypes.data, held[1].ctypes.data, held[2].ctypes.data, w, h, sy, sc, C.byref(win), C.byref(cf),
                               out.ctypes.data, need)
    assert r == 0, r
    return out, need


def check_against_spec(got, need, planes, fmt, rounding, window, what, **lay):
    want, size = ss.surface(planes, fmt, rounding, window, total=len(got), **lay)
    assert need == size, what
    assert got.tobytes() == want.tobytes(), what


def test_struct_layout_and_enums():
    assert C.sizeof(capi.SurfaceFormat) == 32
    assert (capi.SurfaceFormat.pitch_y.offset, capi.SurfaceFormat.pitch_c.offset, capi.SurfaceFormat.offset_c.offset) == (4, 8, 16)
    assert (capi.SURF_NV12, capi.SURF_P010, capi.SURF_I420, capi.SURF_I010) == (ss.NV12, ss.P010, ss.I420, ss.I010) == (0, 1, 2, 3)
    assert (capi.SURF_ROUND, capi.SURF_DITHER) == (ss.ROUND, ss.DITHER) == (0, 1)
    assert capi.OVHIP_ABI_VERSION == 9
    f = engine.surface_format(capi.SURF_I420, capi.SURF_DITHER, 256, 128, (4096, 8192))
    assert (f.format, f.rounding, f.pitch_y, f.pitch_c, tuple(f.offset_c), tuple(f.rsv)) == (2, 1, 256, 128, (4096, 8192), (0, 0))


def test_the_test_planes_hold_the_range_ends_where_the_paths_differ():
    for w, h in ss.SIZES:
        for p in ss.random_planes(w, h, 1):
            ww = p.shape[1]
            assert p.max() <= 1023
            assert set(p[:, 0]) | set(p[:, ww - 1]) >= set(ss.EDGE_VALUES), (w, h)
            assert set(p[:, 1]) | set(p[:, ww - 2]) >= set(ss.EDGE_VALUES), (w, h)
            if ww >= 12:
                assert set(p[:, -(ww % 16 or 16):].ravel()) >= set(ss.EDGE_VALUES), (w, h)


@pytest.mark.parametrize("w,h", ss.SIZES)
def test_host_twin_equals_the_restatement(built_lib, w, h):
    planes = ss.random_planes(w, h, 100 + w)
    for (fmt, rounding) in ss.MODES:
        for wd in ss.windows_for(w, h):
            got, need = host_surface(built_lib, planes, fmt, rounding, wd)
            check_against_spec(got, need, planes, fmt, rounding, wd, (fmt, rounding, wd))


@pytest.mark.parametrize("w,h", ss.SIZES)
def test_host_twin_with_strides_above_the_width(built_lib, w, h):
    planes = ss.random_planes(w, h, 200 + w)
    for (fmt, rounding) in ss.MODES:
        for wd in ss.windows_for(w, h):
            got, need = host_surface(built_lib, planes, fmt, rounding, wd, strides=(w + 7, w // 2 + 3))
            check_against_spec(got, need, planes, fmt, rounding, wd, (fmt, rounding, wd))


@pytest.mark.parametrize("w,h", ss.SIZES)
def test_layouts_with_gaps_leave_the_gaps_unwritten(built_lib, w, h):
    planes = ss.random_planes(w, h, 300 + w)
    for (fmt, rounding) in ss.MODES:
        for wd in ss.windows_for(w, h):
            W, H = w - 2 * (wd[0] + wd[1]), h - 2 * (wd[2] + wd[3])
            lay = ss.loose_layout(fmt, W, H)
            if ss.ELEM[fmt] == 1:
                assert lay["pitch_y"] & 1, "an odd pitch for the 8-bit formats"
            got, need = host_surface(built_lib, planes, fmt, rounding, wd, **lay)
            check_against_spec(got, need, planes, fmt, rounding, wd, (fmt, rounding, wd), **lay)
            # the size is the end of the last row's own bytes, not pitch * rows
            last_rows, last_elems = H // 2, (W if ss.SEMI[fmt] else W // 2)
            last_off = lay["offset_c"][0] if ss.SEMI[fmt] else lay["offset_c"][1]
            assert need == last_off + lay["pitch_c"] * (last_rows - 1) + last_elems * ss.ELEM[fmt]
            assert (got[need:] == ss.FILL).all()


def test_i010_tight_is_the_packed_frame(built_lib):
    sys.path.insert(0, str(ROOT / "oracle"))
    import ovvc_oracle_output as oo                           # the numpy pack tests/test_output_path.py compares the device pack with
    for w, h in ss.SIZES:
        planes = ss.random_planes(w, h, 400 + w)
        for wd in ss.windows_for(w, h):
            got, need = host_surface(built_lib, planes, ss.I010, 0, wd)
            assert need == built_lib.ovhip_output_bytes(w, h, C.byref(capi.Window(*wd)))
            assert got[:need].tobytes() == oo.packed_frame(*planes, wd), (w, h, wd)


def test_relations_between_the_formats(built_lib):
    for w, h in ss.SIZES:
        planes = ss.random_planes(w, h, 500 + w)
        for wd in ss.windows_for(w, h):
            W, H = w - 2 * (wd[0] + wd[1]), h - 2 * (wd[2] + wd[3])
            i010, n16 = host_surface(built_lib, planes, ss.I010, 0, wd)
            p010, m16 = host_surface(built_lib, planes, ss.P010, 0, wd)
            assert n16 == m16 == 3 * W * H
            a, b = i010[:n16].view("<u2"), p010[:n16].view("<u2")
            ny, nc = W * H, W * H // 4
            # P010 is I010 << 6 element for element: its chroma plane is I010's two, interleaved
            assert np.array_equal(b[:ny], a[:ny] << 6)
            assert np.array_equal(b[ny::2], a[ny:ny + nc] << 6) and np.array_equal(b[ny + 1::2], a[ny + nc:] << 6)
            assert not (b & 63).any()
            for rounding in (ss.ROUND, ss.DITHER):
                i420, n8 = host_surface(built_lib, planes, ss.I420, rounding, wd)
                nv12, m8 = host_surface(built_lib, planes, ss.NV12, rounding, wd)
                assert n8 == m8 == 3 * W * H // 2
                assert np.array_equal(nv12[:ny], i420[:ny])
                assert np.array_equal(nv12[ny:n8:2], i420[ny:ny + nc]) and np.array_equal(nv12[ny + 1:n8:2], i420[ny + nc:n8])


def _flat(w, h, s):
    return (np.full((h, w), s, np.uint16), np.full((h // 2, w // 2), s, np.uint16), np.full((h // 2, w // 2), s, np.uint16))


def test_round_at_the_ends_of_the_range(built_lib):
    for s, want in ((1021, 255), (1022, 255), (1023, 255), (1020, 255), (1, 0), (2, 1), (0, 0), (3, 1), (5, 1), (6, 2)):
        for fmt in (ss.NV12, ss.I420):
            got, need = host_surface(built_lib, _flat(8, 8, s), fmt, ss.ROUND)
            assert need == 96 and (got[:need] == want).all(), (s, fmt)


def test_dither_keeps_the_mean_of_every_aligned_cell(built_lib):
    """for every s in 0..1020, on a flat 8x8 picture, the four outputs of every aligned 2x2 cell of every plane sum to s"""
    for s in range(1021):
        flat = _flat(8, 8, s)
        i420, need = host_surface(built_lib, flat, ss.I420, ss.DITHER)
        planes = [i420[:64].reshape(8, 8), i420[64:80].reshape(4, 4), i420[80:96].reshape(4, 4)]
        nv12, _ = host_surface(built_lib, flat, ss.NV12, ss.DITHER)
        c = nv12[64:96].reshape(4, 8)
        planes += [nv12[:64].reshape(8, 8), c[:, 0::2], c[:, 1::2]]
        for p in planes:
            q = p.astype(np.int64)
            cells = q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2]
            assert (cells == s).all(), s
    # above 1020 the clip takes the property away: 1023 gives 255 everywhere
    got, need = host_surface(built_lib, _flat(8, 8, 1023), ss.I420, ss.DITHER)
    assert (got[:need] == 255).all()


def test_dither_pattern_starts_at_the_windows_first_sample(built_lib):
    wd = (1, 0, 0, 1)
    for w, h in ((20, 12), (72, 40)):
        planes = ss.random_planes(w, h, 600 + w)
        for fmt in (ss.NV12, ss.I420):
            got, need = host_surface(built_lib, planes, fmt, ss.DITHER, wd)
            check_against_spec(got, need, planes, fmt, ss.DITHER, wd, (w, h, fmt))
        # dithering the uncropped picture and cropping it then is another picture: in the chroma planes, whose first column under this
        # window is the picture's column 1, the thresholds swap (luma starts at column 2 and row 0: the same phase)
        whole = ss.out_planes(planes, ss.I420, ss.DITHER)
        then_cropped = ss.crop(whole, wd)
        cropped_first = ss.out_planes(planes, ss.I420, ss.DITHER, wd)
        assert np.array_equal(then_cropped[0], cropped_first[0])
        assert not np.array_equal(then_cropped[1], cropped_first[1]) and not np.array_equal(then_cropped[2], cropped_first[2])
        got, need = host_surface(built_lib, planes, ss.I420, ss.DITHER, wd)
        W, H = w - 2, h - 2
        assert got[W * H:W * H + W * H // 4].tobytes() == cropped_first[1].tobytes() != then_cropped[1].tobytes()


def refusal_cases(w, h, need, planes, dst_ptr):
    """name -> (keyword arguments of `call` below, whether ovhip_surface_bytes sees the reason too)"""
    y, cb, cr = planes
    F = c_format
    row = w                                                   # NV12: bytes of a luma row and of a chroma row
    return {
        "null destination": (dict(dptr=None), False),
        "null format": (dict(fmt=None), True),
        "missing luma": (dict(planes=(None, cb, cr)), False),
        "missing Cb": (dict(planes=(y, None, cr)), False),
        "missing Cr": (dict(planes=(y, cb, None)), False),
        "odd width": (dict(size=(w - 1, h)), True),
        "odd height": (dict(size=(w, h - 1)), True),
        "zero width": (dict(size=(0, h)), True),
        "negative height": (dict(size=(w, -2)), True),
        "width above 16384": (dict(size=(16386, h), strides=(16386, 8193)), True),
        "height above 16384": (dict(size=(w, 16386)), True),
        "luma stride below the width": (dict(strides=(w - 1, w // 2)), False),
        "chroma stride below the width": (dict(strides=(w, w // 2 - 1)), False),
        "window that leaves nothing (columns)": (dict(win=(w // 4, w // 4, 0, 0)), True),
        "window that leaves nothing (rows)": (dict(win=(0, 0, h // 2, 0)), True),
        "unknown format": (dict(fmt=F(4)), True),
        "unknown rounding": (dict(fmt=F(ss.NV12, 2)), True),
        "dither on P010": (dict(fmt=F(ss.P010, 1), nbytes=2 * need), True),
        "dither on I010": (dict(fmt=F(ss.I010, 1), nbytes=2 * need), True),
        "non-zero rsv[0]": (dict(fmt=F(ss.NV12), rsv=(1, 0)), True),
        "non-zero rsv[1]": (dict(fmt=F(ss.I420), rsv=(0, 1)), True),
        "offset_c[1] on NV12": (dict(fmt=F(ss.NV12, 0, 0, 0, (0, 4 * need)), nbytes=8 * need), True),
        "offset_c[1] on P010": (dict(fmt=F(ss.P010, 0, 0, 0, (0, 4 * need)), nbytes=8 * need), True),
        "pitch_y below the row": (dict(fmt=F(ss.NV12, 0, row - 1, 0)), True),
        "pitch_c below the row": (dict(fmt=F(ss.NV12, 0, 0, row - 1)), True),
        "pitch_c below the row (planar)": (dict(fmt=F(ss.I420, 0, 0, row // 2 - 1)), True),
        "odd pitch_y on a 16-bit format": (dict(fmt=F(ss.P010, 0, 2 * row + 1, 0), nbytes=4 * need), True),
        "odd pitch_c on a 16-bit format": (dict(fmt=F(ss.I010, 0, 0, row + 1), nbytes=4 * need), True),
        "odd offset_c[0] on a 16-bit format": (dict(fmt=F(ss.P010, 0, 0, 0, (2 * row * h + 1, 0)), nbytes=4 * need), True),
        "odd offset_c[1] on a 16-bit format": (dict(fmt=F(ss.I010, 0, 0, 0, (0, 3 * row * h + 1)), nbytes=8 * need), True),
        "element-misaligned destination": (dict(fmt=F(ss.P010), dptr=dst_ptr + 1, nbytes=4 * need), False),
        "chroma plane inside the luma plane": (dict(fmt=F(ss.NV12, 0, 0, 0, (row * h - 1, 0)), nbytes=4 * need), True),
        "Cr plane inside the Cb plane": (dict(fmt=F(ss.I420, 0, 0, 0, (row * h, row * h + 1)), nbytes=4 * need), True),
        "Cr plane inside the luma plane": (dict(fmt=F(ss.I420, 0, 0, 0, (0, row)), nbytes=4 * need), True),
        "dst_bytes too small": (dict(nbytes=need - 1), False),
        "dst_bytes too small (pitch)": (dict(fmt=F(ss.NV12, 0, row + 8, 0), nbytes=need), False),
        "destination overlapping the luma plane": (dict(dptr=y.ctypes.data + 2 * w, nbytes=1 << 20), False),
        "destination overlapping the Cr plane": (dict(dptr=cr.ctypes.data - need + 2, nbytes=1 << 20), False),
    }


def test_refusals_write_nothing(built_lib):
    lib = built_lib
    w, h = 24, 8
    planes = ss.random_planes(w, h, 3)
    ok = c_format(ss.NV12)
    need = lib.ovhip_surface_bytes(w, h, None, C.byref(ok))
    assert need == w * h * 3 // 2
    dst = np.full(8 * need + 64, ss.FILL, np.uint8)

    def call(fmt=ok, win=None, planes=planes, size=(w, h), strides=(w, w // 2), dptr=dst.ctypes.data, nbytes=need, rsv=None):
        if rsv:
            fmt.rsv[0], fmt.rsv[1] = rsv
        p = [a.ctypes.data if a is not None else None for a in planes]
        cw = C.byref(capi.Window(*win)) if win else None
        cf = C.byref(fmt) if fmt is not None else None
        return (lib.ovhip_surface_host(p[0], p[1], p[2], size[0], size[1], strides[0], strides[1], cw, cf, dptr, nbytes),
                lib.ovhip_surface_bytes(size[0], size[1], cw, cf))

    keep = tuple(a.copy() for a in planes)
    for name, (kw, bytes_sees_it) in refusal_cases(w, h, need, planes, dst.ctypes.data).items():
        r, n = call(**kw)
        assert r == EINVAL, name
        assert (n == 0) == bytes_sees_it, (name, n)
        assert (dst == ss.FILL).all(), name
        assert all(np.array_equal(a, b) for a, b in zip(planes, keep)), name
    assert call()[0] == 0
    assert (dst[:need] != ss.FILL).any() and (dst[need:] == ss.FILL).all()
    # a chroma plane BEFORE nothing and behind a gap is fine, and so is Cr in front of Cb
    assert call(fmt=c_format(ss.I420, 0, 0, 0, (w * h + w * h // 4 + 16, w * h)), nbytes=8 * need)[0] == 0


def test_null_handles(built_lib):
    fmt = c_format(ss.NV12)
    buf = np.zeros(64, np.uint8)
    assert built_lib.ovhip_frame_set_surface_output(None, C.byref(fmt), None, buf.ctypes.data, 64) == EINVAL
    assert built_lib.ovhip_frame_set_surface_output(None, None, None, None, 0) == EINVAL
    assert built_lib.ovhip_stream_set_surface_output(None, C.byref(fmt), None, buf.ctypes.data, 64, 1) == EINVAL
    assert built_lib.ovhip_stream_set_surface_output(None, None, None, None, 0, 0) == EINVAL
    assert built_lib.ovhip_surface_launch(None, None, None, C.byref(fmt), buf.ctypes.data, 64) == EINVAL
    assert built_lib.ovhip_pic_output_surface(None, None, None, C.byref(fmt), buf.ctypes.data, 64) == EINVAL
