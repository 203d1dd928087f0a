"""CPU: reduced-size output on the host (openvvc_amd/csrc/ovvc_reduce.c): the properties of the numpy restatement
tests/spec_reduce.py, ovhip_output_reduce_host against it byte for byte on the whole census, the refusals, the ratios of
ovhip_output_reduce_check, the kernel's division on the host, and the exports.  The definition is integer only: every comparison is
of bytes."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import spec_reduce as sd
from openvvc_amd import capi, engine

ROOT = Path(__file__).resolve().parent.parent
EINVAL, EUNSUP = capi.OVHIP_EINVAL, capi.OVHIP_EUNSUP
SENT = 0xA5A5
NEW = ["ovhip_output_reduce_check", "ovhip_output_reduce_host", "ovhip_output_reduce_divide", "ovhip_output_reduce_launch",
       "ovhip_pic_output_reduced", "ovhip_pic_digest_reduced", "ovhip_frame_set_output_reduce", "ovhip_stream_set_output_reduce"]


def info_of(window=(0, 0, 0, 0), loc=0):
    return capi.ReduceInfo(capi.Window(*window), loc)


def strided(planes, sy, sc):
    """copies of the planes in rows of sy / sc samples, the gap holding the sentinel"""
    held = []
    for p, s in zip(planes, (sy, sc, sc)):
        a = np.full((p.shape[0], s), SENT, np.uint16)
        a[:, :p.shape[1]] = p
        held.append(a)
    return held


def host_reduce(lib, planes, Wd, Hd, window=(0, 0, 0, 0), loc=0, spad=0, dpad=0):
    """ovhip_output_reduce_host of the planes (rows of w + spad) into planes of rows Wd + dpad that held the sentinel -> the three
    destination arrays, gaps included"""
    h, w = planes[0].shape
    src = strided(planes, w + spad, w // 2 + spad)
    dst = [np.full((Hd, Wd + dpad), SENT, np.uint16), np.full((Hd // 2, Wd // 2 + dpad), SENT, np.uint16), np.full((Hd // 2, Wd // 2 + dpad), SENT, np.uint16)]
    sp = capi.Pic(src[0].ctypes.data, src[1].ctypes.data, src[2].ctypes.data, w, h, w + spad, w // 2 + spad)
    dp = capi.Pic(dst[0].ctypes.data, dst[1].ctypes.data, dst[2].ctypes.data, Wd, Hd, Wd + dpad, Wd // 2 + dpad)
    r = lib.ovhip_output_reduce_host(C.byref(sp), C.byref(info_of(window, loc)), C.byref(dp))
    assert r == 0, (r, w, h, Wd, Hd, window, loc)
    return dst


def assert_equal_spec(got, want, what):
    """got: destination arrays with their gaps; want: the restated planes"""
    for g, x in zip(got, want):
        assert g[:, :x.shape[1]].tobytes() == x.tobytes(), what
        assert (g[:, x.shape[1]:] == SENT).all(), what


# ---- the restatement's own properties ----
def test_every_outputs_weights_sum_to_4p_on_few_samples():
    for (src, dst, _locs) in sd.CENSUS:
        for S, D in zip(src, dst):
            p, q = sd.axis(S, D)
            for Sp, Dp, sgs in ((S, D, (0,)), (S // 2, D // 2, (p - q, 0, q - p))):
                for sg in sgs:
                    W = sd.weights(Sp, Dp, p, q, sg)
                    assert (W.sum(axis=1) == 4 * p).all(), (S, D, sg)
                    assert ((W > 0).sum(axis=1) <= -(-p // q) + 1).all(), (S, D, sg)
                    assert (W >= 0).all()


def test_luma_footprints_tile_the_region():
    for (w, h), (Wd, Hd), _locs in sd.CENSUS[:9]:
        y = sd.random_planes(w, h, w + h)[0]
        px, qx = sd.axis(w, Wd)
        py, qy = sd.axis(h, Hd)
        V = sd.plane_V(y, Wd, Hd, px, qx, py, qy)
        assert int(V.sum()) == 16 * qx * qy * int(y.astype(np.int64).sum()), (w, h, Wd, Hd)


def test_identity_and_copy_along_an_axis():
    planes = sd.random_planes(72, 40, 5)
    for loc in range(6):
        assert all(np.array_equal(a, b) for a, b in zip(sd.reduce_picture(*planes, 72, 40, loc=loc), planes))
    # 1/1 on x: every column is reduced on its own
    got = sd.reduce_picture(*planes, 72, 20)
    assert np.array_equal(got[0][:, 7], sd.round_div(sd.plane_V(planes[0][:, 7:8].repeat(4, axis=1), 4, 20, 1, 1, 2, 1), 32)[:, 0])


def test_window_equals_crop():
    (w, h), wd, (Wd, Hd) = sd.WINDOW_CASE
    l, r, a, b = wd
    inner = sd.random_planes(w - 2 * (l + r), h - 2 * (a + b), 3, top=512)
    planes = [np.full((h, w), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16)]
    planes[0][2 * a:h - 2 * b, 2 * l:w - 2 * r] = inner[0]
    planes[1][a:h // 2 - b, l:w // 2 - r] = inner[1]
    planes[2][a:h // 2 - b, l:w // 2 - r] = inner[2]
    for loc in (0, 3, 4):
        got, want = sd.reduce_picture(*planes, Wd, Hd, wd, loc), sd.reduce_picture(*inner, Wd, Hd, loc=loc)
        assert all(np.array_equal(g, x) for g, x in zip(got, want))
        assert max(int(g.max()) for g in got) <= 511, "nothing outside the window is read"


@pytest.mark.parametrize("r", [2, 3, 8])
def test_ramps_at_integer_ratios_land_on_the_outputs_site(r):
    """interior outputs of a ramp: luma output k sits at sample r k + (r - 1) / 2; chroma output k at r k + (r - 1)(1 + 2c) / 4 with
    c = a/2 or b/2, the place that keeps the chroma's location relative to the OUTPUT luma.  In units of V (weights sum to 4r per axis):
    sum_j w j = 4 r^2 k + r (r - 1)(1 + 2c), luma being the case 2c = 1"""
    D = 12
    S = r * D
    jy, jx = np.mgrid[0:S, 0:S]
    ramp = 3 * jx + 5 * jy
    k = np.arange(D)

    def site(c2):
        return 4 * r * r * k + r * (r - 1) * (1 + c2)

    V = sd.plane_V(ramp, D, D, r, 1, r, 1)
    want = 4 * r * (3 * site(1)[None, :] + 5 * site(1)[:, None])
    assert np.array_equal(V[1:-1, 1:-1], want[1:-1, 1:-1])
    for a2 in (0, 1, 2):                                         # 2c: the three signs of sigma
        for b2 in (0, 1, 2):
            V = sd.plane_V(ramp, D, D, r, 1, r, 1, sd.sigma(r, 1, a2), sd.sigma(r, 1, b2))
            want = 4 * r * (3 * site(a2)[None, :] + 5 * site(b2)[:, None])
            assert np.array_equal(V[1:-1, 1:-1], want[1:-1, 1:-1]), (a2, b2)


def test_the_chroma_shift_acts():
    planes = sd.random_planes(104, 56, 11)
    loc0, loc1, loc2 = (sd.reduce_picture(*planes, 52, 28, loc=k) for k in (0, 1, 2))
    assert np.array_equal(loc0[0], loc1[0]) and not np.array_equal(loc0[1], loc1[1]) and not np.array_equal(loc0[1], loc2[1])
    # 2:1 with horizontally co-sited chroma: 1, 4, 3 over 8 on samples 2k-1, 2k, 2k+1
    assert list(sd.weights(52, 26, 2, 1, 1)[5, 9:12]) == [1, 4, 3]
    assert list(sd.weights(52, 26, 2, 1, 0)[5, 10:12]) == [4, 4]


# ---- the host twin ----
@pytest.mark.parametrize("case", range(len(sd.CENSUS)))
def test_host_twin_equals_the_restatement_on_the_census(built_lib, case):
    (w, h), (Wd, Hd), locs = sd.CENSUS[case]
    planes = sd.random_planes(w, h, 100 + case)
    for loc in locs:
        assert_equal_spec(host_reduce(built_lib, planes, Wd, Hd, loc=loc), sd.reduce_picture(*planes, Wd, Hd, loc=loc), (w, h, Wd, Hd, loc))
    if (w, h, Wd, Hd) == (72, 40, 72, 40):
        assert_equal_spec(host_reduce(built_lib, planes, Wd, Hd), planes, "the identity")
    if (w, h, Wd, Hd) == (72, 40, 48, 24):
        assert_equal_spec(host_reduce(built_lib, planes, Wd, Hd, spad=6, dpad=2), sd.reduce_picture(*planes, Wd, Hd), "strides")
    if w == 1024:
        full = [np.full_like(p, 1023) for p in planes]
        got = host_reduce(built_lib, full, Wd, Hd)
        assert all((g == 1023).all() for g in got), "the int32 ceiling: V = 1072693248"


def test_host_twin_on_a_window_reads_nothing_outside_it(built_lib):
    (w, h), wd, (Wd, Hd) = sd.WINDOW_CASE
    l, r, a, b = wd
    inner = sd.random_planes(w - 2 * (l + r), h - 2 * (a + b), 3, top=512)
    planes = [np.full((h, w), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16)]
    planes[0][2 * a:h - 2 * b, 2 * l:w - 2 * r] = inner[0]
    planes[1][a:h // 2 - b, l:w // 2 - r] = inner[1]
    planes[2][a:h // 2 - b, l:w // 2 - r] = inner[2]
    for loc in (0, 5):
        assert_equal_spec(host_reduce(built_lib, planes, Wd, Hd, wd, loc), sd.reduce_picture(*inner, Wd, Hd, loc=loc), loc)


def test_check_returns_the_ratios(built_lib):
    for (src, dst), want in sd.RATIOS.items():
        assert engine.reduce_check(*src, *dst) == (0, want), (src, dst)
    (w, h), wd, (Wd, Hd) = sd.WINDOW_CASE
    assert engine.reduce_check(w, h, Wd, Hd, wd) == (0, (3, 2, 5, 3))
    assert engine.reduce_check(1028, 64, 132, 64) == (EUNSUP, (257, 33, 1, 1))
    assert engine.reduce_check(72, 40, 8, 40) == (EUNSUP, (9, 1, 1, 1))
    for (src, dst) in sd.REFUSED:
        assert not sd.check(*src, *dst)[0]


def test_every_refusal_returns_its_code(built_lib):
    lib = built_lib
    chk = engine.reduce_check
    assert chk(72, 40, 144, 40)[0] == EUNSUP and chk(72, 40, 72, 44)[0] == EUNSUP              # up-sampling
    assert chk(72, 40, 8, 40)[0] == EUNSUP and chk(64, 72, 64, 8)[0] == EUNSUP                 # the ratio
    assert chk(1028, 64, 132, 64)[0] == EUNSUP and chk(64, 1028, 64, 132)[0] == EUNSUP         # p > 256
    assert chk(1024, 1024, 132, 132)[0] == 0 and chk(64, 64, 8, 8)[0] == 0                     # the ceilings themselves
    for bad in ((70, 40, 36, 20), (72, 42, 36, 20), (72, 40, 34, 20), (72, 40, 36, 22), (0, 40, 36, 20), (72, 40, 0, 20), (72, 40, -4, 20),
                (16388, 64, 8192, 64), (64, 16388, 64, 8192)):
        assert chk(*bad)[0] == EINVAL, bad
    assert chk(16384, 64, 16384, 64)[0] == 0
    assert chk(72, 40, 36, 20, (18, 18, 0, 0))[0] == EINVAL and chk(72, 40, 36, 20, (0, 0, 10, 10))[0] == EINVAL       # leaves nothing
    assert chk(72, 40, 36, 20, (1, 0, 0, 0))[0] == EINVAL and chk(72, 40, 36, 20, (0, 0, 0, 1))[0] == EINVAL           # 70 / 38 left
    assert chk(72, 40, 36, 20, chroma_loc=6)[0] == EINVAL and chk(72, 40, 36, 20, chroma_loc=5)[0] == 0
    rsv = info_of()
    rsv.rsv[2] = 1
    ratio = (C.c_int32 * 4)()
    assert lib.ovhip_output_reduce_check(72, 40, C.byref(rsv), 36, 20, ratio) == EINVAL
    assert lib.ovhip_output_reduce_check(72, 40, None, 36, 20, ratio) == EINVAL
    assert lib.ovhip_output_reduce_check(72, 40, C.byref(info_of()), 36, 20, None) == EINVAL
    # the twin: null arguments, a missing plane, strides below the width, dst aliasing src; nothing is written
    planes = sd.random_planes(72, 40, 1)
    src = strided(planes, 72, 36)
    dst = [np.full((20, 36), SENT, np.uint16), np.full((10, 18), SENT, np.uint16), np.full((10, 18), SENT, np.uint16)]
    sp = capi.Pic(src[0].ctypes.data, src[1].ctypes.data, src[2].ctypes.data, 72, 40, 72, 36)
    dp = capi.Pic(dst[0].ctypes.data, dst[1].ctypes.data, dst[2].ctypes.data, 36, 20, 36, 18)
    inf = info_of()
    host = lib.ovhip_output_reduce_host
    assert host(None, C.byref(inf), C.byref(dp)) == EINVAL and host(C.byref(sp), None, C.byref(dp)) == EINVAL and host(C.byref(sp), C.byref(inf), None) == EINVAL

    def pic(base, **kw):
        f = {k: getattr(base, k) for k, _ in capi.Pic._fields_}
        f.update(kw)
        return capi.Pic(f["y"], f["cb"], f["cr"], f["w"], f["h"], f["stride_y"], f["stride_c"])

    assert host(C.byref(pic(sp, cr=None)), C.byref(inf), C.byref(dp)) == EINVAL
    assert host(C.byref(sp), C.byref(inf), C.byref(pic(dp, y=None))) == EINVAL
    assert host(C.byref(pic(sp, stride_y=70)), C.byref(inf), C.byref(dp)) == EINVAL
    assert host(C.byref(sp), C.byref(inf), C.byref(pic(dp, stride_c=16))) == EINVAL
    assert host(C.byref(sp), C.byref(inf), C.byref(pic(dp, cb=sp.cr + 8))) == EINVAL
    assert host(C.byref(sp), C.byref(inf), C.byref(pic(dp, y=sp.y))) == EINVAL
    assert host(C.byref(sp), C.byref(rsv), C.byref(dp)) == EINVAL
    assert host(C.byref(pic(sp, w=32, h=16)), C.byref(inf), C.byref(dp)) == EUNSUP
    assert host(C.byref(sp), C.byref(inf), C.byref(pic(dp, w=8))) == EUNSUP
    assert all((d == SENT).all() for d in dst)
    assert host(C.byref(sp), C.byref(inf), C.byref(dp)) == 0 and not any((d == SENT).all() for d in dst)


def test_the_kernels_division_is_exact_at_every_rounding_boundary(built_lib):
    """for every n of the census and every multiple m n up to the numerator's maximum: V = m n - n/2 - 1, m n - n/2, m n - n/2 + 1, the
    values either side of where (V + n/2) div n steps"""
    div = built_lib.ovhip_output_reduce_divide
    ns = sorted({16 * px * py for (px, _qx, py, _qy) in sd.RATIOS.values()})
    assert ns[0] == 16 and ns[-1] == 1 << 20
    for n in ns:
        for m in range(1, 1024):
            for V in (m * n - n // 2 - 1, m * n - n // 2, m * n - n // 2 + 1):
                if 0 <= V <= 1023 * n:
                    num = V + n // 2
                    assert div(num, n) == num // n, (n, m, V)
        assert div(1023 * n + n // 2, n) == 1023 and div(n // 2, n) == 0
    assert 16 * 256 * 256 * 1023 == 1072693248 and 1072693248 + (1 << 19) < 1 << 31


def test_exports_and_abi(built_lib):
    header = (ROOT / "include" / "ovvc_hip.h").read_text()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(built_lib, name), name
    assert "Reduced-size output on the device" in header
    assert C.sizeof(capi.ReduceInfo) == 12 and capi.ReduceInfo.chroma_loc.offset == 8
    assert capi.OVHIP_ABI_VERSION == 9 and built_lib.ovhip_abi_version() == 9
    assert "ovhip_reduce_refusal_" not in header
