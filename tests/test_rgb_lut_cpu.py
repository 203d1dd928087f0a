"""CPU: RGB output through a colour table on the host (openvvc_amd/csrc/ovvc_rgb_lut.c): ovhip_rgb_lut_host against the numpy
restatement tests/spec_rgb_lut.py, the properties of the definition (lattice table, index order, tie-breaks, half-precision
subnormals), the refusals, and the table builders of openvvc_amd/lut3d.py.  The definition is integer only: every comparison is exact
unless it says otherwise.  (That ovhip_rgb_lut_create names the index of an entry above the peak needs a context: tests/test_gpu_rgb_lut.py.)"""
import ctypes as C
import itertools

import numpy as np
import pytest

import spec_rgb as sr
import spec_rgb_lut as sl
from openvvc_amd import capi, lut3d
from test_rgb_cpu import same_bits

# (w, h, window): a plane of 2.5 runs, a window with a row tail, more than one wave per row pair
CASES = [(20, 12, (0, 0, 0, 0)), (72, 40, (1, 0, 0, 1)), (136, 72, (0, 0, 0, 0))]
PEAKS = (255, 1023, 65535)
DTYPES = [sr.U8, sr.U16, sr.F16, sr.F32]
LAYOUTS = [sr.PLANAR, sr.PACKED]
FORMATS = [(9, 0, 0), (1, 1, 3)]                    # (matrix, full range, chroma location)
EINVAL, EUNSUP = -3, -5


def census_planes(w: int, h: int, seed: int):
    """random planes; the left half's chroma is neutral (R = G = B there: three equal fractions), and its first luma samples are the two ends"""
    y, cb, cr = sr.random_planes(w, h, seed)
    cb[:, :w // 4] = 512
    cr[:, :w // 4] = 512
    y[0, 0:2] = (0, 1023)
    return y, cb, cr


def host_lut(lib, planes, fmt, table, peak, window=(0, 0, 0, 0), strides=None):
    """ovhip_rgb_lut_host of tight (or strided) planes -> array in the format's dtype and shape"""
    h, w = planes[0].shape
    sy, sc = strides or (w, w // 2)
    held = []
    for p, s in zip(planes, (sy, sc, sc)):
        a = np.full((p.shape[0], s), 0xA5A5, np.uint16)
        a[:, :p.shape[1]] = p
        held.append(a)
    win = capi.Window(*window)
    W, H = w - 2 * (window[0] + window[1]), h - 2 * (window[2] + window[3])
    out = np.empty((3, H, W) if fmt.layout == sr.PLANAR else (H, W, 3), sr.NP_DTYPE[fmt.dtype])
    assert lib.ovhip_rgb_bytes(w, h, C.byref(win), C.byref(fmt)) == out.nbytes
    table = np.ascontiguousarray(table)
    r = lib.ovhip_rgb_lut_host(held[0].ctypes.data, held[1].ctypes.data, held[2].ctypes.data, w, h, sy, sc, C.byref(win), C.byref(fmt),
                               table.shape[0], peak, table.ctypes.data, out.ctypes.data, out.nbytes)
    assert r == 0, r
    return out


def test_the_names_are_exported_and_the_abi_version_stays(built_lib):
    names = ["ovhip_rgb_lut_check", "ovhip_rgb_lut_create", "ovhip_rgb_lut_destroy", "ovhip_rgb_lut_host", "ovhip_rgb_lut_launch",
             "ovhip_pic_output_rgb_lut", "ovhip_frame_set_rgb_lut", "ovhip_stream_set_rgb_lut"]
    for n in names:
        assert n in capi.EXPORTED_SYMBOLS and hasattr(built_lib, n), n
    assert capi.OVHIP_ABI_VERSION == 9 and built_lib.ovhip_abi_version() == 9
    header = (capi._PKG.parent / "include" / "ovvc_hip.h").read_text()
    assert "typedef struct ovhip_rgb_lut ovhip_rgb_lut;" in header        # (the ninth name: the opaque type)


def test_check(built_lib):
    for s in range(0, 70):
        assert built_lib.ovhip_rgb_lut_check(s, 1023, None) == (0 if s in sl.SIZES else EINVAL), s
    for p, code in ((0, EINVAL), (1, 0), (255, 0), (65535, 0), (65536, EINVAL), (-1, EINVAL)):
        assert built_lib.ovhip_rgb_lut_check(33, p, None) == code, p
    for dt in DTYPES:
        fmt = capi.RgbFormat(1, 0, 0, dt, 0)
        assert built_lib.ovhip_rgb_lut_check(17, 255, C.byref(fmt)) == 0
        assert built_lib.ovhip_rgb_lut_check(17, 256, C.byref(fmt)) == (EINVAL if dt == sr.U8 else 0)
    assert built_lib.ovhip_rgb_lut_check(17, 255, C.byref(capi.RgbFormat(1, 0, 0, 4, 0))) == EINVAL


@pytest.mark.parametrize("size", sl.SIZES)
@pytest.mark.parametrize("peak", PEAKS)
def test_host_twin_equals_the_restatement(built_lib, size, peak):
    table = sl.random_table(size, peak, 100 * size + peak % 97)
    for k, (w, h, wd) in enumerate(CASES):
        planes = census_planes(w, h, 7 * w + size)
        matrix, full, loc = FORMATS[k % 2]
        o = sl.interpolate(sl.rgb10(*planes, matrix, full, loc, wd), table)           # the reference, once per picture
        for dtype, layout in itertools.product(DTYPES, LAYOUTS):
            if dtype == sr.U8 and peak > 255:
                continue
            fmt = capi.RgbFormat(matrix, full, loc, dtype, layout)
            assert same_bits(host_lut(built_lib, planes, fmt, table, peak, wd), sl.store(o, peak, dtype, layout)), (w, h, dtype, layout)


def test_host_twin_with_strides_above_the_width(built_lib):
    planes = census_planes(20, 12, 5)
    table = sl.random_table(17, 1023, 5)
    fmt = capi.RgbFormat(9, 0, 1, sr.U16, sr.PACKED)
    want = sl.convert(*planes, 9, 0, 1, sr.U16, sr.PACKED, table, 1023, (1, 0, 0, 1))
    assert same_bits(host_lut(built_lib, planes, fmt, table, 1023, (1, 0, 0, 1), strides=(27, 13)), want)


def test_the_matrix_is_at_10_bits_for_a_u8_destination(built_lib):
    """a U8 destination does not select the 8-bit coefficients: through the table that maps v to round(255 v / 1023) it equals the
    10-bit RGB output requantised, which differs from the 8-bit RGB output somewhere"""
    planes = sr.random_planes(72, 40, 21)
    ramp = np.floor(np.arange(1024) * 255 / 1023 + 0.5).astype(np.int64)
    table = lut3d.from_function(lambda x: x, 33, 255)
    got = host_lut(built_lib, planes, capi.RgbFormat(1, 0, 0, sr.U8, sr.PLANAR), table, 255)
    assert same_bits(got, sl.convert(*planes, 1, 0, 0, sr.U8, sr.PLANAR, table, 255))
    ten = sr.rgb_int(*planes, 1, 0, 0, 10)
    assert np.abs(got.astype(np.int64) - ramp[ten]).max() <= 1                                  # (the identity table is only piecewise exact)
    assert not np.array_equal(ramp[ten], sr.rgb_int(*planes, 1, 0, 0, 8))


@pytest.mark.parametrize("size", sl.SIZES)
def test_the_lattice_table_gives_exactly_n_times_the_input(built_lib, size):
    planes = census_planes(72, 40, size)
    table = lut3d.lattice(size)
    assert int(table.max()) == 1023 * (size - 1) <= 65535
    want = (size - 1) * sr.rgb_int(*planes, 1, 0, 0, 10)
    assert np.array_equal(sl.interpolate(sr.rgb_int(*planes, 1, 0, 0, 10), table), want)
    got = host_lut(built_lib, planes, capi.RgbFormat(1, 0, 0, sr.U16, sr.PLANAR), table, 65535)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_a_table_that_reads_one_index_pins_the_index_order(built_lib, axis):
    """T[b][g][r] = 100 * (its r, g or b index) in every output channel: the output is 100 n v / 1023 of THAT input channel, rounded"""
    size = 17
    k = np.arange(size, dtype=np.uint16) * 100
    shape = [1, 1, 1, 1]
    shape[2 - axis] = size                                                   # axis 0 = r: the fastest index
    table = np.ascontiguousarray(np.broadcast_to(k.reshape(shape), (size, size, size, 3)))
    planes = census_planes(72, 40, 40 + axis)
    got = host_lut(built_lib, planes, capi.RgbFormat(1, 0, 0, sr.U16, sr.PLANAR), table, 1600)
    assert same_bits(got, sl.convert(*planes, 1, 0, 0, sr.U16, sr.PLANAR, table, 1600))
    v = sr.rgb_int(*planes, 1, 0, 0, 10)[axis]
    i, f = sl.cells(v, size)
    want = ((1023 - f) * 100 * i + f * 100 * (i + 1) + 511) // 1023
    for c in range(3):
        assert np.array_equal(got[c], want), (axis, c)
    others = [sr.rgb_int(*planes, 1, 0, 0, 10)[a] for a in range(3) if a != axis]
    assert all(not np.array_equal(v, o) for o in others)


def test_two_tie_breaks_give_equal_results():
    for size in sl.SIZES:
        table = sl.random_table(size, 65535, size)
        for w, h, wd in CASES:
            rgb = sl.rgb10(*census_planes(w, h, 7 * w + size), 1, 0, 0, wd)
            _, f = sl.cells(rgb, size)
            assert not np.array_equal(sl.order(f, 0), sl.order(f, 1)), "the inputs hold no tie"
            assert np.array_equal(sl.interpolate(rgb, table, 0), sl.interpolate(rgb, table, 1))


@pytest.mark.parametrize("size", sl.SIZES)
def test_census_of_the_inputs_used(size):
    """what test_host_twin_equals_the_restatement feeds the table step, over its three pictures"""
    px = np.concatenate([sl.rgb10(*census_planes(w, h, 7 * w + size), *FORMATS[k % 2], wd).reshape(3, -1) for k, (w, h, wd) in enumerate(CASES)], axis=1)
    i, f = sl.cells(px, size)
    strict = (f[0] != f[1]) & (f[1] != f[2]) & (f[0] != f[2])
    orders = {tuple(o) for o in sl.order(f, 0)[:, strict].T}
    assert orders == set(itertools.permutations(range(3))), orders
    n_equal = (f[0] == f[1]).astype(int) + (f[1] == f[2]) + (f[0] == f[2])
    assert (n_equal == 1).any(), "no pixel with exactly two equal fractions"
    assert (n_equal == 3).any(), "no pixel with three equal fractions"
    for c in range(3):
        assert (px[c] == 0).any() and (px[c] == 1023).any(), c
    if size == 65:
        assert (i == 63).any() and ((i == 63) & (px < 1023)).any()


def test_f16_in_the_subnormal_range_equals_numpy_bit_for_bit(built_lib):
    """P = 65535 and entries 0..40: every output is below 2^-10, the small ones below 2^-14 are subnormal halves"""
    planes = census_planes(20, 12, 3)
    unit = np.float32(1.0 / 65535)
    for layout in LAYOUTS:
        fmt = capi.RgbFormat(1, 0, 0, sr.F16, layout)
        for k in range(41):                                                   # a constant table gives the constant: each of 0..40 is met
            table = np.full((17, 17, 17, 3), k, np.uint16)
            got = host_lut(built_lib, planes, fmt, table, 65535)
            want = np.float16(np.float32(k) * unit)
            assert got.dtype == np.float16 and (got.view(np.uint16) == want.view(np.uint16)).all(), k
        table = np.random.default_rng(9).integers(0, 41, (17, 17, 17, 3), dtype=np.uint16)
        o = sl.interpolate(sl.rgb10(*planes, 1, 0, 0), table)
        want = np.float16(o.astype(np.float32) * unit)
        got = host_lut(built_lib, planes, fmt, table, 65535)
        assert same_bits(got, np.ascontiguousarray(want if layout == sr.PLANAR else want.transpose(1, 2, 0)))
    assert np.float16(np.float32(3) * unit) < np.float16(2.0 ** -14) and np.float16(np.float32(1) * unit) > 0


def test_refusals_write_nothing(built_lib):
    lib = built_lib
    w, h = 24, 8
    y, cb, cr = sr.random_planes(w, h, 3)
    ok = capi.RgbFormat(1, 0, 0, sr.U16, sr.PLANAR)
    need = lib.ovhip_rgb_bytes(w, h, None, C.byref(ok))
    dst = np.full(need + 64, 0xA5, np.uint8)
    good = sl.random_table(17, 1023, 1)
    above = good.copy()
    above[16, 3, 5, 1] = 1024

    def call(fmt=ok, win=None, planes=(y, cb, cr), size=(w, h), strides=(w, w // 2), dptr=dst.ctypes.data, nbytes=need, table=good, s=17, peak=1023):
        p = [a.ctypes.data if a is not None else None for a in planes]
        return lib.ovhip_rgb_lut_host(p[0], p[1], p[2], size[0], size[1], strides[0], strides[1], C.byref(capi.Window(*win)) if win else None,
                                      C.byref(fmt) if fmt is not None else None, s, peak, table.ctypes.data if table is not None else None, dptr, nbytes)

    cases = {
        # the table's own
        "null table": (dict(table=None), EINVAL),
        "size 16": (dict(s=16), EINVAL),
        "size 0": (dict(s=0), EINVAL),
        "peak 0": (dict(peak=0), EINVAL),
        "peak 65536": (dict(peak=65536), EINVAL),
        "U8 with a peak above 255": (dict(fmt=capi.RgbFormat(1, 0, 0, sr.U8, 0)), EINVAL),
        "an entry above the peak": (dict(table=above), EINVAL),
        "an entry above a smaller peak": (dict(peak=1022, table=np.full((17, 17, 17, 3), 1023, np.uint16)), EINVAL),
        # the RGB output's
        "null destination": (dict(dptr=None), EINVAL),
        "dst_bytes too small": (dict(nbytes=need - 1), EINVAL),
        "destination overlapping the luma plane": (dict(dptr=y.ctypes.data, nbytes=1 << 20), EINVAL),
        "destination overlapping the Cr plane": (dict(dptr=cr.ctypes.data + 2, nbytes=1 << 20), EINVAL),
        "window that leaves nothing (columns)": (dict(win=(6, 6, 0, 0)), EINVAL),
        "window that leaves nothing (rows)": (dict(win=(0, 0, 2, 2)), EINVAL),
        "missing luma": (dict(planes=(None, cb, cr)), EINVAL),
        "missing Cb": (dict(planes=(y, None, cr)), EINVAL),
        "missing Cr": (dict(planes=(y, cb, None)), EINVAL),
        "luma stride below the width": (dict(strides=(w - 1, w // 2)), EINVAL),
        "chroma stride below the width": (dict(strides=(w, w // 2 - 1)), EINVAL),
        "width not a multiple of 4": (dict(size=(w - 2, h)), EINVAL),
        "height not a multiple of 4": (dict(size=(w, h - 2)), EINVAL),
        "zero size": (dict(size=(0, h)), EINVAL),
        "bad dtype": (dict(fmt=capi.RgbFormat(1, 0, 0, 4, 0)), EINVAL),
        "bad layout": (dict(fmt=capi.RgbFormat(1, 0, 0, 1, 2)), EINVAL),
        "bad chroma location": (dict(fmt=capi.RgbFormat(1, 0, 6, 1, 0)), EINVAL),
        "bad range": (dict(fmt=capi.RgbFormat(1, 2, 0, 1, 0)), EINVAL),
        "matrix unspecified": (dict(fmt=capi.RgbFormat(2, 0, 0, 1, 0)), EINVAL),
        "matrix not built": (dict(fmt=capi.RgbFormat(0, 0, 0, 1, 0)), EUNSUP),
        "null format": (dict(fmt=None), EINVAL),
        "element-misaligned destination": (dict(dptr=dst.ctypes.data + 1), EINVAL),
    }
    keep = (y.copy(), cb.copy(), cr.copy())
    for name, (kw, code) in cases.items():
        assert call(**kw) == code, name
        assert (dst == 0xA5).all(), name
        assert all(np.array_equal(a, b) for a, b in zip((y, cb, cr), keep)), name
    assert call() == 0
    assert (dst[:need] != 0xA5).any() and (dst[need:] == 0xA5).all()
    dst[:] = 0xA5
    assert call(fmt=capi.RgbFormat(1, 0, 0, sr.U8, 0), peak=255, table=sl.random_table(17, 255, 2), nbytes=need // 2) == 0


# ---- openvvc_amd/lut3d.py ----

def test_cube_round_trip_is_identical(tmp_path):
    for size, peak in ((17, 255), (33, 1023), (17, 65535)):
        table = sl.random_table(size, peak, size + peak)
        path = tmp_path / f"t{size}_{peak}.cube"
        lut3d.write_cube(path, table, peak, title="round trip")
        text = path.read_text().splitlines()
        assert text[0] == 'TITLE "round trip"' and text[1] == f"LUT_3D_SIZE {size}"
        path.write_text("# a comment\n\n" + "\n".join(text) + "\n")
        back = lut3d.read_cube(path, peak)
        assert back.dtype == np.uint16 and np.array_equal(back, table)
    # red is the fastest index of the file: its second entry is table[0][0][1]
    assert text[5].split() == [f"{v / 65535:.10f}" for v in table[0, 0, 1]]
    bad = tmp_path / "bad.cube"
    bad.write_text("LUT_3D_SIZE 17\nDOMAIN_MAX 2 2 2\n")
    with pytest.raises(ValueError):
        lut3d.read_cube(bad, 255)
    bad.write_text("LUT_1D_SIZE 17\n")
    with pytest.raises(ValueError):
        lut3d.read_cube(bad, 255)
    bad.write_text("LUT_3D_SIZE 17\n0 0 0\n")
    with pytest.raises(ValueError):
        lut3d.read_cube(bad, 255)


def test_from_function_of_the_identity():
    for size in sl.SIZES:
        n = size - 1
        t = lut3d.from_function(lambda x: x, size, 1023)
        k = np.array([int(np.floor(1023 * j / n + 0.5)) for j in range(size)])
        assert t.shape == (size, size, size, 3) and t.dtype == np.uint16
        assert np.array_equal(t[..., 0], np.broadcast_to(k[None, None, :], t.shape[:3]))
        assert np.array_equal(t[..., 1], np.broadcast_to(k[None, :, None], t.shape[:3]))
        assert np.array_equal(t[..., 2], np.broadcast_to(k[:, None, None], t.shape[:3]))
    assert np.array_equal(lut3d.from_function(lambda x: 2 * x - 0.5, 17, 255)[[0, 16], 0, 0, 2], [0, 255])       # clipped to the table's range
    with pytest.raises(ValueError):
        lut3d.from_function(lambda x: x, 16, 1023)


def test_lattice():
    t = lut3d.lattice(17)
    assert tuple(t[3, 2, 1]) == (1023, 2046, 3069) and t.dtype == np.uint16


def test_pq_inverse_eotf_values():
    assert abs(float(lut3d.pq_inverse_eotf(100.0)) - 0.508078421517399) < 1e-12
    assert abs(float(lut3d.pq_inverse_eotf(1000.0)) - 0.751827096247041) < 1e-12
    assert abs(float(lut3d.pq_inverse_eotf(10000.0)) - 1.0) < 1e-12 and float(lut3d.pq_inverse_eotf(0.0)) < 1e-6
    x = np.linspace(0.0, 1.0, 101)[1:]          # (ST 2084 codes 0 cd/m^2 as c1^m2 = 7.3e-7, not as 0: the round trip starts above it)
    assert np.abs(lut3d.pq_inverse_eotf(lut3d.pq_eotf(x)) - x).max() < 1e-9
    assert np.abs(lut3d.bt2020_to_bt709_matrix().sum(axis=1) - 1.0).max() < 1e-12


@pytest.mark.parametrize("size", sl.SIZES)
@pytest.mark.parametrize("src,dst", [(1000.0, 100.0), (4000.0, 203.0)])
def test_pq_bt2020_to_bt709_grey_diagonal(size, src, dst):
    for peak in (255, 1023):
        t = lut3d.pq_bt2020_to_bt709(size, peak, src, dst)
        assert t.shape == (size, size, size, 3) and int(t.max()) <= peak
        d = t[np.arange(size), np.arange(size), np.arange(size)].astype(np.int64)          # (size, 3)
        assert (np.diff(d, axis=0) >= 0).all(), "not non-decreasing"
        assert tuple(d[0]) == (0, 0, 0) and tuple(d[-1]) == (peak, peak, peak)
        assert (d.max(axis=1) - d.min(axis=1)).max() <= 1, "not neutral within 1 code"
        assert len(np.unique(d[:, 0])) > size // 2
