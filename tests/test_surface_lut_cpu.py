"""CPU: surface output through a colour table on the host (openvvc_amd/csrc/ovvc_surface_lut.c): ovhip_surface_lut_host against the
numpy restatement tests/spec_surface_lut.py, the coefficients against exact rationals, a census of what the inputs exercise, the pin
of the window clamp, the properties of the definition, the distance to the real-valued model, and the refusals.  The definition is
integer only: every comparison is of bytes unless it says otherwise.

Two statements of the census are weaker on purpose than "the clip occurs at both ends", because the definition makes the stronger
ones impossible, and the tests assert THAT instead:
  * part 5 (luma): the three luma coefficients sum to rnd(sy) and q <= 16368, so (Y14 + 8) >> 4 lies in 0..1023 for every table -- the
    clip never acts.  Asserted: both ends, 0 and 1023, are reached, and no value before the clip lies outside.
  * part 6 (chroma): the value before the clip reaches 1024 (full range, a saturated blue or red: the clip acts at the upper end) but
    is never below 1 (8192 - 8184 = 8 is the smallest C14; (16 * 8 + 128) >> 8 = 1).  Asserted: 1024 and 1 both occur.
  * the halo clamp: W and H are even, so the taps 2i + 1 <= W - 1 and 2j + 1 <= H - 1 are never clamped; only column -1 and row -1
    are.  Asserted: the destination filter's clamp acts on the left and the top edge and on no tap of the right and the bottom
    edge, and the SOURCE's chroma taps (clamped to the picture) act on all four edges of the picture."""
import ctypes as C
import itertools

import numpy as np
import pytest

import spec_rgb as sr
import spec_rgb_lut as sl
import spec_surface as ss
import spec_surface_lut as sx
import surface_lut_cases as cs
from openvvc_amd import capi, engine, lut3d

EINVAL, EUNSUP = cs.EINVAL, cs.EUNSUP
NAMES = ["ovhip_surface_lut_check", "ovhip_surface_lut_coefs", "ovhip_surface_lut_host", "ovhip_surface_lut_launch", "ovhip_pic_output_surface_lut",
         "ovhip_frame_set_surface_lut", "ovhip_stream_set_surface_lut"]


def twin_cases():
    """every (conversion, source location, destination location), twice: each time with one table size, peak and window, in two
    rotations with different offsets.  Every value of every axis is met; every destination location meets every source location under
    every conversion, every table size, every window and every peak; every case runs all formats and roundings, so those are crossed
    with everything"""
    out = []
    for n, (k, sloc, dloc) in enumerate(itertools.product(range(len(cs.CONVS)), cs.SRC_LOCS, sx.DST_LOCS)):
        out.append((cs.conv_of(k, sloc, dloc), cs.TABLE_SIZES[n % 3], cs.PEAKS[(n // 3) % 4], cs.WINDOWS[(n + n // 4) % 3]))
    for n, (k, sloc, dloc) in enumerate(itertools.product(range(len(cs.CONVS)), cs.SRC_LOCS, sx.DST_LOCS)):
        out.append((cs.conv_of(k, sloc, dloc), cs.TABLE_SIZES[(n + 1) % 3], cs.PEAKS[(n // 4 + dloc) % 4], cs.WINDOWS[(n + n // 4 + 1) % 3]))
    return out


def test_the_rotation_meets_every_value():
    cases = twin_cases()
    assert len(cases) == 72 and len(set(cases)) == 72
    assert {c[1] for c in cases} == set(cs.TABLE_SIZES) and {c[2] for c in cases} == set(cs.PEAKS) and {c[3] for c in cases} == set(cs.WINDOWS)
    for dloc in sx.DST_LOCS:
        mine = [c for c in cases if c[0][5] == dloc]
        assert {c[3] for c in mine} == set(cs.WINDOWS) and {c[1] for c in mine} == set(cs.TABLE_SIZES) and {c[2] for c in mine} == set(cs.PEAKS), dloc


def test_the_names_are_exported_and_the_abi_version_stays(built_lib):
    for n in NAMES:
        assert n in capi.EXPORTED_SYMBOLS and hasattr(built_lib, n), n
    assert capi.OVHIP_ABI_VERSION == 9 and built_lib.ovhip_abi_version() == 9
    assert C.sizeof(capi.SurfaceConv) == 8
    header = (capi._PKG.parent / "include" / "ovvc_hip.h").read_text()
    for n in NAMES:
        assert f" {n}(" in header, n
    assert "} ovhip_surface_conv;" in header


def test_surface_bytes_is_unchanged(built_lib):
    for (w, h), wd, (fmt, _) in itertools.product(cs.PICTURES, cs.WINDOWS, ss.MODES):
        W, H = cs.window_size(w, h, wd)
        shapes = [(H, W), (H // 2, W)] if ss.SEMI[fmt] else [(H, W), (H // 2, W // 2), (H // 2, W // 2)]
        for lay in ({}, cs.loose(fmt, W, H)):
            cf = engine.surface_format(fmt, 0, **lay)
            assert built_lib.ovhip_surface_bytes(w, h, C.byref(capi.Window(*wd)), C.byref(cf)) == ss.layout(shapes, ss.ELEM[fmt], **lay)[1]


@pytest.mark.parametrize("matrix", sx.DST_MATRICES)
@pytest.mark.parametrize("full", (0, 1))
def test_coefficients_equal_the_fractions(built_lib, matrix, full):
    want, yoff = sx.coefs(matrix, full)
    got, y = (C.c_int32 * 9)(), C.c_int32(-1)
    assert built_lib.ovhip_surface_lut_coefs(C.byref(capi.SurfaceConv(9, 0, 0, matrix, full, 0)), got, C.byref(y)) == 0
    assert tuple(got) == want and y.value == yoff
    assert sum(want[3:6]) == 0 and sum(want[6:9]) == 0
    assert sum(want[0:3]) == sx.rnd((sx.F(1) if full else sx.F(876, 1023)) * 2 ** 14)
    if (matrix, full) == (1, 0):
        assert want == (2983, 10034, 1013, -1644, -5531, 7175, 7175, -6517, -658)


def test_coefficient_refusals(built_lib):
    got, y = (C.c_int32 * 9)(), C.c_int32()
    for m, code in ((2, EINVAL), (0, EUNSUP), (3, EUNSUP), (4, EUNSUP), (7, EUNSUP), (8, EUNSUP), (10, EUNSUP), (14, EUNSUP), (255, EUNSUP)):
        assert built_lib.ovhip_surface_lut_coefs(C.byref(capi.SurfaceConv(9, 0, 0, m, 0, 0)), got, C.byref(y)) == code, m
    assert built_lib.ovhip_surface_lut_coefs(C.byref(capi.SurfaceConv(9, 0, 0, 1, 2, 0)), got, C.byref(y)) == EINVAL
    assert built_lib.ovhip_surface_lut_coefs(None, got, C.byref(y)) == EINVAL


@pytest.mark.parametrize("case", twin_cases(), ids=lambda c: "-".join(str(v) for v in c[0]) + f"-S{c[1]}-P{c[2]}")
def test_host_twin_equals_the_restatement(built_lib, case):
    """both pictures, the four formats with both roundings, tight and with a pitch with gaps and plane offsets over a sentinel; strides
    above the widths throughout"""
    conv, size, peak, wd = case
    table = cs.census_table(size, peak)
    for w, h in cs.PICTURES:
        planes = cs.census_planes(w, h)
        W, H = cs.window_size(w, h, wd)
        for fmt, rounding in ss.MODES:
            for lay in ({}, cs.loose(fmt, W, H)):
                got, need = cs.host_twin(built_lib, planes, conv, fmt, rounding, table, peak, wd, **lay)
                want, size_want = cs.reference(w, h, conv, size, peak, wd, fmt, rounding, total=len(got), **lay)
                assert need == size_want
                assert got.tobytes() == want.tobytes(), (w, h, fmt, rounding, bool(lay))         # (the sentinel in gaps and tail included)


def test_census_of_the_inputs_used():
    """over what test_host_twin_equals_the_restatement feeds the twin (see the module's text for the two ends)"""
    y_lo = y_hi = c_lo = c_hi = None
    orders = set()
    for conv, size, peak, wd in twin_cases():
        for w, h in cs.PICTURES:
            cen = cs.census_of(w, h, conv, size, peak, wd)
            (a, b), (c, d) = cen["y_pre"][0], cen["c_pre"][0]
            y_lo, y_hi = min(a, y_lo if y_lo is not None else a), max(b, y_hi if y_hi is not None else b)
            c_lo, c_hi = min(c, c_lo if c_lo is not None else c), max(d, c_hi if c_hi is not None else d)
            _, f = sl.cells(cen["rgb"][0], size)
            strict = (f[0] != f[1]) & (f[1] != f[2]) & (f[0] != f[2])
            orders |= {tuple(o) for o in sl.order(f, 0)[:, strict].T}
    assert (y_lo, y_hi) == (0, 1023), "the luma plane does not reach both ends, or leaves them"
    assert (c_lo, c_hi) == (1, 1024), "the chroma planes do not reach 1 and the clipped 1024, or pass them"
    assert orders == set(itertools.permutations(range(3))), orders


def test_census_of_the_clamps():
    for w, h in cs.PICTURES:
        for wd in cs.WINDOWS:
            W, H = cs.window_size(w, h, wd)
            for three in (False, True):
                for n_out, n_in in ((W // 2, W), (H // 2, H)):
                    pos = np.stack([p for p, _ in sx.taps(n_out, n_in, three)])
                    raw = np.stack([2 * np.arange(n_out) + d for d in ((-1, 0, 1) if three else (0, 1))])
                    assert ((pos != raw).any(axis=0) == ([True] + [False] * (n_out - 1) if three else [False] * n_out)).all()     # the first edge only
                    assert raw.max() == n_in - 1                                                  # the last tap is the last sample: nothing to clamp
        # the source's chroma taps, clamped to the picture: before the clamp they leave it on every edge for some location
        for n_luma, n_chroma in ((w, w // 2), (h, h // 2)):
            below = above = False
            for off in (0, 1, 2):
                p = 2 * np.arange(n_luma) - off
                below |= bool(((p >> 2) < 0).any())
                above |= bool(((p >> 2) + 1 > n_chroma - 1).any())
            assert below and above


def test_luma_outside_the_window_is_never_read_and_the_taps_clamp_to_the_window(built_lib):
    w, h, wd, size, peak = 72, 40, (1, 1, 1, 1), 17, 1023
    planes = cs.census_planes(w, h)
    table = cs.census_table(size, peak)
    other = planes[0].copy()
    inside = np.zeros_like(other, bool)
    inside[2:h - 2, 2:w - 2] = True
    other[~inside] ^= 0x155
    differs = 0
    for dloc in sx.DST_LOCS:
        conv = cs.conv_of(0, 0, dloc)
        got, _ = cs.host_twin(built_lib, planes, conv, ss.I010, 0, table, peak, wd)
        got2, _ = cs.host_twin(built_lib, (other, planes[1], planes[2]), conv, ss.I010, 0, table, peak, wd)
        assert got.tobytes() == got2.tobytes(), dloc
        want, _ = sx.surface(planes, conv, table, peak, ss.I010, window=wd, total=len(got))
        assert got.tobytes() == want.tobytes()
        # the variant that clamps to the picture reads the column and the row before the window, where the definition repeats its own
        variant, _ = sx.surface(planes, conv, table, peak, ss.I010, window=wd, total=len(got), clamp_to_picture=True)
        if dloc == 1:
            assert variant.tobytes() == want.tobytes()             # centred both ways: no tap outside, nothing to tell apart
        else:
            assert variant.tobytes() != want.tobytes(), dloc
            differs += 1
    assert differs == 3


@pytest.mark.parametrize("size", cs.TABLE_SIZES)
def test_flat_grey_through_the_lattice_table_is_flat_and_neutral(built_lib, size):
    """limited to limited, the same matrix: Cb = Cr = 512 exactly, the luma flat and the input's value to within one (two roundings)"""
    n = size - 1
    table, peak = lut3d.lattice(size), 1023 * n                   # with this peak the normalised value is exactly 16 (R, G, B)
    w, h = 20, 12
    for matrix, v in itertools.product((1, 5, 9), (64, 65, 300, 511, 512, 940)):
        planes = (np.full((h, w), v, np.uint16), np.full((h // 2, w // 2), 512, np.uint16), np.full((h // 2, w // 2), 512, np.uint16))
        for dloc in sx.DST_LOCS:
            got, need = cs.host_twin(built_lib, planes, (matrix, 0, 0, matrix, 0, dloc), ss.I010, 0, table, peak)
            s = got[:need].view("<u2")
            yy, cc = s[:w * h], s[w * h:]
            assert len(set(yy)) == 1 and abs(int(yy[0]) - v) <= 1, (matrix, v, int(yy[0]))
            assert (cc == 512).all(), (matrix, v)


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_a_table_that_reads_one_index_pins_the_index_order_through_to_luma(built_lib, axis):
    """T[b][g][r][c] = 100 * (its r, g or b index) for ONE output channel c, 0 for the others: Y14 is y_c times the normalised
    interpolation of THAT input channel, and no other reading of the index order gives it"""
    size, peak, w, h = 17, 1600, 72, 40
    planes = cs.census_planes(w, h)
    k = np.arange(size, dtype=np.uint16) * 100
    shape = [1, 1, 1]
    shape[2 - axis] = size                                                   # axis 0 = r: the fastest index
    ramp = np.broadcast_to(k.reshape(shape), (size, size, size))
    rgb = sl.rgb10(*planes, 9, 0, 0)
    i, f = sl.cells(rgb[axis], size)
    o = ((1023 - f) * 100 * i + f * 100 * (i + 1) + 511) // 1023
    coef, yoff = sx.coefs(1, 0)
    wants = []
    for c in range(3):
        table = np.zeros((size, size, size, 3), np.uint16)
        table[..., c] = ramp
        got, _ = cs.host_twin(built_lib, planes, (9, 0, 0, 1, 0, 0), ss.I010, 0, table, peak)
        want = np.clip((16 * yoff + ((coef[c] * sx.normalise(o, peak) + 2 ** 13) >> 14) + 8) >> 4, 0, 1023)
        assert np.array_equal(got[:2 * w * h].view("<u2").reshape(h, w), want), (axis, c)
        wants.append(want)
    assert not np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[1], wants[2])
    assert all(not np.array_equal(rgb[axis], rgb[a]) for a in range(3) if a != axis)


@pytest.mark.parametrize("matrix,full", [(1, 0), (1, 1), (5, 0), (9, 1)])
def test_a_saturated_red_table_against_the_real_valued_model(built_lib, matrix, full):
    """a constant table R = P, G = B = 0: every sample of the converted picture is the model's Y, Cb, Cr to within the derived bound
    (in units of 2^-4 of a step) plus the half step of the final rounding.  The bound is against the model, never against the code"""
    w, h = 20, 12
    planes = cs.census_planes(w, h)
    by, bb, br = sx.bound14(matrix, full)
    for peak in (1, 255, 1023, 4000, 65535):
        table = np.zeros((17, 17, 17, 3), np.uint16)
        table[..., 0] = peak
        got, need = cs.host_twin(built_lib, planes, (9, 0, 2, matrix, full, 2), ss.I010, 0, table, peak)
        s = got[:need].view("<u2").astype(np.float64)
        m = sx.model14(np.array([[peak], [0], [0]]), peak, matrix, full)[:, 0] / 16
        yy, cb, cr = s[:w * h], s[w * h:w * h + w * h // 4], s[w * h + w * h // 4:]
        assert len(set(yy)) == len(set(cb)) == len(set(cr)) == 1
        assert abs(yy[0] - m[0]) <= by / 16 + 0.5 and abs(cb[0] - m[1]) <= bb / 16 + 0.5, (peak, yy[0], cb[0], m)
        assert abs(min(cr[0], 1023.5) - min(m[2], 1023.5)) <= br / 16 + 0.5, (peak, cr[0], m)          # (Cr of red is clipped in full range)


@pytest.mark.parametrize("matrix", (1, 5, 9))
@pytest.mark.parametrize("full", (0, 1))
def test_distance_to_the_real_valued_model(matrix, full):
    """200 000 random triples per peak: |integer - model| of Y14, Cb14, Cr14 stays inside the derived bound; the largest distance over
    all cells is printed, and quoted in DESIGN section 7 (a measurement: nothing is asserted about it but the bound)"""
    bound = sx.bound14(matrix, full)
    assert max(bound) <= 3.5                                       # the a-priori bound: 1/2 + 1/2 + (1/2 + 1/2 + 3/2) * 16368 / 16384
    rng = np.random.default_rng(100 * matrix + full)
    worst = 0.0
    for peak in (1, 255, 1023, 4000, 65535):
        o = rng.integers(0, peak + 1, (3, 200000))
        o[:, :8] = np.array(list(itertools.product((0, peak), repeat=3))).T
        d = np.abs(sx.forward14(o, peak, matrix, full) - sx.model14(o, peak, matrix, full))
        print(f"matrix {matrix} full {full} peak {peak}: max distance {d.max(axis=1)} bound {bound}")
        for k in range(3):
            assert d[k].max() <= bound[k], (peak, k, d[k].max(), bound[k])
        worst = max(worst, float(d.max()))
        grey = np.broadcast_to(rng.integers(0, peak + 1, (1, 1000)), (3, 1000))
        assert (sx.forward14(grey, peak, matrix, full)[1:] == 8192).all()
        y = sx.forward14(np.array([[0, peak]] * 3), peak, matrix, full)[0]
        assert tuple(y) == ((0, 16368) if full else (16 * 64, 16 * (64 + 876)))
    print(f"matrix {matrix} full {full}: largest distance {worst:.4f}")


def test_refusals_write_nothing(built_lib):
    lib = built_lib
    w, h = 24, 8
    y, cb, cr = sr.random_planes(w, h, 3)
    ok = engine.surface_format(ss.P010)
    okc = capi.SurfaceConv(9, 0, 2, 1, 0, 0)
    need = lib.ovhip_surface_bytes(w, h, None, C.byref(ok))
    dst = np.full(need + 64, 0xA5, np.uint8)
    good = sl.random_table(17, 1023, 1)
    above = good.copy()
    above[16, 3, 5, 1] = 1024

    def conv(**kw):
        c = capi.SurfaceConv(9, 0, 2, 1, 0, 0)
        for k, v in kw.items():
            if k == "rsv":
                c.rsv[v] = 1
            else:
                setattr(c, k, v)
        return c

    def fmt(**kw):
        f = engine.surface_format(kw.pop("format", ss.P010), kw.pop("rounding", 0), **kw)
        return f

    def rsv_fmt():
        f = engine.surface_format(ss.P010)
        f.rsv[1] = 1
        return f

    def call(cv=okc, f=ok, win=None, planes=(y, cb, cr), size=(w, h), strides=(w, w // 2), dptr=dst.ctypes.data, nbytes=need, table=good, s=17, peak=1023):
        p = [a.ctypes.data if a is not None else None for a in planes]
        return lib.ovhip_surface_lut_host(p[0], p[1], p[2], size[0], size[1], strides[0], strides[1], C.byref(capi.Window(*win)) if win else None,
                                          C.byref(cv) if cv is not None else None, C.byref(f) if f is not None else None, s, peak,
                                          table.ctypes.data if table is not None else None, dptr, nbytes)

    cases = {
        # the conversion's
        "null conversion": (dict(cv=None), EINVAL),
        "conv rsv[0]": (dict(cv=conv(rsv=0)), EINVAL),
        "conv rsv[1]": (dict(cv=conv(rsv=1)), EINVAL),
        "source matrix unspecified": (dict(cv=conv(src_matrix=2)), EINVAL),
        "source matrix not built": (dict(cv=conv(src_matrix=0)), EUNSUP),
        "source range": (dict(cv=conv(src_full_range=2)), EINVAL),
        "source chroma location": (dict(cv=conv(src_chroma_loc=6)), EINVAL),
        "destination matrix unspecified": (dict(cv=conv(dst_matrix=2)), EINVAL),
        "destination matrix not built": (dict(cv=conv(dst_matrix=14)), EUNSUP),
        "destination matrix 0": (dict(cv=conv(dst_matrix=0)), EUNSUP),
        "destination range": (dict(cv=conv(dst_full_range=2)), EINVAL),
        "destination chroma location 4": (dict(cv=conv(dst_chroma_loc=4)), EUNSUP),
        "destination chroma location 5": (dict(cv=conv(dst_chroma_loc=5)), EUNSUP),
        "destination chroma location 6": (dict(cv=conv(dst_chroma_loc=6)), EINVAL),
        # the table's
        "null table": (dict(table=None), EINVAL),
        "size 16": (dict(s=16), EINVAL),
        "size 0": (dict(s=0), EINVAL),
        "peak 0": (dict(peak=0), EINVAL),
        "peak 65536": (dict(peak=65536), EINVAL),
        "an entry above the peak": (dict(table=above), EINVAL),
        # the RGB side's of the picture
        "width not a multiple of 4": (dict(size=(w - 2, h)), EINVAL),
        "height not a multiple of 4": (dict(size=(w, h - 2)), EINVAL),
        # the surface output's
        "null format": (dict(f=None), EINVAL),
        "unknown format": (dict(f=fmt(format=4)), EINVAL),
        "unknown rounding": (dict(f=fmt(format=ss.NV12, rounding=2)), EINVAL),
        "dither on a 16-bit format": (dict(f=fmt(rounding=1)), EINVAL),
        "format rsv": (dict(f=rsv_fmt()), EINVAL),
        "offset_c[1] on a semi-planar format": (dict(f=fmt(offset_c=(0, 4096))), EINVAL),
        "pitch below the row": (dict(f=fmt(pitch_y=2 * w - 2)), EINVAL),
        "odd pitch on a 16-bit format": (dict(f=fmt(pitch_y=2 * w + 1)), EINVAL),
        "planes overlapping one another": (dict(f=fmt(offset_c=(2 * w, 0))), EINVAL),
        "null destination": (dict(dptr=None), EINVAL),
        "dst_bytes too small": (dict(nbytes=need - 1), EINVAL),
        "element-misaligned destination": (dict(dptr=dst.ctypes.data + 1), EINVAL),
        "destination overlapping the luma plane": (dict(dptr=y.ctypes.data, nbytes=1 << 20), EINVAL),
        "destination overlapping the Cr plane": (dict(dptr=cr.ctypes.data + 2, nbytes=1 << 20), EINVAL),
        "window that leaves nothing (columns)": (dict(win=(6, 6, 0, 0)), EINVAL),
        "window that leaves nothing (rows)": (dict(win=(0, 0, 2, 2)), EINVAL),
        "missing luma": (dict(planes=(None, cb, cr)), EINVAL),
        "missing Cb": (dict(planes=(y, None, cr)), EINVAL),
        "missing Cr": (dict(planes=(y, cb, None)), EINVAL),
        "luma stride below the width": (dict(strides=(w - 1, w // 2)), EINVAL),
        "chroma stride below the width": (dict(strides=(w, w // 2 - 1)), EINVAL),
        "zero size": (dict(size=(0, h)), EINVAL),
        "size above 16384": (dict(size=(16388, h), strides=(16388, 8194)), EINVAL),
    }
    keep = (y.copy(), cb.copy(), cr.copy())
    for name, (kw, code) in cases.items():
        assert call(**kw) == code, name
        assert (dst == 0xA5).all(), name
        assert all(np.array_equal(a, b) for a, b in zip((y, cb, cr), keep)), name
    assert call() == 0
    assert (dst[:need] != 0xA5).any() and (dst[need:] == 0xA5).all()
    # no restriction on the peak: an 8-bit surface from a table of 65535, a 16-bit one from a table of 1
    dst[:] = 0xA5
    assert call(f=fmt(format=ss.NV12), peak=65535, table=sl.random_table(17, 65535, 2)) == 0
    assert call(peak=1, table=sl.random_table(17, 1, 2)) == 0


def test_check(built_lib):
    lib = built_lib
    ok, okc = engine.surface_format(ss.NV12, 1), capi.SurfaceConv(9, 0, 2, 1, 0, 0)
    assert lib.ovhip_surface_lut_check(C.byref(okc), C.byref(ok), 33, 4000) == 0
    assert lib.ovhip_surface_lut_check(None, C.byref(ok), 33, 4000) == EINVAL
    assert lib.ovhip_surface_lut_check(C.byref(okc), None, 33, 4000) == EINVAL
    assert lib.ovhip_surface_lut_check(C.byref(okc), C.byref(ok), 32, 4000) == EINVAL
    assert lib.ovhip_surface_lut_check(C.byref(okc), C.byref(ok), 33, 0) == EINVAL
    assert lib.ovhip_surface_lut_check(C.byref(capi.SurfaceConv(9, 0, 2, 1, 0, 4)), C.byref(ok), 33, 255) == EUNSUP
    assert lib.ovhip_surface_lut_check(C.byref(capi.SurfaceConv(9, 0, 2, 2, 0, 0)), C.byref(ok), 33, 255) == EINVAL
    assert lib.ovhip_surface_lut_check(C.byref(okc), C.byref(engine.surface_format(ss.P010, 1)), 33, 255) == EINVAL
    c = engine.surface_conv()
    assert (c.src_matrix, c.src_full_range, c.src_chroma_loc, c.dst_matrix, c.dst_full_range, c.dst_chroma_loc, tuple(c.rsv)) == (9, 0, 2, 1, 0, 0, (0, 0))
