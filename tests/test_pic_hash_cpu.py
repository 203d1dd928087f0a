"""CPU: the decoded picture hash SEI on the host (openvvc_amd/csrc/ovvc_pichash.c): ovhip_pic_hash_host, the payload reader and the
comparison against the numpy / hashlib restatement tests/spec_pic_hash.py and the vector table the definitions came with.  Every
comparison is exact.  The stand-alone sanitizer program over the same sizes is tools/pichash_check (`make asan`)."""
import ctypes as C

import numpy as np
import pytest

import spec_pic_hash as sp
from openvvc_amd import capi

# 520x264 reaches x >> 8 and y >> 8 in the luma mask; 8x520 is the only shape whose chroma reaches y >> 8, 4 samples wide
SIZES = [(8, 8), (24, 8), (72, 40), (520, 264), (8, 520)]
METHODS = [sp.MD5, sp.CRC, sp.CHECKSUM]


def random_picture(w, h, seed):
    """uniformly random FULL 16-bit words: with 10-bit content the high byte is only 0..3"""
    rs = np.random.RandomState(seed)
    return tuple(rs.randint(0, 65536, shape).astype(np.uint16) for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def host_hash(lib, method, planes, n_planes=3, strides=None):
    h, w = planes[0].shape
    sy, sc = strides or (w, w // 2)
    held = []
    for p, s in zip(planes, (sy, sc, sc)):
        a = np.full((p.shape[0], s), 0xA5A5, np.uint16)
        a[:, :p.shape[1]] = p
        held.append(a)
    out = capi.PicHashValue()
    r = lib.ovhip_pic_hash_host(method, n_planes, held[0].ctypes.data, held[1].ctypes.data if n_planes == 3 else None,
                                held[2].ctypes.data if n_planes == 3 else None, w, h, sy, sc, C.byref(out))
    assert r == 0, r
    assert (out.method, out.n_planes) == (method, n_planes)
    return out


def check_value(out, method, want):
    """every byte of the struct: the significant ones, then zeros, and zero rows for absent planes"""
    nb = sp.VALUE_BYTES[method]
    for c in range(3):
        row = bytes(out.value[c])
        assert row == (want[c] + bytes(16 - nb) if c < len(want) else bytes(16)), (method, c, row.hex())
    assert bytes(out.rsv) == b"\0\0"


def test_struct_layout():
    assert C.sizeof(capi.PicHashValue) == 52
    assert (capi.HASH_MD5, capi.HASH_CRC, capi.HASH_CHECKSUM) == (sp.MD5, sp.CRC, sp.CHECKSUM) == (0, 1, 2)


def test_restatement_reproduces_the_vector_table():
    for (w, h), (crcs, sums, md5_y) in sp.VECTORS.items():
        planes = sp.formula_picture(w, h)
        assert [v.hex() for v in sp.picture_hash(sp.CRC, planes)] == list(crcs), (w, h)
        assert [v.hex() for v in sp.picture_hash(sp.CHECKSUM, planes)] == list(sums), (w, h)
        assert sp.plane_value(sp.MD5, planes[0]).hex() == md5_y, (w, h)
        if w * h <= 72 * 40:                                            # the bit-by-bit definition against the table form
            for p in planes:
                assert sp.crc_literal(sp.plane_bytes(p)) == sp.crc(sp.plane_bytes(p))
    rs = np.random.RandomState(3)
    for n in (0, 1, 2, 17, 300):
        data = rs.bytes(n)
        assert sp.crc_literal(data) == sp.crc(data)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("method", METHODS)
def test_host_equals_the_vectors_and_the_restatement(built_lib, w, h, method):
    planes = sp.formula_picture(w, h)
    out = host_hash(built_lib, method, planes)
    check_value(out, method, sp.picture_hash(method, planes))
    if (w, h) in sp.VECTORS:
        crcs, sums, md5_y = sp.VECTORS[(w, h)]
        got = [v.hex() for v in out.planes()]
        assert got == list(crcs) if method == sp.CRC else got == list(sums) if method == sp.CHECKSUM else got[0] == md5_y
    # full 16-bit words, and the edges of the 10-bit range
    rnd = random_picture(w, h, w * 1000 + h)
    check_value(host_hash(built_lib, method, rnd), method, sp.picture_hash(method, rnd))
    for fill in (0, 1023):
        flat = tuple(np.full_like(p, fill) for p in planes)
        check_value(host_hash(built_lib, method, flat), method, sp.picture_hash(method, flat))


@pytest.mark.parametrize("method", METHODS)
def test_strides_and_plane_count(built_lib, method):
    planes = random_picture(72, 40, 5)
    want = sp.picture_hash(method, planes)
    check_value(host_hash(built_lib, method, planes, strides=(72 + 9, 36 + 5)), method, want)
    check_value(host_hash(built_lib, method, planes, n_planes=1), method, want[:1])          # rows 1 and 2 are zero


def test_host_refusals(built_lib):
    lib, out = built_lib, capi.PicHashValue()
    y, c = np.zeros((8, 8), np.uint16), np.zeros((4, 4), np.uint16)
    args = lambda **k: [k.get("method", 1), k.get("n", 3), y.ctypes.data, k.get("cb", c.ctypes.data), c.ctypes.data,
                        k.get("w", 8), k.get("h", 8), k.get("sy", 8), k.get("sc", 4), C.byref(out)]
    assert lib.ovhip_pic_hash_host(*args()) == 0
    for bad in (dict(method=3), dict(method=-1), dict(n=2), dict(n=0), dict(cb=None), dict(w=7), dict(h=0), dict(sy=7), dict(sc=3)):
        assert lib.ovhip_pic_hash_host(*args(**bad)) == capi.OVHIP_EINVAL, bad
    assert lib.ovhip_pic_hash_host(1, 1, y.ctypes.data, None, None, 8, 8, 8, 0, C.byref(out)) == 0      # one plane: chroma is not looked at
    assert lib.ovhip_pic_hash_host(1, 3, y.ctypes.data, c.ctypes.data, c.ctypes.data, 8, 8, 8, 4, None) == capi.OVHIP_EINVAL


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("single", (0, 1))
def test_sei_reader_round_trip(built_lib, method, single):
    lib = built_lib
    planes = sp.formula_picture(24, 8)
    n_planes = 1 if single else 3
    want = sp.picture_hash(method, planes, n_planes)
    payload = sp.sei_payload(method, want)
    assert len(payload) == 2 + n_planes * sp.VALUE_BYTES[method]
    buf = (C.c_uint8 * len(payload)).from_buffer_copy(payload)
    out = capi.PicHashValue()
    assert lib.ovhip_pic_hash_parse_sei(buf, len(payload), C.byref(out)) == 0
    assert (out.method, out.n_planes) == (method, n_planes)
    check_value(out, method, want)
    # what was read is what the host computes
    mine = host_hash(lib, method, planes, n_planes)
    assert lib.ovhip_pic_hash_equal(C.byref(out), C.byref(mine)) == 1
    # the reserved bits are not looked at; bytes behind the last value neither
    loose = bytes([payload[0], payload[1] | 0x55]) + payload[2:] + b"\xEE"
    out2 = capi.PicHashValue()
    assert lib.ovhip_pic_hash_parse_sei((C.c_uint8 * len(loose)).from_buffer_copy(loose), len(loose), C.byref(out2)) == 0
    assert lib.ovhip_pic_hash_equal(C.byref(out), C.byref(out2)) == 1
    # one byte short: refused, and nothing is written
    out3 = capi.PicHashValue()
    out3.method = 77
    assert lib.ovhip_pic_hash_parse_sei(buf, len(payload) - 1, C.byref(out3)) == capi.OVHIP_EINVAL and out3.method == 77
    for n in (0, 1):
        assert lib.ovhip_pic_hash_parse_sei(buf, n, C.byref(out3)) == capi.OVHIP_EINVAL


def test_sei_reader_refuses_hash_type_3(built_lib):
    payload = bytes([3, 0]) + bytes(48)
    out = capi.PicHashValue()
    assert built_lib.ovhip_pic_hash_parse_sei((C.c_uint8 * 50).from_buffer_copy(payload), 50, C.byref(out)) == capi.OVHIP_EINVAL
    assert built_lib.ovhip_pic_hash_parse_sei(None, 50, C.byref(out)) == capi.OVHIP_EINVAL
    assert built_lib.ovhip_pic_hash_parse_sei((C.c_uint8 * 50).from_buffer_copy(payload), 50, None) == capi.OVHIP_EINVAL


def test_equal_compares_method_count_and_significant_bytes(built_lib):
    lib = built_lib
    planes = sp.formula_picture(24, 8)
    a, b = host_hash(lib, sp.CRC, planes), host_hash(lib, sp.CRC, planes)
    eq = lambda p, q: lib.ovhip_pic_hash_equal(C.byref(p), C.byref(q))
    assert eq(a, b) == 1
    b.value[1][2] = 9                                                   # behind the CRC's two bytes: not significant
    assert eq(a, b) == 1
    b.value[1][1] ^= 1
    assert eq(a, b) == 0
    assert eq(a, host_hash(lib, sp.CRC, planes, 1)) == 0               # another plane count
    assert eq(a, host_hash(lib, sp.CHECKSUM, planes)) == 0             # another method
    assert lib.ovhip_pic_hash_equal(None, C.byref(a)) == 0


@pytest.mark.parametrize("method", METHODS)
def test_a_single_bit_changes_its_plane_and_no_other(built_lib, method):
    planes = random_picture(72, 40, 11)
    base = host_hash(built_lib, method, planes).planes()
    for c, (yy, xx, bit) in enumerate(((39, 71, 0), (0, 0, 15), (19, 35, 8))):
        changed = [p.copy() for p in planes]
        changed[c][yy, xx] ^= 1 << bit
        got = host_hash(built_lib, method, changed).planes()
        assert got == sp.picture_hash(method, changed)
        for k in range(3):
            assert (got[k] != base[k]) == (k == c), (method, c, k)


def test_device_entry_points_refuse_without_a_context(built_lib):
    lib, a, out = built_lib, capi.Pic(), capi.PicHashValue()
    assert lib.ovhip_pic_hash_launch(None, C.byref(a), sp.CRC, 3, None) == capi.OVHIP_EINVAL
    assert lib.ovhip_pic_hash(None, C.byref(a), sp.CRC, 3, C.byref(out)) == capi.OVHIP_EINVAL
    assert lib.ovhip_frame_set_picture_hash(None, sp.CRC, 3, None) == capi.OVHIP_EINVAL
    assert lib.ovhip_frame_picture_hash(None, C.byref(out)) == capi.OVHIP_EINVAL
    assert lib.ovhip_stream_set_picture_hashes(None, sp.CRC, 3, None) == capi.OVHIP_EINVAL
    assert lib.ovhip_stream_picture_hashes(None, None, None, None) == capi.OVHIP_EINVAL


def test_dry_frame_accepts_the_setter_and_computes_nothing(built_lib):
    """a DPB on a counting memory back-end (no device): the setting is taken, the picture is submitted and published as before"""
    from test_dpb_cpu import FakeMem
    lib = built_lib
    mem, h, f = FakeMem(), C.c_void_p(), C.c_void_p()
    assert lib.ovhip_dpb_create_ex(C.byref(h), 1, C.byref(mem.ops)) == 0
    assert lib.ovhip_frame_create(h, 0, 64, 64, C.byref(f)) == 0
    out = capi.PicHashValue()
    assert lib.ovhip_frame_picture_hash(f, C.byref(out)) == capi.OVHIP_EINVAL                 # nothing computed yet
    exp = host_hash(lib, sp.CRC, sp.formula_picture(64, 64))
    assert lib.ovhip_frame_set_picture_hash(f, sp.CRC, 3, C.byref(exp)) == 0
    # the setter's own refusals
    assert lib.ovhip_frame_set_picture_hash(f, 3, 3, None) == capi.OVHIP_EINVAL
    assert lib.ovhip_frame_set_picture_hash(f, sp.CRC, 2, None) == capi.OVHIP_EINVAL
    assert lib.ovhip_frame_set_picture_hash(f, sp.CHECKSUM, 3, C.byref(exp)) == capi.OVHIP_EINVAL      # an expectation of another method
    assert lib.ovhip_frame_begin_tag(f, C.c_void_p(0x10), 1) == 0
    p = capi.JobParams()
    assert lib.ovhip_frame_submit(f, None, None, C.byref(p), None) == 0
    assert lib.ovhip_frame_picture_hash(f, C.byref(out)) == capi.OVHIP_EINVAL                 # dry: nothing to hash
    dev, pic = C.c_int(-1), capi.Pic()
    assert lib.ovhip_dpb_lookup(h, C.c_void_p(0x10), C.byref(dev), C.byref(pic)) == 0 and (pic.w, pic.h) == (64, 64)
    assert lib.ovhip_frame_set_picture_hash(f, -1, 0, None) == 0                              # off
    lib.ovhip_frame_destroy(f)
    lib.ovhip_dpb_destroy(h)
