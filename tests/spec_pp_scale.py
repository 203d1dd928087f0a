"""Test infrastructure: numpy restatement of the output resampler (the reference's pp_sample_rate_conv, pp_pic_scale.c:250-377) for
up-sampling and equal size, and the reader of its fixture tests/golden/pp_scale/*.ovg (tools/pp_scale_golden/gen_pp_scale.c).

Per plane (luma: bits 13, mask 15, 8 taps; chroma: bits 14, mask 31, 4 taps), source ow x oh, destination sw x sh:
    extra_w = (win_left + win_right) << 1 (<< 2 for luma), held in 16 bits; extra_h likewise
    scale_hor = ((ow - extra_w) << bits) / sw          (C division)
    chroma: add_x = ((1 - hor_col) * 8 * (scale_hor - (1 << bits)) + (1 << (bits - 1))) >> bits   (arithmetic), luma 0
    column i: ref = i * scale_hor + add_x, xi = ref >> bits, ph = ref & mask   -- the LOW bits of the position, the reference's quirk
    tmp[j][i] = sum_k f[ph][k] * src[j][clamp(xi + k - taps / 2 + 1)]          (int32, no shift)
    row j likewise from tmp; out = clip((sum + 2048) >> 12, 0, 1023)
"""
import numpy as np

import golden_io

OK, EINVAL, EUNSUP = 0, -3, -5

MC_LUMA = np.array([
    [0, 0, 0, 64, 0, 0, 0, 0], [0, 1, -3, 63, 4, -2, 1, 0], [-1, 2, -5, 62, 8, -3, 1, 0], [-1, 3, -8, 60, 13, -4, 1, 0],
    [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 52, 26, -8, 3, -1], [-1, 3, -9, 47, 31, -10, 4, -1], [-1, 4, -11, 45, 34, -10, 4, -1],
    [-1, 4, -11, 40, 40, -11, 4, -1], [-1, 4, -10, 34, 45, -11, 4, -1], [-1, 4, -10, 31, 47, -9, 3, -1], [-1, 3, -8, 26, 52, -11, 4, -1],
    [0, 1, -5, 17, 58, -10, 4, -1], [0, 1, -4, 13, 60, -8, 3, -1], [0, 1, -3, 8, 62, -5, 2, -1], [0, 1, -2, 4, 63, -3, 1, 0]], dtype=np.int64)
MC_CHROMA = np.array([
    [0, 64, 0, 0], [-1, 63, 2, 0], [-2, 62, 4, 0], [-2, 60, 7, -1], [-2, 58, 10, -2], [-3, 57, 12, -2], [-4, 56, 14, -2], [-4, 55, 15, -2],
    [-4, 54, 16, -2], [-5, 53, 18, -2], [-6, 52, 20, -2], [-6, 49, 24, -3], [-6, 46, 28, -4], [-5, 44, 29, -4], [-4, 42, 30, -4], [-4, 39, 33, -4],
    [-4, 36, 36, -4], [-4, 33, 39, -4], [-4, 30, 42, -4], [-4, 29, 44, -5], [-4, 28, 46, -6], [-3, 24, 49, -6], [-2, 20, 52, -6], [-2, 18, 53, -5],
    [-2, 16, 54, -4], [-2, 15, 55, -4], [-2, 14, 56, -4], [-2, 12, 57, -3], [-2, 10, 58, -2], [-1, 7, 60, -2], [0, 4, 62, -2], [0, 2, 63, -1]], dtype=np.int64)

NO_WINDOW = (0, 0, 0, 0)


def plane_params(ow, oh, sw, sh, win, col, luma):
    """(bits, mask, scale_hor, scale_ver, add_x, add_y, avail_w, avail_h) of one plane; win = (left, right, top, bottom), col = (hor, ver)"""
    bits, mask = (13, 15) if luma else (14, 31)
    extra_w = ((win[0] + win[1]) << (2 if luma else 1)) & 0xFFFF
    extra_h = ((win[2] + win[3]) << (2 if luma else 1)) & 0xFFFF
    aw, ah = ow - extra_w, oh - extra_h
    if aw <= 0 or ah <= 0:
        return bits, mask, 0, 0, 0, 0, aw, ah
    scale_hor, scale_ver = (aw << bits) // sw, (ah << bits) // sh
    add_x = add_y = 0
    if not luma:
        add_x = ((1 - col[0]) * 8 * (scale_hor - (1 << bits)) + (1 << (bits - 1))) >> bits      # Python's >> is arithmetic
        add_y = ((1 - col[1]) * 8 * (scale_ver - (1 << bits)) + (1 << (bits - 1))) >> bits
    return bits, mask, scale_hor, scale_ver, add_x, add_y, aw, ah


def check(src_w, src_h, win, col, dst_w, dst_h):
    """What ovhip_output_scale_check returns: (code, [luma hor, luma ver, chroma hor, chroma ver])."""
    if min(src_w, src_h, dst_w, dst_h) <= 0 or any(v % 4 for v in (src_w, src_h, dst_w, dst_h)):
        return EINVAL, None
    pl = plane_params(src_w, src_h, dst_w, dst_h, win, col, True)
    pc = plane_params(src_w // 2, src_h // 2, dst_w // 2, dst_h // 2, win, col, False)
    if min(pl[6], pl[7], pc[6], pc[7]) <= 0:
        return EINVAL, None
    scale = [pl[2], pl[3], pc[2], pc[3]]
    if pl[2] > 1 << 13 or pl[3] > 1 << 13 or pc[2] > 1 << 14 or pc[3] > 1 << 14:
        return EUNSUP, scale
    return OK, scale


def is_upsampling(src_w, src_h, win, col, dst_w, dst_h) -> bool:
    return check(src_w, src_h, win, col, dst_w, dst_h)[0] == OK


def scale_plane(src, sw, sh, win=NO_WINDOW, col=(0, 0), luma=True):
    """One plane, src[oh][ow] -> uint16 [sh][sw]."""
    src = np.asarray(src).astype(np.int64)
    oh, ow = src.shape
    bits, mask, scale_hor, scale_ver, add_x, add_y, aw, ah = plane_params(ow, oh, sw, sh, win, col, luma)
    assert aw > 0 and ah > 0 and scale_hor <= 1 << bits and scale_ver <= 1 << bits, "not up-sampling"
    f = MC_LUMA if luma else MC_CHROMA
    taps = f.shape[1]
    ref = np.arange(sw, dtype=np.int64) * scale_hor + add_x
    xi, ph = ref >> bits, ref & mask
    tmp = np.zeros((oh, sw), dtype=np.int64)
    for k in range(taps):
        tmp += f[ph, k][None, :] * src[:, np.clip(xi + k - taps // 2 + 1, 0, ow - 1)]
    ref = np.arange(sh, dtype=np.int64) * scale_ver + add_y
    yi, ph = ref >> bits, ref & mask
    acc = np.zeros((sh, sw), dtype=np.int64)
    for k in range(taps):
        acc += f[ph, k][:, None] * tmp[np.clip(yi + k - taps // 2 + 1, 0, oh - 1), :]
    return np.clip((acc + 2048) >> 12, 0, 1023).astype(np.uint16)


def scale_picture(y, cb, cr, out_w, out_h, win=NO_WINDOW, col=(0, 0)):
    """The three planes of a 4:2:0 picture at out_w x out_h (luma)."""
    return (scale_plane(y, out_w, out_h, win, col, True), scale_plane(cb, out_w // 2, out_h // 2, win, col, False),
            scale_plane(cr, out_w // 2, out_h // 2, win, col, False))


def load_cases():
    """The fixture: a list of dicts src_w, src_h, dst_w, dst_h, win, col, src = (y, cb, cr), exp = (y, cb, cr)."""
    g = {}
    for name in ("pp_scale.ovg", "pp_scale_large.ovg"):     # two files: each stays below the size limit of a committed file
        g.update(golden_io.load(name, golden_io.GOLDEN / "pp_scale"))
    cases = []
    for k in sorted(int(n[1:-5]) for n in g if n.endswith("_geom")):
        geom = [int(v) for v in g[f"c{k}_geom"]]
        cases.append(dict(idx=k, src_w=geom[0], src_h=geom[1], dst_w=geom[2], dst_h=geom[3], win=tuple(geom[4:8]), col=tuple(geom[8:10]),
                          src=tuple(g[f"c{k}_s{p}"] for p in ("y", "cb", "cr")), exp=tuple(g[f"c{k}_d{p}"] for p in ("y", "cb", "cr"))))
    return cases
