"""What the inverse transform slot fixtures (tests/golden/itx.ovg, itx_cells_*.ovg) reach: every transform block command labelled from the
command itself and from the recorder's split, and the counting test_oracle_golden.py asserts.

Which body of k_itx_all reconstructs a command depends on the ROUTE it takes:
  "itx"      ovhip_itx_launch: every command in the four-wave body;
  "classes"  ovhip_itx_launch_classes on the recorder's split: the large class four-wave, the small class one wave per block;
  "job"      the picture job (ovhip_itx_launch_ex_): as "classes", but the tiny tail of the small class a lane per sample.
body() restates the class rule of ovhip_rec_tb_split_range_ (ovvc_record.c) and the switch of k_itx_all (kernels_itx.hip)."""
import numpy as np

from openvvc_amd import capi

FOUR, GENERIC, SPEC, TINY, DC1 = range(5)
BODY_NAMES = ("four-wave", "one-wave generic", "one-wave specialised", "tiny", "one-wave DC")
ROUTES = ("itx", "classes", "job")
TB_FLAG_BDPCM = 0x40
RES_SCALE_IDX, RES_STORE = 8, 16
# the shapes k_itx_all's switch has a body for (log2_w, log2_h), and the four that itx_tiny takes (8x8, 4x8, 8x4, 4x4: the split's order)
SPEC_SHAPES = ((2, 2), (3, 2), (2, 3), (3, 3), (4, 2), (2, 4), (4, 3), (3, 4), (4, 4), (5, 2), (2, 5), (5, 3), (3, 5))
TINY_SHAPES = ((3, 3), (2, 3), (3, 2), (2, 2))
TINY_GROUP = {(3, 3): 4, (2, 3): 8, (3, 2): 8, (2, 2): 16}          # blocks per workgroup
LUMA_SHAPES = [(a, b) for a in range(2, 7) for b in range(2, 7)]
ONE_WAVE_SHAPES = [s for s in LUMA_SHAPES if s[0] + s[1] <= 8 and max(s) <= 5]
IQ_SCALE = ((40, 45, 51, 57, 64, 72), (57, 64, 72, 80, 90, 102))
KIND_NAMES = ("TR", "DC", "TS", "TS_RAW", "raster TR", "raster DC", "BDPCM horizontal", "BDPCM vertical", "1-D")
K_TR, K_DC, K_TS, K_TS_RAW, K_RASTER_TR, K_RASTER_DC, K_BDPCM_H, K_BDPCM_V, K_1D = range(9)

assert set(SPEC_SHAPES) == set(ONE_WAVE_SHAPES)


def small(c):
    """TB_CLASS's second bit: what one wavefront and a slice of LDS take"""
    return (c["log2_w"].astype(int) + c["log2_h"] <= 8) & (c["log2_w"] <= 5) & (c["log2_h"] <= 5)


def split_class(c):
    return (c["plane"] != 0) * 2 + small(c)


def tiny_shape(c):
    """TB_SHAPE: 0 a wave of its own; 1..4 = TINY_SHAPES"""
    plain = (c["kind"] == capi.TB_DC) | ((c["kind"] == capi.TB_TR) & ((c["lfnst"] & 1) == 0))
    out = np.zeros(len(c), int)
    for k, (lw, lh) in enumerate(TINY_SHAPES):
        out[plain & (c["log2_w"] == lw) & (c["log2_h"] == lh)] = k + 1
    return out


def split_order(c):
    """the order ovhip_rec_tb_split_range_ puts the commands in (a stable sort by class, then tiny shape), and its four class counts"""
    key = 5 * split_class(c) + tiny_shape(c)
    return np.argsort(key, kind="stable"), tuple(int((split_class(c) == k).sum()) for k in range(4))


def body(c, route):
    """the body of k_itx_all each command takes on `route`"""
    if route == "itx":
        return np.full(len(c), FOUR)
    kind = c["kind"] & 0x3f
    plain = (kind == capi.TB_TR) & ((c["kind"] & (capi.TB_FLAG_RASTER | TB_FLAG_BDPCM)) == 0) & ((c["lfnst"] & 1) == 0)
    spec = np.array([(int(a), int(b)) in SPEC_SHAPES for a, b in zip(c["log2_w"], c["log2_h"])], bool)
    one = np.where(kind == capi.TB_DC, DC1, np.where(plain & spec, SPEC, GENERIC))
    if route == "job":
        one = np.where(tiny_shape(c) > 0, TINY, one)
    return np.where(small(c), one, FOUR)


def extent(c):
    """(nb_row, nb_col) as itx_block derives them for a transform block (0, 0 for the kinds that have none); nb_row counts the
    coefficient COLUMNS that can hold data (derive_nb_rows works on the transposed tile), nb_col the rows"""
    m = c["sig_sb_map"].astype(np.uint64)
    cols = np.zeros(len(c), np.uint64)
    for r in range(8):
        cols |= (m >> np.uint64(8 * r)) & np.uint64(0xff)
    cols |= np.uint64(1)
    nb_row = np.array([int(v).bit_length() for v in cols]) * 4
    nb_col = np.array([(int(v | 1).bit_length() + 7) // 8 for v in m]) * 4
    kind = c["kind"] & 0x3f
    w, h = 1 << c["log2_w"].astype(int), 1 << c["log2_h"].astype(int)
    raster = (c["kind"] & capi.TB_FLAG_RASTER) != 0
    nb_row = np.where(raster, (nb_row >> 2) << np.where(c["log2_w"] > 2, 3, 1), nb_row)
    nb_col = np.where(raster, np.minimum(h, 32), nb_col)
    lf = (c["lfnst"] & 1) != 0
    lf_rows = np.where((c["log2_w"] >= 3) & (c["log2_h"] >= 3), 8, 4)
    nb_row, nb_col = np.where(lf, lf_rows, nb_row), np.where(lf, np.maximum(nb_col, lf_rows), nb_col)
    is_tr = (kind == capi.TB_TR) & (c["log2_w"] > 0) & (c["log2_h"] > 0)
    return np.where(is_tr, np.minimum(nb_row, w), 0), np.where(is_tr, np.minimum(nb_col, np.minimum(h, 32)), 0)


def lfnst_size_class(lw, lh):
    return "4x4" if (lw, lh) == (2, 2) else "4xN" if min(lw, lh) == 2 else "8x8" if (lw, lh) == (3, 3) else "larger"


def label(c):
    """-> dict of arrays over the commands: shape, tr (tr_v, tr_h), kind (K_*), lfnst (None or (set, index, transposed, size class)),
    nb_row, nb_col, dq (None where the levels are not de-quantised, or (scale, sqrt2 table, dq_neg, dq_shift)), sink
    ((first plane, mode, second mode or None, STORE, chroma scale on); the second plane of a joint block is the other chroma plane)"""
    kind = c["kind"] & 0x3f
    raster, bd = (c["kind"] & capi.TB_FLAG_RASTER) != 0, (c["kind"] & TB_FLAG_BDPCM) != 0
    one_d = (kind == capi.TB_TR) & ((c["log2_w"] == 0) | (c["log2_h"] == 0))
    k = np.where(bd, np.where(c["tr_h"] == 0, K_BDPCM_H, K_BDPCM_V), np.where(one_d, K_1D, np.where(kind == capi.TB_TS, K_TS,
                 np.where(kind == capi.TB_TS_RAW, K_TS_RAW, np.where(kind == capi.TB_DC, np.where(raster, K_RASTER_DC, K_DC),
                          np.where(raster, K_RASTER_TR, K_TR))))))
    nb_row, nb_col = extent(c)
    lf, dq, sink = [], [], []
    for i in range(len(c)):
        f, lw, lh = int(c["lfnst"][i]), int(c["log2_w"][i]), int(c["log2_h"][i])
        lf.append(((f >> 1) & 3, (f >> 3) & 1, (f >> 4) & 1, lfnst_size_class(lw, lh)) if f & 1 else None)
        ts = int(k[i]) in (K_TS, K_TS_RAW, K_BDPCM_H, K_BDPCM_V)
        if int(kind[i]) == capi.TB_TS_RAW:
            dq.append(None)
        else:
            table = 0 if ts else (lw + lh) & 1
            assert int(c["dq_scale"][i]) in IQ_SCALE[table], "a scale that is not in the table of the block's parity"
            dq.append((int(c["dq_scale"][i]), table, int(c["dq_neg"][i]), int(c["dq_shift"][i])))
        m, two = int(c["res_mode"][i]), int(c["plane2"][i]) != 0xff
        scaled = bool(m & capi.RES_SCALE) and int(c["c_scale"][i]) != 1 << 11
        sink.append((int(c["plane"][i]), m & 7, int(c["res_mode2"][i]) & 7 if two else None, bool(m & RES_STORE), scaled))
    return dict(shape=list(zip(c["log2_w"].tolist(), c["log2_h"].tolist())), tr=list(zip(c["tr_v"].tolist(), c["tr_h"].tolist())),
                kind=k, lfnst=lf, nb_row=nb_row, nb_col=nb_col, dq=dq, sink=sink, luma=c["plane"] == 0)


def derive_dq(kind, qp, l2s):
    """ovvc_record.c derive_dq: kind 0 regular, 1 dependent quantisation, 2 transform skip -> label()'s dq tuple"""
    if kind == 2:
        shift, table, idx = 6 - qp // 6, 0, qp % 6
    elif kind == 1:
        shift, table, idx = 2 - (qp + 1) // 6 + (l2s >> 1) + (l2s & 1), l2s & 1, (qp + 1) % 6
    else:
        shift, table, idx = 1 - qp // 6 + (l2s >> 1) + (l2s & 1), l2s & 1, qp % 6
    return IQ_SCALE[table][idx], table, int(shift < 0), abs(shift)


def pairs_of(shape):
    """the (tr_v, tr_h) a luma transform block of `shape` can carry: DCT-II / DCT-II, with no side above 32 the four explicit MTS
    pairs, and with a side of at most 16 the implicit pair (DST-VII along the sides of at most 16, DCT-II along the others)"""
    lw, lh = shape
    out = {(capi.DCT_II, capi.DCT_II)}
    if max(lw, lh) <= 5:
        out |= {(v, h) for v in (capi.DST_VII, capi.DCT_VIII) for h in (capi.DST_VII, capi.DCT_VIII)}
    if min(lw, lh) <= 4:
        out.add((capi.DST_VII if lh <= 4 else capi.DCT_II, capi.DST_VII if lw <= 4 else capi.DCT_II))
    return out


def tr_cells_that_exist():
    """(body, shape, (tr_v, tr_h)) of plain luma transform blocks: the four-wave body takes every shape (route "itx"), the specialised
    bodies their 13, the tiny bodies their 4"""
    out = set()
    for s in LUMA_SHAPES:
        for p in pairs_of(s):
            out.add((FOUR, s, p))
            if s in SPEC_SHAPES:
                out.add((SPEC, s, p))
            if s in TINY_SHAPES:
                out.add((TINY, s, p))
    return out


def lfnst_cells_that_exist():
    """(set, index, transposed, size class): set 0 (planar, DC) is never transposed"""
    return {(s, i, t, z) for s in range(4) for i in (0, 1) for t in (0, 1) for z in ("4x4", "4xN", "8x8", "larger") if not (s == 0 and t)}


def extent_cells_that_exist():
    """(shape, nb_row, nb_col) of the one-wave shapes: every multiple of 4 up to the width / the height"""
    return {(s, r, q) for s in ONE_WAVE_SHAPES for r in range(4, (1 << s[0]) + 1, 4) for q in range(4, (1 << s[1]) + 1, 4)}


def dq_cells_that_exist():
    """every class the QPs 0..75 give a block of an even and of an odd log2 sum (4x4, 8x4, 16x16, 32x16: the enumerated shapes), with
    and without dependent quantisation, and a transform-skip block from QP 16"""
    out = {derive_dq(k, qp, l2s) for k in (0, 1) for qp in range(76) for l2s in (4, 5, 8, 9)}
    return out | {derive_dq(2, qp, 4) for qp in range(16, 76)}


def sink_cells_that_exist():
    """label()'s sink tuples the recorder can emit without STORE: the luma add, the Cb and the Cr add without and with a scale, and per
    ict_type the three joint forms (ovvc_record.c ict_mode: first plane mode 0 (+ scale); Cb first with the second plane's k = 1
    (cbf 3) or k = 2 (cbf 2), Cr first with k = 2 (cbf 1))"""
    A, S, AH, SH = capi.RES_ADD, capi.RES_SUB, capi.RES_ADD_HALF, capi.RES_SUB_HALF
    out = {(0, A, None, False, False)}
    for ict in range(4):
        sc = capi.RES_SCALE if ict & 1 else 0
        full, half = ((A, AH) if ict < 2 else (S, SH))
        for scaled in ((False, True) if sc else (False,)):
            for plane in (1, 2):
                out.add((plane, A | sc, None, False, scaled))
            out |= {(1, A | sc, full | sc, False, scaled), (1, A | sc, half | sc, False, scaled), (2, A | sc, half | sc, False, scaled)}
    return out


def load(names):
    """the commands of the fixtures `names` in recording order, with the restatement of the split asserted against the recorder's own on
    every file -> (commands, {name: (first command, cases' command counts)})"""
    import golden_cases
    out, where, n0 = [], {}, 0
    for n in names:
        _, rec, n_cmds, _, _ = golden_cases.itx_cases_rec(n)
        cmds = rec.tb_cmds().copy()
        order, counts = split_order(cmds)
        split, rec_counts = rec.tb_cmds_split()
        assert counts == rec_counts and split.tobytes() == cmds[order].tobytes(), f"{n}: the census restates another split than the recorder's"
        out.append(cmds)
        where[n] = (n0, n_cmds)
        n0 += len(cmds)
    return np.concatenate(out), where


def oracle_blocks(pred, cmd, coefs):
    """the oracle's reconstruction of ONE command (moved to its band's first rows) on a copy of the 128x128 picture pred = (y, cb, cr)
    -> the block of every plane it writes"""
    import oracle_lib
    c = np.array([cmd], dtype=capi.TB_CMD_DTYPE)
    c["y"] %= 128 if c["plane"][0] == 0 else 64
    pic = oracle_lib.HostPic(128, 128, pred[0].copy(), pred[1].copy(), pred[2].copy())
    oracle_lib.itx(pic, c, coefs)
    x, y, w, h = int(c["x"][0]), int(c["y"][0]), 1 << int(c["log2_w"][0]), 1 << int(c["log2_h"][0])
    planes = [int(c["plane"][0])] + ([int(c["plane2"][0])] if c["plane2"][0] != 0xff else [])
    return [pic.planes()[p][y:y + h, x:x + w].copy() for p in planes]


def changes(pred, cmd, coefs, **fields):
    """does the command with `fields` replaced reconstruct another block than the command as it is?"""
    edited = cmd.copy()
    for k, v in fields.items():
        edited[k] = v
    return any(not np.array_equal(a, b) for a, b in zip(oracle_blocks(pred, cmd, coefs), oracle_blocks(pred, edited, coefs)))


def reach(cmds, routes=ROUTES):
    """-> dict of sets over the commands on the given routes: tr (body, shape, pair) of plain luma transform blocks, lfnst cells, lfnst_body
    (body, cell), extent (body, shape, nb_row, nb_col) of plain luma transform blocks, dq, kind_body (body, kind name, luma?), sink, and
    body_cells: everything a body ran, (body, shape, pair, kind, lfnst cell, nb_row, nb_col)"""
    lb = label(cmds)
    out = dict(tr=set(), lfnst=set(), lfnst_body=set(), extent=set(), dq=set(), kind_body=set(), sink=set(), body_cells=set())
    out["dq"] = {d for d in lb["dq"] if d is not None}
    out["sink"] = set(lb["sink"])
    out["lfnst"] = {f for f in lb["lfnst"] if f is not None}
    for route in routes:
        b = body(cmds, route)
        for i in range(len(cmds)):
            bi, k = int(b[i]), int(lb["kind"][i])
            out["kind_body"].add((bi, KIND_NAMES[k], bool(lb["luma"][i])))
            out["body_cells"].add((bi, lb["shape"][i], lb["tr"][i], k, lb["lfnst"][i], int(lb["nb_row"][i]), int(lb["nb_col"][i])))
            if lb["lfnst"][i] is not None:
                out["lfnst_body"].add((bi, lb["lfnst"][i]))
            elif k == K_TR and lb["luma"][i]:
                out["tr"].add((bi, lb["shape"][i], lb["tr"][i]))
                out["extent"].add((bi, lb["shape"][i], int(lb["nb_row"][i]), int(lb["nb_col"][i])))
    return out
