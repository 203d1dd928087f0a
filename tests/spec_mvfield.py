"""Numpy restatement of the motion field output (include/ovvc_hip.h, "Motion field output on the device"), written from the header's
text: unit lists in, the dense field on the 4x4 luma grid out.  It does not call the library.  Every implementation (ovhip_mvfield_host,
k_mvfield) is compared with it byte for byte.  Also here: the directed unit lists the CPU and the GPU tests share."""
import numpy as np

I32, F32, F16 = 0, 1, 2                                       # dtype
PLANAR, CELLS = 0, 1                                          # layout
UNIT, REFINED = 0, 1                                          # vectors
INTER, AFFINE, GPM, DMVR, BDOF, BCW, PROF = 1, 2, 4, 8, 16, 32, 64
EMPTY = 0x0000FFFF
FILL = 0xA5
NP_DTYPE = {I32: np.int32, F32: np.float32, F16: np.float16}
ELEM = {I32: 4, F32: 4, F16: 2}
DTYPES, LAYOUTS, VECTORS = (I32, F32, F16), (PLANAR, CELLS), (UNIT, REFINED)

# the unit structs of the header, field by field
MC_UNIT = np.dtype([("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("dir", "u1"), ("flags", "u1"), ("ref0", "u1"), ("ref1", "u1"),
                    ("w0", "i1"), ("w1", "i1"), ("mv0x", "<i4"), ("mv0y", "<i4"), ("mv1x", "<i4"), ("mv1y", "<i4"), ("aux", "<u4")])
AFF_UNIT = np.dtype([("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("dir", "u1"), ("flags", "u1"), ("ref0", "u1"), ("ref1", "u1"),
                     ("w0", "i1"), ("w1", "i1"), ("prof_dir", "u1"), ("ident_c", "u1"), ("ident_l", "<u2"), ("side_off", "<u4"),
                     ("prof_off", "<u4"), ("pad", "<u4", 2)])
RPR_SIDE = np.dtype([("pos_x", "<i4"), ("pos_y", "<i4"), ("cpos_x", "<i4"), ("cpos_y", "<i4"), ("step_x", "<u2"), ("step_y", "<u2"),
                     ("filt", "u1"), ("filt_c", "u1"), ("ref", "u1"), ("pad", "u1")])
RPR_UNIT = np.dtype([("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("ox", "u1"), ("oy", "u1"), ("dir", "u1"), ("flags", "u1"),
                     ("w0", "i1"), ("w1", "i1"), ("aux", "<u4"), ("s", RPR_SIDE, 2)])
AFFR_LIST = np.dtype([("step_x", "<u2"), ("step_y", "<u2"), ("filt", "u1"), ("filt_c", "u1"), ("ref", "u1"), ("pad", "u1")])
AFFR_UNIT = np.dtype([("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("dir", "u1"), ("flags", "u1"), ("w0", "i1"), ("w1", "i1"),
                      ("prof_dir", "u1"), ("ident_c", "u1"), ("ident_l", "<u2"), ("pad0", "<u2"), ("side_off", "<u4"), ("prof_off", "<u4"),
                      ("s", AFFR_LIST, 2), ("pad", "<u4", 2)])
assert (MC_UNIT.itemsize, AFF_UNIT.itemsize, RPR_UNIT.itemsize, AFFR_UNIT.itemsize) == (32, 32, 64, 48)

MC_NO_LUMA, MC_BDOF, MC_DMVR, MC_GPM = 4, 32, 64, 128         # ovhip_mc_unit.flags
AFF_PROF = 1                                                  # ovhip_aff_unit.flags
RPR_S0, RPR_S1, RPR_NO_LUMA, RPR_GPM = 1, 2, 4, 128           # ovhip_rpr_unit.flags
AFFR_S0, AFFR_S1, AFFR_PROF, AFFR_NO_CHROMA = 1, 2, 4, 8      # ovhip_aff_rpr_unit.flags


def grid(w, h):
    return (w + 3) >> 2, (h + 3) >> 2


def sizes(w, h, dtype):
    """(bytes of the vectors, bytes of the info)"""
    w4, h4 = grid(w, h)
    return 4 * w4 * h4 * ELEM[dtype], 4 * w4 * h4


def lists(mc=None, mcx=None, aff=None, rpr=None, affr=None, side=None, refined=None):
    """the five lists (structured arrays of the dtypes above, or None), the side arena and the refined array as one dict"""
    def arr(a, dt):
        return np.zeros(0, dt) if a is None or not len(a) else np.ascontiguousarray(a).view(dt).reshape(-1)
    return dict(mc=arr(mc, MC_UNIT), mcx=arr(mcx, MC_UNIT), aff=arr(aff, AFF_UNIT), rpr=arr(rpr, RPR_UNIT), affr=arr(affr, AFFR_UNIT),
                side=np.zeros(0, np.int32) if side is None else np.ascontiguousarray(side, dtype=np.int32),
                refined=None if refined is None else np.ascontiguousarray(refined, dtype=np.int32).reshape(-1, 4))


def _info(d, ref0, ref1, kind, gpm, w0, w1, scaled):
    if gpm:
        kind |= GPM
    elif d == 3 and (w0 != 4 or w1 != 4):
        kind |= BCW
    return (ref0 if d & 1 else 0xFF) | (ref1 if d & 2 else 0xFF) << 8 | kind << 16 | (scaled & d) << 24


def dense(w, h, L, vectors=UNIT):
    """-> (V int64 [4][H4][W4] in 1/16 sample, info uint32 [H4][W4], covered bool [H4][W4]); asserts that every unit that carries luma
    is 4-aligned and that no cell is covered twice"""
    w4, h4 = grid(w, h)
    V = np.zeros((4, h4, w4), np.int64)
    info = np.full((h4, w4), EMPTY, np.uint32)
    covered = np.zeros((h4, w4), bool)

    def cover(u, word, vec_of_cell):
        x, y, uw, uh = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])
        assert x % 4 == 0 and y % 4 == 0 and uw % 4 == 0 and uh % 4 == 0 and uw and uh, (x, y, uw, uh)
        for cy in range(y // 4, min((y + uh) // 4, h4)):
            for cx in range(x // 4, min((x + uw) // 4, w4)):
                assert not covered[cy, cx], f"cell ({cx}, {cy}) is covered twice"
                covered[cy, cx] = True
                info[cy, cx] = word
                V[:, cy, cx] = vec_of_cell((cy - y // 4) * (uw // 4) + (cx - x // 4))

    def masked(v, use):
        return [v[0] if use & 1 else 0, v[1] if use & 1 else 0, v[2] if use & 2 else 0, v[3] if use & 2 else 0]

    for name in ("mc", "mcx"):
        for i, u in enumerate(L[name]):
            fl, d = int(u["flags"]), int(u["dir"])
            if name == "mc" and fl & MC_NO_LUMA:
                continue
            kind = INTER
            if name == "mcx":
                kind |= (DMVR if fl & MC_DMVR else 0) | (BDOF if fl & MC_BDOF else 0)
            v = [int(u["mv0x"]), int(u["mv0y"]), int(u["mv1x"]), int(u["mv1y"])]
            if name == "mcx" and vectors == REFINED and fl & MC_DMVR:
                v = [int(q) for q in L["refined"][i]]
            v = masked(v, d)
            cover(u, _info(d, int(u["ref0"]), int(u["ref1"]), kind, fl & MC_GPM, int(u["w0"]), int(u["w1"]), 0), lambda k, v=v: v)
    side = L["side"]
    for u in L["aff"]:
        d, off = int(u["dir"]), int(u["side_off"])
        kind = INTER | AFFINE | (PROF if int(u["flags"]) & AFF_PROF else 0)
        cover(u, _info(d, int(u["ref0"]), int(u["ref1"]), kind, 0, int(u["w0"]), int(u["w1"]), 0),
              lambda k, d=d, off=off: masked([int(q) for q in side[off + 4 * k:off + 4 * k + 4]], d))
    for u in L["rpr"]:
        fl, d = int(u["flags"]), int(u["dir"])
        if fl & RPR_NO_LUMA:
            continue
        scaled = fl & (RPR_S0 | RPR_S1)
        v = masked([int(u["s"][0]["pos_x"]), int(u["s"][0]["pos_y"]), int(u["s"][1]["pos_x"]), int(u["s"][1]["pos_y"])], d & ~scaled)
        cover(u, _info(d, int(u["s"][0]["ref"]), int(u["s"][1]["ref"]), INTER, fl & RPR_GPM, int(u["w0"]), int(u["w1"]), scaled), lambda k, v=v: v)
    for u in L["affr"]:
        fl, d, off = int(u["flags"]), int(u["dir"]), int(u["side_off"])
        scaled = fl & (AFFR_S0 | AFFR_S1)
        kind = INTER | AFFINE | (PROF if fl & AFFR_PROF else 0)
        cover(u, _info(d, int(u["s"][0]["ref"]), int(u["s"][1]["ref"]), kind, 0, int(u["w0"]), int(u["w1"]), scaled),
              lambda k, use=d & ~scaled, off=off: masked([int(q) for q in side[off + 4 * k:off + 4 * k + 4]], use))
    return V, info, covered


def field(w, h, L, dtype=I32, layout=PLANAR, vectors=UNIT):
    """-> (the vectors as an array of the dtype, [4][H4][W4] or [H4][W4][4]; the info, uint32 [H4][W4])"""
    V, info, _ = dense(w, h, L, vectors)
    assert np.abs(V).max(initial=0) < 1 << 24
    if dtype == I32:
        out = V.astype(np.int32)
    else:
        out = V.astype(np.float32) * np.float32(0.0625)       # exact
        if dtype == F16:
            out = out.astype(np.float16)                      # round to nearest even
    if layout == CELLS:
        out = np.ascontiguousarray(out.transpose(1, 2, 0))
    return out, info


# ---- the directed lists at 72 x 40 (W4 = 18: planar rows are 72 bytes and start on 8-byte boundaries) ----
DIRECTED_SIZE = (72, 40)
BIG, ODD = (1 << 17) - 1, 2049                                # 2049 / 16 = 128.0625 needs 12 bits: F16 rounds it, F32 does not


def _mc(x, y, w, h, d, flags=0, ref=(0, 1), wts=(4, 4), mv=(0, 0, 0, 0)):
    u = np.zeros(1, MC_UNIT)
    u["x"], u["y"], u["w"], u["h"], u["dir"], u["flags"] = x, y, w, h, d, flags
    u["ref0"], u["ref1"], u["w0"], u["w1"] = ref[0], ref[1], wts[0], wts[1]
    u["mv0x"], u["mv0y"], u["mv1x"], u["mv1y"] = mv
    return u


def _aff(x, y, w, h, d, flags, side_off, ref=(0, 1), wts=(4, 4)):
    u = np.zeros(1, AFF_UNIT)
    u["x"], u["y"], u["w"], u["h"], u["dir"], u["flags"], u["side_off"] = x, y, w, h, d, flags, side_off
    u["ref0"], u["ref1"], u["w0"], u["w1"], u["ident_l"], u["ident_c"] = ref[0], ref[1], wts[0], wts[1], 0x5A5A, 0x5
    return u


def _rpr(x, y, w, h, d, flags, pos, ref=(2, 3), wts=(4, 4)):
    u = np.zeros(1, RPR_UNIT)
    u["x"], u["y"], u["w"], u["h"], u["dir"], u["flags"], u["w0"], u["w1"] = x, y, w, h, d, flags, wts[0], wts[1]
    for l in (0, 1):
        u["s"][0][l]["pos_x"], u["s"][0][l]["pos_y"], u["s"][0][l]["ref"] = pos[2 * l], pos[2 * l + 1], ref[l]
        u["s"][0][l]["step_x"] = u["s"][0][l]["step_y"] = 16384 if flags & (1 << l) else 0
    return u


def _affr(x, y, w, h, d, flags, side_off, ref=(4, 5), wts=(4, 4)):
    u = np.zeros(1, AFFR_UNIT)
    u["x"], u["y"], u["w"], u["h"], u["dir"], u["flags"], u["side_off"], u["w0"], u["w1"] = x, y, w, h, d, flags, side_off, wts[0], wts[1]
    for l in (0, 1):
        u["s"][0][l]["ref"] = ref[l]
    return u


def directed_lists():
    """every rule of the definition at least once; no two units that carry luma overlap"""
    mc = np.concatenate([
        _mc(0, 0, 8, 8, 2, ref=(0, 1), mv=(777, -777, ODD, -ODD)),           # uni on list 1 only: ref0 is 0xFF, mv0 is 0
        _mc(8, 0, 4, 8, 1, ref=(1, 0), mv=(BIG, -BIG, 55, 66)),              # 4x8
        _mc(12, 0, 8, 4, 3, mv=(-BIG, BIG, -ODD, ODD)),                      # 8x4
        _mc(12, 4, 4, 4, 3, wts=(3, 5), mv=(1, -1, 16, -16)),                # 4x4, BCW
        _mc(20, 0, 8, 8, 3, flags=MC_GPM, wts=(3, 5), mv=(40, 41, 42, 43)),  # GPM: never BCW
        _mc(56, 24, 16, 16, 3, ref=(7, 9), mv=(-3, 4, -5, 6)),               # 16x16 in the bottom-right corner
        _mc(64, 8, 16, 8, 1, mv=(100, 200, 0, 0)),                           # reaches past the grid to the right: clipped
        _mc(32, 32, 8, 16, 3, mv=(9, 8, 7, 6)),                              # reaches past the grid at the bottom: clipped
        _mc(0, 0, 8, 8, 3, flags=MC_NO_LUMA, mv=(1, 2, 3, 4)),               # chroma only: skipped
        _mc(44, 8, 4, 4, 1, flags=MC_DMVR | MC_BDOF, mv=(5, 5, 0, 0)),       # the refined units' flags mean nothing in the mc list
    ])
    mcx = np.concatenate([
        _mc(28, 0, 16, 16, 3, flags=MC_DMVR | MC_BDOF, mv=(160, -160, -160, 160)),
        _mc(44, 0, 8, 8, 3, flags=MC_BDOF, mv=(33, 34, 35, 36)),             # no DMVR: never reads the refined array
        _mc(52, 0, 8, 8, 3, flags=MC_DMVR, mv=(ODD, 0, 0, -ODD)),
    ])
    refined = np.array([[172, -148, -172, 148], [-9999, 9999, -9999, 9999], [ODD + 32, -16, -32, -ODD + 16]], np.int32)
    rs = np.random.RandomState(5)
    side = rs.randint(-BIG, BIG + 1, size=240).astype(np.int32)
    side[0:4] = (BIG, -BIG, ODD, -ODD)
    aff = np.concatenate([
        _aff(0, 8, 16, 16, 3, AFF_PROF, 0, wts=(5, 3)),                      # 16 sub-blocks, PROF, BCW
        _aff(16, 16, 16, 8, 1, 0, 96),                                       # uni on list 0: the side words of list 1 are not exported
    ])
    rpr = np.concatenate([
        _rpr(0, 24, 8, 8, 1, RPR_S0, (1 << 20, -(1 << 20), 11, 12)),         # scaled on list 0
        _rpr(8, 24, 8, 8, 3, RPR_S1, (BIG, -ODD, 1 << 21, 1 << 22)),         # scaled on list 1: list 0 exports its vector
        _rpr(16, 24, 8, 8, 3, RPR_S0 | RPR_S1, (1 << 20, 2, 3, 1 << 20), wts=(3, 5)),        # scaled on both, BCW
        _rpr(24, 24, 8, 8, 2, RPR_S0, (1 << 20, 1 << 20, -ODD, BIG)),        # the scaled list is not used: no scaled bit
        _rpr(24, 24, 8, 8, 3, RPR_NO_LUMA | RPR_S0, (1, 2, 3, 4)),           # chroma only: skipped
        _rpr(32, 24, 8, 8, 3, RPR_GPM | RPR_S0, (1 << 19, 5, -6, 7)),
    ])
    affr = np.concatenate([
        _affr(0, 32, 16, 8, 3, AFFR_S1 | AFFR_PROF, 160),                    # 16x8, one scaled list
        _affr(20, 32, 4, 4, 1, AFFR_S0 | AFFR_NO_CHROMA, 205),               # a lone 4x4 (its side words are only 4-byte aligned)
        _affr(24, 32, 8, 8, 3, 0, 212, wts=(3, 5)),
    ])
    return lists(mc, mcx, aff, rpr, affr, side, refined)


def other_lists():
    """a second, sparser set for the same grid: whatever the directed lists covered and these do not must read EMPTY afterwards"""
    return lists(mc=_mc(4, 4, 16, 8, 3, ref=(2, 2), mv=(-1, -2, -3, -4)), side=np.zeros(4, np.int32))
