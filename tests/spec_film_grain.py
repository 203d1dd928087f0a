"""numpy restatement of the reference's film grain synthesis (fg_grain_apply_pic, pp_film_grain.c:814-978, as pp_process_frame calls
it: no IDR offset, edge smoothing on, 10 bit, 4:2:0), vectorised over the 8x8 blocks of a plane.  The grain database and the seed
table come from the fixture tests/golden/film_grain/fg_db.ovg, which holds what the reference built.

Where the reference is undefined (include/ovvc_hip.h, "Film grain synthesis") this follows the back-end: only blocks inside the plane
exist, an entry with scale 0 gives grain 0 whatever its cut-offs, a cancelled SEI copies the picture."""
import functools
import numpy as np

import golden_io

N_SEI = 133
_LO, _HI, _VAL = 13, 37, 61                 # offsets of lower[3][8], upper[3][8], value[3][8][3] in the flat form
COLOUR_OFFSET = (0, 85, 170)


@functools.lru_cache(maxsize=None)
def tables():
    t = golden_io.load("film_grain/fg_db.ovg")
    return t["db"].astype(np.int32), t["seed"]


def parse(flat):
    """the fixture's flat SEI (i32[133]) -> dict"""
    f = np.asarray(flat, dtype=np.int64)
    assert f.shape == (N_SEI,)
    return {"cancel": int(f[0]), "model_id": int(f[1]), "blending_mode": int(f[2]), "log2_scale": int(f[3]),
            "present": f[4:7].copy(), "num_intervals": f[7:10].copy(), "num_model_values": f[10:13].copy(),
            "lower": f[_LO:_HI].reshape(3, 8).copy(), "upper": f[_HI:_VAL].reshape(3, 8).copy(), "value": f[_VAL:].reshape(3, 8, 3).copy()}


def flatten(s):
    return np.concatenate([[s["cancel"], s["model_id"], s["blending_mode"], s["log2_scale"]], s["present"], s["num_intervals"],
                           s["num_model_values"], s["lower"].ravel(), s["upper"].ravel(), s["value"].ravel()]).astype(np.int32)


def make_sei(log2_scale=2, comps=((8, 3, 200, 8, 8), None, None), cancel=0, model_id=0, blending_mode=0):
    """comps: per component None (no model) or (intervals tiling 0..255, model values, scale, h, v)"""
    s = parse(np.zeros(N_SEI, np.int32))
    s.update(cancel=cancel, model_id=model_id, blending_mode=blending_mode, log2_scale=log2_scale)
    for c, k in enumerate(comps):
        if k is None:
            continue
        n, nv, scale, h, v = k
        s["present"][c], s["num_intervals"][c], s["num_model_values"][c] = 1, n, nv
        s["value"][c, :, 1:] = 8
        for i in range(n):
            s["lower"][c, i], s["upper"][c, i] = 256 * i // n, 256 * (i + 1) // n - 1
            s["value"][c, i] = (max(scale - 7 * i, 1), 2 + (h - 2 + i) % 13, 2 + (v - 2 + 2 * i) % 13)
    return s


def derive(sei):
    """one call's model derivation (fg_compute_model_values, :768-807) -> (present[3], table[3][256][4] of valid / scale / h / v with
    h, v = cut-off - 2, the fields after the call).  The cut-offs of a scale-0 entry are stored as 0, 0."""
    a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sei.items()}
    table = np.zeros((3, 256, 4), np.int64)
    present = np.zeros(3, np.int64)
    for c in range(3):
        if not a["present"][c]:
            continue
        interval = np.full(256, -1)
        for i in range(8):
            interval[a["lower"][c, i]:a["upper"][c, i] + 1] = i      # empty when lower > upper
            v = a["value"][c, i]
            if a["num_model_values"][c] == 1:
                v[1] = v[2] = 8
            elif a["num_model_values"][c] == 2:
                v[2] = v[1]
            if c > 0:
                v[0] >>= 1
                v[1:] = np.clip(v[1:] << 1, 2, 14)
        if a["cancel"]:
            continue
        present[c] = 1
        for avg in range(256):
            if interval[avg] >= 0:
                s, h, v = a["value"][c, interval[avg]]
                table[c, avg] = (1, s, h - 2, v - 2) if s else (1, 0, 0, 0)
    return present, table, a


def packed_table(table):
    """the table as ovhip_fg_model.entry holds it"""
    t = table.astype(np.int64)
    return np.where(t[..., 0] != 0, (1 << 24) | (t[..., 1] & 0xFFFF) | (t[..., 2] << 16) | (t[..., 3] << 20), 0).astype(np.uint32)


def prng(x):
    return ((x << 1) + (1 ^ ((x >> 2) & 1) ^ ((x >> 30) & 1))) & 0xFFFFFFFF


def block_seeds(start, n):
    out = np.empty(n, np.int64)
    x = int(start)
    for i in range(n):
        out[i] = x
        x = prng(x)
    return out


def grain_plane(src, table, log2_scale, start_seed):
    """one component with a model: src [h][w] u16 -> [h][w] u16"""
    db, _ = tables()
    h, w = src.shape
    nbx, nby = (w + 7) // 8, (h + 7) // 8
    pad = np.zeros((nby * 8, nbx * 8), np.int64)
    pad[:h, :w] = src
    sums = pad.reshape(nby, 8, nbx, 8).sum(axis=(1, 3))
    count = np.outer(np.minimum(8, h - 8 * np.arange(nby)), np.minimum(8, w - 8 * np.arange(nbx)))
    avg = np.minimum((sums // count) >> 2, 255)
    n16x, n16y = (w + 15) // 16, (h + 15) // 16
    seed16 = block_seeds(start_seed, n16x * n16y).reshape(n16y, n16x)
    seed = seed16[np.arange(nby)[:, None] // 2, np.arange(nbx)[None, :] // 2]
    k_off = (((seed >> 16) % 52) & ~3) + (np.arange(nbx)[None, :] & 1) * 8
    l_off = (((seed & 0xFFFF) % 56) & ~7) + (np.arange(nby)[:, None] & 1) * 8
    e = table[avg]                                             # [nby][nbx][4]
    scale = np.where(seed & 1, -e[..., 1], e[..., 1]) * e[..., 0]
    r = np.arange(8)
    pat = db[e[..., 2][:, :, None, None], e[..., 3][:, :, None, None], l_off[:, :, None, None] + r[None, None, :, None],
             k_off[:, :, None, None] + r[None, None, None, :]]          # [nby][nbx][8 rows][8 columns]
    g = (scale[:, :, None, None] * pat) >> (log2_scale + 6)
    g = g.transpose(0, 2, 1, 3).reshape(nby * 8, nbx * 8)[:h, :w]
    edges = np.arange(8, w, 8)
    if len(edges):
        old = g.copy()
        g[:, edges] = (old[:, edges - 1] + 2 * old[:, edges] + old[:, edges + 1]) >> 2
        g[:, edges - 1] = (old[:, edges - 2] + 2 * old[:, edges - 1] + old[:, edges]) >> 2
    return np.clip(src.astype(np.int64) + (g << 2), 0, 1023).astype(np.uint16)


def start_seed(poc, c, idr_offset=0):
    _, seed_lut = tables()
    return int(seed_lut[(poc + (idr_offset << 5) + COLOUR_OFFSET[c]) % 256])


def apply(planes, sei, poc):
    """planes: (y, cb, cr) u16 arrays; sei: parse()'s dict.  -> (grained planes, the fields after the call)"""
    present, table, after = derive(sei)
    out = tuple(grain_plane(p, table[c], sei["log2_scale"], start_seed(poc, c)) if present[c] else p.copy() for c, p in enumerate(planes))
    return out, after
