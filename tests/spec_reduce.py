"""Reduced-size output restated in numpy with exact integers (include/ovvc_hip.h, "Reduced-size output on the device"): the weights as
dense matrices built from the definition's intervals, sample by sample, the clamped samples' weights added onto the region's edge
sample; V = Wy s Wx^T in int64.  Independent of the closed forms the C twin and the kernel share."""
from math import gcd

import numpy as np

MAX_DIM, MAX_RATIO, MAX_P = 16384, 8, 256

# source -> output, chroma locations to run ("the census" of the issue); every size the smallest that reaches its case
CENSUS = [
    ((104, 56), (52, 28), range(6)),        # 2/1; 2/1: narrower than a 64-column tile, chroma 26 wide
    ((72, 40), (48, 24), range(6)),         # 3/2; 5/3: different p/q per axis, partial weights
    ((96, 48), (32, 16), (0,)),             # 3/1; 3/1
    ((64, 64), (8, 8), range(6)),           # 8/1; 8/1: the ceiling, 9 weights under a shifted footprint
    ((72, 40), (72, 20), (0,)),             # 1/1 on x
    ((72, 40), (36, 40), (0,)),             # 1/1 on y
    ((72, 40), (72, 40), (0,)),             # the identity
    ((100, 52), (52, 28), (0,)),            # 25/13; 13/7: long periods
    ((200, 20), (136, 12), (0,)),           # 25/17; 5/3: more than two column tiles, 6 chroma rows
    ((1024, 1024), (132, 132), (0,)),       # 256/33: the int32 ceiling
]
RATIOS = {((104, 56), (52, 28)): (2, 1, 2, 1), ((72, 40), (48, 24)): (3, 2, 5, 3), ((96, 48), (32, 16)): (3, 1, 3, 1),
          ((64, 64), (8, 8)): (8, 1, 8, 1), ((72, 40), (72, 20)): (1, 1, 2, 1), ((72, 40), (36, 40)): (2, 1, 1, 1),
          ((72, 40), (72, 40)): (1, 1, 1, 1), ((100, 52), (52, 28)): (25, 13, 13, 7), ((200, 20), (136, 12)): (25, 17, 5, 3),
          ((1024, 1024), (132, 132)): (256, 33, 256, 33)}
REFUSED = [((1028, 64), (132, 64)), ((72, 40), (8, 40))]          # p = 257 on x; 9/1 on x
WINDOW_CASE = ((80, 48), (1, 3, 2, 2), (48, 24))                  # region 72x40 at luma (2, 4)


def ab(loc):
    return loc & 1, (1, 1, 0, 0, 2, 2)[loc]


def axis(S, D):
    g = gcd(S, D)
    return S // g, D // g


def sigma(p, q, c):
    """c = a (horizontal) or b (vertical)"""
    return (p - q) * (1 - c)


def weights(Sp, Dp, p, q, sg):
    """W[k, j]: the weight of sample j of the region's Sp in output k of Dp"""
    W = np.zeros((Dp, Sp), np.int64)
    for k in range(Dp):
        A = 4 * p * k - sg
        B = A + 4 * p
        for j in range(A // (4 * q), (B - 1) // (4 * q) + 1):         # (floor division)
            w = min(B, 4 * q * (j + 1)) - max(A, 4 * q * j)
            assert w > 0
            W[k, min(max(j, 0), Sp - 1)] += w
    return W


def plane_V(s, Dw, Dh, px, qx, py, qy, sgx=0, sgy=0):
    s = np.asarray(s, np.int64)
    return weights(s.shape[0], Dh, py, qy, sgy) @ s @ weights(s.shape[1], Dw, px, qx, sgx).T


def round_div(V, n):
    return ((V + n // 2) // n).astype(np.uint16)


def check(w, h, Wd, Hd, window=(0, 0, 0, 0), loc=0):
    """(ok, (px, qx, py, qy)) by the definition's requirements"""
    l, r, a, b = window
    Ws, Hs = w - 2 * (l + r), h - 2 * (a + b)
    if any(v <= 0 or v % 4 or v > MAX_DIM for v in (w, h, Wd, Hd)) or Ws <= 0 or Hs <= 0 or Ws % 4 or Hs % 4 or loc > 5:
        return False, None
    px, qx = axis(Ws, Wd)
    py, qy = axis(Hs, Hd)
    ok = Wd <= Ws and Hd <= Hs and Ws <= MAX_RATIO * Wd and Hs <= MAX_RATIO * Hd and px <= MAX_P and py <= MAX_P
    return ok, (px, qx, py, qy)


def reduce_picture(y, cb, cr, Wd, Hd, window=(0, 0, 0, 0), loc=0):
    """the reduced picture (y, cb, cr) of Wd x Hd"""
    h, w = y.shape
    ok, (px, qx, py, qy) = check(w, h, Wd, Hd, window, loc)
    assert ok
    l, r, a, b = window
    Ws, Hs = w - 2 * (l + r), h - 2 * (a + b)
    n = 16 * px * py
    ca, cb_ = ab(loc)
    sgx, sgy = sigma(px, qx, ca), sigma(py, qy, cb_)
    out = [round_div(plane_V(y[2 * a:2 * a + Hs, 2 * l:2 * l + Ws], Wd, Hd, px, qx, py, qy), n)]
    for c in (cb, cr):
        out.append(round_div(plane_V(c[a:a + Hs // 2, l:l + Ws // 2], Wd // 2, Hd // 2, px, qx, py, qy, sgx, sgy), n))
    return tuple(out)


def random_planes(w, h, seed, top=1024):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, top, s, dtype=np.uint16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def packed(planes, window=(0, 0, 0, 0)):
    """the packed output's samples of a picture under a window in chroma units"""
    l, r, a, b = window
    y, cb, cr = planes
    h, w = y.shape
    return np.concatenate([y[2 * a:h - 2 * b, 2 * l:w - 2 * r].ravel(), cb[a:h // 2 - b, l:w // 2 - r].ravel(), cr[a:h // 2 - b, l:w // 2 - r].ravel()])
