"""Test infrastructure: random affine coding units for the reference-picture-resampling tests (6-parameter motion fields per
list, as the affine drivers leave them in the motion context)."""
import random

import numpy as np

SHAPES = [(3, 3), (4, 3), (3, 4), (4, 4), (5, 3), (3, 5), (5, 5), (6, 6), (6, 4), (4, 6), (5, 4), (6, 3)]


def motion_field(rnd, nsx, nsy, span, integer=False):
    bx, by = rnd.randrange(-span, span), rnd.randrange(-span, span)
    ax, ay, cx, cy = (rnd.randrange(-24, 25) for _ in range(4))
    if integer:
        ax = ay = cx = cy = 0
        bx &= ~15
        by &= ~15
    m = np.zeros((nsy, nsx, 2), dtype=np.int32)
    for j in range(nsy):
        for i in range(nsx):
            m[j, i] = (bx + ((ax * i + cx * j) >> 1), by + ((ay * i + cy * j) >> 1))
    return m


def random_affine_cus(pic_w, pic_h, n_slots, n, seed, far=False, cell=64, cells=None):
    """Non-overlapping affine CUs, one per `cell` x `cell` grid cell (cells: the cells to use, default all, shuffled)."""
    rnd = random.Random(seed)
    if cells is None:
        cells = [(x, y) for y in range(0, pic_h - cell + 1, cell) for x in range(0, pic_w - cell + 1, cell)]
        rnd.shuffle(cells)
    cus = []
    for k, (cx, cy) in enumerate(cells[:n]):
        lw, lh = rnd.choice([s for s in SHAPES if (1 << s[0]) <= cell and (1 << s[1]) <= cell])
        w, h = 1 << lw, 1 << lh
        x0 = cx + rnd.randrange(0, cell - w + 1, 8)
        y0 = cy + rnd.randrange(0, cell - h + 1, 8)
        d = rnd.choice([1, 2, 3, 3, 3])
        r0, r1 = rnd.randrange(n_slots), rnd.randrange(n_slots)
        span = 40000 if far and k % 2 == 0 else 400
        m0 = motion_field(rnd, w >> 2, h >> 2, span, k % 7 == 2)
        m1 = motion_field(rnd, w >> 2, h >> 2, span, k % 7 == 2)
        prof = 0 if k % 3 == 0 else (rnd.randrange(1, 4) if d == 3 else d)
        ident = d == 3 and k % 9 == 4
        if ident:
            m1, prof = m0.copy(), 0
        cus.append(dict(x0=x0, y0=y0, log2_w=lw, log2_h=lh, inter_dir=d, ref0=r0, ref1=r1, mv0=m0, mv1=m1,
                        bcw_idx_plus1=rnd.choice([0, 0, 1, 2, 4, 5]), prof_dir=prof, poc0=r0 if ident else 10 + r0,
                        poc1=r1 if ident else 20 + r1, lmcs=int(rnd.random() < 0.3),
                        dmv_scale=np.array([[rnd.randrange(-31, 32) for _ in range(16)] for _ in range(4)], dtype=np.int16)))
    return cus


def reads_scaled(cu, scales) -> bool:
    d = cu["inter_dir"] & 3
    if d != 3 and d & 2:
        d = 2
    return any((cu["ref1"] if l else cu["ref0"]) in scales for l in (0, 1) if d & (1 << l))
