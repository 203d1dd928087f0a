"""TEST INFRASTRUCTURE: directed deblocking cells -- a synthetic picture and synthetic edge lists, built in Python.

One cell = one isolated 4-sample edge segment (2 chroma lines) with the content that drives ONE decision outcome:
(component, direction, lp, lq, bS, QP, offset-pair index, wanted branch).  Nothing is read from the reference; the
expected picture comes from tests/spec_dbf.py, which tests/test_dbf_spec_cpu.py pins to the reference.

Every side of a matrix, lines03, gate, pinned and fill cell is a ramp (pick_slopes): all of p0..p7 and q0..q7 differ.

The vertical chroma cells at ODD unit columns (ux = 8 k + 1) are synthetic: the recorder puts chroma edges on even unit columns
only, and the dense planes cannot even hold an odd one.  They exist to drive the scalar fallback of the list kernel's line load
(a line that is not 8-byte aligned); no caller-visible shape is meant.

Layout (luma 320 x 320).  Vertical edges lie at x = 32 k, horizontal edges at y = 32 m.  A cell owns the samples it may read:
8 on each side of the edge, 4 (2) lines.  Vertical cells stack along their column (different lines never meet); horizontal
cells keep off the columns a vertical cell may WRITE (unit columns 6, 7, 0, 1 of every 8; chroma: all but 3, 4, 5), so the
horizontal pass reads nothing the vertical pass changed and no two segments of one direction share a sample: the result does
not depend on the order of the lists.

`build()` is deterministic.  Every cell carries the label it was built for; test_dbf_spec_cpu.py asserts on the CPU that
spec_dbf gives every cell exactly that label.
"""
from dataclasses import dataclass, field

import numpy as np

import spec_dbf
from openvvc_amd import capi

W = H = 320
LUMA_PAIRS = ((1, 1), (2, 2), (3, 3), (3, 5), (3, 7), (5, 3), (5, 5), (5, 7), (7, 3), (7, 5), (7, 7))
LONG_PAIRS = tuple(p for p in LUMA_PAIRS if max(p) > 3)
# 8 distinct (beta, tc) pairs: both ends of the legal -24..24, mixed signs; index 5 is the pair of the dense-plane route,
# index 4 the negative pair of the single-pair wrapper; NEVER_LIVE: see build()
OFF_BETA = (0, -24, 24, 24, -24, 6, -10, 12)
OFF_TC = (0, 24, -24, 24, -24, -2, 14, -18)
DENSE_IDX, NEG_IDX, NEVER_LIVE = 5, 4, 2
TC_TARGETS = (-5, 0, 17, 18, 65, 66, 80)
BETA_TARGETS = (-5, 0, 15, 16, 63, 64, 80)


@dataclass
class Cell:
    comp: int
    dir: int                      # 0 vertical edge, 1 horizontal edge
    ux: int
    uy: int
    word: int
    off: int
    want: str                     # the kind spec_dbf must report
    ext: tuple = None             # weak luma: (dEp, dEq)
    gate: int = None              # weak luma: lines that pass |delta| < 10 tC
    clip: str = None              # "lo" / "hi": a Clip1() of the weak filter acts
    group: str = ""
    note: dict = field(default_factory=dict)


def luma_word(bs, lp, lq, qp):
    return bs | (lp << 2) | (lq << 5) | (qp << 8)


def chroma_word(bs, large, ctb_b, qp):
    return spec_dbf.C_ON | (spec_dbf.C_BS2 if bs == 2 else 0) | (spec_dbf.C_LARGE if large else 0) | (spec_dbf.C_CTB_B if ctb_b else 0) | (qp << 8)


def lim(qp, bs, off):
    tc, beta, tc_idx, beta_idx = spec_dbf.limits(qp, bs, OFF_TC[off], OFF_BETA[off])
    return tc, beta, tc_idx, beta_idx


# ------------------------------------------------------------------------------------------------------------ content
SLOPES = ((2, 1), (1, 2), (2, 2), (3, 1), (1, 3), (-1, 2), (2, -1), (-2, -1), (1, 1), (-1, -1), (1, -1))


def pick_slopes(want, lp, lq, beta, k, chroma=False):
    """The k-th ramp (slope per sample on the P side, on the Q side) gentle enough for the decision `want` needs.  Each side of a
    cell is a ramp, so that p0..p7 and q0..q7 all differ: a filter or decision tap that reads the neighbouring sample, or two taps
    with their weights swapped, changes the result -- on a flat side any taps with the right sum give the same sample."""
    def sp(l, g):                                        # 8.8.3.6.6 on a linear ramp: |p3 - p0| (+ |p3 - p_l|, halved)
        g = abs(g)
        return 3 * g if l <= 3 else (3 * g + (l - 3) * g + 1) >> 1
    for j in range(2 * len(SLOPES) if chroma else len(SLOPES)):
        gp, gq = SLOPES[(k + j) % len(SLOPES)]
        if chroma and j < len(SLOPES):                   # chroma taps are >> 3 over few samples: steeper first, where beta allows
            gp, gq = 2 * gp, 2 * gq
        if want == "long" and not sp(lp, gp) + sp(lq, gq) < (3 * beta) >> 5:
            continue
        if want == "strong" and not 3 * (abs(gp) + abs(gq)) < beta >> 3:
            continue
        return gp, gq
    return 0, 0


def luma_lines(want, lp, lq, tc, beta, base=400, ext=(True, True), variant="", slopes=(0, 0)):
    """4 lines x 16 samples (index 7 - i = p_i, 8 + i = q_i) that make an (lp, lq) segment take `want`."""
    a = np.zeros((4, 16), np.int64)
    sign = -1 if base > 700 else 1                       # near the top of the range the step goes down
    half = (5 * tc + 1) >> 1
    for l in range(4):
        b = base + sign * 5 * l                          # every line has its own level: mixed-up lines show
        p, q = b + sign * slopes[0] * np.arange(8), b + sign * slopes[1] * np.arange(8)     # index i = p_i / q_i
        if want in ("long", "strong"):
            q += sign * max(half - 1 - l, 0)             # a step just below 2.5 tC (the filter's tC clips act), another on every line
            if want == "strong" and variant == "far6":   # the long decision fails through |p7 - p6 - p5 + p4| alone
                if lp == 7:
                    p[6] -= sign * beta
                elif lq == 7:
                    q[6] -= sign * beta
            elif want == "strong":                       # the long decision must fail: far samples off, near ones a ramp
                if lp > 3:
                    p[4] += sign * beta
                if lq > 3:
                    q[4] += sign * beta
            elif variant in ("far_ramp_p", "far_ramp_q"):    # long, with a steep but straight far part: |p5 - 2 p4 + p3| = 0
                side, n = (p, lp) if variant == "far_ramp_p" else (q, lq)
                side[4:] += sign * (12 if n == 5 else 4) * np.arange(1, 5)
        elif want == "weak":
            q += sign * 3 * tc                           # a step above 2.5 tC: neither strong decision passes
            c = beta // 16 + 1                           # curvature next to the edge: dp0 + dp3 >= 3 beta / 16, d < beta
            if not ext[0]:
                p[1] += sign * c
            if not ext[1]:
                q[1] += sign * c
        elif want == "off":
            p[1] += sign * (beta // 8 + 1)               # noise above beta
            q[1] += sign * (beta // 8 + 1)
        a[l, :8], a[l, 8:] = p[::-1], q
    if variant == "mid_noise":                           # lines 1 and 2 would be `off`: the decision must not look at them
        for l in (1, 2):
            a[l, 6] += sign * (beta // 4 + 8); a[l, 9] += sign * (beta // 4 + 8); a[l, 4] -= sign * 9; a[l, 12] -= sign * 7
    if variant in ("gate1", "gate2"):                    # lines above the 10 tC gate of the weak filter: left untouched
        for l in ((1,) if variant == "gate1" else (1, 2)):
            a[l, 8:] = a[l, 7] + sign * 30 * tc
    assert a.min() >= 0 and a.max() <= 1023, (want, lp, lq, tc, beta, base, int(a.min()), int(a.max()))
    return a


def clip_lines(end):
    """p = 1, q = (0, 8, 8, ...): the weak filter's delta is -2, p0 + delta = -1 -> Clip1 acts; mirrored at the top."""
    a = np.ones((4, 16), np.int64)
    a[:, 8] = 0
    a[:, 9:] = 8
    return a if end == "lo" else 1023 - a


def chroma_lines(want, large, ctb_b, tc, beta, base=500, slopes=(0, 0)):
    """2 lines x 8 samples (3 - i = p_i, 4 + i = q_i)."""
    a = np.zeros((2, 8), np.int64)
    half = (5 * tc + 1) >> 1
    for l in range(2):
        b = base + 6 * l
        a[l, :4] = b + slopes[0] * np.arange(3, -1, -1)
        a[l, 4:] = b + (max(half - 1 - l, 1) if want == "strong" or not large else 3 * tc) + slopes[1] * np.arange(4)
        if not large:
            a[l, 2] += 2; a[l, 5] -= 3                   # the weak filter reads p1 and q1
        if ctb_b:
            a[l, 0] += 90; a[l, 1] -= 70                 # p3, p2: outside a CTU-boundary segment's reach, must be ignored
    return np.clip(a, 0, 1023)


# ------------------------------------------------------------------------------------------------------------ placement
class _Slots:
    """free cell positions, handed out in a fixed order"""

    def __init__(self):
        self.luma = {0: [(8 * k, uy) for uy in range(H // 4) for k in range(1, W // 32)],
                     1: [(ux, 8 * m) for m in range(1, H // 32) for ux in range(W // 4) if ux % 8 in (2, 3, 4, 5)]}
        # chroma vertical edges: every second column sits at an ODD unit position (ux = 8 k + 1): the line is then not
        # 8-byte aligned and load_line_q takes its scalar path
        self.chroma = {c: {0: [(8 * k + (k % 2), uy) for uy in range(H // 4) for k in range(1, W // 32)],
                           1: [(ux, 8 * m) for m in range(1, H // 32) for ux in range(W // 4) if ux % 8 in (3, 4, 5)]} for c in (1, 2)}

    def take(self, comp, d, odd=None):
        pool = self.luma[d] if comp == 0 else self.chroma[comp][d]
        for i, (ux, uy) in enumerate(pool):
            if odd is None or comp == 0 or d == 1 or bool(ux % 2) == odd:
                return pool.pop(i)
        raise RuntimeError("no free cell position")


def _paint(planes, cell, lines):
    comp, d = cell.comp, cell.dir
    unit = 4 if comp == 0 else 2
    n = lines.shape[1] // 2
    x, y = cell.ux * unit, cell.uy * unit
    if d == 0:
        planes[comp][y:y + lines.shape[0], x - n:x + n] = lines
    else:
        planes[comp][y - n:y + n, x:x + lines.shape[0]] = lines.T


def build(seed=0x266):
    """-> (y, cb, cr, edges_v, edges_h, offsets (capi.DbfOffsets), cells_v, cells_h); cells_* parallel to edges_* (raster order)."""
    rng = np.random.default_rng(seed)
    planes = [rng.integers(0, 1024, (H, W)).astype(np.int64), rng.integers(0, 1024, (H // 2, W // 2)).astype(np.int64),
              rng.integers(0, 1024, (H // 2, W // 2)).astype(np.int64)]      # noise everywhere else: a stray write shows
    slots = _Slots()
    cells = []

    def luma_cell(d, lp, lq, bs, qp, off, want, group, ext=(True, True), variant="", base=400, lines=None, clip=None, gate=None):
        tc, beta, _, _ = lim(qp, bs, off)
        slopes = pick_slopes(want, lp, lq, beta, len(cells))
        if variant.startswith("far_ramp"):                       # the far ramp uses the decision's room on its side
            slopes = (0, 1) if variant == "far_ramp_p" else (1, 0)
        if base in (0, 1023):
            slopes = (abs(slopes[0]), abs(slopes[1]))            # pinned at an end of the range: ramps lead away from it
        ux, uy = slots.take(0, d)
        if want == "weak":
            ext = (ext[0] and lp > 1, ext[1] and lp > 1)          # spec_dbf Q2: maxFilterLengthP gates both sides
            if gate is None:
                gate = {"": 4, "gate1": 3, "gate2": 2}.get(variant, 4)
        c = Cell(0, d, ux, uy, luma_word(bs, lp, lq, qp), off, want, ext if want == "weak" else None, gate if want == "weak" else None, clip, group,
                 dict(lp=lp, lq=lq, bs=bs, qp=qp, tc=tc, beta=beta, variant=variant, slopes=slopes if lines is None else None))
        _paint(planes, c, lines if lines is not None else luma_lines(want, lp, lq, tc, beta, base, ext, variant, slopes))
        cells.append(c)
        return c

    def chroma_cell(comp, d, large, ctb_b, bs, qp, off, want, group, odd=None, base=500):
        tc, beta, _, _ = lim(qp, bs, off)
        ux, uy = slots.take(comp, d, odd)
        slopes = pick_slopes(want, 3, 3, beta, len(cells), chroma=True)
        c = Cell(comp, d, ux, uy, chroma_word(bs, large, ctb_b, qp), off, want, None, None, None, group,
                 dict(large=large, ctb_b=ctb_b, bs=bs, qp=qp, tc=tc, beta=beta, slopes=slopes))
        _paint(planes, c, chroma_lines(want, large, ctb_b, tc, beta, base, slopes))
        cells.append(c)
        return c

    # ---- luma matrix: 11 pairs x 2 directions x bS x every outcome the pair can reach, all with the dense route's pair
    for d in (0, 1):
        for lp, lq in LUMA_PAIRS:
            for bs in (1, 2):
                qp = 38 if bs == 1 else 41
                luma_cell(d, lp, lq, bs, qp, DENSE_IDX, "off", "matrix")
                if max(lp, lq) > 3:                                  # three times: different pairs of ramps
                    luma_cell(d, lp, lq, bs, qp, DENSE_IDX, "long", "matrix")
                    luma_cell(d, lp, lq, bs, qp, DENSE_IDX, "long", "matrix", base=520)
                    luma_cell(d, lp, lq, bs, qp, DENSE_IDX, "long", "matrix", base=300)
                    # single terms of the long decision: a far part that is steep but straight (long), one far sample off (strong)
                    if lp > 3:
                        luma_cell(d, lp, lq, bs, qp, DENSE_IDX, "long", "farterm", variant="far_ramp_p")
                    if lq > 3:
                        luma_cell(d, lp, lq, bs, qp, DENSE_IDX, "long", "farterm", variant="far_ramp_q")
                    if lp > 2 and 7 in (lp, lq):
                        luma_cell(d, lp, lq, bs, qp, DENSE_IDX, "strong", "farterm", variant="far6")
                if lp > 2:
                    luma_cell(d, lp, lq, bs, qp, DENSE_IDX, "strong", "matrix")
                    luma_cell(d, lp, lq, bs, qp, DENSE_IDX, "strong", "matrix", base=520)
                for ext in (((True, True), (True, False), (False, True), (False, False)) if lp > 1 else ((False, False),)):
                    luma_cell(d, lp, lq, bs, qp, DENSE_IDX, "weak", "matrix", ext=ext)
        # decisions follow lines 0 and 3 only; lines across the 10 tC gate; samples pinned at both ends of the range
        for lp, lq in ((7, 7), (5, 3), (3, 3)):
            luma_cell(d, lp, lq, 1, 38, DENSE_IDX, "long" if max(lp, lq) > 3 else "strong", "lines03", variant="mid_noise")
        luma_cell(d, 3, 7, 2, 38, DENSE_IDX, "strong", "lines03", variant="mid_noise")
        for lp, lq, var in ((3, 3, "gate1"), (7, 5, "gate2"), (1, 1, "gate1")):
            luma_cell(d, lp, lq, 1, 30, DENSE_IDX, "weak", "gate", variant=var, base=300)
        for lp, lq in ((1, 1), (2, 2)):
            for end in ("lo", "hi"):
                luma_cell(d, lp, lq, 1, 38, DENSE_IDX, "weak", "pinned", lines=clip_lines(end), clip=end, ext=(True, True))
        for lp, lq, want in ((7, 7, "long"), (3, 7, "long"), (5, 5, "long"), (3, 3, "strong")):
            luma_cell(d, lp, lq, 2, 38, DENSE_IDX, want, "pinned", base=0)
            luma_cell(d, lp, lq, 2, 38, DENSE_IDX, want, "pinned", base=1023)

    # ---- chroma matrix: both planes, both directions, large x ctb_b (horizontal only) x bS x strong / weak, either limit 0,
    # vertical edges at both alignments
    for comp in (1, 2):
        for d in (0, 1):
            for odd in ((False, True) if d == 0 else (None,)):
                for large in (0, 1):
                    for ctb_b in ((0, 1) if d == 1 else (0,)):
                        for bs in (1, 2):
                            for want in (("strong", "weak") if large else ("weak",)):
                                chroma_cell(comp, d, large, ctb_b, bs, 38 + bs, DENSE_IDX, want, "cmatrix", odd)
                chroma_cell(comp, d, 1, 0, 1, 20, 2, "skip", "climit", odd)        # tc == 0, beta > 0
                chroma_cell(comp, d, 1, 0, 1, 20, 1, "skip", "climit", odd)        # beta == 0, tc > 0
                chroma_cell(comp, d, 0, d, 2, 10, 0, "skip", "climit", odd)        # both 0

    # ---- table ends: every target index of either table, reached through QP and a pair of the table
    def table_cells(which, target):
        found = []
        for off in range(8):
            for bs in (1, 2):
                qp = target - (2 * (bs - 1) + OFF_TC[off] if which == "tc" else OFF_BETA[off])
                if 0 <= qp <= 63:
                    tc, beta, _, _ = lim(qp, bs, off)
                    found.append((-(tc > 0) - (beta > 0), off, bs, qp, tc, beta))       # most live limits first
        found.sort()
        return found[:2]

    for which, targets in (("tc", TC_TARGETS), ("beta", BETA_TARGETS)):
        for target in targets:
            picks = table_cells(which, target)
            assert picks, (which, target)
            for k, (_, off, bs, qp, tc, beta) in enumerate(picks):
                d = k % 2 if len(picks) > 1 else 0
                for dd in ((d,) if len(picks) > 1 else (0, 1)):
                    step = min(max(((5 * tc + 1) >> 1) - 1, 4), 100)
                    lines = np.full((4, 16), 400, np.int64); lines[:, 8:] += step; lines += 3 * np.arange(4)[:, None]
                    want = "skip" if tc == 0 and beta == 0 else "off" if beta == 0 else "strong" if tc > 0 else "weak"
                    c = luma_cell(dd, 3, 3, bs, qp, off, want, "table", lines=lines, gate=0 if want == "weak" else None)
                    c.note.update(which=which, target=target)
                    cc = chroma_cell(1 + k % 2, dd, 1, 0, bs, qp, off, "skip" if tc == 0 or beta == 0 else "strong", "table")
                    cc.note.update(which=which, target=target)

    # ---- offset indices: the same content at 5 QPs under each of the 8 pairs, both directions.  With the reference's tables
    # (spec_dbf Q1) pair 1 = (-24, 24) has both limits above 0 at QP 40 and 41 only, and pair 2 = (24, -24) at no QP at all:
    # its cells are there to be left alone
    for d in (0, 1):
        for qp, step in ((30, 10), (38, 10), (40, 10), (38, 100), (44, 100), (50, 100)):    # step 100: the weak filter's tC clip decides
            for off in range(8):
                tc, beta, _, _ = lim(qp, 1, off)
                lines = np.full((4, 16), 600, np.int64); lines[:, 8:] -= step; lines -= 4 * np.arange(4)[:, None]
                want = "skip" if tc == 0 and beta == 0 else "off" if beta == 0 else "strong" if step < ((5 * tc + 1) >> 1) else "weak"
                gate = None
                if want == "weak":
                    gate = 4 if abs((-9 * step + 3 * step + 8) >> 4) < 10 * tc else 0     # flat sides: q1 - p1 = q0 - p0 = -step
                c = luma_cell(d, 3, 3, 1, qp, off, want, "offsets", lines=lines, gate=gate)
                c.note.update(slot=(d, qp, step))

    # ---- fill the lists up (more than 64 * 9 + 3 edges per direction) with seeded cells of every kind and pair index
    def live(bs):
        while True:
            qp, off = int(rng.integers(24, 60)), int(rng.integers(0, 8))
            tc, beta, _, _ = lim(qp, bs, off)
            if 3 <= tc <= 60 and beta >= 120:                   # beta: room for a ramp on each side in every decision
                return qp, off

    for d in (0, 1):
        while slots.luma[d] and len([c for c in cells if c.dir == d and c.comp == 0]) < 330:
            lp, lq = LUMA_PAIRS[int(rng.integers(0, 11))]
            bs = int(rng.integers(1, 3))
            qp, off = live(bs)
            wants = ["off", "weak"] + (["long"] if max(lp, lq) > 3 else []) + (["strong"] if lp > 2 else [])
            want = wants[int(rng.integers(0, len(wants)))]
            ext = (bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
            luma_cell(d, lp, lq, bs, qp, off, want, "fill", ext=ext, base=int(rng.integers(200, 600)))
        for comp in (1, 2):
            for _ in range(130):
                large, bs = int(rng.integers(0, 2)), int(rng.integers(1, 3))
                qp, off = live(bs)
                want = "strong" if large and rng.integers(0, 2) else "weak"
                chroma_cell(comp, d, large, int(rng.integers(0, 2)) if d else 0, bs, qp, off, want, "fill", base=int(rng.integers(100, 800)))

    out = []
    for d in (0, 1):
        cs = sorted((c for c in cells if c.dir == d), key=lambda c: (c.comp, c.uy, c.ux))
        e = np.zeros(len(cs), capi.DBF_EDGE_DTYPE)
        for k, c in enumerate(cs):
            e[k] = (c.ux, c.uy, c.word, c.comp, c.off)
        out.append((e, cs))
    offs = capi.DbfOffsets()
    for k in range(8):
        offs.beta[k], offs.tc[k] = OFF_BETA[k], OFF_TC[k]
    y, cb, cr = (p.astype(np.uint16) for p in planes)
    return y, cb, cr, out[0][0], out[1][0], offs, out[0][1], out[1][1]


def check_labels(cells, branch):
    """every cell took the branch it was built for; returns the list of those that did not"""
    bad = []
    for k, (c, b) in enumerate(zip(cells, branch)):
        ok = b["kind"] == c.want
        if c.ext is not None:
            ok = ok and (bool(b["ext_p"]), bool(b["ext_q"])) == tuple(c.ext)
        if c.gate is not None:
            ok = ok and int(b["gate"]) == c.gate
        if c.clip is not None:
            ok = ok and bool(b["clip_lo" if c.clip == "lo" else "clip_hi"])
        if not ok:
            bad.append((k, c.group, c.comp, c.dir, c.want, c.ext, c.gate, c.note, str(b["kind"]), bool(b["ext_p"]), bool(b["ext_q"]), int(b["gate"])))
    return bad
