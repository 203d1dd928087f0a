"""TEST INFRASTRUCTURE: a plain restatement of the VVC deblocking filter's sample process.

Written from H.266 clause 8.8.3.6 (decisions 8.8.3.6.2 / .3 / .6, luma filters .7 / .8, chroma filter .10), in the
specification's own vocabulary (dE, dEp, dEq, refMiddle, tCPD, ...), one scalar Python step per clause.  It takes the
edge segments the recorder emits (capi.DBF_EDGE_DTYPE: position, bS, maximum filter lengths, average QP, offset-pair
index) and filters all vertical edges, then all horizontal edges of a picture.

Where the compiled reference (libovvc/rcn_df.c) departs from the specification the reference wins, because the
fixtures under tests/golden/ are its output.  Each departure is marked QUIRK below:
  Q1  the threshold tables carry one entry more than Table 43 and the index is clipped to that longer range: tC'[66]
      and beta'[64] are 0 where the specification would clip to 395 / 88 (rcn_df.c:42, :52-75, :179-180);
  Q2  the weak luma filter's Q-side extension (dEq) is gated by maxFilterLengthP > 1, not ...Q (rcn_df.c:1505, :2080);
  Q3  a chroma segment is left alone when EITHER limit is 0, so beta = 0 disables even the weak chroma filter, which
      the specification runs whenever tC > 0 (rcn_df.c:1121, :1291).

Every edge also gets a label of the branch it took (BRANCH_DTYPE).  The labels are derived here and nowhere else:
the tests use them to prove that a fixture or a directed cell reached the path it was built for.  Speed is no goal.
"""
import numpy as np

BIT_DEPTH = 10
PIX_MAX = (1 << BIT_DEPTH) - 1

# Table 43 (tC' for Q = 0..65, beta' for Q = 0..63) + QUIRK Q1: one further entry each, 0
TC_TABLE = [0] * 18 + [3, 4, 4, 4, 4, 5, 5, 5, 5, 7, 7, 8, 9, 10, 10, 11, 13, 14, 15, 17, 19, 21, 24, 25, 29, 33, 36, 41, 45, 51, 57,
                       64, 71, 80, 89, 100, 112, 125, 141, 157, 177, 198, 222, 250, 280, 314, 352, 395] + [0]
BETA_TABLE = [0] * 16 + list(range(6, 19)) + list(range(20, 90, 2)) + [0]
assert len(TC_TABLE) == 67 and len(BETA_TABLE) == 65 and TC_TABLE[65] == 395 and BETA_TABLE[63] == 88 and BETA_TABLE[28] == 18

# 8.8.3.6.8: interpolation weights and clipping steps of the long luma filter, by maxFilterLength
LONG_F = {7: (59, 50, 41, 32, 23, 14, 5), 5: (58, 45, 32, 19, 6), 3: (53, 32, 11)}
LONG_TCPD = {7: (6, 5, 4, 3, 2, 1, 1), 5: (6, 5, 4, 3, 2), 3: (6, 4, 2)}

# word layout of an edge record (include/ovvc_hip.h: OVHIP_DBF_LUMA, OVHIP_DBF_C_*)
C_ON, C_BS2, C_LARGE, C_CTB_B = 1, 2, 4, 8

BRANCH_DTYPE = np.dtype([
    ("comp", "u1"), ("kind", "U6"),         # luma: skip / off / long / strong / weak; chroma: skip / strong / weak
    ("lp", "u1"), ("lq", "u1"), ("bs", "u1"),
    ("ext_p", "?"), ("ext_q", "?"),         # weak luma: dEp, dEq
    ("gate", "u1"),                         # weak luma: how many of the 4 lines passed |delta| < 10 * tC
    ("large", "?"), ("ctb_b", "?"),         # chroma
    ("tc_idx", "i2"), ("beta_idx", "i2"),   # table indices BEFORE clipping
    ("tc", "i2"), ("beta", "i2"),
    ("off", "u1"),                          # offset-pair index the edge carries
    ("changed", "?"),                       # at least one sample of the picture changed
    ("clip_lo", "?"), ("clip_hi", "?"),     # a weak filter's Clip1() acted at 0 / at the maximum
])


def clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def limits(qp, bs, tc_offset, beta_offset):
    """8.8.3.6.2 for 10 bit: (tC, beta, unclipped tC index, unclipped beta index)."""
    tc_idx, beta_idx = qp + 2 * (bs - 1) + tc_offset, qp + beta_offset
    tc = TC_TABLE[clip3(0, 66, tc_idx)]                         # Q1 (10 bit: tC = tC')
    beta = BETA_TABLE[clip3(0, 64, beta_idx)] * (1 << (BIT_DEPTH - 8))
    return tc, beta, tc_idx, beta_idx


class _Line:
    """One line of samples across an edge: p(i) / q(i) as the specification numbers them."""

    def __init__(self, plane, along, line, vertical):
        self.a, self.x, self.l, self.v = plane, along, line, vertical

    def p(self, i):
        return int(self.a[self.l, self.x - 1 - i] if self.v else self.a[self.x - 1 - i, self.l])

    def q(self, i):
        return int(self.a[self.l, self.x + i] if self.v else self.a[self.x + i, self.l])

    def set_p(self, i, val):
        if self.v:
            self.a[self.l, self.x - 1 - i] = val
        else:
            self.a[self.x - 1 - i, self.l] = val

    def set_q(self, i, val):
        if self.v:
            self.a[self.l, self.x + i] = val
        else:
            self.a[self.x + i, self.l] = val


def _d2(a, b, c):
    return abs(a - 2 * b + c)


def _luma_sample_decision(ln, dpq, sp, sq, spq, large_p, large_q, lp, lq, beta, tc):
    """8.8.3.6.6: dSam for one line."""
    if large_p or large_q:
        if large_p:
            if lp == 7:
                sp += abs(ln.p(7) - ln.p(6) - ln.p(5) + ln.p(4))
            sp = (sp + abs(ln.p(3) - ln.p(lp)) + 1) >> 1
        if large_q:
            if lq == 7:
                sq += abs(ln.q(4) - ln.q(5) - ln.q(6) + ln.q(7))
            sq = (sq + abs(ln.q(3) - ln.q(lq)) + 1) >> 1
        s_thr1, s_thr2 = (3 * beta) >> 5, beta >> 4
    else:
        s_thr1, s_thr2 = beta >> 3, beta >> 2
    return dpq < s_thr2 and sp + sq < s_thr1 and spq < (5 * tc + 1) >> 1


def _luma_edge(plane, along, line0, vertical, lp, lq, tc, beta, br):
    """8.8.3.6.2 (decisions on lines 0 and 3) and 8.8.3.6.7 / .8 (filters on the 4 lines) for one 4-sample segment."""
    if tc == 0 and beta == 0:
        br["kind"] = "skip"
        return
    lines = [_Line(plane, along, line0 + k, vertical) for k in range(4)]
    l0, l3 = lines[0], lines[3]
    dp0, dp3 = _d2(l0.p(2), l0.p(1), l0.p(0)), _d2(l3.p(2), l3.p(1), l3.p(0))
    dq0, dq3 = _d2(l0.q(2), l0.q(1), l0.q(0)), _d2(l3.q(2), l3.q(1), l3.q(0))
    d = dp0 + dq0 + dp3 + dq3
    if d >= beta:
        br["kind"] = "off"                                        # dE = 0
        return
    large_p, large_q = lp > 3, lq > 3
    d_e = 1
    if large_p or large_q:
        dp0l, dp3l, dq0l, dq3l = dp0, dp3, dq0, dq3
        if large_p:
            dp0l = (dp0 + _d2(l0.p(5), l0.p(4), l0.p(3)) + 1) >> 1
            dp3l = (dp3 + _d2(l3.p(5), l3.p(4), l3.p(3)) + 1) >> 1
        if large_q:
            dq0l = (dq0 + _d2(l0.q(5), l0.q(4), l0.q(3)) + 1) >> 1
            dq3l = (dq3 + _d2(l3.q(5), l3.q(4), l3.q(3)) + 1) >> 1
        if dp0l + dq0l + dp3l + dq3l < beta:
            sam = [_luma_sample_decision(ln, 2 * (dpl + dql), abs(ln.p(0) - ln.p(3)), abs(ln.q(0) - ln.q(3)), abs(ln.p(0) - ln.q(0)),
                                         large_p, large_q, lp, lq, beta, tc)
                   for ln, dpl, dql in ((l0, dp0l, dq0l), (l3, dp3l, dq3l))]
            if all(sam):
                d_e = 3
    if d_e != 3 and lp > 2:                                       # the short strong filter needs 3 samples on each side
        sam = [_luma_sample_decision(ln, 2 * (dp + dq), abs(ln.p(0) - ln.p(3)), abs(ln.q(0) - ln.q(3)), abs(ln.p(0) - ln.q(0)),
                                     False, False, lp, lq, beta, tc)
               for ln, dp, dq in ((l0, dp0, dq0), (l3, dp3, dq3))]
        if all(sam):
            d_e = 2
    if d_e == 3:
        br["kind"] = "long"
        for ln in lines:
            _luma_long(ln, lp, lq, tc)
    elif d_e == 2:
        br["kind"] = "strong"
        for ln in lines:
            p = [ln.p(i) for i in range(4)]
            q = [ln.q(i) for i in range(4)]
            ln.set_p(0, clip3(p[0] - 3 * tc, p[0] + 3 * tc, (p[2] + 2 * p[1] + 2 * p[0] + 2 * q[0] + q[1] + 4) >> 3))
            ln.set_p(1, clip3(p[1] - 2 * tc, p[1] + 2 * tc, (p[2] + p[1] + p[0] + q[0] + 2) >> 2))
            ln.set_p(2, clip3(p[2] - tc, p[2] + tc, (2 * p[3] + 3 * p[2] + p[1] + p[0] + q[0] + 4) >> 3))
            ln.set_q(0, clip3(q[0] - 3 * tc, q[0] + 3 * tc, (p[1] + 2 * p[0] + 2 * q[0] + 2 * q[1] + q[2] + 4) >> 3))
            ln.set_q(1, clip3(q[1] - 2 * tc, q[1] + 2 * tc, (p[0] + q[0] + q[1] + q[2] + 2) >> 2))
            ln.set_q(2, clip3(q[2] - tc, q[2] + tc, (p[0] + q[0] + q[1] + 3 * q[2] + 2 * q[3] + 4) >> 3))
    else:
        br["kind"] = "weak"
        side = (beta + (beta >> 1)) >> 3
        d_ep = dp0 + dp3 < side and lp > 1
        d_eq = dq0 + dq3 < side and lp > 1                        # Q2: the specification tests maxFilterLengthQ here
        br["ext_p"], br["ext_q"] = d_ep, d_eq
        gate = 0
        for ln in lines:
            p0, p1, p2, q0, q1, q2 = ln.p(0), ln.p(1), ln.p(2), ln.q(0), ln.q(1), ln.q(2)
            delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
            if abs(delta) >= 10 * tc:
                continue
            gate += 1
            delta = clip3(-tc, tc, delta)
            out = [(ln.set_p, 0, p0 + delta), (ln.set_q, 0, q0 - delta)]
            if d_ep:
                out.append((ln.set_p, 1, p1 + clip3(-(tc >> 1), tc >> 1, (((p2 + p0 + 1) >> 1) - p1 + delta) >> 1)))
            if d_eq:
                out.append((ln.set_q, 1, q1 + clip3(-(tc >> 1), tc >> 1, (((q2 + q0 + 1) >> 1) - q1 - delta) >> 1)))
            for setter, i, v in out:
                if v < 0:
                    br["clip_lo"] = True
                if v > PIX_MAX:
                    br["clip_hi"] = True
                setter(i, clip3(0, PIX_MAX, v))
        br["gate"] = gate


def _luma_long(ln, lp, lq, tc):
    """8.8.3.6.8 for one line."""
    p = [ln.p(i) for i in range(lp + 1)]
    q = [ln.q(i) for i in range(lq + 1)]
    if lp == lq == 5:
        mid = (p[4] + p[3] + 2 * (p[2] + p[1] + p[0] + q[0] + q[1] + q[2]) + q[3] + q[4] + 8) >> 4
    elif lp == lq:
        mid = (sum(p[1:7]) + 2 * (p[0] + q[0]) + sum(q[1:7]) + 8) >> 4
    elif {lp, lq} == {7, 5}:
        mid = (sum(p[2:6]) + 2 * (p[1] + p[0] + q[0] + q[1]) + sum(q[2:6]) + 8) >> 4
    elif {lp, lq} == {5, 3}:
        mid = (sum(p[0:4]) + sum(q[0:4]) + 4) >> 3
    elif lq == 7:                                                 # (3, 7)
        mid = (2 * (p[2] + p[1] + p[0] + q[0]) + p[0] + p[1] + sum(q[1:7]) + 8) >> 4
    else:                                                         # (7, 3)
        mid = (2 * (q[2] + q[1] + q[0] + p[0]) + q[0] + q[1] + sum(p[1:7]) + 8) >> 4
    ref_p, ref_q = (p[lp] + p[lp - 1] + 1) >> 1, (q[lq] + q[lq - 1] + 1) >> 1
    for i in range(lp):
        c = (tc * LONG_TCPD[lp][i]) >> 1
        ln.set_p(i, clip3(p[i] - c, p[i] + c, (mid * LONG_F[lp][i] + ref_p * (64 - LONG_F[lp][i]) + 32) >> 6))
    for i in range(lq):
        c = (tc * LONG_TCPD[lq][i]) >> 1
        ln.set_q(i, clip3(q[i] - c, q[i] + c, (mid * LONG_F[lq][i] + ref_q * (64 - LONG_F[lq][i]) + 32) >> 6))


def _chroma_edge(plane, along, line0, vertical, large, ctb_b, tc, beta, br):
    """8.8.3.6.3 and .10 for one segment of 2 chroma lines (4:2:0).  ctb_b: horizontal edge on a CTB boundary, where
    maxFilterLengthP is 1 and p1 stands in for p2 and p3."""
    if tc == 0 or beta == 0:                                      # Q3
        br["kind"] = "skip"
        return
    lines = [_Line(plane, along, line0 + k, vertical) for k in range(2)]
    strong = False
    if large:                                                     # maxFilterLengthCbCr == 3
        d, sam = [], []
        for ln in lines:
            p0, p1, q0 = ln.p(0), ln.p(1), ln.q(0)
            p2, p3 = (p1, p1) if ctb_b else (ln.p(2), ln.p(3))
            dpq = _d2(p2, p1, p0) + _d2(ln.q(2), ln.q(1), q0)
            d.append(dpq)
            sam.append(2 * dpq < beta >> 2 and abs(p3 - p0) + abs(q0 - ln.q(3)) < beta >> 3 and abs(p0 - q0) < (5 * tc + 1) >> 1)
        strong = d[0] + d[1] < beta and all(sam)
    br["kind"] = "strong" if strong else "weak"
    for ln in lines:
        p = [ln.p(i) for i in range(4)]
        q = [ln.q(i) for i in range(4)]
        if strong and ctb_b:
            ln.set_p(0, clip3(p[0] - tc, p[0] + tc, (3 * p[1] + 2 * p[0] + q[0] + q[1] + q[2] + 4) >> 3))
            ln.set_q(0, clip3(q[0] - tc, q[0] + tc, (2 * p[1] + p[0] + 2 * q[0] + q[1] + q[2] + q[3] + 4) >> 3))
            ln.set_q(1, clip3(q[1] - tc, q[1] + tc, (p[1] + p[0] + q[0] + 2 * q[1] + q[2] + 2 * q[3] + 4) >> 3))
            ln.set_q(2, clip3(q[2] - tc, q[2] + tc, (p[0] + q[0] + q[1] + 2 * q[2] + 3 * q[3] + 4) >> 3))
        elif strong:
            ln.set_p(0, clip3(p[0] - tc, p[0] + tc, (p[3] + p[2] + p[1] + 2 * p[0] + q[0] + q[1] + q[2] + 4) >> 3))
            ln.set_p(1, clip3(p[1] - tc, p[1] + tc, (2 * p[3] + p[2] + 2 * p[1] + p[0] + q[0] + q[1] + 4) >> 3))
            ln.set_p(2, clip3(p[2] - tc, p[2] + tc, (3 * p[3] + 2 * p[2] + p[1] + p[0] + q[0] + 4) >> 3))
            ln.set_q(0, clip3(q[0] - tc, q[0] + tc, (p[2] + p[1] + p[0] + 2 * q[0] + q[1] + q[2] + q[3] + 4) >> 3))
            ln.set_q(1, clip3(q[1] - tc, q[1] + tc, (p[1] + p[0] + q[0] + 2 * q[1] + q[2] + 2 * q[3] + 4) >> 3))
            ln.set_q(2, clip3(q[2] - tc, q[2] + tc, (p[0] + q[0] + q[1] + 2 * q[2] + 3 * q[3] + 4) >> 3))
        else:
            delta = clip3(-tc, tc, ((((q[0] - p[0]) << 2) + p[1] - q[1] + 4) >> 3))
            for setter, v in ((ln.set_p, p[0] + delta), (ln.set_q, q[0] - delta)):
                if v < 0:
                    br["clip_lo"] = True
                if v > PIX_MAX:
                    br["clip_hi"] = True
                setter(0, clip3(0, PIX_MAX, v))


def _pass(planes, edges, vertical, offsets):
    beta_off, tc_off = offsets
    out = np.zeros(len(edges), BRANCH_DTYPE)
    for k, e in enumerate(edges):
        br = out[k]
        comp, word, ux, uy, oi = int(e["comp"]), int(e["word"]), int(e["ux"]), int(e["uy"]), int(e["pad"]) & 7
        plane = planes[comp]
        br["comp"], br["off"] = comp, oi
        unit = 4 if comp == 0 else 2                              # samples per 4-luma-sample unit in this plane
        along, line0 = (ux * unit, uy * unit) if vertical else (uy * unit, ux * unit)
        n_side, n_lines = 4, (4 if comp == 0 else 2)
        if comp == 0:
            bs, lp, lq = word & 3, (word >> 2) & 7, (word >> 5) & 7
            assert bs in (1, 2), "an edge record always carries bS 1 or 2"
            n_side = 8 if lp > 3 or lq > 3 else 4
        else:
            assert word & C_ON
            bs, lp, lq = 1 + bool(word & C_BS2), 0, 0
        tc, beta, tc_idx, beta_idx = limits(word >> 8, bs, int(tc_off[oi]), int(beta_off[oi]))
        br["bs"], br["lp"], br["lq"], br["tc_idx"], br["beta_idx"], br["tc"], br["beta"] = bs, lp, lq, tc_idx, beta_idx, tc, beta
        a, b = (slice(line0, line0 + n_lines), slice(along - n_side, along + n_side))
        before = (plane[a, b] if vertical else plane[b, a]).copy()
        if comp == 0:
            _luma_edge(plane, along, line0, vertical, lp, lq, tc, beta, br)
        else:
            br["large"], br["ctb_b"] = bool(word & C_LARGE), bool(word & C_CTB_B)
            _chroma_edge(plane, along, line0, vertical, bool(word & C_LARGE), bool(word & C_CTB_B), tc, beta, br)
        br["changed"] = not np.array_equal(before, plane[a, b] if vertical else plane[b, a])
    return out


def filter(y, cb, cr, edges_v, edges_h, offsets):
    """Deblock one 4:2:0 10-bit picture.  edges_*: capi.DBF_EDGE_DTYPE; offsets: (beta[8], tc[8]) signed, or an object with
    .beta / .tc (capi.DbfOffsets).  All vertical edges first, then all horizontal edges (8.8.3.1).
    Returns (y, cb, cr, branch_v, branch_h): new uint16 planes and one BRANCH_DTYPE label per edge."""
    if hasattr(offsets, "beta"):
        offsets = (list(offsets.beta), list(offsets.tc))
    planes = [np.array(p, dtype=np.int32) for p in (y, cb, cr)]
    branch_v = _pass(planes, edges_v, True, offsets)
    branch_h = _pass(planes, edges_h, False, offsets)
    y, cb, cr = (p.astype(np.uint16) for p in planes)
    return y, cb, cr, branch_v, branch_h


def single_pair(beta_offset, tc_offset):
    return ([beta_offset] * 8, [tc_offset] * 8)
