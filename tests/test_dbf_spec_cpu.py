"""CPU: the plain restatement of the deblocking filter (tests/spec_dbf.py) against the compiled reference's pictures, against
the oracle, and the branch census of the two slot-level fixtures.

dbf.ovg      : the first generator profile.  No long luma filter, the table indices stay inside both tables, one offset pair.
dbf_ends.ovg : the second profile (oracle/ref_harness/gen_golden.c, g_dbf_ends): flat / ramp / noisy / pinned CUs, QP 0..63,
               (beta, tc) offset pairs that change from CTU to CTU (8 pairs in picture 0, 3 in picture 1, 1 in picture 2).
The census below is computed by spec_dbf on the reference's INPUT planes; because spec_dbf's output equals the reference's
on every sample (asserted first), the labels describe what the reference did.  It is asserted, so a regenerated fixture
cannot silently lose a path.
"""
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest

import dbf_cells
import golden_cases
import oracle_lib
import oracle_pipeline
import pipe_cases
import spec_dbf
from openvvc_amd import capi

FIXTURES = ("dbf.ovg", "dbf_ends.ovg")
MAIN_LONG = ((7, 7), (7, 3), (3, 7), (5, 5))
OTHER_LONG = ((3, 5), (5, 3), (5, 7), (7, 5))


@lru_cache(maxsize=None)
def cases(name):
    return golden_cases.dbf_cases(name)


@lru_cache(maxsize=None)
def spec_results(name):
    """[(y, cb, cr, branch_v, branch_h)] of spec_dbf per picture, computed once and shared."""
    out = []
    for pic, planes, _ in cases(name):
        (ev, offs), (eh, _) = planes["edges"]
        out.append(spec_dbf.filter(pic.y, pic.cb, pic.cr, ev, eh, offs))
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_spec_equals_reference(built_lib, name):
    assert len(cases(name)) == 3
    for i, ((pic, _, exp), got) in enumerate(zip(cases(name), spec_results(name))):
        for plane, a, b, c in (("Y", got[0], exp.y, pic.y), ("Cb", got[1], exp.cb, pic.cb), ("Cr", got[2], exp.cr, pic.cr)):
            assert (b != c).sum() > 300, "fixture does not exercise the filter"
            bad = np.argwhere(a != b)
            assert len(bad) == 0, f"{name} picture {i} plane {plane}: {len(bad)} samples differ, first at (y,x) {bad[:6].tolist()}"


@pytest.mark.parametrize("name", FIXTURES)
def test_spec_equals_oracle(built_lib, name):
    """oracle_dbf over the dense planes where the picture has them, oracle_dbf_edges over the lists on every picture."""
    n_dense = 0
    for i, ((pic, planes, _), got) in enumerate(zip(cases(name), spec_results(name))):
        (ev, offs), (eh, _) = planes["edges"]
        works = [("edges", pic.copy())]
        oracle_lib.dbf_edges(works[0][1], ev, eh, offs)
        if planes["meta"]["planes_status"] == 0:
            works.append(("planes", pic.copy()))
            oracle_lib.dbf(works[1][1], planes)
            n_dense += 1
        for how, work in works:
            for plane, a, b in (("Y", work.y, got[0]), ("Cb", work.cb, got[1]), ("Cr", work.cr, got[2])):
                assert np.array_equal(a, b), f"{name} picture {i} ({how}) plane {plane}: {int((a != b).sum())} samples differ"
    assert n_dense == (3 if name == "dbf.ovg" else 1)


def test_ends_oracle_matches_reference(built_lib):
    for i, (pic, planes, exp) in enumerate(cases("dbf_ends.ovg")):
        (ev, offs), (eh, _) = planes["edges"]
        work = pic.copy()
        oracle_lib.dbf_edges(work, ev, eh, offs)
        for plane, a, b in (("Y", work.y, exp.y), ("Cb", work.cb, exp.cb), ("Cr", work.cr, exp.cr)):
            assert np.array_equal(a, b), f"dbf_ends picture {i} plane {plane}: {int((a != b).sum())} samples differ"


@pytest.mark.parametrize("name,k", [("pipe", 1), ("tiles_b", 1)])
def test_spec_equals_oracle_on_a_chained_picture(built_lib, name, k):
    """One B picture each of two chained streams, where the long filters are pinned through the whole pipeline: the deblocking
    stage of the oracle pipeline, from the picture its prediction and transform stages made."""
    P = pipe_cases.Pipe(name)
    wl = P.workload(k, {j: P.frames[j] for j in range(P.n)})
    before = oracle_pipeline.decode(wl, stages=("mc", "itx"))
    after = oracle_pipeline.decode(wl, stages=("mc", "itx", "dbf"))
    offs = spec_dbf.single_pair(wl.dbf_planes["beta_offset"], wl.dbf_planes["tc_offset"])
    y, cb, cr, bv, bh = spec_dbf.filter(before.y, before.cb, before.cr, wl.dbf_edges[0], wl.dbf_edges[1], offs)
    for plane, a, b in (("Y", y, after.y), ("Cb", cb, after.cb), ("Cr", cr, after.cr)):
        assert np.array_equal(a, b), f"{name} picture {k} plane {plane}: {int((a != b).sum())} samples differ"
    assert not np.array_equal(before.y, after.y)
    for b in (bv, bh):
        assert (b["kind"][b["comp"] == 0] == "long").sum() >= 8, "the chained picture no longer takes a long filter"


# ---------------------------------------------------------------------------------------------------------------- census
def census(name, pictures=None):
    """What the reference's pictures of one fixture (all, or the listed ones) took, per direction (0 vertical, 1 horizontal)."""
    out = []
    for d in (0, 1):
        br = np.concatenate([r[3 + d] for k, r in enumerate(spec_results(name)) if pictures is None or k in pictures])
        luma, chroma = br[br["comp"] == 0], br[br["comp"] > 0]
        lng = luma[luma["kind"] == "long"]
        weak = br[br["kind"] == "weak"]
        out.append(dict(
            long=Counter(zip(lng["lp"].tolist(), lng["lq"].tolist())),
            pairs=set(zip(luma["lp"].tolist(), luma["lq"].tolist())),
            kinds=Counter(luma["kind"].tolist()), kinds_c=Counter(chroma["kind"].tolist()),
            strong_ctb_b=int(((chroma["kind"] == "strong") & chroma["ctb_b"]).sum()),
            tc_idx=(int(br["tc_idx"].min()), int(br["tc_idx"].max())), beta_idx=(int(br["beta_idx"].min()), int(br["beta_idx"].max())),
            tc_idx_set=set(br["tc_idx"].tolist()), beta_idx_set=set(br["beta_idx"].tolist()),
            tc_max=int(br["tc"].max()),
            clip_lo=int(weak["clip_lo"].sum()), clip_hi=int(weak["clip_hi"].sum()),
            clip_lo_luma=int((weak["clip_lo"] & (weak["comp"] == 0)).sum()), clip_hi_luma=int((weak["clip_hi"] & (weak["comp"] == 0)).sum()),
            off_changed=set(br["off"][br["changed"]].tolist()), off_all=set(br["off"].tolist())))
    return out


def test_census_of_the_first_profile(built_lib):
    """What dbf.ovg does NOT reach (the reason dbf_ends.ovg exists); if the first profile ever changes, this records it."""
    got = census("dbf.ovg")
    assert len(got[0]["pairs"] | got[1]["pairs"]) == 11       # every (lp, lq) the recorder emits occurs, none of them takes `long`
    for c in got:
        assert not c["long"]
        assert 0 < c["beta_idx"][0] and c["beta_idx"][1] < 63 and 0 < c["tc_idx"][0] and c["tc_idx"][1] < 65     # neither end of either table
        assert c["tc_max"] <= 125 and c["clip_lo"] == 0 and c["clip_hi"] == 0
        assert c["off_all"] == {0} and c["kinds"]["skip"] == 0


def test_census_of_the_ends_profile(built_lib):
    got = census("dbf_ends.ovg")
    reached = []
    for d, c in enumerate(got):
        for pair in MAIN_LONG:
            assert c["long"][pair] >= 8, f"dir {d}: long {pair} taken {c['long'][pair]} times"
        # the remaining long pairs: REACHED_OTHER_LONG lists which of them the fixture takes per direction (all four, in both);
        # tests/test_gpu_dbf_cells.py covers all eight long pairs in both directions on the device whatever this fixture reaches
        reached.append(sorted(p for p in OTHER_LONG if c["long"][p] >= 1))
        assert c["strong_ctb_b"] >= 8 or d == 0
        assert c["tc_idx"][0] <= 0 and 65 in c["tc_idx_set"] and c["tc_idx"][1] >= 66, c["tc_idx"]
        assert c["beta_idx"][0] <= 0 and 63 in c["beta_idx_set"] and c["beta_idx"][1] >= 64, c["beta_idx"]
        assert c["tc_max"] == 395                         # the last real table entry, with it the widest p +- 3 * tc clips
        assert c["kinds"]["skip"] >= 1                    # the luma tc == 0 && beta == 0 early-out
        assert c["kinds"]["off"] >= 8 and c["kinds"]["weak"] >= 8 and c["kinds"]["strong"] >= 8
        assert c["kinds_c"]["skip"] >= 8 and c["kinds_c"]["weak"] >= 8 and c["kinds_c"]["strong"] >= 8
    assert got[0]["strong_ctb_b"] == 0                    # ctb_b exists on horizontal edges only
    for d, c in enumerate(census("dbf_ends.ovg", pictures=(0,))):        # the picture with 8 pairs: every index changes samples
        assert c["off_changed"] == set(range(8)), f"dir {d}: offset indices on edges that change samples: {c['off_changed']}"
    # the weak luma filter's Clip1() acts at both ends: a sample leaves as 0 / 1023 whose unclipped value lay outside
    assert sum(c["clip_lo_luma"] for c in got) >= 1 and sum(c["clip_hi_luma"] for c in got) >= 1
    assert reached == REACHED_OTHER_LONG, reached


def test_census_of_the_dense_route_picture(built_lib):
    """Picture 2 of dbf_ends.ovg is the only picture of the fixture with a single offset pair, so the only one that reaches the
    dense-plane kernel (ovhip_dbf_launch).  What it takes is pinned here: seven long pairs on vertical edges (no (5,5)), six on
    horizontal ones (no (7,7), no (5,3)), index 66 of tC' and 64 of beta', no luma early-out on horizontal edges, no strong chroma
    filter on a CTU boundary.  What it lacks, the dense-route test of the directed cells has (tests/test_gpu_dbf_cells.py)."""
    v, h = census("dbf_ends.ovg", pictures=(2,))
    assert dict(v["long"]) == {(3, 5): 8, (3, 7): 9, (5, 3): 4, (5, 7): 8, (7, 3): 10, (7, 5): 12, (7, 7): 5}
    assert dict(h["long"]) == {(3, 5): 8, (3, 7): 9, (5, 5): 4, (5, 7): 6, (7, 3): 4, (7, 5): 4}
    for c in (v, h):
        assert c["tc_idx"][1] >= 66 and 65 in c["tc_idx_set"] and c["beta_idx"][1] >= 64 and 63 in c["beta_idx_set"] and c["tc_max"] == 395
        assert min(c["kinds"][k] for k in ("off", "weak", "strong", "long")) >= 8
        assert min(c["kinds_c"][k] for k in ("skip", "weak", "strong")) >= 8
        assert c["strong_ctb_b"] == 0 and c["off_all"] == {0}
    assert v["kinds"]["skip"] == 4 and h["kinds"]["skip"] == 0


# which of the remaining long pairs the reference's pictures take, per direction (vertical, horizontal)
REACHED_OTHER_LONG = [[(3, 5), (5, 3), (5, 7), (7, 5)], [(3, 5), (5, 3), (5, 7), (7, 5)]]


def test_ends_offset_pairs(built_lib):
    """8, 3 and 1 distinct pairs; both ends of -24..24 and mixed signs.  Every edge carries the pair of the CTU during whose
    call the reference filters it: a vertical edge belongs to the CTU of its Q side; the horizontal pass of a CTU is shifted
    8 samples (2 units) to the left, so a horizontal edge in the last 2 unit columns of a CTU belongs to the CTU on its right
    (rcn_df.c:2099-2106, :2169-2198).  Edges ON a boundary between CTUs that carry different pairs exist in both directions
    and change samples, and so do horizontal edges whose owner is not the CTU that contains them."""
    n_pairs = []
    for i, ((pic, planes, _), got) in enumerate(zip(cases("dbf_ends.ovg"), spec_results("dbf_ends.ovg"))):
        pair_of = {(cx, cy): (b, t) for cx, cy, b, t in planes["meta"]["ctu_offsets"]}
        nx = max(cx for cx, _ in pair_of) + 1
        distinct = sorted(set(pair_of.values()))
        n_pairs.append(len(distinct))
        offs = planes["edges"][0][1]
        table = [(offs.beta[k], offs.tc[k]) for k in range(len(distinct))]
        assert sorted(table) == distinct
        if len(distinct) == 1:
            continue
        for d in (0, 1):
            e, br = planes["edges"][d][0], got[3 + d]
            n_cross = n_shifted = 0
            for k in range(len(e)):
                ux, uy = int(e["ux"][k]), int(e["uy"][k])
                q_ctu = (ux // 32, uy // 32)
                p_ctu = ((ux - 1) // 32, uy // 32) if d == 0 else (ux // 32, (uy - 1) // 32)
                owner = q_ctu if d == 0 else (min((ux + 2) // 32, nx - 1), uy // 32)
                assert table[int(e["pad"][k])] == pair_of[owner], f"picture {i} dir {d} edge {k} at unit ({ux}, {uy})"
                n_cross += pair_of[p_ctu] != pair_of[q_ctu] and bool(br["changed"][k])
                n_shifted += owner != q_ctu and pair_of[owner] != pair_of[q_ctu] and bool(br["changed"][k])
            assert n_cross >= 8, f"picture {i} dir {d}: {n_cross} changed edges between CTUs with different pairs"
            assert d == 0 or n_shifted >= 8, f"picture {i}: {n_shifted} changed horizontal edges filtered with the next CTU's pair"
    assert n_pairs == [8, 3, 1]
    allp = {(b, t) for _, pl, _ in cases("dbf_ends.ovg") for _, _, b, t in pl["meta"]["ctu_offsets"]}
    vals = {v for p in allp for v in p}
    assert -24 in vals and 24 in vals and any(b < 0 < t for b, t in allp) and any(t < 0 < b for b, t in allp)


# ---------------------------------------------------------------------------------------------------------------- recorder
def test_ends_recorder_lists_planes_and_refusals(built_lib):
    lib = capi.load()
    key = lambda a: sorted(zip(a["comp"].tolist(), a["uy"].tolist(), a["ux"].tolist(), a["word"].tolist()))
    n_single = 0
    for i, (_, planes, _) in enumerate(cases("dbf_ends.ovg")):
        n = len({(b, t) for _, _, b, t in planes["meta"]["ctu_offsets"]})
        if n > 1:
            assert planes["meta"]["planes_status"] == capi.OVHIP_EUNSUP, f"picture {i}: {n} pairs, ovhip_rec_dbf_planes -> {planes['meta']['planes_status']}"
            assert max(int(planes["edges"][d][0]["pad"].max()) for d in (0, 1)) == n - 1
            continue
        n_single += 1
        assert planes["meta"]["planes_status"] == 0
        for d in (0, 1):
            direct, offs = planes["edges"][d]
            assert key(direct) == key(capi.dbf_compact(planes, d)), f"picture {i} dir {d}"
            assert len(direct) > 100 and (direct["pad"] == 0).all()
            assert offs.beta[0] == planes["beta_offset"] and offs.tc[0] == planes["tc_offset"]
    assert n_single == 1


def test_ninth_offset_pair_is_refused(built_lib):
    """A recorder that holds 8 distinct pairs refuses a CTU with a 9th one and leaves its lists and its table as they were."""
    import golden_io
    g = golden_io.load("dbf_ends.ovg")
    y = g["p0_in_y"]
    rec = capi.Recorder(y.shape[1], y.shape[0])
    raws = [r.tobytes() for r in g["p0_ctus"]]
    for raw in raws:
        rec.dbf_ctu(raw)
    before = [rec.dbf_edges(d) for d in (0, 1)]
    assert len({(before[0][1].beta[k], before[0][1].tc[k]) for k in range(8)}) == 8
    ninth = np.frombuffer(raws[-1], capi.DBF_CTU_DTYPE).copy()
    ninth["beta_offset"], ninth["tc_offset"] = 8, -8
    buf = ninth.tobytes()
    assert rec.lib.ovhip_rec_dbf_ctu(rec.h, buf) == capi.OVHIP_EUNSUP
    after = [rec.dbf_edges(d) for d in (0, 1)]
    for (ea, oa), (eb, ob) in zip(before, after):
        assert np.array_equal(ea, eb) and bytes(oa) == bytes(ob)
    rec.dbf_ctu(raws[-1])                                   # a pair it already knows is still taken
    assert len(rec.dbf_edges(0)[0]) > len(before[0][0])


# ---------------------------------------------------------------------------------------------------------------- directed cells
def test_directed_cells_take_their_branches(built_lib):
    """tests/dbf_cells.py (what tests/test_gpu_dbf_cells.py runs on the device): EVERY cell takes the branch it was built for,
    the cells cover what they claim, and the oracle agrees with the restatement on them."""
    y, cb, cr, ev, eh, offs, cv, ch = dbf_cells.build()
    oy, ocb, ocr, bv, bh = spec_dbf.filter(y, cb, cr, ev, eh, offs)
    assert len(ev) >= 64 * 9 + 3 and len(eh) >= 64 * 9 + 3
    for d, (cs, br, e) in enumerate(((cv, bv, ev), (ch, bh, eh))):
        bad = dbf_cells.check_labels(cs, br)
        assert not bad, f"dir {d}: {len(bad)} cells left their branch, first: {bad[:4]}"
        luma = [c for c in cs if c.comp == 0 and c.group == "matrix"]
        for lp, lq in dbf_cells.LUMA_PAIRS:
            for bs in (1, 2):
                got = {(c.want, c.ext) for c in luma if (c.note["lp"], c.note["lq"], c.note["bs"]) == (lp, lq, bs)}
                want = {("off", None)} | ({("long", None)} if max(lp, lq) > 3 else set()) | ({("strong", None)} if lp > 2 else set())
                want |= {("weak", (a, b)) for a in (False, True) for b in (False, True)} if lp > 1 else {("weak", (False, False))}
                assert got == want, (d, lp, lq, bs, got ^ want)
        assert {c.gate for c in cs if c.group == "gate"} == {2, 3} and {c.clip for c in cs if c.clip} == {"lo", "hi"}
        for comp in (1, 2):
            cm = {(c.note["large"], c.note["ctb_b"], c.note["bs"], c.want) for c in cs if c.comp == comp and c.group == "cmatrix"}
            assert len(cm) == (6 if d == 0 else 12), (d, comp, cm)
            assert sum(c.want == "skip" for c in cs if c.comp == comp) >= 3
            if d == 0:
                assert {int(c.ux) % 2 for c in cs if c.comp == comp and c.group == "cmatrix"} == {0, 1}         # both alignments
        assert set(br["tc_idx"][[c.group == "table" for c in cs]].tolist()) >= set(dbf_cells.TC_TARGETS)
        assert set(br["beta_idx"][[c.group == "table" for c in cs]].tolist()) >= set(dbf_cells.BETA_TARGETS)
        # every pair index, and for any two indices a cell position whose filtered samples differ between them
        assert set(e["pad"].tolist()) == set(range(8)) and set(br["off"][br["changed"]].tolist()) == set(range(8)) - {dbf_cells.NEVER_LIVE}
        res = {}
        for c in cs:
            if c.group == "offsets":
                x0, y0 = c.ux * 4, c.uy * 4
                blk = oy[y0:y0 + 4, x0 - 8:x0 + 8] if d == 0 else oy[y0 - 8:y0 + 8, x0:x0 + 4].T
                res.setdefault(c.off, {})[c.note["slot"]] = blk.tobytes()
        for i in range(8):
            for j in range(i):
                assert any(res[i][s] != res[j][s] for s in res[i]), f"dir {d}: pairs {i} and {j} give the same samples everywhere"
    work = oracle_lib.HostPic(dbf_cells.W, dbf_cells.H, y.copy(), cb.copy(), cr.copy())
    oracle_lib.dbf_edges(work, ev, eh, offs)
    assert np.array_equal(work.y, oy) and np.array_equal(work.cb, ocb) and np.array_equal(work.cr, ocr)
    assert (oy != y).sum() > 5000 and (ocb != cb).sum() > 300 and (ocr != cr).sum() > 300


# one changed tap, index or term of the restatement each: (what, text in spec_dbf.py, replacement)
TAP_MUTATIONS = (
    ("(7,7) refMiddle reads p7 for p6", "mid = (sum(p[1:7]) + 2 * (p[0] + q[0]) + sum(q[1:7]) + 8) >> 4", "mid = (sum(p[1:6]) + p[7] + 2 * (p[0] + q[0]) + sum(q[1:7]) + 8) >> 4"),
    ("(5,5) refMiddle reads p5 for p4", "mid = (p[4] + p[3] + 2 * (p[2]", "mid = (p[5] + p[3] + 2 * (p[2]"),
    ("(7,5) refMiddle takes p1..p4", "mid = (sum(p[2:6]) + 2 * (p[1] + p[0] + q[0] + q[1]) + sum(q[2:6]) + 8) >> 4", "mid = (sum(p[1:5]) + 2 * (p[1] + p[0] + q[0] + q[1]) + sum(q[2:6]) + 8) >> 4"),
    ("(3,7) refMiddle reads p2 for p1", "+ p[0] + p[1] + sum(q[1:7]) + 8) >> 4", "+ p[0] + p[2] + sum(q[1:7]) + 8) >> 4"),
    ("(5,3) refMiddle reads p2 twice", "mid = (sum(p[0:4]) + sum(q[0:4]) + 4) >> 3", "mid = (sum(p[0:3]) + p[2] + sum(q[0:4]) + 4) >> 3"),
    ("refP from p[lp] twice", "ref_p, ref_q = (p[lp] + p[lp - 1] + 1) >> 1", "ref_p, ref_q = (p[lp] + p[lp] + 1) >> 1"),
    ("one f5 weight", "5: (58, 45, 32, 19, 6)", "5: (58, 44, 32, 19, 6)"),
    ("long decision without its lp == 7 term", "                sp += abs(ln.p(7) - ln.p(6) - ln.p(5) + ln.p(4))\n", "                sp += 0\n"),
    ("long decision without its lq == 7 term", "                sq += abs(ln.q(4) - ln.q(5) - ln.q(6) + ln.q(7))\n", "                sq += 0\n"),
    ("large-block dp term does not read p5", "dp0l = (dp0 + _d2(l0.p(5), l0.p(4), l0.p(3)) + 1) >> 1", "dp0l = (dp0 + _d2(l0.p(4), l0.p(4), l0.p(3)) + 1) >> 1"),
    ("luma strong p2 tap, weights of p3 and p2 swapped", "(2 * p[3] + 3 * p[2] + p[1] + p[0] + q[0] + 4) >> 3", "(3 * p[3] + 2 * p[2] + p[1] + p[0] + q[0] + 4) >> 3"),
    ("weak p1 extension does not read p2", "(((p2 + p0 + 1) >> 1) - p1 + delta) >> 1", "(((p1 + p0 + 1) >> 1) - p1 + delta) >> 1"),
    ("chroma strong p1 tap, weights of p3 and p2 swapped", "(2 * p[3] + p[2] + 2 * p[1] + p[0] + q[0] + q[1] + 4) >> 3", "(p[3] + 2 * p[2] + 2 * p[1] + p[0] + q[0] + q[1] + 4) >> 3"),
    ("chroma CTU-boundary q0 tap reads q2 for q3", "(2 * p[1] + p[0] + 2 * q[0] + q[1] + q[2] + q[3] + 4) >> 3", "(2 * p[1] + p[0] + 2 * q[0] + q[1] + q[2] + q[2] + 4) >> 3"),
    ("chroma weak filter reads p2 for p1", "((((q[0] - p[0]) << 2) + p[1] - q[1] + 4) >> 3)", "((((q[0] - p[0]) << 2) + p[2] - q[1] + 4) >> 3)"),
)


def test_directed_cells_pin_the_taps(built_lib):
    """The cells' sides are ramps so that a wrong tap shows.  Proof on the restatement, the stand-in for a kernel with the same
    slip: each single-tap change above must change samples of the cells' expected planes, both of the full lists and of the
    subset the dense-plane route runs.  (On flat sides, any taps with the right sum of weights give the same picture.)"""
    import types
    from pathlib import Path
    src = Path(spec_dbf.__file__).read_text()
    y, cb, cr, ev, eh, offs, _, _ = dbf_cells.build()
    dense = [e[(e["pad"] == dbf_cells.DENSE_IDX) & ~((e["comp"] > 0) & (e["ux"] % 2 == 1))] for e in (ev, eh)]
    routes = (("lists", ev, eh), ("dense subset", dense[0], dense[1]))
    want = [spec_dbf.filter(y, cb, cr, a, b, offs)[:3] for _, a, b in routes]
    for what, old, new in TAP_MUTATIONS:
        assert src.count(old) == 1, f"spec_dbf.py no longer holds the text of: {what}"
        m = types.ModuleType("spec_dbf_mutant")
        exec(compile(src.replace(old, new), "spec_dbf_mutant", "exec"), m.__dict__)
        for (route, a, b), w in zip(routes, want):
            got = m.filter(y, cb, cr, a, b, offs)[:3]
            n = sum(int((g != x).sum()) for g, x in zip(got, w))
            assert n >= 4, f"{what}: only {n} samples of the cells change ({route})"
