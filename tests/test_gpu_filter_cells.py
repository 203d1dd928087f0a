"""GPU: k_sao and k_alf on the enumerated cells (tests/golden/sao_cells_*.ovg, alf_cells_*.ovg: the reference's own SAO and ALF slots on
content and parameters chosen so that every decision of the two kernels is reached; tests/filter_census.py says which, and
tests/test_oracle_golden.py asserts it).  Every file runs through four routes, sample for sample against the reference, into
destinations that start as a sentinel picture:
  kernel  ovhip_sao_launch / ovhip_alf_launch on pictures whose strides are multiples of 16 samples (the 16-byte paths)
  rows    ovhip_sao_launch_rows / ovhip_alf_launch_rows over two partitions of the rows
  view    the picture is the left W columns of a (W + 2)-wide allocation: no stride is a multiple of 4 samples, every load and
          store goes sample by sample, every ALF tile is staged through clamped coordinates
  job     engine.Job with STAGE_SAO | STAGE_ALF
SAO runs at CTU 128, 64 and 32, ALF at 128 and 64 (ALF at CTU 32 is refused: tests/test_gpu_ctu_sizes.py)."""
import ctypes as C
import types

import numpy as np
import pytest

import filter_census as fc
import golden_cases
from oracle_lib import HostPic
from openvvc_amd import capi, engine

pytestmark = pytest.mark.gpu
SENTINEL = 777
SAO_FILES, ALF_FILES = golden_cases.sao_cell_files(), golden_cases.alf_cell_files()


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cells():
    """{file: (input, parameters, the reference's picture, log2 of the CTU size)}, read once"""
    out = {}
    for f in SAO_FILES + ALF_FILES:
        (pic, prm, exp), = golden_cases.sao_cases(f) if f in SAO_FILES else golden_cases.alf_cases(f)
        out[f] = (pic, prm, exp, golden_cases.filter_cell_ctu(f))
    return out


class Pool:
    """device buffers and pictures of one test, freed when it ends"""
    def __init__(self, ctx):
        self.ctx, self.items = ctx, []

    def keep(self, it):
        self.items.append(it)
        return it


@pytest.fixture
def pool(ctx):
    p = Pool(ctx)
    yield p
    ctx.sync()
    for it in p.items:
        it.free()


def _wide(ctx, pool, planes, stride_y, rng):
    """(allocation, its start planes, view): the planes are the left columns of a picture stride_y samples wide whose other columns
    hold random samples -- a kernel that reads them computes another picture, one that writes them is found out"""
    h, w = planes[0].shape
    big = []
    for k, p in enumerate(planes):
        b = rng.integers(0, 1024, (p.shape[0], stride_y >> (k > 0)), dtype=np.uint16)
        b[:, :p.shape[1]] = p
        big.append(b)
    d = pool.keep(ctx.upload_pic(*big))
    assert (d.s.stride_y, d.s.stride_c) == (stride_y, stride_y // 2)
    return d, big, engine.DevPic(ctx, capi.Pic(d.s.y, d.s.cb, d.s.cr, w, h, d.s.stride_y, d.s.stride_c), owns=False)


def _sentinel(pic):
    return [np.full_like(p, SENTINEL) for p in pic.planes()]


def _check(d, start, want, what, rows=None):
    """the view's samples equal `want` (in the luma rows `rows` = [(r0, r1)], the sentinel elsewhere); the columns outside it are untouched"""
    for name, g, s, p in zip(("Y", "Cb", "Cr"), d.download(), start, want.planes()):
        w, sh = p.shape[1], name != "Y"
        exp = p
        if rows is not None:
            exp = np.full_like(p, SENTINEL)
            for r0, r1 in rows:
                exp[r0 >> sh:r1 >> sh] = p[r0 >> sh:r1 >> sh]
        bad = np.argwhere(g[:, :w] != exp)
        assert len(bad) == 0, f"{what}, plane {name}: {len(bad)} samples differ from the reference, first at (y, x) {bad[:6].tolist()}"
        assert np.array_equal(g[:, w:], s[:, w:]), f"{what}, plane {name}: columns outside the picture changed"


def _launch(ctx, pool, f, cells, dst, src, rows=None):
    pic, prm, _, l2 = cells[f]
    if f in SAO_FILES:
        d_prm = pool.keep(ctx.upload(prm))
        for r0, r1 in rows or [(0, pic.h)]:
            ctx._chk(ctx.lib.ovhip_sao_launch_rows(ctx.h, C.byref(dst.s), C.byref(src.s), d_prm.ptr, l2, r0, r1), "sao_launch_rows")
    else:
        dalf = pool.keep(engine.DevAlf(ctx, prm, pic.w, pic.h, log2_ctu=l2))
        for r0, r1 in rows or [(0, pic.h)]:
            ctx._chk(ctx.lib.ovhip_alf_launch_rows(ctx.h, C.byref(dst.s), C.byref(src.s), C.byref(dalf.s), r0, r1), "alf_launch_rows")
    ctx.sync()


def _gpu_files():
    return SAO_FILES + [f for f in ALF_FILES if golden_cases.filter_cell_ctu(f) >= 6]


def _aligned(w):
    return (w + 15) & ~15


@pytest.mark.parametrize("f", _gpu_files())
def test_kernel(ctx, pool, cells, f):
    """ctx.sao / ctx.alf (the whole-picture launches) on strides that are multiples of 16 (luma) and 8 (chroma) samples"""
    pic, prm, exp, l2 = cells[f]
    rng = np.random.default_rng(11)
    _, _, src = _wide(ctx, pool, pic.planes(), _aligned(pic.w), rng)
    d, start, dst = _wide(ctx, pool, _sentinel(pic), _aligned(pic.w), rng)
    if f in SAO_FILES:
        ctx.sao(dst, src, pool.keep(ctx.upload(prm)), l2)
    else:
        ctx.alf(dst, src, pool.keep(engine.DevAlf(ctx, prm, pic.w, pic.h, log2_ctu=l2)))
    ctx.sync()
    _check(d, start, exp, f"{f} at CTU {1 << l2}")


def _partitions(h, ctu):
    """(the cut at the CTU rows, the cut 8 rows above every CTU row of full height: 4 rows above the virtual boundary at ctu - 4)"""
    out = []
    for cuts in (range(ctu, h, ctu), [b + ctu - 8 for b in range(0, h - ctu + 1, ctu)]):
        edges = [0] + [c for c in cuts if 0 < c < h] + [h]
        out.append(list(zip(edges[:-1], edges[1:])))
    return out


@pytest.mark.parametrize("f", _gpu_files())
def test_rows(ctx, pool, cells, f):
    """ovhip_sao_launch_rows / ovhip_alf_launch_rows: every partition of the rows gives the whole-picture result, and a launch writes
    its window only -- the second partition runs every other window first: the rows between them keep the sentinel"""
    pic, prm, exp, l2 = cells[f]
    ctu = 1 << l2
    by_ctu, by_vb = _partitions(pic.h, ctu)
    vbs = [b + ctu - 4 for b in range(0, pic.h - ctu + 1, ctu)]
    assert all(r0 % 8 == 0 for r0, _ in by_vb) and all(min(abs(r0 - v) for v in vbs) <= 4 for r0, _ in by_vb[1:])
    assert len(by_vb) == 1 + len(vbs) or by_vb[-1][0] + 8 == pic.h
    rng = np.random.default_rng(12)
    _, _, src = _wide(ctx, pool, pic.planes(), _aligned(pic.w), rng)
    d, start, dst = _wide(ctx, pool, _sentinel(pic), _aligned(pic.w), rng)
    _launch(ctx, pool, f, cells, dst, src, by_ctu)
    _check(d, start, exp, f"{f}, windows {by_ctu}")
    d, start, dst = _wide(ctx, pool, _sentinel(pic), _aligned(pic.w), rng)
    _launch(ctx, pool, f, cells, dst, src, by_vb[0::2])
    _check(d, start, exp, f"{f}, windows {by_vb[0::2]} alone", rows=by_vb[0::2])
    _launch(ctx, pool, f, cells, dst, src, by_vb[1::2])
    _check(d, start, exp, f"{f}, windows {by_vb}")


@pytest.mark.parametrize("f", _gpu_files())
def test_view(ctx, pool, cells, f):
    """the pictures are the left W columns of (W + 2)-wide ones: luma stride W + 2, chroma W / 2 + 1, neither a multiple of 4"""
    pic, prm, exp, l2 = cells[f]
    assert (pic.w + 2) % 4 and (pic.w // 2 + 1) % 4
    rng = np.random.default_rng(13)
    _, _, src = _wide(ctx, pool, pic.planes(), pic.w + 2, rng)
    d, start, dst = _wide(ctx, pool, _sentinel(pic), pic.w + 2, rng)
    _launch(ctx, pool, f, cells, dst, src)
    _check(d, start, exp, f"{f}, {pic.w}-wide view of {pic.w + 2}")


def _job(ctx, pic, sao_prm, alf, l2):
    job = engine.Job(ctx, pic.w, pic.h)
    job.begin()
    params = job.make_params(types.SimpleNamespace(sao_params=sao_prm, alf=alf, lmcs=None), l2, capi.STAGE_SAO | capi.STAGE_ALF)
    dst = ctx.upload_pic(pic.y, pic.cb, pic.cr)
    try:
        job.flush(dst, [], None, params)
        job.wait()
        return dst.download()
    finally:
        job.close()
        dst.free()


def _same(got, want, what):
    for name, a, b in zip(("Y", "Cb", "Cr"), got, want.planes()):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what}, plane {name}: {len(bad)} samples differ, first at (y, x) {bad[:6].tolist()}"


# the ALF tables a SAO picture runs with in the job: a file of the same CTU size and CTU grid (the entry pictures go together, border flags and all)
_JOB_TABLES = {"sao_cells_sao_00.ovg": "alf_cells_taps_01.ovg", "sao_cells_sao_01.ovg": "alf_cells_taps_02.ovg",
               "sao_cells_sao64_00.ovg": "alf_cells_entry64_00.ovg", "sao_cells_entry64_00.ovg": "alf_cells_entry64_00.ovg"}


@pytest.mark.parametrize("f", [f for f in SAO_FILES if f in _JOB_TABLES])
def test_job_sao_cells(ctx, cells, f):
    """STAGE_SAO | STAGE_ALF on a SAO picture with an ALF picture's tables; expected: the census's restatement of ALF (equal to the
    reference on every ALF fixture) of its restatement of SAO (equal to the reference on every SAO fixture, this picture included)"""
    pic, prm, exp, l2 = cells[f]
    _, alf, _, l2a = cells[_JOB_TABLES[f]]
    ctu = 1 << l2
    assert l2a == l2 and len(alf["ctus"]) == len(prm) == -(-pic.w // ctu) * -(-pic.h // ctu)
    mid, _ = fc.sao(pic, prm, l2)
    _same(mid.planes(), exp, "the restated SAO")
    want, _ = fc.alf(mid, alf, l2, discriminate=False)
    assert (want.y != mid.y).sum() > 1000
    _same(_job(ctx, pic, prm, alf, l2), want, f"job with SAO and ALF on {f} with the tables of {_JOB_TABLES[f]}")


@pytest.mark.parametrize("f", [f for f in ALF_FILES if golden_cases.filter_cell_ctu(f) >= 6])
def test_job_alf_cells(ctx, cells, f):
    """STAGE_SAO | STAGE_ALF on an ALF picture with SAO off in every CTU (the SAO stage copies): the reference's ALF picture"""
    pic, alf, exp, l2 = cells[f]
    prm = np.zeros(len(alf["ctus"]), capi.SAO_CTU_DTYPE)
    _same(_job(ctx, pic, prm, alf, l2), exp, f"job with SAO off and ALF on {f}")


def test_routes_enter_every_path_the_census_claims(ctx, pool, cells):
    """The load, store and staging paths of both kernels are chosen from the strides and from where a lane or tile lies; the census
    restates those selectors (filter_census.sao_paths / alf_paths).  From the strides of the pictures the routes above really
    allocate: kernel and rows enter the 16-byte paths and, in the last group of a row, the ragged one; view enters the scalar and the
    clamped paths for every lane and tile and nothing else.  Between the routes every path label is entered."""
    seen_sao, seen_alf = set(), set()
    for f in _gpu_files():
        pic, prm, _, l2 = cells[f]
        rng = np.random.default_rng(14)
        for route, stride in (("kernel", _aligned(pic.w)), ("view", pic.w + 2)):
            d, _, v = _wide(ctx, pool, pic.planes(), stride, rng)
            assert all(p % 16 == 0 for p in (d.s.y, d.s.cb, d.s.cr)), "the planes of an allocation start 16-byte aligned"
            if f in SAO_FILES:
                paths = fc.sao_paths(pic.w, pic.h, v.s.stride_y, v.s.stride_c)
                ragged = {(p, "ragged") for p in range(3) if (pic.w >> (p > 0)) % 8}
                assert paths == {(p, "16-byte" if route == "kernel" else "scalar") for p in range(3)} | ragged, (f, route)
                seen_sao |= paths
            else:
                paths, sides = fc.alf_paths(pic.w, pic.h, v.s.stride_y, v.s.stride_c, prm, l2)
                staged = {p for p in paths if p[0] in ("luma", "chroma") and p[1] in ("16-byte", "clamped")}
                if route == "view":
                    assert staged and all(p[1:] == ("clamped", "scalar") for p in staged), (f, sorted(staged))
                else:
                    assert {p[1:] for p in staged if p[0] == "luma"} >= {("16-byte", "8-byte"), ("clamped", "8-byte")}, (f, sorted(staged))
                seen_alf |= paths | {("sides",) + s for s in sides}
        ctx.sync()
        for it in pool.items:
            it.free()
        pool.items.clear()
    assert seen_sao == {(p, k) for p in range(3) for k in ("16-byte", "scalar", "ragged")}
    # (a tile staged 16 bytes at a time lies inside the picture on a stride that is a multiple of 8: it never stores sample by sample)
    want = {(pl, st, sto) for pl in ("luma", "chroma") for st in ("16-byte", "clamped") for sto in ("8-byte", "scalar")} - {("luma", "16-byte", "scalar"), ("chroma", "16-byte", "scalar")}
    want |= {("luma", "copy", "scalar"), ("chroma", "none", "8-byte"), ("chroma", "none", "scalar"), ("cc", "inside"), ("cc", "clamped")}
    assert {p for p in seen_alf if p[0] != "sides"} == want, sorted(want ^ {p for p in seen_alf if p[0] != "sides"})
    one_side = {("sides",) + tuple(i == k for i in range(4)) for k in range(4)}
    assert one_side | {("sides", False, False, False, False)} <= seen_alf
