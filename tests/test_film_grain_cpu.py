"""CPU: film grain synthesis (include/ovvc_hip.h, "Film grain synthesis").  The numpy restatement (tests/spec_film_grain.py) against what
the reference's fg_grain_apply_pic wrote (tests/golden/film_grain/*.ovg, tools/fg_golden/gen_fg.c), the census of those cases, the host
side (ovhip_fg_derive, ovhip_fg_database, the seeds) against the restatement and the recorded fields, every refusal, and the
frame-level setter on a dry frame.  tests/test_gpu_film_grain.py runs the kernel.  Every comparison is exact: integers."""
import ctypes as C

import numpy as np
import pytest

import golden_io
import spec_film_grain as sf
from openvvc_amd import capi

G = golden_io.load("film_grain/fg.ovg")
N_CASES = sum(1 for k in G if k.endswith("_geom"))
PLANES = ("y", "cb", "cr")


def case(k):
    w, h, poc = (int(v) for v in G[f"c{k}_geom"])
    return {"w": w, "h": h, "poc": poc, "sei": sf.parse(G[f"c{k}_sei"]), "after": G[f"c{k}_sei_after"],
            "src": tuple(G[f"c{k}_s{p}"] for p in PLANES), "exp": tuple(G[f"c{k}_d{p}"] for p in PLANES)}


def c_params(sei) -> capi.FgParams:
    return capi.fg_params(**{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in sei.items()})


def flat_of(p: capi.FgParams) -> np.ndarray:
    return sf.flatten({k: np.asarray(v) if isinstance(v, list) else v for k, v in capi.fg_params_dict(p).items()})


def block_table(src, table):
    """per 8x8 block of a plane: the model's (valid, scale, h, v) and the block average"""
    h, w = src.shape
    nbx, nby = (w + 7) // 8, (h + 7) // 8
    pad = np.zeros((nby * 8, nbx * 8), np.int64)
    pad[:h, :w] = src
    count = np.outer(np.minimum(8, h - 8 * np.arange(nby)), np.minimum(8, w - 8 * np.arange(nbx)))
    avg = np.minimum((pad.reshape(nby, 8, nbx, 8).sum(axis=(1, 3)) // count) >> 2, 255)
    return table[avg], avg


def test_census():
    """what tools/fg_golden/gen_fg.c asserts when it writes the fixture, from the file"""
    cells, sizes, nval, nint, log2, pocs = set(), set(), set(), set(), set(), set()
    none_beside_grain = avg0_last_wins = clip0 = clip1023 = absent = 0
    for k in range(N_CASES):
        c = case(k)
        sei = c["sei"]
        sizes.add((c["w"], c["h"])); log2.add(sei["log2_scale"]); pocs.add(c["poc"])
        present, table, _ = sf.derive(sei)
        for p in range(3):
            ph, pw = c["src"][p].shape
            assert pw % 16 in (0, 8, 9, 10, 11, 12, 13, 14, 15) and ph % 16 in (0, 8, 9, 10, 11, 12, 13, 14, 15), "the reference is undefined there"
            if not present[p]:
                absent += 1
                assert np.array_equal(c["src"][p], c["exp"][p])
                continue
            nval.add(int(sei["num_model_values"][p])); nint.add(int(sei["num_intervals"][p]))
            e, avg = block_table(c["src"][p], table[p])
            grained = (e[..., 0] != 0) & (e[..., 1] != 0)
            cells |= {(int(a), int(b)) for a, b in zip(e[..., 2][grained], e[..., 3][grained])} if p == 0 else set()
            none = e[..., 0] == 0
            beside = np.zeros_like(none)
            beside[:, 1:] |= grained[:, :-1]
            beside[:, :-1] |= grained[:, 1:]
            none_beside_grain += int((none & beside).sum())
            if sei["num_intervals"][p] < 8 and sei["lower"][p, 0] > 0:
                avg0_last_wins += int(((avg == 0) & (e[..., 0] != 0) & (e[..., 1] == 0)).sum())
            # unclipped result: grain << 2 is a multiple of 4
            s, d = c["src"][p].astype(np.int64), c["exp"][p].astype(np.int64)
            clip0 += int(((d == 0) & (s & 3 != 0)).sum())
            clip1023 += int(((d == 1023) & (s & 3 != 3)).sum())
    assert cells == {(a, b) for a in range(13) for b in range(13)}                       # luma alone walks all 169 cells
    assert {(88, 56), (92, 60), (64, 16), (16, 16)} <= sizes
    assert any(h >= 48 and w >= 96 for w, h in sizes)                                   # >= 3 stripes, >= 6 blocks of 16 per row
    assert nval == {1, 2, 3} and {1, 3, 8} <= nint
    assert none_beside_grain >= 50 and avg0_last_wins > 0
    assert {2, 7} <= log2 and clip0 >= 20 and clip1023 >= 20 and absent > 0
    assert {0, 5, 255, 256, -3, 100000} <= pocs


def test_three_consecutive_calls_drift():
    """the last three cases are one struct handed to three pictures: chroma 100 / 4 / 6 -> 50 / 8 / 12 -> 25 / 14 / 14 -> 12 / 14 / 14"""
    seq = [case(k) for k in range(N_CASES - 3, N_CASES)]
    want = [(100, 4, 6), (50, 8, 12), (25, 14, 14)]
    for c, w in zip(seq, want):
        assert tuple(int(v) for v in c["sei"]["value"][1, 0]) == w and tuple(int(v) for v in c["sei"]["value"][2, 3]) == w
    assert np.array_equal(sf.flatten(seq[1]["sei"]), seq[0]["after"]) and np.array_equal(sf.flatten(seq[2]["sei"]), seq[1]["after"])
    assert tuple(int(v) for v in sf.parse(seq[2]["after"])["value"][1, 0]) == (12, 14, 14)
    assert np.array_equal(sf.parse(seq[2]["after"])["value"][0], seq[0]["sei"]["value"][0])          # luma does not drift


@pytest.mark.parametrize("k", range(N_CASES))
def test_restatement_equals_the_reference(k):
    c = case(k)
    got, after = sf.apply(c["src"], c["sei"], c["poc"])
    for p, name in enumerate(PLANES):
        assert got[p].tobytes() == c["exp"][p].tobytes(), (k, name, int((got[p] != c["exp"][p]).sum()))
    assert np.array_equal(sf.flatten(after), c["after"])


def test_database_equals_the_reference(built_lib):
    db = np.frombuffer(C.string_at(built_lib.ovhip_fg_database(), capi.FG_DB_BYTES), np.int8)
    want = golden_io.load("film_grain/fg_db.ovg")["db"]
    assert want.shape == (13, 13, 64, 64) and db.tobytes() == want.tobytes()
    assert int(want.min()) == -127 and int(want.max()) == 127                           # the reference's signed clip is symmetric


def test_database_from_several_threads(built_lib):
    import threading
    got = []
    ts = [threading.Thread(target=lambda: got.append(built_lib.ovhip_fg_database())) for _ in range(8)]
    [t.start() for t in ts]; [t.join() for t in ts]
    assert len(set(got)) == 1 and got[0]


def test_seeds(built_lib):
    _, seed_lut = sf.tables()
    for poc in (0, 5, 255, 256, -3, 100000):
        for c in range(3):
            assert built_lib.ovhip_fg_seed(poc, 0, c) == sf.start_seed(poc, c)
    assert built_lib.ovhip_fg_seed(7, 3, 1) == sf.start_seed(7, 1, 3)
    x = int(seed_lut[17])
    for _ in range(200):
        assert built_lib.ovhip_fg_prng(x) == sf.prng(x)
        x = sf.prng(x)


def test_stripe_seeds_jump_to_where_stepping_gets(built_lib):
    """every stripe's start value against the restatement's step-by-step sequence: few stripes (stepped), many (the affine jump), two
    widths in turn and a third (the per-thread table is rebuilt), one block per stripe"""
    _, seed_lut = sf.tables()
    for start, per_stripe, stripes in ((int(seed_lut[0]), 240, 135), (int(seed_lut[85]), 120, 68), (int(seed_lut[170]), 120, 68), (int(seed_lut[3]), 240, 135),
                                       (int(seed_lut[9]), 6, 3), (int(seed_lut[200]), 26, 15), (0xFFFFFFFF, 1, 40), (0, 7, 9), (int(seed_lut[77]), 1024, 5)):
        out = (C.c_uint32 * stripes)()
        built_lib.ovhip_fg_stripe_seeds(start, per_stripe, stripes, out)
        want = sf.block_seeds(start, per_stripe * (stripes - 1) + 1)[::per_stripe]
        assert [int(v) for v in out] == [int(v) for v in want], (start, per_stripe, stripes)


@pytest.mark.parametrize("k", range(N_CASES))
def test_derive_equals_the_restatement_and_the_recorded_fields(built_lib, k):
    c = case(k)
    r, model, after = capi.fg_derive(built_lib, c_params(c["sei"]))
    present, table, _ = sf.derive(c["sei"])
    assert r == 0 and model.log2_scale == c["sei"]["log2_scale"] and list(model.present) == [int(v) for v in present]
    assert np.array_equal(np.ctypeslib.as_array(model.entry), sf.packed_table(table))
    assert np.array_equal(flat_of(after), c["after"])
    # in place, and without `after`
    p = c_params(c["sei"])
    m2 = capi.FgModel()
    assert built_lib.ovhip_fg_derive(C.byref(p), C.byref(m2), C.byref(p)) == 0 and np.array_equal(flat_of(p), c["after"])
    assert built_lib.ovhip_fg_derive(C.byref(c_params(c["sei"])), C.byref(m2), None) == 0 and bytes(m2) == bytes(model)


def _refused(lib, sei, code):
    p = c_params(sei)
    model, after = capi.FgModel(), capi.FgParams()
    C.memset(C.byref(model), 0xA5, C.sizeof(model)); C.memset(C.byref(after), 0xA5, C.sizeof(after))
    assert lib.ovhip_fg_derive(C.byref(p), C.byref(model), C.byref(after)) == code
    assert bytes(model) == b"\xa5" * C.sizeof(model) and bytes(after) == b"\xa5" * C.sizeof(after), "a refusal writes nothing"
    assert np.array_equal(flat_of(p), sf.flatten(sei))


def test_derive_refuses(built_lib):
    lib = built_lib
    _refused(lib, sf.make_sei(model_id=1), capi.OVHIP_EUNSUP)
    _refused(lib, sf.make_sei(blending_mode=1), capi.OVHIP_EUNSUP)
    # a luma cut-off outside 2..14 under a non-zero scale
    for n, bad in ((1, 1), (1, 15), (2, 0), (2, 15)):
        s = sf.make_sei()
        s["value"][0, 3, n] = bad
        _refused(lib, s, capi.OVHIP_EINVAL)
    # three model values, three intervals from 32 up: average 0 falls to the last unused interval, whose cut-offs are 0 -> h = 254
    s = sf.make_sei(comps=((3, 3, 200, 8, 8), None, None))
    s["lower"][0, :3], s["upper"][0, :3] = (32, 100, 180), (99, 179, 255)
    s["value"][0, 3:] = 0
    s["value"][0, 7] = (9, 0, 0)
    _refused(lib, s, capi.OVHIP_EINVAL)
    # ... with scale 0 the product is 0 whatever the cut-offs: accepted, grain 0
    s["value"][0, 7] = (0, 0, 0)
    r, model, _ = capi.fg_derive(lib, c_params(s))
    assert r == 0 and model.entry[0][0] == capi.FG_VALID and model.entry[0][1] == 0 and model.entry[0][32] != 0
    # an interval nothing selects may hold anything
    s = sf.make_sei(comps=((8, 3, 200, 8, 8), None, None))
    s["lower"][0, 4], s["upper"][0, 4] = 9, 8
    s["value"][0, 4] = (50, 99, -4)
    assert capi.fg_derive(lib, c_params(s))[0] == 0
    # chroma is clamped, never refused
    s = sf.make_sei(comps=(None, (8, 3, 200, 8, 8), None))
    s["value"][1, 2] = (77, 0, 40)
    r, model, after = capi.fg_derive(lib, c_params(s))
    assert r == 0 and list(after.comp[1].value[2]) == [38, 2, 14]
    # a cancelled SEI is derived (the reference mutates it all the same) and copies the picture
    s = sf.make_sei(comps=((8, 3, 200, 8, 8), (3, 2, 100, 4, 6), None), cancel=1)
    r, model, after = capi.fg_derive(lib, c_params(s))
    assert r == 0 and list(model.present) == [0, 0, 0] and np.array_equal(flat_of(after), sf.flatten(sf.derive(s)[2]))
    assert after.comp[1].value[0][0] == 50
    m = capi.FgModel()
    assert lib.ovhip_fg_derive(None, C.byref(m), None) == capi.OVHIP_EINVAL and lib.ovhip_fg_derive(C.byref(c_params(s)), None, None) == capi.OVHIP_EINVAL


def test_launch_refuses_without_a_context(built_lib):
    a, b, m = capi.Pic(), capi.Pic(), capi.FgModel()
    out = (C.c_uint8 * 16)()
    assert built_lib.ovhip_film_grain_launch(None, C.byref(a), C.byref(m), 0, 0, C.byref(b)) == capi.OVHIP_EINVAL
    assert built_lib.ovhip_pic_digest_grain(None, C.byref(a), C.byref(m), 0, None, out) == capi.OVHIP_EINVAL
    assert built_lib.ovhip_pic_output_grain(None, C.byref(a), C.byref(m), 0, None, out) == capi.OVHIP_EINVAL
    assert built_lib.ovhip_frame_set_film_grain(None, None, 0) == capi.OVHIP_EINVAL
    assert built_lib.ovhip_stream_set_film_grain(None, None) == capi.OVHIP_EINVAL


def test_dry_frame_accepts_film_grain_and_refuses_it_beside_an_output_scale(built_lib):
    """a DPB on a counting memory back-end (no device): the setter is accepted, the picture is submitted and published as before;
    grain and an output scale exclude each other, whichever is set second"""
    from test_dpb_cpu import FakeMem
    lib = built_lib
    mem, h = FakeMem(), C.c_void_p()
    assert lib.ovhip_dpb_create_ex(C.byref(h), 1, C.byref(mem.ops)) == 0
    f = C.c_void_p()
    assert lib.ovhip_frame_create(h, 0, 64, 64, C.byref(f)) == 0
    fg = c_params(sf.make_sei())
    assert lib.ovhip_frame_set_film_grain(f, C.byref(fg), 5) == 0
    assert lib.ovhip_frame_begin_tag(f, C.c_void_p(0x10), 1) == 0
    p = capi.JobParams()
    out = capi.FrameOutput()
    out.mode = capi.OUT_DIGEST
    assert lib.ovhip_frame_submit(f, None, None, C.byref(p), C.byref(out)) == 0
    assert bytes(out.digest) == bytes(16)                                       # dry: no output
    dev, pic = C.c_int(-1), capi.Pic()
    assert lib.ovhip_dpb_lookup(h, C.c_void_p(0x10), C.byref(dev), C.byref(pic)) == 0 and (pic.w, pic.h) == (64, 64)
    # the refusals of the derivation come back from the setter and leave the setting as it was
    assert lib.ovhip_frame_set_film_grain(f, C.byref(c_params(sf.make_sei(model_id=2))), 5) == capi.OVHIP_EUNSUP
    # grain is set: an output scale is refused; switching the scale off is not
    assert lib.ovhip_frame_set_output_scale(f, 128, 128, None) == capi.OVHIP_EUNSUP
    assert lib.ovhip_frame_set_output_scale(f, 0, 0, None) == 0
    # the other order
    assert lib.ovhip_frame_set_film_grain(f, None, 0) == 0
    assert lib.ovhip_frame_set_output_scale(f, 128, 128, None) == 0
    assert lib.ovhip_frame_set_film_grain(f, C.byref(fg), 5) == capi.OVHIP_EUNSUP
    assert lib.ovhip_frame_set_film_grain(f, None, 0) == 0                      # switching grain off is not refused
    assert lib.ovhip_frame_set_output_scale(f, 0, 0, None) == 0
    assert lib.ovhip_frame_set_film_grain(f, C.byref(fg), 6) == 0
    lib.ovhip_frame_destroy(f)
    lib.ovhip_dpb_destroy(h)
