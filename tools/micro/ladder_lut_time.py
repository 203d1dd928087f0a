"""Output ladder through a colour table (k_ladder_lut) on the device: the numbers LABBOOK 37 quotes.

    python tools/micro/ladder_lut_time.py launches [N] [smooth|noise|both] [0|1|both]
        per picture (3840x2160, a smooth ramp or noise) and destination chroma location (0: co-sited, the halo column on; 1: centred):
        warm-up, then N (default 100) rounds of ONE ovhip_ladder_lut_launch -> NV12 at 1920x1080, 1280x720, 960x540 and 640x360 through
        a 33-point table, then the EIGHT launches that make the same four surfaces without it (ovhip_output_reduce_launch into a 16-bit
        picture + ovhip_surface_lut_launch, per rung), each side between two events on the context's stream, alternating in one
        process: prints the medians and percentiles of the event times (which hold a few microseconds of the events' own) and the
        bytes the algorithm has to move.  The surfaces of both sides are compared for equality first.  Run it under
        `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python ...` (one picture and one location per run) for the
        isolated kernel times, and read them with
    python tools/micro/ladder_lut_time.py trace <dir or kernel_trace.csv>
        the median, minimum, percentiles and count of end - start per kernel and grid size of such a trace (no device needed); the sum
        of the eight medians beside k_ladder_lut's; the sum of the eight per round with its own percentiles -- the run-to-run spread
        that is the only margin of LABBOOK 37's condition; the bytes, TB/s and the share of the 8 TB/s HBM peak.
"""
import csv
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
HBM_PEAK = 8.0e12
SRC = (3840, 2160)
RUNGS = [(1920, 1080), (1280, 720), (960, 540), (640, 360)]
TABLE = 33
CONV = (9, 0, 0, 1, 0)                                       # BT.2020 limited, chroma left -> BT.709 limited; + the destination's location


def pic_bytes(s):
    return s[0] * s[1] * 3                                  # 4:2:0, 16-bit samples


def nv12_bytes(s):
    return s[0] * s[1] * 3 // 2


def ladder_moved():
    """the source read once + every surface written once (the table stays in cache)"""
    return pic_bytes(SRC) + sum(nv12_bytes(d) for d in RUNGS)


def parent_moved():
    """per rung: the source read, the 16-bit picture written and read again, the surface written"""
    return sum(pic_bytes(SRC) + 2 * pic_bytes(d) + nv12_bytes(d) for d in RUNGS)


def planes(kind, w, h, seed):
    rs = np.random.RandomState(seed)
    shapes = ((h, w), (h // 2, w // 2), (h // 2, w // 2))
    if kind == "noise":
        return [rs.randint(0, 1024, s).astype(np.uint16) for s in shapes]
    out = []
    for k, (hh, ww) in enumerate(shapes):                     # a ramp per plane along x, y and the diagonal, + 4 of noise
        x, y = np.meshgrid(np.arange(ww) / (ww - 1.0), np.arange(hh) / (hh - 1.0))
        v = ((1.0, 0.0), (0.0, 1.0), (0.5, 0.5))[k]
        out.append(np.clip(np.rint((v[0] * x + v[1] * y) * 1023 + rs.randint(-4, 5, (hh, ww))), 0, 1023).astype(np.uint16))
    return out


def launches(n, kinds, locs):
    import torch
    from openvvc_amd import capi, engine
    ctx = engine.Context(0)
    fmt = engine.surface_format(capi.SURF_NV12)
    table = np.random.default_rng(37).integers(0, 1024, (TABLE, TABLE, TABLE, 3), dtype=np.uint16)
    lut = engine.RgbLut(ctx, table, 1023)
    stream = torch.cuda.ExternalStream(ctx.stream)
    bufs = [ctx.alloc(nv12_bytes(d)) for d in RUNGS]
    other = [ctx.alloc(nv12_bytes(d)) for d in RUNGS]
    mids = [ctx.new_pic(*d) for d in RUNGS]
    rungs = [engine.ladder_rung(d[0], d[1], fmt, b.ptr.value, b.nbytes) for d, b in zip(RUNGS, bufs)]
    for kind in kinds:
        pic = ctx.upload_pic(*planes(kind, SRC[0], SRC[1], 37))
        for loc in locs:
            conv = engine.surface_conv(*CONV, loc)

            def ladder():
                pic.ladder_into(rungs, lut=lut, conv=conv)

            def eight():
                for m, o in zip(mids, other):
                    pic.reduce_into(m)
                    m.surface_into(o.ptr.value, o.nbytes, fmt, lut=lut, conv=conv)

            ladder(); eight(); ctx.sync()
            for b, o in zip(bufs, other):
                assert b.download().tobytes() == o.download().tobytes(), "the ladder's surfaces differ from surface_lut(reduce())"
            sides = [("k_ladder_lut, one launch", ladder_moved(), ladder), ("k_output_reduce + k_surface_lut, eight launches", parent_moved(), eight)]
            for _ in range(10):
                for _name, _nb, fn in sides:
                    fn()
            ctx.sync()
            evs = {name: [] for name, _nb, _fn in sides}
            for _ in range(n):                               # alternating, in one process
                for name, _nb, fn in sides:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    fn()
                    b.record(stream)
                    evs[name].append((a, b))
            ctx.sync()
            for name, nb, _fn in sides:
                us = np.array([1e3 * a.elapsed_time(b) for a, b in evs[name]])
                print(f"{kind}, destination location {loc}: {SRC[0]}x{SRC[1]} -> NV12 x {len(RUNGS)}, {name}: {n} rounds, median {np.median(us):.1f} us, "
                      f"min {us.min():.1f} us, 10th..90th percentile {np.percentile(us, 10):.1f}..{np.percentile(us, 90):.1f} us between events; "
                      f"{nb / 1e6:.2f} MB to move", flush=True)
        pic.free()
    lut.close()
    [p.free() for p in mids]
    [b.free() for b in bufs + other]
    ctx.close()


def trace(path):
    p = Path(path)
    files = [p] if p.is_file() else sorted(p.rglob("*kernel_trace.csv"))
    if not files:
        sys.exit(f"{path}: no *kernel_trace.csv")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                for k in ("k_ladder_lut", "k_output_reduce", "k_surface_lut"):
                    if k in row["Kernel_Name"]:
                        rows.append((int(row["Start_Timestamp"]), k, int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0),
                                     (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows.sort()
    times = {}
    for _t, k, grid, us in rows:
        times.setdefault((k, grid), []).append(us)
    med = {}
    for key, us in sorted(times.items()):
        us = np.array(us)
        med[key] = float(np.median(us))
        print(f"{key[0]} grid {key[1]}: {len(us)} dispatches, median {np.median(us):.1f} us, min {us.min():.1f} us, 10th..90th percentile "
              f"{np.percentile(us, 10):.1f}..{np.percentile(us, 90):.1f} us")
    # the rounds: every run of eight reduce / surface_lut dispatches between two ladder dispatches
    sums, cur = [], []
    for _t, k, _grid, us in rows:
        if k == "k_ladder_lut":
            if len(cur) == 2 * len(RUNGS):
                sums.append(sum(cur))
            cur = []
        else:
            cur.append(us)
    if len(cur) == 2 * len(RUNGS):
        sums.append(sum(cur))
    lad = [v for (k, _g), v in med.items() if k == "k_ladder_lut"]
    parts = [v for (k, _g), v in med.items() if k != "k_ladder_lut"]
    if len(lad) == 1 and len(parts) == 2 * len(RUNGS):
        for what, us, nb in (("k_ladder_lut", lad[0], ladder_moved()), ("the eight dispatches, sum of medians", sum(parts), parent_moved())):
            print(f"{what}: {us:.1f} us; {nb / 1e6:.2f} MB = {nb / us / 1e6:.2f} TB/s = {100 * nb / (us * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak"
                  f"; floor at the peak {nb / HBM_PEAK * 1e6:.1f} us")
    else:
        print(f"{len(lad)} k_ladder_lut grids and {len(parts)} other grids in the trace: one picture and one location per run give 1 and {2 * len(RUNGS)}")
    if sums:
        s = np.array(sums)
        print(f"the eight dispatches, summed per round: {len(s)} rounds, median {np.median(s):.1f} us, 10th..90th percentile "
              f"{np.percentile(s, 10):.1f}..{np.percentile(s, 90):.1f} us")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 100
        kind = sys.argv[3] if len(sys.argv) > 3 else "both"
        loc = sys.argv[4] if len(sys.argv) > 4 else "both"
        launches(n, ("smooth", "noise") if kind == "both" else (kind,), (0, 1) if loc == "both" else (int(loc),))
    elif mode == "trace":
        trace(sys.argv[2])
    else:
        sys.exit(__doc__)
