"""RGB pyramid (k_rgb_pyramid) on the device: the numbers LABBOOK 39 quotes.

    python tools/micro/rgb_pyramid_time.py launches [N] [smooth|noise|both] [plain|table|both]
        per picture (3840x2160, a smooth ramp or noise), without a table and through a 33-point table of peak 255: warm-up, then N
        (default 100) rounds of ONE ovhip_rgb_pyramid_launch -> 1920x1080 F16 CHW, 960x540 F16 CHW and 640x360 U8 HWC, then the SIX
        launches that make the same three tensors without it (ovhip_output_reduce_launch into a 16-bit picture + ovhip_rgb_launch or
        ovhip_rgb_lut_launch, per level), each side between two events on the context's stream, alternating in one process: prints the
        medians and percentiles of the event times (which hold a few microseconds of the events' own) and the bytes the algorithm has
        to move.  The tensors of both sides are compared for equality first.  Run it under
        `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python ...` (one picture and one mode per run) for the
        isolated kernel times, and read them with
    python tools/micro/rgb_pyramid_time.py trace <dir or kernel_trace.csv>
        the median, minimum, percentiles and count of end - start per kernel and grid size of such a trace (no device needed); the sum
        of the six medians beside k_rgb_pyramid's; the sum of the six per round with its own percentiles -- the run-to-run spread that
        is the only margin of LABBOOK 39's condition; the bytes, TB/s and the share of the 8 TB/s HBM peak.
    python tools/micro/rgb_pyramid_time.py stream [N]
        the stream driver on 832x480 pictures with OVHIP_OUT_NONE, N (default 5) runs alternating without and with a three-level
        pyramid (416x240 F16 CHW, 208x120 F16 CHW, 104x60 U8 HWC) into slots: frames per second of each run and the medians.
"""
import csv
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
HBM_PEAK = 8.0e12
SRC = (3840, 2160)
U8, F16, CHW, HWC = 0, 2, 0, 1
LEVELS = [(1920, 1080, F16, CHW), (960, 540, F16, CHW), (640, 360, U8, HWC)]
ES = {U8: 1, F16: 2}
TABLE, PEAK = 33, 255
MATRIX, LOC = 9, 0                                           # BT.2020 limited, chroma left
KERNELS = ("k_rgb_pyramid", "k_output_reduce", "k_rgb_lut", "k_rgb")


def pic_bytes(s):
    return s[0] * s[1] * 3                                  # 4:2:0, 16-bit samples


def level_bytes(lv):
    return 3 * lv[0] * lv[1] * ES[lv[2]]


def pyramid_moved():
    """the source read once + every tensor written once (the table stays in cache)"""
    return pic_bytes(SRC) + sum(level_bytes(lv) for lv in LEVELS)


def parent_moved():
    """per level: the source read, the 16-bit picture written and read again, the tensor written"""
    return sum(pic_bytes(SRC) + 2 * pic_bytes(lv) + level_bytes(lv) for lv in LEVELS)


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


def launches(n, kinds, modes):
    import torch
    from openvvc_amd import engine
    ctx = engine.Context(0)
    table = np.random.default_rng(38).integers(0, PEAK + 1, (TABLE, TABLE, TABLE, 3), dtype=np.uint16)
    the_lut = engine.RgbLut(ctx, table, PEAK)
    stream = torch.cuda.ExternalStream(ctx.stream)
    fmts = [engine.rgb_format(MATRIX, 0, LOC, lv[2], lv[3]) for lv in LEVELS]
    bufs = [ctx.alloc(level_bytes(lv)) for lv in LEVELS]
    other = [ctx.alloc(level_bytes(lv)) for lv in LEVELS]
    mids = [ctx.new_pic(lv[0], lv[1]) for lv in LEVELS]
    levels = [engine.rgb_level(lv[0], lv[1], f, b.ptr.value, nbytes=b.nbytes) for lv, f, b in zip(LEVELS, fmts, bufs)]
    for kind in kinds:
        pic = ctx.upload_pic(*planes(kind, SRC[0], SRC[1], 38))
        for mode in modes:
            lut = the_lut if mode == "table" else None

            def pyramid():
                pic.rgb_pyramid_into(levels, lut=lut)

            def six():
                for m, o, f in zip(mids, other, fmts):
                    pic.reduce_into(m)
                    m.rgb_into(o.ptr.value, o.nbytes, f, lut=lut)

            pyramid(); six(); ctx.sync()
            for b, o in zip(bufs, other):
                assert b.download().tobytes() == o.download().tobytes(), "the pyramid's tensors differ from rgb(reduce())"
            second = "k_rgb_lut" if lut is not None else "k_rgb"
            sides = [("k_rgb_pyramid, one launch", pyramid_moved(), pyramid), (f"k_output_reduce + {second}, six launches", parent_moved(), six)]
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
                print(f"{kind}, {mode}: {SRC[0]}x{SRC[1]} -> {len(LEVELS)} tensors, {name}: {n} rounds, median {np.median(us):.1f} us, "
                      f"min {us.min():.1f} us, 10th..90th percentile {np.percentile(us, 10):.1f}..{np.percentile(us, 90):.1f} us between events; "
                      f"{nb / 1e6:.2f} MB to move", flush=True)
        pic.free()
    the_lut.close()
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
                for k in KERNELS:                             # (k_rgb last: a prefix of the others' names)
                    if k in row["Kernel_Name"]:
                        rows.append((int(row["Start_Timestamp"]), k, int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0),
                                     (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
                        break
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
    # the rounds: every run of six reduce / rgb dispatches between two pyramid dispatches
    sums, cur = [], []
    for _t, k, _grid, us in rows:
        if k == "k_rgb_pyramid":
            if len(cur) == 2 * len(LEVELS):
                sums.append(sum(cur))
            cur = []
        else:
            cur.append(us)
    if len(cur) == 2 * len(LEVELS):
        sums.append(sum(cur))
    pyr = [v for (k, _g), v in med.items() if k == "k_rgb_pyramid"]
    parts = [v for (k, _g), v in med.items() if k != "k_rgb_pyramid"]
    if len(pyr) == 1 and len(parts) == 2 * len(LEVELS):
        for what, us, nb in (("k_rgb_pyramid", pyr[0], pyramid_moved()), ("the six dispatches, sum of medians", sum(parts), parent_moved())):
            print(f"{what}: {us:.1f} us; {nb / 1e6:.2f} MB = {nb / us / 1e6:.2f} TB/s = {100 * nb / (us * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak"
                  f"; floor at the peak {nb / HBM_PEAK * 1e6:.1f} us")
    else:
        print(f"{len(pyr)} k_rgb_pyramid grids and {len(parts)} other grids in the trace: one picture and one mode per run give 1 and {2 * len(LEVELS)}")
    if sums:
        s = np.array(sums)
        print(f"the six dispatches, summed per round: {len(s)} rounds, median {np.median(s):.1f} us, 10th..90th percentile "
              f"{np.percentile(s, 10):.1f}..{np.percentile(s, 90):.1f} us")


def stream(n_runs):
    """frames per second of the stream driver with OVHIP_OUT_NONE, without and with the pyramid, alternating in one session"""
    import torch
    from openvvc_amd import capi, engine, gop
    from test_gpu_stream import _contents, _jobs_for, _make_contents, _stream_pics
    w, h = 832, 480
    wls = _contents(w, h, (41, 42), 43)
    spics = _stream_pics(gop.build_stream(2, 8, 16, 1), 2)
    n = len(spics)
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = _jobs_for(ctx, wls, spics, w, h)
    strm = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4, output=capi.OUT_NONE)
    arr = strm.pics_array(spics)
    specs = [(416, 240, F16, CHW), (208, 120, F16, CHW), (104, 60, U8, HWC)]
    tdt = {U8: torch.uint8, F16: torch.float16}
    ts = [torch.zeros((n,) + ((3, lh, lw) if lay == CHW else (lh, lw, 3)), dtype=tdt[dt], device="cuda:0") for lw, lh, dt, lay in specs]
    torch.cuda.synchronize()
    levels = [engine.rgb_level(lw, lh, engine.rgb_format(MATRIX, 0, LOC, dt, lay), t, slots=True) for (lw, lh, dt, lay), t in zip(specs, ts)]
    strm.run(arr, n, 0, n)                                    # warm-up
    fps = {"OVHIP_OUT_NONE": [], "OVHIP_OUT_NONE + RGB pyramid": []}
    for _ in range(n_runs):
        for name in fps:
            strm.set_rgb_pyramid_output(levels if "pyramid" in name else None)
            t0 = time.perf_counter()
            res, _dg = strm.run(arr, n, 0, n)
            dt = time.perf_counter() - t0
            assert res.status == 0 and res.n_decoded == n
            fps[name].append(n / dt)
    for name, v in fps.items():
        print(f"stream {w}x{h}, {n} pictures, {name}: {n_runs} runs, median {np.median(v):.1f} frames/s, min..max {min(v):.1f}..{max(v):.1f}", flush=True)
    strm.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 100
        kind = sys.argv[3] if len(sys.argv) > 3 else "both"
        tab = sys.argv[4] if len(sys.argv) > 4 else "both"
        launches(n, ("smooth", "noise") if kind == "both" else (kind,), ("plain", "table") if tab == "both" else (tab,))
    elif mode == "trace":
        trace(sys.argv[2])
    elif mode == "stream":
        stream(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    else:
        sys.exit(__doc__)
