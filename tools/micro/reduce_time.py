"""Reduced-size output (k_output_reduce) on the device: the numbers LABBOOK 29 / DESIGN 8 f3 quote.

    python tools/micro/reduce_time.py launches [N]
        warm-up, then N (default 100) launches of ovhip_output_reduce_launch for 3840x2160 -> 1920x1080, 3840x2160 -> 1280x720 and
        1920x1080 -> 1280x720, of ovhip_output_scale_launch 1920x1080 -> 3840x2160 (the resampler's recorded case, 31 MB) and of
        ovhip_surface_launch NV12 at 3840x2160, each launch between two events on the context's stream: prints the median of the N
        event times (which hold a few microseconds of the events' own) and the bytes each has to move.  Run it under
        `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python ...` for the isolated kernel times, and read them with
    python tools/micro/reduce_time.py trace <dir or kernel_trace.csv>
        the median, minimum and count of end - start per kernel and grid size of such a trace (no device needed), with the bytes, TB/s
        and the share of the 8 TB/s HBM peak beside the cases above.
    python tools/micro/reduce_time.py stream [threads]
        one 3840x2160 stream (I + 4 GOPs of 32, intra period 64, two recorded B contents, 16 frame threads by default) through the C
        stream driver three times in one process, alternating, profiler off: OVHIP_OUT_NONE with NV12 surfaces of 1920x1080 out of
        the reduce step, OVHIP_OUT_NONE with NV12 surfaces at the coded size, OVHIP_OUT_NONE alone.  The first intra period warms
        up, the second is timed; three rounds, pictures/s each.
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
REDUCE = [((3840, 2160), (1920, 1080)), ((3840, 2160), (1280, 720)), ((1920, 1080), (1280, 720))]
SCALE = ((1920, 1080), (3840, 2160))
SURFACE = (3840, 2160)


def pic_bytes(s):
    return s[0] * s[1] * 3                                  # 4:2:0, 16-bit samples


def moved(src, dst):
    """the source read once + the destination written once"""
    return pic_bytes(src) + pic_bytes(dst)


def reduce_grid(dst):
    """work-items of k_output_reduce: one wave of 64 per 64 x 8 destination tile, luma and both chroma planes"""
    tiles = lambda w, h: ((w + 63) // 64) * ((h + 7) // 8)
    return 64 * (tiles(*dst) + 2 * tiles(dst[0] // 2, dst[1] // 2))


def noise_pic(ctx, w, h, seed):
    rs = np.random.RandomState(seed)
    return ctx.upload_pic(*(rs.randint(0, 1024, shape).astype(np.uint16) for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2))))


def launches(n):
    import torch
    from openvvc_amd import capi, engine
    ctx = engine.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)

    def timed(name, nbytes, fn):
        for _ in range(10):
            fn()
        ctx.sync()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in evs:
            a.record(stream)
            fn()
            b.record(stream)
        ctx.sync()
        us = np.array([1e3 * a.elapsed_time(b) for a, b in evs])
        print(f"{name}: {n} launches, median {np.median(us):.1f} us, min {us.min():.1f} us between events; {nbytes / 1e6:.2f} MB to move per launch")

    pics = {s: noise_pic(ctx, s[0], s[1], s[0]) for s in {src for src, _d in REDUCE} | {SCALE[0]}}
    for src, dst in REDUCE:
        d = ctx.new_pic(*dst)
        timed(f"k_output_reduce {src[0]}x{src[1]} -> {dst[0]}x{dst[1]}", moved(src, dst), lambda: pics[src].reduce_into(d))
        d.free()
    d = ctx.new_pic(*SCALE[1])
    timed(f"k_output_scale {SCALE[0][0]}x{SCALE[0][1]} -> {SCALE[1][0]}x{SCALE[1][1]}", moved(*SCALE), lambda: pics[SCALE[0]].scale_into(d))
    d.free()
    buf = ctx.alloc(SURFACE[0] * SURFACE[1] * 3 // 2)
    f = engine.surface_format(capi.SURF_NV12)
    timed(f"k_surface NV12 {SURFACE[0]}x{SURFACE[1]}", pic_bytes(SURFACE) + SURFACE[0] * SURFACE[1] * 3 // 2, lambda: pics[SURFACE].surface_into(buf.ptr.value, buf.nbytes, f))
    buf.free()
    [p.free() for p in pics.values()]
    ctx.close()


def trace(path):
    p = Path(path)
    files = [p] if p.is_file() else sorted(p.rglob("*kernel_trace.csv"))
    if not files:
        sys.exit(f"{path}: no kernel_trace.csv")
    # the grid says the destination only: two cases with one destination are told apart by their order in `launches`
    grids = {}
    for src, dst in REDUCE:
        grids.setdefault(reduce_grid(dst), []).append((f"{src[0]}x{src[1]} -> {dst[0]}x{dst[1]}", moved(src, dst)))
    times, by_grid = {}, {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                grid = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)
                if "k_output_reduce" in name:
                    by_grid.setdefault(grid, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
                    continue
                elif "k_output_scale" in name:
                    key = ("k_output_scale", f"{SCALE[0][0]}x{SCALE[0][1]} -> {SCALE[1][0]}x{SCALE[1][1]}", moved(*SCALE))
                elif "k_surface" in name:
                    key = ("k_surface NV12", f"{SURFACE[0]}x{SURFACE[1]}", pic_bytes(SURFACE) + SURFACE[0] * SURFACE[1] * 3 // 2)
                else:
                    continue
                times.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for grid, rows in by_grid.items():
        cases = grids.get(grid, [(f"grid {grid}", 0)])
        us = [u for _t, u in sorted(rows)]
        per = len(us) // len(cases)
        for k, (what, nb) in enumerate(cases):
            times[("k_output_reduce", what, nb)] = us[k * per:(k + 1) * per if k + 1 < len(cases) else len(us)]
    for (kernel, what, nb), us in times.items():
        us = np.array(us)
        line = f"{kernel} {what}: {len(us)} dispatches, median {np.median(us):.1f} us, min {us.min():.1f} us"
        if nb:
            line += f"; {nb / 1e6:.2f} MB = {nb / np.median(us) / 1e6:.2f} TB/s = {100 * nb / (np.median(us) * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak"
        print(line)


def stream(threads):
    import ctypes as C
    import torch
    from openvvc_amd import capi, engine, gop
    from test_gpu_stream import _contents, _make_contents, _stream_pics
    w, h, ow, oh = 3840, 2160, 1920, 1080
    wls = _contents(w, h, (11, 12), 14)
    pics = gop.build_stream(4, 32, 64, 1)
    spics = _stream_pics(pics, 2)
    n_i = 0
    for p, q in zip(spics, pics):                  # 40 jobs in rotation for the B pictures (job k <-> content k % 2), two for the I pictures
        if q.intra:
            p["job"], p["content"] = 40 + n_i % 2, 2
            n_i += 1
        else:
            p["job"] = q.idx % 40
            p["content"] = p["job"] % 2
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = []
    for k in range(42):
        j = engine.Job(ctx, w, h)
        j.load_workload(wls[k % 2 if k < 40 else 2])
        jobs.append(j)
    contents = _make_contents(wls)
    n, n_warm = len(spics), 65
    fmt = engine.surface_format(capi.SURF_NV12)
    need_full = ctx.lib.ovhip_surface_bytes(w, h, None, C.byref(fmt))
    need_red = ctx.lib.ovhip_surface_bytes(ow, oh, None, C.byref(fmt))
    t_full = torch.zeros((32, need_full), dtype=torch.uint8, device="cuda:0")
    t_red = torch.zeros((32, need_red), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    variants = [(f"NV12 surfaces at {ow}x{oh}, reduce on", t_red, True), (f"NV12 surfaces at {w}x{h}", t_full, False), ("OVHIP_OUT_NONE", None, False)]
    rates = {name: [] for name, _t, _r in variants}
    for rnd in range(3):
        for name, t, red in variants:
            st = engine.Stream(dpb, w, h, contents, jobs, threads_per_device=threads, output=capi.OUT_NONE)
            arr = st.pics_array(spics)
            if red:
                st.set_output_reduce(ow, oh)
            if t is not None:
                st.set_surface_output(t, fmt)
            st.run(arr, n, 0, n_warm, flags=capi.STREAM_KEEP)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, _ = st.run(arr, n, n_warm, n - n_warm, flags=capi.STREAM_KEEP)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert res.status == 0 and res.n_decoded == n - n_warm
            rates[name].append((n - n_warm) / dt)
            st.close()
    for name, r in rates.items():
        print(f"{w}x{h} {threads} frame threads, {name}: " + ", ".join(f"{v:.0f}" for v in r) + f" pictures/s (median {float(np.median(r)):.0f})")
    assert t_red.any().item() and t_full.any().item(), "a surface run wrote nothing"
    [j.close() for j in jobs]; dpb.close(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        launches(int(sys.argv[2]) if len(sys.argv) > 2 else 100)
    elif mode == "trace":
        trace(sys.argv[2])
    elif mode == "stream":
        stream(int(sys.argv[2]) if len(sys.argv) > 2 else 16)
    else:
        sys.exit(__doc__)
