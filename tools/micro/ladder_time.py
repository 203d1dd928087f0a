"""Output ladder (k_output_ladder) on the device: the numbers LABBOOK 34 quotes.

    python tools/micro/ladder_time.py launches [N]
        warm-up, then N (default 100) rounds of: ONE ovhip_ladder_launch of 3840x2160 -> NV12 at 1920x1080, 1280x720, 960x540 and
        640x360, then the EIGHT launches that make the same four surfaces without it (ovhip_output_reduce_launch into a 16-bit
        picture + ovhip_surface_launch, per rung), each side between two events on the context's stream: prints the medians of the
        event times (which hold a few microseconds of the events' own) and the bytes the algorithm has to move.  The surfaces of both
        sides are compared for equality first.  Run it under
        `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python ...` for the isolated kernel times, and read them with
    python tools/micro/ladder_time.py trace <dir or kernel_trace.csv>
        the median, minimum and count of end - start per kernel (k_output_reduce and k_surface per grid size) of such a trace (no
        device needed), the sum of the eight medians beside the ladder's, the bytes, TB/s and the share of the 8 TB/s HBM peak.
    python tools/micro/ladder_time.py ladder [N]
        N ladder launches and nothing else: the run to put under `rocprofv3 --pmc FETCH_SIZE` (counters in a run of their own), read with
    python tools/micro/ladder_time.py fetch <dir or counter_collection.csv>
        the median FETCH_SIZE (KB) per k_output_ladder dispatch of such a run, beside the source's and the surfaces' bytes.
    python tools/micro/ladder_time.py stream [threads]
        one 3840x2160 stream (I + 4 GOPs of 32, intra period 64, two recorded B contents, 16 frame threads by default) through the C
        stream driver three times in one process, alternating, profiler off: OVHIP_OUT_NONE with the four-rung NV12 ladder,
        OVHIP_OUT_NONE with the single 1920x1080 NV12 surface out of the reduce setting, OVHIP_OUT_NONE alone.  The first intra period
        warms up, the second is timed; three rounds, pictures/s each.
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
RUNGS = [(1920, 1080), (1280, 720), (960, 540), (640, 360)]


def pic_bytes(s):
    return s[0] * s[1] * 3                                  # 4:2:0, 16-bit samples


def nv12_bytes(s):
    return s[0] * s[1] * 3 // 2


def ladder_moved():
    """the source read once + every surface written once"""
    return pic_bytes(SRC) + sum(nv12_bytes(d) for d in RUNGS)


def parent_moved():
    """per rung: the source read, the 16-bit picture written and read again, the surface written"""
    return sum(pic_bytes(SRC) + 2 * pic_bytes(d) + nv12_bytes(d) for d in RUNGS)


def tiles(w, h):
    return ((w + 63) // 64) * ((h + 7) // 8)


def reduce_grid(dst):
    """work-items of k_output_reduce: one wave of 64 per 64 x 8 destination tile, luma and both chroma planes"""
    return 64 * (tiles(*dst) + 2 * tiles(dst[0] // 2, dst[1] // 2))


def ladder_grid():
    """work-items of k_output_ladder for NV12 rungs: luma tiles and ONE chroma tile for the Cb and the Cr of an interleaved plane"""
    return 64 * sum(tiles(*d) + tiles(d[0] // 2, d[1] // 2) for d in RUNGS)


def surface_grid(dst):
    """work-items of k_surface NV12: a lane per run of 16 elements, workgroups of 256"""
    items = ((dst[0] + 15) // 16) * (dst[1] + dst[1] // 2)
    return 256 * ((items + 255) // 256)


def noise_pic(ctx, w, h, seed):
    rs = np.random.RandomState(seed)
    return ctx.upload_pic(*(rs.randint(0, 1024, shape).astype(np.uint16) for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2))))


def _setup():
    from openvvc_amd import capi, engine
    ctx = engine.Context(0)
    pic = noise_pic(ctx, SRC[0], SRC[1], 34)
    fmt = engine.surface_format(capi.SURF_NV12)
    bufs = [ctx.alloc(nv12_bytes(d)) for d in RUNGS]
    rungs = [engine.ladder_rung(d[0], d[1], fmt, b.ptr.value, b.nbytes) for d, b in zip(RUNGS, bufs)]
    return ctx, pic, fmt, bufs, rungs


def launches(n, ladder_only=False):
    import torch
    ctx, pic, fmt, bufs, rungs = _setup()
    stream = torch.cuda.ExternalStream(ctx.stream)
    mids = [ctx.new_pic(*d) for d in RUNGS]
    other = [ctx.alloc(nv12_bytes(d)) for d in RUNGS]

    def ladder():
        pic.ladder_into(rungs)

    def eight():
        for d, m, o in zip(RUNGS, mids, other):
            pic.reduce_into(m)
            m.surface_into(o.ptr.value, o.nbytes, fmt)

    ladder(); eight(); ctx.sync()
    for b, o in zip(bufs, other):
        assert b.download().tobytes() == o.download().tobytes(), "the ladder's surfaces differ from surface(reduce())"
    sides = [("k_output_ladder, one launch", ladder_moved(), ladder)] + ([] if ladder_only else [("k_output_reduce + k_surface, eight launches", parent_moved(), eight)])
    for _ in range(10):
        for _name, _nb, fn in sides:
            fn()
    ctx.sync()
    evs = {name: [] for name, _nb, _fn in sides}
    for _ in range(n):                                       # alternating, in one call
        for name, _nb, fn in sides:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            evs[name].append((a, b))
    ctx.sync()
    for name, nb, _fn in sides:
        us = np.array([1e3 * a.elapsed_time(b) for a, b in evs[name]])
        print(f"{SRC[0]}x{SRC[1]} -> NV12 x {len(RUNGS)}, {name}: {n} rounds, median {np.median(us):.1f} us, min {us.min():.1f} us, "
              f"10th..90th percentile {np.percentile(us, 10):.1f}..{np.percentile(us, 90):.1f} us between events; {nb / 1e6:.2f} MB to move")
    [p.free() for p in mids + [pic]]
    [b.free() for b in bufs + other]
    ctx.close()


def _csv_files(path, pattern):
    p = Path(path)
    files = [p] if p.is_file() else sorted(p.rglob(pattern))
    if not files:
        sys.exit(f"{path}: no {pattern}")
    return files


def trace(path):
    times = {}
    for f in _csv_files(path, "*kernel_trace.csv"):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                grid = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)
                for k in ("k_output_ladder", "k_output_reduce", "k_surface"):
                    if k in name:
                        times.setdefault((k, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    med = {}
    for (k, grid), us in sorted(times.items()):
        us = np.array(us)
        med[(k, grid)] = float(np.median(us))
        print(f"{k} grid {grid}: {len(us)} dispatches, median {np.median(us):.1f} us, min {us.min():.1f} us, 10th..90th percentile "
              f"{np.percentile(us, 10):.1f}..{np.percentile(us, 90):.1f} us")
    lad = med.get(("k_output_ladder", ladder_grid()))
    parts = [med.get(("k_output_reduce", reduce_grid(d))) for d in RUNGS] + [med.get(("k_surface", surface_grid(d))) for d in RUNGS]
    for what, us, nb in (("k_output_ladder", lad, ladder_moved()), ("the eight dispatches, sum of medians", sum(parts) if all(parts) else None, parent_moved())):
        if us:
            print(f"{what}: {us:.1f} us; {nb / 1e6:.2f} MB = {nb / us / 1e6:.2f} TB/s = {100 * nb / (us * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak"
                  f"; floor at the peak {nb / HBM_PEAK * 1e6:.1f} us")
        else:
            print(f"{what}: not in the trace")


def fetch(path):
    vals = []
    for f in _csv_files(path, "*counter_collection.csv"):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                if "k_output_ladder" in row.get("Kernel_Name", "") and row.get("Counter_Name") == "FETCH_SIZE":
                    vals.append(float(row["Counter_Value"]))
    if not vals:
        sys.exit(f"{path}: no FETCH_SIZE of k_output_ladder")
    v = np.array(vals)
    print(f"k_output_ladder: {len(v)} dispatches, FETCH_SIZE median {np.median(v):.0f} KB, min {v.min():.0f} KB, max {v.max():.0f} KB; the source is "
          f"{pic_bytes(SRC) / 1024:.0f} KB, read once per rung {len(RUNGS) * pic_bytes(SRC) / 1024:.0f} KB")


def stream(threads):
    import ctypes as C
    import torch
    from openvvc_amd import capi, engine, gop
    from test_gpu_stream import _contents, _make_contents, _stream_pics
    w, h = SRC
    ow, oh = RUNGS[0]
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
    ts = [torch.zeros((32, nv12_bytes(d)), dtype=torch.uint8, device="cuda:0") for d in RUNGS]
    t_red = torch.zeros((32, ctx.lib.ovhip_surface_bytes(ow, oh, None, C.byref(fmt))), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    variants = ["the four-rung NV12 ladder", f"one NV12 surface at {ow}x{oh}, reduce on", "OVHIP_OUT_NONE"]
    rates = {name: [] for name in variants}
    for rnd in range(3):
        for k, name in enumerate(variants):
            st = engine.Stream(dpb, w, h, contents, jobs, threads_per_device=threads, output=capi.OUT_NONE)
            arr = st.pics_array(spics)
            if k == 0:
                st.set_ladder_output([engine.ladder_rung(d[0], d[1], fmt, t, slots=True) for d, t in zip(RUNGS, ts)])
            elif k == 1:
                st.set_output_reduce(ow, oh)
                st.set_surface_output(t_red, fmt)
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
    assert all(t.any().item() for t in ts) and t_red.any().item(), "a surface run wrote nothing"
    [j.close() for j in jobs]; dpb.close(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode in ("launches", "ladder"):
        launches(int(sys.argv[2]) if len(sys.argv) > 2 else 100, ladder_only=mode == "ladder")
    elif mode == "trace":
        trace(sys.argv[2])
    elif mode == "fetch":
        fetch(sys.argv[2])
    elif mode == "stream":
        stream(int(sys.argv[2]) if len(sys.argv) > 2 else 16)
    else:
        sys.exit(__doc__)
