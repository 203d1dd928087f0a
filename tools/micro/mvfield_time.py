"""Motion field output (k_mvfield_clear, k_mvfield) on the device: the numbers the LABBOOK's motion field section quotes.

    python tools/micro/mvfield_time.py launches 3840x2160 [N]
        one picture of the benchmark's B content (seed 0x266, every tool, 12 % intra CUs) through a picture job, then warm-up and N
        (default 200) calls of ovhip_job_mvfield per dtype and layout on the job's device arrays, each between two events on the
        context's stream: prints the median of the N event times (which hold a few microseconds of the events' own and cover BOTH
        launches) and the bytes written.  Run it under `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python ...` for the
        isolated kernel times, and read them with
    python tools/micro/mvfield_time.py trace <dir or kernel_trace.csv>
        the median, minimum and count of end - start per kernel name (k_mvfield_clear, k_mvfield<dtype, layout>) of such a trace (no
        device needed).
    python tools/micro/mvfield_time.py stream [3840x2160] [threads]
        one stream (I + 4 GOPs of 32, intra period 64, two recorded B contents, 16 frame threads by default) through the C stream
        driver twice in one process, alternating, profiler off: OVHIP_OUT_NONE, and OVHIP_OUT_NONE with the motion field on (I32 cells
        + info, into device-resident torch tensors of 32 slots).  The first intra period warms up, the second is timed; three rounds,
        pictures/s each.
"""
import csv
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
DTYPES = {0: "I32", 1: "F32", 2: "F16"}
LAYOUTS = {0: "planar", 1: "cells"}


def size(s):
    w, h = s.split("x")
    return int(w), int(h)


def launches(s, n):
    import torch
    from openvvc_amd import engine, synth
    w, h = s
    wl = synth.make_workload(w, h, 0x266, tools=synth.INTRA_TOOLS, intra_frac=0.12)
    ctx = engine.Context(0)
    job = engine.Job(ctx, w, h)
    refs = [ctx.upload_pic(*r) for r in wl.refs]
    dst = ctx.new_pic(w, h)
    job.load_workload(wl)
    job.flush(dst, refs, None)
    job.wait()
    units = {k: 0 if a is None else len(a) for k, a in (("mc", wl.mc_units), ("mcx", wl.mcx_units), ("aff", wl.aff_units))}
    print(f"{w}x{h}: {units} units, {4 * sum(units.values())} lanes of k_mvfield")
    stream = torch.cuda.ExternalStream(ctx.stream)
    for dtype in DTYPES:
        for layout in LAYOUTS:
            fmt = engine.mvfield_format(dtype, layout, 1)
            vec = torch.zeros(engine.mvfield_shape(fmt, w, h)[0], dtype={0: torch.int32, 1: torch.float32, 2: torch.float16}[dtype], device="cuda:0")
            info = torch.zeros(engine.mvfield_shape(fmt, w, h)[1], dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            for _ in range(20):
                job.mvfield(fmt, vec, info)
            ctx.sync()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for a, b in evs:
                a.record(stream)
                job.mvfield(fmt, vec, info)
                b.record(stream)
            ctx.sync()
            us = np.array([1e3 * a.elapsed_time(b) for a, b in evs])
            nb = vec.numel() * vec.element_size() + info.numel() * 4
            print(f"{w}x{h} {DTYPES[dtype]} {LAYOUTS[layout]}: {n} calls, median {np.median(us):.1f} us, min {us.min():.1f} us between events (clear + scatter); "
                  f"{vec.numel() * vec.element_size() / 1e6:.2f} MB of vectors + {info.numel() * 4 / 1e6:.2f} MB of info, each written once by the clear "
                  f"and the covered share again by the scatter ({nb / 1e6:.2f} MB)")
            assert (info != 0xFFFF).any().item(), "the field is empty"
    job.close(); ctx.close()


def trace(path):
    p = Path(path)
    files = [p] if p.is_file() else sorted(p.rglob("*kernel_trace.csv"))
    if not files:
        sys.exit(f"{path}: no kernel_trace.csv")
    times = {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                if "k_mvfield" not in name:
                    continue
                m = re.search(r"k_mvfield<\(?(?:int\))?(\d)\)?, \(?(?:int\))?(\d)\)?>", name)
                key = f"k_mvfield {DTYPES.get(int(m.group(1)), '?')} {LAYOUTS.get(int(m.group(2)), '?')}" if m else ("k_mvfield_clear" if "clear" in name else name)
                times.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for key, us in times.items():
        us = np.array(us)
        print(f"{key}: {len(us)} dispatches, median {np.median(us):.1f} us, min {us.min():.1f} us, max {us.max():.1f} us")


def stream(s, threads):
    import torch
    from openvvc_amd import capi, engine, gop
    from test_gpu_stream import _contents, _make_contents, _stream_pics
    w, h = s
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
    fmt = engine.mvfield_format(capi.MVF_I32, capi.MVF_CELLS, capi.MVF_REFINED)
    vshape, ishape = engine.mvfield_shape(fmt, w, h)
    vec = torch.zeros((32,) + vshape, dtype=torch.int32, device="cuda:0")
    info = torch.zeros((32,) + ishape, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    variants = [("OVHIP_OUT_NONE", False), ("OVHIP_OUT_NONE + motion field (I32 cells + info)", True)]
    rates = {name: [] for name, _m in variants}
    for rnd in range(3):
        for name, on in variants:
            st = engine.Stream(dpb, w, h, contents, jobs, threads_per_device=threads, output=capi.OUT_NONE)
            arr = st.pics_array(spics)
            if on:
                st.set_mvfield_output(fmt, vec, info)
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
    assert (info != 0).any().item(), "the motion field run wrote nothing"
    [j.close() for j in jobs]; dpb.close(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        launches(size(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 200)
    elif mode == "trace":
        trace(sys.argv[2])
    elif mode == "stream":
        stream(size(sys.argv[2]) if len(sys.argv) > 2 else (3840, 2160), int(sys.argv[3]) if len(sys.argv) > 3 else 16)
    else:
        sys.exit(__doc__)
