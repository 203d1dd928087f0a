"""Surface output (k_surface) on the device: the numbers LABBOOK 25 / DESIGN 8 f3 quote.

    python tools/micro/surface_time.py launches 3840x2160 [N]
        warm-up, then N (default 200) launches of ovhip_surface_launch per format and rounding, of ovhip_output_pack_launch (the kernel
        every PACKED output runs: the bytes of I010) and of ovhip_rgb_launch U8 planar (the same kind of access, 49.8 MB) on the same
        picture, each launch between two events on the context's stream: prints the median of the N event times (which hold a few
        microseconds of the events' own) and the bytes each has to move.  Run it under
        `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python ...` for the isolated kernel times, and read them with
    python tools/micro/surface_time.py trace <dir or kernel_trace.csv> [3840x2160]
        the median, minimum and count of end - start per kernel name (k_surface<format, dither>, k_output_pack, k_rgb) of such a trace
        (no device needed); with a size, GB/s and the share of the 8 TB/s HBM peak beside the surface kernels.
    python tools/micro/surface_time.py stream [3840x2160] [threads]
        one stream (I + 4 GOPs of 32, intra period 64, two recorded B contents, 16 frame threads by default) through the C stream
        driver three times in one process, alternating, profiler off: OVHIP_OUT_NONE, OVHIP_OUT_NONE with surface output on (NV12,
        tight, into a device-resident torch tensor of 32 slots), OVHIP_OUT_PACKED.  The first intra period warms up, the second is
        timed; three rounds, pictures/s each.
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
HBM_PEAK = 8.0e12
MODES = [("NV12", 0, 0, 1), ("NV12 dither", 0, 1, 1), ("P010", 1, 0, 2), ("I420", 2, 0, 1), ("I420 dither", 2, 1, 1), ("I010", 3, 0, 2)]
TEMPLATE = {(0, 0): "NV12", (0, 1): "NV12 dither", (1, 0): "P010", (2, 0): "I420", (2, 1): "I420 dither", (3, 0): "I010"}


def size(s):
    w, h = s.split("x")
    return int(w), int(h)


def surface_bytes(s, es):
    """the three planes read once (4:2:0, 16-bit samples) + 1.5 elements per pixel written once"""
    return s[0] * s[1] * 3 + s[0] * s[1] * 3 * es // 2


def pack_bytes(s):
    """k_output_pack: the three planes read once and written once"""
    return s[0] * s[1] * 3 * 2


def rgb_u8_bytes(s):
    """k_rgb U8: the three planes read once + three channels of one byte written once"""
    return s[0] * s[1] * 3 + s[0] * s[1] * 3


def noise_pic(ctx, w, h, seed):
    rs = np.random.RandomState(seed)
    return ctx.upload_pic(*(rs.randint(0, 1024, shape).astype(np.uint16) for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2))))


def launches(s, n):
    import ctypes as C
    import torch
    from openvvc_amd import capi, engine
    ctx = engine.Context(0)
    pic, d = noise_pic(ctx, s[0], s[1], 1), ctx.alloc(s[0] * s[1] * 3 * 2)
    stream = torch.cuda.ExternalStream(ctx.stream)

    def timed(name, nbytes, fn):
        for _ in range(20):
            fn()
        ctx.sync()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in evs:
            a.record(stream)
            fn()
            b.record(stream)
        ctx.sync()
        us = np.array([1e3 * a.elapsed_time(b) for a, b in evs])
        print(f"{s[0]}x{s[1]} {name}: {n} launches, median {np.median(us):.1f} us, min {us.min():.1f} us between events; {nbytes / 1e6:.2f} MB to move per launch")

    for name, fmt, rounding, es in MODES:
        f = engine.surface_format(fmt, rounding)
        timed(f"k_surface {name}", surface_bytes(s, es), lambda: pic.surface_into(d.ptr.value, d.nbytes, f))
    f = engine.surface_format(capi.SURF_NV12, 0, pitch_y=(s[0] + 255) // 256 * 256 + 256, pitch_c=(s[0] + 255) // 256 * 256 + 256)
    timed("k_surface NV12, pitch of 256-byte multiples", surface_bytes(s, 1), lambda: pic.surface_into(d.ptr.value, d.nbytes, f))
    win = capi.Window(0, 0, 0, 0)
    timed("k_output_pack", pack_bytes(s), lambda: ctx._chk(ctx.lib.ovhip_output_pack_launch(ctx.h, C.byref(pic.s), C.byref(win), d.ptr), "pack"))
    rgb = capi.RgbFormat(1, 0, 0, capi.RGB_U8, capi.RGB_PLANAR)
    timed("k_rgb U8 planar", rgb_u8_bytes(s), lambda: pic.rgb_into(d.ptr.value, d.nbytes, rgb))
    d.free(); pic.free(); ctx.close()


def trace(path, s):
    p = Path(path)
    files = [p] if p.is_file() else sorted(p.rglob("*kernel_trace.csv"))
    if not files:
        sys.exit(f"{path}: no kernel_trace.csv")
    times = {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                m = re.search(r"k_surface<\(?(?:int\))?(\d)\)?, \(?(?:int\))?(\d)\)?>", name)
                if m:
                    key = "k_surface " + TEMPLATE.get((int(m.group(1)), int(m.group(2))), m.group(0))
                elif "k_surface" in name:
                    key = name
                elif "k_output_pack" in name:
                    key = "k_output_pack"
                elif "k_rgb" in name:
                    key = "k_rgb " + name[name.index("k_rgb") + 5:].split("(")[0]
                else:
                    continue
                times.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    es = {name: e for name, _f, _r, e in MODES}
    for key, us in times.items():
        us = np.array(us)
        line = f"{key}: {len(us)} dispatches, median {np.median(us):.1f} us, min {us.min():.1f} us"
        fmt = key[len("k_surface "):] if key.startswith("k_surface ") else None
        if s and fmt in es:
            nb = surface_bytes(s, es[fmt])
            line += f"; {nb / 1e6:.2f} MB = {nb / np.median(us) / 1e3:.0f} GB/s = {100 * nb / (np.median(us) * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak"
        print(line)


def stream(s, threads):
    import ctypes as C
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
    fmt = engine.surface_format(capi.SURF_NV12)
    need = ctx.lib.ovhip_surface_bytes(w, h, None, C.byref(fmt))
    t = torch.zeros((32, need), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    variants = [("OVHIP_OUT_NONE", capi.OUT_NONE, False), ("OVHIP_OUT_NONE + NV12 surfaces", capi.OUT_NONE, True), ("OVHIP_OUT_PACKED", capi.OUT_PACKED, False)]
    rates = {name: [] for name, _o, _r in variants}
    for rnd in range(3):
        for name, out, surf in variants:
            st = engine.Stream(dpb, w, h, contents, jobs, threads_per_device=threads, output=out)
            arr = st.pics_array(spics)
            if surf:
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
    assert t.any().item(), "the surface run wrote nothing"
    [j.close() for j in jobs]; dpb.close(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        launches(size(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 200)
    elif mode == "trace":
        trace(sys.argv[2], size(sys.argv[3]) if len(sys.argv) > 3 else None)
    elif mode == "stream":
        stream(size(sys.argv[2]) if len(sys.argv) > 2 else (3840, 2160), int(sys.argv[3]) if len(sys.argv) > 3 else 16)
    else:
        sys.exit(__doc__)
