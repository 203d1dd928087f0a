"""RGB output (k_rgb) on the device: the numbers LABBOOK / DESIGN 8 f3 quote.

    python tools/micro/rgb_time.py launches 3840x2160 [N] [out.json]
        warm-up, then N (default 200) launches of ovhip_rgb_launch per dtype and layout, and of ovhip_output_pack_launch on the same
        picture (the comparison: the kernel every PACKED output runs), one synchronise each: run it under
        `rocprofv3 --kernel-trace --stats -d <dir> -- python ...` and read the averages of k_rgb<dtype, packed, a> and k_output_pack
        from its output (the `kernels` view of the results database: avg(end - start) by name).  Prints the bytes each has to move and, from a host clock around the N launches (enqueue included: NOT the kernel
        time), the time per launch; with out.json, those times as a file.
    python tools/micro/rgb_time.py share 3840x2160 <dtype> <kernel_us>
        those bytes over a kernel time taken from the trace: GB/s and the share of the 8 TB/s HBM peak (no device needed).
    python tools/micro/rgb_time.py stream [3840x2160] [threads]
        one stream (I + 4 GOPs of 32, intra period 64, two recorded B contents, 16 frame threads by default) through the C stream
        driver three times in one process, alternating, profiler off: OVHIP_OUT_NONE, OVHIP_OUT_NONE with RGB output on (F16 planar
        into a device-resident torch tensor of 32 slots), OVHIP_OUT_PACKED.  The first intra period warms up, the second is timed;
        three rounds, pictures/s each.
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
HBM_PEAK = 8.0e12
DTYPES = {0: ("U8", 1), 1: ("U16", 2), 2: ("F16", 2), 3: ("F32", 4)}


def size(s):
    w, h = s.split("x")
    return int(w), int(h)


def rgb_bytes(s, es):
    """the three planes read once (4:2:0, 16-bit samples) + three channels written once"""
    return s[0] * s[1] * 3 + s[0] * s[1] * 3 * es


def pack_bytes(s):
    """k_output_pack: the three planes read once and written once"""
    return s[0] * s[1] * 3 * 2


def noise_pic(ctx, w, h, seed):
    rs = np.random.RandomState(seed)
    return ctx.upload_pic(*(rs.randint(0, 1024, shape).astype(np.uint16) for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2))))


def launches(s, n, out=None):
    import ctypes as C
    from openvvc_amd import capi, engine
    ctx = engine.Context(0)
    pic, d = noise_pic(ctx, s[0], s[1], 1), ctx.alloc(s[0] * s[1] * 3 * 4)
    results = {"size": f"{s[0]}x{s[1]}", "launches": n, "unit": "us per launch on the host clock, enqueue included", "figures": {}}

    def timed(name, nbytes, fn):
        for _ in range(20):
            fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        ctx.sync()
        dt = (time.perf_counter() - t0) / n
        results["figures"][name] = round(1e6 * dt, 2)
        print(f"{s[0]}x{s[1]} {name}: {n} launches, {1e6 * dt:.1f} us per launch on the host clock (enqueue included); {nbytes / 1e6:.2f} MB to move per launch")

    for dtype, (dn, es) in DTYPES.items():
        for layout, ln in ((0, "planar"), (1, "packed")):
            fmt = capi.RgbFormat(1, 0, 0, dtype, layout)
            timed(f"k_rgb {dn} {ln}", rgb_bytes(s, es), lambda: pic.rgb_into(d.ptr.value, d.nbytes, fmt))
    win = capi.Window(0, 0, 0, 0)
    timed("k_output_pack", pack_bytes(s), lambda: ctx._chk(ctx.lib.ovhip_output_pack_launch(ctx.h, C.byref(pic.s), C.byref(win), d.ptr), "pack"))
    d.free(); pic.free(); ctx.close()
    if out:
        Path(out).write_text(json.dumps(results, indent=1) + "\n")


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
    fmt = engine.rgb_format(1, 0, 0, capi.RGB_F16, capi.RGB_PLANAR)
    t = torch.zeros((32, 3, h, w), dtype=torch.float16, device="cuda:0")
    torch.cuda.synchronize()
    variants = [("OVHIP_OUT_NONE", capi.OUT_NONE, False), ("OVHIP_OUT_NONE + RGB F16 planar", capi.OUT_NONE, True), ("OVHIP_OUT_PACKED", capi.OUT_PACKED, False)]
    rates = {name: [] for name, _o, _r in variants}
    for rnd in range(3):
        for name, out, rgb in variants:
            st = engine.Stream(dpb, w, h, contents, jobs, threads_per_device=threads, output=out)
            arr = st.pics_array(spics)
            if rgb:
                st.set_rgb_output(t, fmt)
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
    assert t.any().item(), "the RGB run wrote nothing"
    [j.close() for j in jobs]; dpb.close(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        launches(size(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 200, sys.argv[4] if len(sys.argv) > 4 else None)
    elif mode == "share":
        s, es, us = size(sys.argv[2]), {v[0]: v[1] for v in DTYPES.values()}[sys.argv[3]], float(sys.argv[4])
        nb = rgb_bytes(s, es)
        print(f"{nb / 1e6:.2f} MB in {us:.1f} us = {nb / us / 1e3:.0f} GB/s = {100 * nb / (us * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    elif mode == "stream":
        stream(size(sys.argv[2]) if len(sys.argv) > 2 else (3840, 2160), int(sys.argv[3]) if len(sys.argv) > 3 else 16)
    else:
        sys.exit(__doc__)
