"""Film grain synthesis (k_film_grain) on the device: the numbers LABBOOK / DESIGN 4 quote.

    python tools/micro/fg_time.py launches 3840x2160 [N]
        warm-up, then N (default 400) launches of ovhip_film_grain_launch and one synchronise: run it under
        `rocprofv3 --kernel-trace --stats -d <dir> -- python ...`, one size per run, and read k_film_grain's average there.
        Prints the bytes the algorithm has to move (source planes read once + destination planes written once; the halo blocks
        the waves re-read add a quarter to the LOADS, which the L2 serves) and, from a host clock around the N launches (seed
        stepping and enqueue included: NOT the kernel time), the time per launch.
    python tools/micro/fg_time.py share 3840x2160 <kernel_us>
        those bytes over a kernel time taken from the trace: GB/s and the share of the 8 TB/s HBM peak (no device needed).
    python tools/micro/fg_time.py e2e
        ovhip_pic_output_grain beside ovhip_pic_output of the same 3840x2160 picture (each ends in one 24.9 MB download),
        alternating in one process, profiler off: median / min of 60 calls each; and the host's share of a launch (derivation
        and the stepping of the shift register to every stripe's start).
"""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
HBM_PEAK = 8.0e12


def size(s):
    w, h = s.split("x")
    return int(w), int(h)


def algorithm_bytes(s):
    """source planes read once + destination planes written once (4:2:0, 16-bit samples)"""
    return s[0] * s[1] * 3 * 2


def params():
    """luma 8 intervals with three model values, Cb 3 with two, Cr one with one: every block is grained"""
    from openvvc_amd import capi
    lo = [[256 * i // n for i in range(n)] + [0] * (8 - n) for n in (8, 3, 1)]
    hi = [[256 * (i + 1) // n - 1 for i in range(n)] + [0] * (8 - n) for n in (8, 3, 1)]
    val = [[[200 - 7 * i, 2 + (6 + i) % 13, 2 + (6 + 2 * i) % 13] if i < n else [0, 8, 8] for i in range(8)] for n in (8, 3, 1)]
    return capi.fg_params(log2_scale=2, present=(1, 1, 1), num_intervals=(8, 3, 1), num_model_values=(3, 2, 1), lower=lo, upper=hi, value=val)


def ramp_pic(ctx, w, h, seed):
    rs = np.random.RandomState(seed)
    ramp = lambda hh, ww: np.clip(np.add.outer(np.arange(hh) * 400 // hh, np.arange(ww) * 800 // ww) - 80 + rs.randint(-30, 31, (hh, ww)), 0, 1023).astype(np.uint16)
    return ctx.upload_pic(ramp(h, w), ramp(h // 2, w // 2), ramp(h // 2, w // 2))


def launches(s, n):
    from openvvc_amd import capi, engine
    ctx = engine.Context(0)
    a, b = ramp_pic(ctx, s[0], s[1], 1), ctx.new_pic(s[0], s[1])
    r, model, _ = capi.fg_derive(ctx.lib, params())
    assert r == 0
    go = lambda poc: ctx._chk(ctx.lib.ovhip_film_grain_launch(ctx.h, C.byref(a.s), C.byref(model), poc, 0, C.byref(b.s)), "film_grain")
    for k in range(20):
        go(k)
    ctx.sync()
    t0 = time.perf_counter()
    for k in range(n):
        go(k)
    ctx.sync()
    dt = (time.perf_counter() - t0) / n
    print(f"{s[0]}x{s[1]}: {n} launches, {1e6 * dt:.1f} us per launch on the host clock (seed stepping and enqueue included); "
          f"{algorithm_bytes(s) / 1e6:.2f} MB to move per launch")
    a.free(); b.free(); ctx.close()


def e2e():
    from openvvc_amd import capi, engine
    ctx = engine.Context(0)
    w, h = 3840, 2160
    pic, fg = ramp_pic(ctx, w, h, 4), params()
    calls = {"output_grain 3840x2160": lambda k: pic.output_grain(fg, k), "output 3840x2160 (no grain)": lambda k: pic.output()}
    times = {k: [] for k in calls}
    for rep in range(65):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f(rep)
            if rep >= 5:
                times[k].append(time.perf_counter() - t0)
    for k, t in times.items():
        print(f"{k}: median {1e3 * float(np.median(t)):.3f} ms, min {1e3 * min(t):.3f} ms over {len(t)} calls ({w * h * 3 / 1e6:.1f} MB downloaded each)")
    # the host's share: the derivation, and a launch's host side (the stepping to every stripe's start) with the device idle
    t0 = time.perf_counter()
    for _ in range(200):
        capi.fg_derive(ctx.lib, fg)
    print(f"ovhip_fg_derive: {1e6 * (time.perf_counter() - t0) / 200:.1f} us per call (ctypes included)")
    dst = ctx.new_pic(w, h)
    r, model, _ = capi.fg_derive(ctx.lib, fg)
    t = []
    for k in range(40):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.lib.ovhip_film_grain_launch(ctx.h, C.byref(pic.s), C.byref(model), k, 0, C.byref(dst.s))
        t.append(time.perf_counter() - t0)
    ctx.sync()
    print(f"ovhip_film_grain_launch, host side at 3840x2160: median {1e6 * float(np.median(t[5:])):.1f} us per call")
    pic.free(); dst.free(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        launches(size(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 400)
    elif mode == "share":
        nb, us = algorithm_bytes(size(sys.argv[2])), float(sys.argv[3])
        print(f"{nb / 1e6:.2f} MB in {us:.1f} us = {nb / us / 1e3:.0f} GB/s = {100 * nb / (us * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    elif mode == "e2e":
        e2e()
    else:
        sys.exit(__doc__)
