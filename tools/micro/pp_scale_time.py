"""Output resampling (k_output_scale) on the device: the numbers LABBOOK / DESIGN 4 quote.

    python tools/micro/pp_scale_time.py launches 1920x1080 3840x2160 [N]
        warm-up, then N (default 400) launches of ovhip_output_scale_launch and one synchronise: run it under
        `rocprofv3 --kernel-trace --stats -d <dir> -- python ...`, one size pair per run, and read k_output_scale's average there.
        Prints the bytes the algorithm has to move (source planes read once + destination planes written once) and, from a host
        clock around the N launches (enqueue-bound when the kernel is short: NOT the kernel time), the time per launch.
    python tools/micro/pp_scale_time.py share 1920x1080 3840x2160 <kernel_us>
        those bytes over a kernel time taken from the trace: GB/s and the share of the 8 TB/s HBM peak (no device needed).
    python tools/micro/pp_scale_time.py e2e
        ovhip_pic_output_scaled of a 1920x1080 and a 2560x1440 picture to 3840x2160 beside ovhip_pic_output of a 3840x2160
        picture (each ends in one 24.9 MB download), alternating in one process, profiler off: median / min of 60 calls each.
"""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
HBM_PEAK = 8.0e12


def size(s):
    w, h = s.split("x")
    return int(w), int(h)


def algorithm_bytes(src, dst):
    """source planes read once + destination planes written once (4:2:0, 16-bit samples)"""
    return (src[0] * src[1] + dst[0] * dst[1]) * 3


def random_pic(ctx, w, h, seed):
    rs = np.random.RandomState(seed)
    return ctx.upload_pic(rs.randint(0, 1024, (h, w)).astype(np.uint16), rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16),
                          rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16))


def launches(src, dst, n):
    from openvvc_amd import engine
    ctx = engine.Context(0)
    a, b = random_pic(ctx, src[0], src[1], 1), ctx.new_pic(dst[0], dst[1])
    for _ in range(20):
        a.scale_into(b)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        a.scale_into(b)
    ctx.sync()
    dt = (time.perf_counter() - t0) / n
    print(f"{src[0]}x{src[1]} -> {dst[0]}x{dst[1]}: {n} launches, {1e6 * dt:.1f} us per launch on the host clock (enqueue included); "
          f"{algorithm_bytes(src, dst) / 1e6:.2f} MB to move per launch")
    a.free(); b.free(); ctx.close()


def e2e():
    from openvvc_amd import engine
    ctx = engine.Context(0)
    out = (3840, 2160)
    pics = {"output_scaled 1920x1080 -> 3840x2160": random_pic(ctx, 1920, 1080, 2), "output_scaled 2560x1440 -> 3840x2160": random_pic(ctx, 2560, 1440, 3),
            "output 3840x2160 (no resampling)": random_pic(ctx, 3840, 2160, 4)}
    times = {k: [] for k in pics}
    for rep in range(65):
        for k, p in pics.items():
            t0 = time.perf_counter()
            if p.w == out[0]:
                p.output()
            else:
                p.output_scaled(*out)
            if rep >= 5:
                times[k].append(time.perf_counter() - t0)
    for k, t in times.items():
        print(f"{k}: median {1e3 * float(np.median(t)):.3f} ms, min {1e3 * min(t):.3f} ms over {len(t)} calls ({out[0] * out[1] * 3 / 1e6:.1f} MB downloaded each)")
    for p in pics.values():
        p.free()
    ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        launches(size(sys.argv[2]), size(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 400)
    elif mode == "share":
        nb, us = algorithm_bytes(size(sys.argv[2]), size(sys.argv[3])), float(sys.argv[4])
        print(f"{nb / 1e6:.2f} MB in {us:.1f} us = {nb / us / 1e3:.0f} GB/s = {100 * nb / (us * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    elif mode == "e2e":
        e2e()
    else:
        sys.exit(__doc__)
