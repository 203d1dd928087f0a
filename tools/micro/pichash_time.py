"""Decoded picture hash (k_pic_hash, k_pic_hash_rows) on the device: the numbers LABBOOK / DESIGN 4 quote.

    python tools/micro/pichash_time.py launches 3840x2160 [N]
        warm-up, then N (default 400) launches of ovhip_pic_hash_launch per method (CRC, then checksum) and one synchronise each:
        run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...`, one size per run, and read the averages of
        k_pic_hash<true> (CRC), k_pic_hash<false> (checksum) and k_pic_hash_rows<...> there.  Prints the bytes the algorithm has to
        move (the planes read once) and, from a host clock around the N launches (enqueue included: NOT the kernel time), the time
        per launch.
    python tools/micro/pichash_time.py share 3840x2160 <kernel_us>
        those bytes over a kernel time taken from the trace: GB/s and the share of the 8 TB/s HBM peak (no device needed).
    python tools/micro/pichash_time.py e2e [3840x2160]
        ovhip_pic_hash (CRC, checksum: 12 bytes leave the device) beside ovhip_pic_download of the same picture (24.9 MB at 4K,
        the floor of any host route), alternating in one process, profiler off: median / min of 60 calls each.  The MD5 route
        (download + host MD5 on the calling thread) is timed over 5 calls.  Exits non-zero if a device route is not below the
        download.
"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
HBM_PEAK = 8.0e12
CRC, CHECKSUM, MD5 = 1, 2, 0


def size(s):
    w, h = s.split("x")
    return int(w), int(h)


def algorithm_bytes(s):
    """the three planes read once (4:2:0, 16-bit samples); 12 bytes are written"""
    return s[0] * s[1] * 3


def noise_pic(ctx, w, h, seed):
    rs = np.random.RandomState(seed)
    return ctx.upload_pic(*(rs.randint(0, 1024, shape).astype(np.uint16) for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2))))


def launches(s, n):
    from openvvc_amd import engine
    ctx = engine.Context(0)
    pic, d = noise_pic(ctx, s[0], s[1], 1), ctx.alloc(12)
    for method, name in ((CRC, "CRC"), (CHECKSUM, "checksum")):
        for _ in range(20):
            pic.hash_launch(method, 3, d)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            pic.hash_launch(method, 3, d)
        ctx.sync()
        dt = (time.perf_counter() - t0) / n
        print(f"{s[0]}x{s[1]} {name}: {n} launches, {1e6 * dt:.1f} us per launch on the host clock (enqueue included); "
              f"{algorithm_bytes(s) / 1e6:.2f} MB to read per launch")
    d.free(); pic.free(); ctx.close()


def e2e(s):
    from openvvc_amd import engine
    import spec_pic_hash as sp
    ctx = engine.Context(0)
    w, h = s
    pic = noise_pic(ctx, w, h, 4)
    planes = pic.download()
    for method in (CRC, CHECKSUM):                                      # faster and different is not faster
        assert pic.hash(method).planes() == sp.picture_hash(method, planes), method
    calls = {"pic_hash CRC": lambda: pic.hash(CRC), "pic_hash checksum": lambda: pic.hash(CHECKSUM), "pic_download": lambda: pic.download()}
    times = {k: [] for k in calls}
    for rep in range(65):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            if rep >= 5:
                times[k].append(time.perf_counter() - t0)
    med = {}
    for k, t in times.items():
        med[k] = float(np.median(t))
        print(f"{w}x{h} {k}: median {1e3 * med[k]:.3f} ms, min {1e3 * min(t):.3f} ms over {len(t)} calls")
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        pic.hash(MD5)
        t.append(time.perf_counter() - t0)
    print(f"{w}x{h} pic_hash MD5 (download + host MD5, the conformance route): median {1e3 * float(np.median(t)):.1f} ms over {len(t)} calls")
    pic.free(); ctx.close()
    ok = med["pic_hash CRC"] < med["pic_download"] and med["pic_hash checksum"] < med["pic_download"]
    print("device routes below the download alone:", "yes" if ok else "NO")
    return 0 if ok else 1


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        launches(size(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 400)
    elif mode == "share":
        nb, us = algorithm_bytes(size(sys.argv[2])), float(sys.argv[3])
        print(f"{nb / 1e6:.2f} MB in {us:.1f} us = {nb / us / 1e3:.0f} GB/s = {100 * nb / (us * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    elif mode == "e2e":
        sys.exit(e2e(size(sys.argv[2]) if len(sys.argv) > 2 else (3840, 2160)))
    else:
        sys.exit(__doc__)
