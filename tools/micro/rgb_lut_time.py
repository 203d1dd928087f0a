"""RGB output through a colour table (k_rgb_lut) on the device: the numbers LABBOOK 30 / DESIGN 8 f3 quote.

    python tools/micro/rgb_lut_time.py launches 3840x2160 [N] [out.json]
        per dtype (planar): k_rgb -- kernels_rgb.hip is byte for byte the parent commit's, so this IS the parent's k_rgb, in the same
        process -- then k_rgb_lut for each table size (17, 33, 65) and each of three tables: `smooth` (lut3d.pq_bt2020_to_bt709),
        `lattice` (lut3d.lattice; peak 65535, so not for U8) and `random` (the worst case for locality), then k_rgb again.  Each
        figure: warm-up, then N (default 200) launches back to back between two device events on the context's stream, divided by N
        -- the time per launch on the device clock, the gap between two launches included; three rounds, the median.  Each on two
        pictures: noise (every pixel has a cell of its own: no locality, whatever the table holds) and a smooth one (ramps:
        neighbours share cells, as in a decoded picture).  Where the loads go is the picture's doing; what the texels hold is the
        table's, and does not show (LABBOOK 30).
        The same kernel names under `rocprofv3 --kernel-trace --stats` give the kernels' own times, all tables of a dtype under one name.
    python tools/micro/rgb_lut_time.py stream [3840x2160] [threads]
        rgb_time.py's stream, three ways in one process, alternating, profiler off: OVHIP_OUT_NONE, OVHIP_OUT_NONE with RGB output on
        (F16 planar into a device-resident torch tensor of 32 slots), the same through a table (size 33, smooth).  Pictures/s each.
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
DTYPES = {0: "U8", 1: "U16", 2: "F16", 3: "F32"}


def size(s):
    w, h = s.split("x")
    return int(w), int(h)


def pictures(ctx, w, h):
    """noise (every pixel its own cell) and a smooth picture (neighbours share cells)"""
    rs = np.random.RandomState(1)
    noise = ctx.upload_pic(*(rs.randint(0, 1024, shape).astype(np.uint16) for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2))))
    yy, xx = np.mgrid[0:h, 0:w]
    y = (64 + (xx * 876 // w + yy * 3) % 877).astype(np.uint16)
    cb = (64 + (yy[:h // 2, :w // 2] * 896 // (h // 2))).astype(np.uint16)
    cr = (64 + (xx[:h // 2, :w // 2] * 896 // (w // 2))).astype(np.uint16)
    return {"noise": noise, "smooth": ctx.upload_pic(y, cb, cr)}


def tables(s, peak):
    from openvvc_amd import lut3d
    out = {"smooth": lut3d.pq_bt2020_to_bt709(s, peak), "random": np.random.default_rng(s).integers(0, peak + 1, (s, s, s, 3), dtype=np.uint16)}
    if peak == 65535:
        out["lattice"] = lut3d.lattice(s)
    return out


def launches(s, n, out=None):
    import torch
    from openvvc_amd import capi, engine
    stream = torch.cuda.Stream()
    ctx = engine.Context(0, stream=stream.cuda_stream)
    w, h = s
    pics = pictures(ctx, w, h)
    d = ctx.alloc(w * h * 3 * 4)

    def timed(fn):
        rounds = []
        for _ in range(3):
            for _ in range(20):
                fn()
            ctx.sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(n):
                fn()
            e1.record(stream)
            e1.synchronize()
            rounds.append(1e3 * e0.elapsed_time(e1) / n)
        return float(np.median(rounds)), rounds

    results = {"size": f"{w}x{h}", "launches_per_round": n, "unit": "us per launch, median of 3 rounds", "figures": {}}

    def note(name, us, r):
        results["figures"][name] = {"median_us": round(us, 2), "rounds_us": [round(v, 2) for v in r]}

    for dtype, dn in DTYPES.items():
        peak = 255 if dtype == 0 else 65535
        fmt = capi.RgbFormat(9, 0, 0, dtype, 0)
        base = {}
        for pn, pic in pics.items():
            base[pn], r = timed(lambda: pic.rgb_into(d.ptr.value, d.nbytes, fmt))
            note(f"k_rgb {dn} planar, {pn}", base[pn], r)
            print(f"{w}x{h} {dn} planar, {pn} picture, k_rgb: {base[pn]:.1f} us per launch (rounds: {', '.join(f'{v:.1f}' for v in r)})", flush=True)
        for sz in (17, 33, 65):
            for tn, table in tables(sz, peak).items():
                with engine.RgbLut(ctx, table, peak) as lut:
                    for pn, pic in pics.items():
                        us, r = timed(lambda: pic.rgb_into(d.ptr.value, d.nbytes, fmt, lut=lut))
                        note(f"k_rgb_lut {dn} planar S={sz} {tn} table, {pn}", us, r)
                        print(f"{w}x{h} {dn} planar, {pn} picture, k_rgb_lut S={sz} {tn} table: {us:.1f} us per launch = {us / base[pn]:.2f} x k_rgb "
                              f"(rounds: {', '.join(f'{v:.1f}' for v in r)})", flush=True)
        for pn, pic in pics.items():
            again, r = timed(lambda: pic.rgb_into(d.ptr.value, d.nbytes, fmt))
            note(f"k_rgb {dn} planar again, {pn}", again, r)
            print(f"{w}x{h} {dn} planar, {pn} picture, k_rgb again: {again:.1f} us per launch (first: {base[pn]:.1f})", flush=True)
    d.free(); [p.free() for p in pics.values()]; ctx.close()
    if out:
        Path(out).write_text(json.dumps(results, indent=1) + "\n")


def stream(s, threads):
    import torch
    from openvvc_amd import capi, engine, gop, lut3d
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
    fmt = engine.rgb_format(9, 0, 0, capi.RGB_F16, capi.RGB_PLANAR)
    table = lut3d.pq_bt2020_to_bt709(33, 1023)
    t = torch.zeros((32, 3, h, w), dtype=torch.float16, device="cuda:0")
    torch.cuda.synchronize()
    variants = [("OVHIP_OUT_NONE", False, False), ("OVHIP_OUT_NONE + RGB F16 planar", True, False), ("OVHIP_OUT_NONE + RGB F16 planar through a table (S=33)", True, True)]
    rates = {name: [] for name, _r, _l in variants}
    for rnd in range(3):
        for name, rgb, lut in variants:
            st = engine.Stream(dpb, w, h, contents, jobs, threads_per_device=threads, output=capi.OUT_NONE)
            arr = st.pics_array(spics)
            if rgb:
                st.set_rgb_output(t, fmt)
            if lut:
                st.set_rgb_lut(table, 1023)
            st.run(arr, n, 0, n_warm, flags=capi.STREAM_KEEP)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, _ = st.run(arr, n, n_warm, n - n_warm, flags=capi.STREAM_KEEP)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert res.status == 0 and res.n_decoded == n - n_warm
            rates[name].append((n - n_warm) / dt)
            st.close()
            print(f"round {rnd}, {name}: {rates[name][-1]:.0f} pictures/s", flush=True)
    for name, r in rates.items():
        print(f"{w}x{h} {threads} frame threads, {name}: " + ", ".join(f"{v:.0f}" for v in r) + f" pictures/s (median {float(np.median(r)):.0f})")
    assert t.any().item(), "the RGB runs wrote nothing"
    [j.close() for j in jobs]; dpb.close(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        launches(size(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 200, sys.argv[4] if len(sys.argv) > 4 else None)
    elif mode == "stream":
        stream(size(sys.argv[2]) if len(sys.argv) > 2 else (3840, 2160), int(sys.argv[3]) if len(sys.argv) > 3 else 16)
    else:
        sys.exit(__doc__)
