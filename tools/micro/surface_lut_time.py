"""Surface output through a colour table (k_surface_lut) on the device: the numbers LABBOOK 35 / DESIGN 8 f3 quote.

    python tools/micro/surface_lut_time.py launches 3840x2160 [N] [out.json]
        k_surface_lut for NV12 and P010, destination chroma locations 0 (co-sited, centred: a halo column), 1 (centred both ways: no
        halo) and 2 (co-sited, top: a halo column and a halo row), a table of 33 points (lut3d.pq_bt2020_to_bt709, peak 1023), BT.2020
        limited to BT.709 limited; beside them, in the same process, k_rgb_lut U8 planar through the same table at peak 255 (the same
        gathers without the way back) and k_surface NV12 (the same store without the conversion).  Each figure: warm-up, then N
        (default 200) launches back to back between two device events on the context's stream, divided by N -- the time per launch on
        the device clock, the gap between two launches included; three rounds, the median.  Each on two pictures: noise (every pixel
        has a cell of its own: no locality) and a smooth one (ramps: neighbours share cells, as in a decoded picture).
    python tools/micro/surface_lut_time.py stream [3840x2160] [threads] [out.json]
        rgb_lut_time.py's stream, three ways in one process, alternating, profiler off: OVHIP_OUT_NONE, OVHIP_OUT_NONE with NV12
        surfaces into a device-resident torch tensor of 32 slots, the same through the table.  Pictures/s each.
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools" / "micro"))

from rgb_lut_time import pictures, size          # noqa: E402  (the same two pictures as k_rgb_lut's figures)


def launches(s, n, out):
    import torch
    from openvvc_amd import capi, engine, lut3d
    stream = torch.cuda.Stream()
    ctx = engine.Context(0, stream=stream.cuda_stream)
    w, h = s
    pics = pictures(ctx, w, h)
    d = ctx.alloc(w * h * 3)

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

    results = {"size": f"{w}x{h}", "launches_per_round": n, "table_points": 33, "unit": "us per launch, median of 3 rounds", "figures": {}}

    def report(name, pn, fn):
        us, r = timed(fn)
        results["figures"][f"{name}, {pn}"] = {"median_us": round(us, 2), "rounds_us": [round(v, 2) for v in r]}
        print(f"{w}x{h} {pn} picture, {name}: {us:.1f} us per launch (rounds: {', '.join(f'{v:.1f}' for v in r)})", flush=True)
        return us

    nv12, p010 = engine.surface_format(capi.SURF_NV12), engine.surface_format(capi.SURF_P010)
    rgb8 = capi.RgbFormat(9, 0, 2, capi.RGB_U8, capi.RGB_PLANAR)
    with engine.RgbLut(ctx, lut3d.pq_bt2020_to_bt709(33, 1023), 1023) as lut, engine.RgbLut(ctx, lut3d.pq_bt2020_to_bt709(33, 255), 255) as lut8:
        for pn, pic in pics.items():
            report("k_surface NV12", pn, lambda: pic.surface_into(d.ptr.value, d.nbytes, nv12))
            report("k_rgb_lut U8 planar", pn, lambda: pic.rgb_into(d.ptr.value, d.nbytes, rgb8, lut=lut8))
            for fn_, fmt in (("NV12", nv12), ("P010", p010)):
                for dloc in (0, 1, 2):
                    conv = engine.surface_conv(9, 0, 2, 1, 0, dloc)
                    report(f"k_surface_lut {fn_} dst_chroma_loc {dloc}", pn, lambda: pic.surface_into(d.ptr.value, d.nbytes, fmt, lut=lut, conv=conv))
            report("k_surface NV12 again", pn, lambda: pic.surface_into(d.ptr.value, d.nbytes, nv12))
    d.free(); [p.free() for p in pics.values()]; ctx.close()
    if out:
        Path(out).write_text(json.dumps(results, indent=1) + "\n")


def stream(s, threads, out):
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
    fmt = engine.surface_format(capi.SURF_NV12)
    table = lut3d.pq_bt2020_to_bt709(33, 1023)
    t = torch.zeros((32, w * h * 3 // 2), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    variants = [("OVHIP_OUT_NONE", False, False), ("OVHIP_OUT_NONE + NV12 surfaces", True, False), ("OVHIP_OUT_NONE + NV12 surfaces through a table (S=33)", True, True)]
    rates = {name: [] for name, _r, _l in variants}
    for rnd in range(3):
        for name, surf, lut in variants:
            st = engine.Stream(dpb, w, h, contents, jobs, threads_per_device=threads, output=capi.OUT_NONE)
            arr = st.pics_array(spics)
            if surf:
                st.set_surface_output(t, fmt)
            if lut:
                st.set_surface_lut(table, 1023, engine.surface_conv())
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
    assert t.any().item(), "the surface runs wrote nothing"
    [j.close() for j in jobs]; dpb.close(); ctx.close()
    if out:
        Path(out).write_text(json.dumps({"size": f"{w}x{h}", "frame_threads": threads, "unit": "pictures/s, three alternating rounds",
                                         "rates": {k: [round(v, 1) for v in r] for k, r in rates.items()},
                                         "medians": {k: round(float(np.median(r)), 1) for k, r in rates.items()}}, indent=1) + "\n")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "launches":
        launches(size(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 200, sys.argv[4] if len(sys.argv) > 4 else None)
    elif mode == "stream":
        stream(size(sys.argv[2]) if len(sys.argv) > 2 else (3840, 2160), int(sys.argv[3]) if len(sys.argv) > 3 else 16, sys.argv[4] if len(sys.argv) > 4 else None)
    else:
        sys.exit(__doc__)
