"""What an intra-block-copy hop costs in the ordered pass: the numbers LABBOOK quotes.

    python tools/micro/ibc_time.py [WxH] [N]

Two 1920x1080 (default) pictures of IBC coding units, each through the picture job with only the ordered pass's stages, under the flow
launch (default) and one launch per level (OVHIP_STAGE_INTRA_LEVELS):
    flat    16x16 CUs over the right half of every CTU but those of the first column, every source in the left half of the CTU to the left
            (which nothing writes): depth 1
    chain   the 32-chain of the fixtures' scenario a (8x8 CUs, each a copy of the one before it), tiled over the picture: 32 levels
Prints, per picture and route, tasks, levels, and the median over N (default 20) flushes of the host time from flush to wait, per picture
and per level, in microseconds.  (Host clock around flush + wait: it holds the uploads and the launch chain as well as the pass.)
"""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
FLG_IBC = 1 << 12


def record(rec, capi, cus):
    st = capi.TuState()
    for x0, y0, l2, mx, my in cus:
        d = capi.TuDesc()
        d.x0, d.y0, d.log2_tb_w, d.log2_tb_h, d.cu_flags = x0, y0, l2, l2, FLG_IBC
        r = rec.tu_ibc(st, d, capi.IbcDesc(x0, y0, l2, l2, 7, 1, mx, my, 0, 0))
        assert r >= 0, (x0, y0, mx, my, rec.refusal())


def flat(w, h):
    return [(x, y, 4, -192, 0) for y in range(0, h - 15, 16) for x in range(128, w - 15, 16) if x % 128 >= 64]


def chain(w, h):
    """rows of 32 CUs of 8x8 from x = 8 on, each a copy of its left neighbour, as many rows as fit side by side and below each other"""
    out = []
    for y in range(0, h - 7, 8):
        for x0 in range(8, w - 32 * 8 + 1, 33 * 8):
            out += [(x0 + 8 * k, y, 3, -8, 0) for k in range(32)]
    return out


def main():
    from openvvc_amd import capi, engine
    w, h = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "1920x1080").split("x"))
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    ctx = engine.Context(0)
    rs = np.random.RandomState(1)
    bg = [rs.randint(0, 1024, (h, w)).astype(np.uint16), rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16), rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16)]
    dst = ctx.upload_pic(*bg)
    for name, cus in (("flat", flat(w, h)), ("chain", chain(w, h))):
        for route, extra in (("flow", 0), ("levels", capi.STAGE_INTRA_LEVELS)):
            job = engine.Job(ctx, w, h)
            p = capi.JobParams()
            p.log2_ctu_s, p.stages = 7, capi.STAGE_MC | capi.STAGE_ITX | capi.STAGE_INTRA | extra
            times = []
            for _ in range(n + 3):
                job.begin()
                record(job.rec, capi, cus)
                ctx.sync()
                t0 = time.perf_counter()
                job.flush(dst, [], None, params=p)
                job.wait()
                times.append(time.perf_counter() - t0)
            st = job.stats()
            us = 1e6 * float(np.median(times[3:]))
            print(f"{name:5s} {route:6s} {w}x{h}: {st.n_itasks} tasks, {st.n_ilevels} levels, {st.n_launches} launches, retries {st.n_ordered_retries}: "
                  f"{us:9.1f} us per picture, {us / max(st.n_ilevels, 1):8.2f} us per level", flush=True)
            job.close()


if __name__ == "__main__":
    main()
