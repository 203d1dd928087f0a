"""Numpy restatement of "Surface output on the device" (include/ovvc_hip.h), written from the header's text: a 10-bit 4:2:0 picture
as an NV12 / P010 / I420 / I010 surface with row pitches and chroma plane offsets.  Integer only: what it gives is compared for
equality with ovhip_surface_host and k_surface."""
import numpy as np

NV12, P010, I420, I010 = 0, 1, 2, 3
ROUND, DITHER = 0, 1
FORMATS = (NV12, P010, I420, I010)
ELEM = {NV12: 1, P010: 2, I420: 1, I010: 2}
SEMI = {NV12: True, P010: True, I420: False, I010: False}
# every format with every rounding it takes
MODES = [(NV12, ROUND), (NV12, DITHER), (P010, ROUND), (I420, ROUND), (I420, DITHER), (I010, ROUND)]
SIZES = [(8, 8), (16, 8), (20, 12), (34, 18), (72, 40), (136, 72), (264, 136)]
WINDOWS = [(0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 1, 0)]
EDGE_VALUES = (0, 1, 2, 3, 1020, 1021, 1022, 1023)
D = np.array([[0, 2], [3, 1]], np.int64)
FILL = 0xA5


def windows_for(w, h):
    return WINDOWS + ([(1, 1, 1, 1)] if (w, h) == (72, 40) else [])


def random_planes(w, h, seed):
    """seeded random 10-bit planes with the values at both ends of the range planted in every plane, the value moving on from row to
    row: in the first and the last column of every row (a plane has at least 4 rows: the two columns hold all eight between them), in
    the columns next to them (the first and the last under a window of one chroma sample; of two luma samples: the third from either
    end, part of the tail below) and, from 12 columns on, in the 8 columns before those, which reach into the last run of 16 (the
    row's tail)"""
    rs = np.random.RandomState(seed)
    planes = [rs.randint(0, 1024, (hh, ww)).astype(np.uint16) for hh, ww in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    E = EDGE_VALUES
    for p in planes:
        ww = p.shape[1]
        for r in range(p.shape[0]):
            if ww >= 12:
                for j in range(8):
                    p[r, ww - 3 - j] = E[(r + j) % 8]
            p[r, 0], p[r, ww - 1] = E[r % 8], E[(r + 4) % 8]
            p[r, 1], p[r, ww - 2] = E[(r + 2) % 8], E[(r + 6) % 8]
    return tuple(planes)


def crop(planes, window):
    y, cb, cr = planes
    l, r, a, b = window
    h, w = y.shape
    return (y[2 * a:h - 2 * b, 2 * l:w - 2 * r], cb[a:h // 2 - b, l:w // 2 - r], cr[a:h // 2 - b, l:w // 2 - r])


def values(plane, fmt, rounding):
    """the stored values of one OUTPUT plane (after the crop: (x, y) counts from the window's first sample)"""
    s = plane.astype(np.int64)
    if fmt == I010:
        return s.astype(np.uint16)
    if fmt == P010:
        return (s << 6).astype(np.uint16)
    if rounding == ROUND:
        return np.minimum(255, (s + 2) >> 2).astype(np.uint8)
    yy, xx = np.indices(s.shape)
    return np.minimum(255, (s + D[yy & 1, xx & 1]) >> 2).astype(np.uint8)


def out_planes(planes, fmt, rounding, window=(0, 0, 0, 0)):
    """the surface's planes as 2-D arrays of elements: [Y, CbCr interleaved] or [Y, Cb, Cr]"""
    y, cb, cr = (values(p, fmt, rounding) for p in crop(planes, window))
    if not SEMI[fmt]:
        return [y, cb, cr]
    c = np.empty((cb.shape[0], 2 * cb.shape[1]), cb.dtype)       # the Cb and the Cr of a pair were given the pair's column above
    c[:, 0::2], c[:, 1::2] = cb, cr
    return [y, c]


def layout(shapes, es, pitch_y=0, pitch_c=0, offset_c=(0, 0)):
    """[(offset, pitch, row bytes, rows)] per plane and the surface's size"""
    out, size = [], 0
    for k, (rows, elems) in enumerate(shapes):
        row = elems * es
        pitch = (pitch_c if k else pitch_y) or row
        given = offset_c[k - 1] if k else 0
        off = given or (out[-1][0] + out[-1][1] * out[-1][3] if k else 0)
        out.append((off, pitch, row, rows))
        size = max(size, off + pitch * (rows - 1) + row)
    return out, size


def surface(planes, fmt, rounding=ROUND, window=(0, 0, 0, 0), pitch_y=0, pitch_c=0, offset_c=(0, 0), total=None, fill=FILL):
    """(bytes of the surface in a buffer of `total` bytes (default: the surface's size) that held `fill` before, the surface's size)"""
    ps = out_planes(planes, fmt, rounding, window)
    lay, size = layout([p.shape for p in ps], ELEM[fmt], pitch_y, pitch_c, offset_c)
    buf = np.full(size if total is None else total, fill, np.uint8)
    for p, (off, pitch, row, rows) in zip(ps, lay):
        raw = p.astype("<u2").view(np.uint8).reshape(rows, row) if ELEM[fmt] == 2 else p
        for r in range(rows):
            buf[off + r * pitch:off + r * pitch + row] = raw[r]
    return buf, size


def loose_layout(fmt, W, H):
    """the non-tight layout of the tests: pitch_y = row bytes + one element, pitch_c = row bytes + 3 elements, the chroma plane 64 bytes
    behind the end of the luma rows' pitch, and for the planar formats a gap of 32 bytes before Cr too"""
    es = ELEM[fmt]
    pitch_y = (W + 1) * es
    pitch_c = ((W if SEMI[fmt] else W // 2) + 3) * es
    off0 = pitch_y * H + 64
    off1 = 0 if SEMI[fmt] else off0 + pitch_c * (H // 2) + 32
    return dict(pitch_y=pitch_y, pitch_c=pitch_c, offset_c=(off0, off1))
