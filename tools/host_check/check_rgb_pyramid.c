/* tools/host_check -- the host half of the RGB pyramid (openvvc_amd/csrc/ovvc_rgb_pyramid.c) as a stand-alone program:
 * ovhip_rgb_pyramid_host over pyramids of tests/spec_rgb_pyramid.py's kind, with and without a table, every plane of the source, the
 * table and every level's tensor in a heap block of exactly its size (source strides equal to the widths; the tensor's block is
 * ovhip_rgb_bytes long), so that a read or a write one byte outside is the sanitizer's to see; every level against ovhip_rgb_host or
 * ovhip_rgb_lut_host of ovhip_output_reduce_host into blocks of their own -- the definitions the pyramid composes, which check_reduce,
 * check_rgb and check_rgb_lut hold against theirs --, byte for byte; and the refusals, which must write nothing.  `make asan`.  Host
 * code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"

#define FILL 0xA5

static uint32_t rng = 2463534242u;
static uint32_t next(void) { rng = rng * 1664525u + 1013904223u; return rng >> 12; }

static uint16_t *
plane(int w, int h, int fill)
{
    uint16_t *p = (uint16_t *)malloc((size_t)w * h * 2);
    if (!p) exit(2);
    /* a ramp along the row plus noise, so that the reduced pictures spread over the table */
    for (int i = 0; i < w * h; ++i) p[i] = fill >= 0 ? (uint16_t)fill : (uint16_t)(((i % w) * 895 / (w > 1 ? w - 1 : 1) + next() % 129) & 1023);
    return p;
}

static uint16_t *
table_of(int size, int peak)
{
    const size_t n = (size_t)3 * size * size * size;
    uint16_t *t = (uint16_t *)malloc(n * 2);
    if (!t) exit(2);
    for (size_t i = 0; i < n; ++i) t[i] = (uint16_t)(next() % ((uint32_t)peak + 1));
    return t;
}

static uint8_t *
block(size_t n)
{
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    if (!p) exit(2);
    memset(p, FILL, n);
    return p;
}

typedef struct { int w, h, dtype, layout; } level_spec;

static ovhip_rgb_format
format_of(const level_spec *g, int matrix, int full, int loc)
{
    ovhip_rgb_format f;
    memset(&f, 0, sizeof(f));
    f.matrix = (uint8_t)matrix; f.full_range = (uint8_t)full; f.chroma_loc = (uint8_t)loc; f.dtype = (uint8_t)g->dtype; f.layout = (uint8_t)g->layout;
    return f;
}

static long n_pyramids, n_levels, n_bytes, n_refused;

/* size 0: without a table */
static int
one(int w, int h, ovhip_window win, const level_spec *spec, int n, int matrix, int full, int loc, int size, int peak, int fill)
{
    uint16_t *sp[3] = { plane(w, h, fill), plane(w / 2, h / 2, fill), plane(w / 2, h / 2, fill) };
    uint16_t *table = size ? table_of(size, peak) : NULL;
    const ovhip_pic src = { sp[0], sp[1], sp[2], w, h, w, w / 2 };
    ovhip_reduce_info info;
    memset(&info, 0, sizeof(info));
    info.win = win; info.chroma_loc = (uint8_t)loc;
    ovhip_rgb_level lv[OVHIP_PYRAMID_MAX_LEVELS];
    int32_t ratio[OVHIP_PYRAMID_MAX_LEVELS][4];
    for (int k = 0; k < n; ++k) {
        lv[k].out_w = spec[k].w; lv[k].out_h = spec[k].h; lv[k].fmt = format_of(&spec[k], matrix, full, loc);
        lv[k].dst_bytes = ovhip_rgb_bytes(spec[k].w, spec[k].h, NULL, &lv[k].fmt);
        lv[k].dst = block(lv[k].dst_bytes);
    }
    int r = ovhip_rgb_pyramid_check(w, h, &info, lv, n, size, peak, ratio);
    if (r == OVHIP_OK) r = ovhip_rgb_pyramid_host(&src, &info, lv, n, size, peak, table);
    int bad = r != OVHIP_OK;
    if (bad) fprintf(stderr, "%dx%d, %d levels: %d\n", w, h, n, r);
    for (int k = 0; k < n && !bad; ++k) {
        const int W = spec[k].w, H = spec[k].h;
        uint16_t *rp[3] = { plane(W, H, 0), plane(W / 2, H / 2, 0), plane(W / 2, H / 2, 0) };
        const ovhip_pic red = { rp[0], rp[1], rp[2], W, H, W, W / 2 };
        uint8_t *want = block(lv[k].dst_bytes);
        int32_t one_ratio[4];
        bad = ovhip_output_reduce_check(w, h, &info, W, H, one_ratio) != OVHIP_OK || memcmp(one_ratio, ratio[k], sizeof(one_ratio)) != 0
              || ovhip_output_reduce_host(&src, &info, &red) != OVHIP_OK
              || (size ? ovhip_rgb_lut_host(rp[0], rp[1], rp[2], W, H, W, W / 2, NULL, &lv[k].fmt, size, peak, table, want, lv[k].dst_bytes)
                       : ovhip_rgb_host(rp[0], rp[1], rp[2], W, H, W, W / 2, NULL, &lv[k].fmt, want, lv[k].dst_bytes)) != OVHIP_OK
              || memcmp(want, lv[k].dst, lv[k].dst_bytes) != 0;
        if (bad) fprintf(stderr, "%dx%d location %d table %d level %d (%dx%d, dtype %d, layout %d): differs from rgb(reduce())\n", w, h, loc, size, k, W, H, spec[k].dtype, spec[k].layout);
        n_bytes += (long)lv[k].dst_bytes; ++n_levels;
        for (int c = 0; c < 3; ++c) free(rp[c]);
        free(want);
    }
    for (int k = 0; k < n; ++k) free(lv[k].dst);
    for (int c = 0; c < 3; ++c) free(sp[c]);
    free(table);
    ++n_pyramids;
    return bad;
}

/* a pyramid of three levels over 72x40 of which `spoil` makes one thing wrong: `want` comes back and every destination keeps the sentinel */
enum { BAD_RATIO, BAD_UP, BAD_SIZE, BAD_SIZE4, BAD_N0, BAD_N9, BAD_SMALL, BAD_NULL, BAD_UNALIGNED, BAD_OVERLAP, BAD_PICTURE, BAD_DTYPE, BAD_LAYOUT, BAD_MATRIX2,
       BAD_MATRIX3, BAD_INFO_RSV, BAD_WINDOW, BAD_PLANE, BAD_STRIDE, BAD_MIX_MATRIX, BAD_MIX_RANGE, BAD_MIX_LOC, BAD_LOC_INFO, BAD_TABLE_NULL, BAD_TABLE_SIZE, BAD_PEAK,
       BAD_PEAK_U8, BAD_ENTRY, N_BAD };
static int
refused(int spoil, int want)
{
    static const level_spec spec[3] = { { 48, 24, OVHIP_RGB_F16, OVHIP_RGB_PLANAR }, { 36, 20, OVHIP_RGB_U8, OVHIP_RGB_PACKED }, { 72, 40, OVHIP_RGB_U16, OVHIP_RGB_PLANAR } };
    uint16_t *sp[3] = { plane(72, 40, -1), plane(36, 20, -1), plane(36, 20, -1) };
    uint16_t *table = table_of(17, 255);
    const uint16_t *tab = NULL;
    ovhip_pic src = { sp[0], sp[1], sp[2], 72, 40, 72, 36 };
    ovhip_reduce_info info;
    memset(&info, 0, sizeof(info));
    ovhip_rgb_level lv[OVHIP_PYRAMID_MAX_LEVELS + 1];
    uint8_t *mem[3];
    size_t bytes[3];
    for (int k = 0; k < 3; ++k) {
        lv[k].out_w = spec[k].w; lv[k].out_h = spec[k].h; lv[k].fmt = format_of(&spec[k], 1, 0, 0);
        lv[k].dst_bytes = bytes[k] = ovhip_rgb_bytes(spec[k].w, spec[k].h, NULL, &lv[k].fmt);
        lv[k].dst = mem[k] = block(bytes[k]);
    }
    for (int k = 3; k <= OVHIP_PYRAMID_MAX_LEVELS; ++k) lv[k] = lv[0];
    int n = 3, size = 0, peak = 0;
    switch (spoil) {
    case BAD_RATIO: lv[2].out_w = 8; break;                                      /* 9/1, in the last position */
    case BAD_UP: lv[2].out_w = 144; break;
    case BAD_SIZE: lv[2].out_w = 34; break;
    case BAD_SIZE4: lv[1].out_h = 18; break;                                     /* even, but the RGB output takes multiples of 4 */
    case BAD_N0: n = 0; break;
    case BAD_N9: n = OVHIP_PYRAMID_MAX_LEVELS + 1; break;
    case BAD_SMALL: lv[2].dst_bytes -= 1; break;
    case BAD_NULL: lv[1].dst = NULL; break;
    case BAD_UNALIGNED: lv[0].dst = mem[0] + 1; lv[0].dst_bytes -= 2; lv[0].out_h = 20; break;
    case BAD_OVERLAP: lv[1].dst = mem[0] + bytes[0] - 1; break;
    case BAD_PICTURE: lv[1].dst = (uint8_t *)sp[1] + 36 * 20 * 2 - 1; break;
    case BAD_DTYPE: lv[0].fmt.dtype = 4; break;
    case BAD_LAYOUT: lv[0].fmt.layout = 2; break;
    case BAD_MATRIX2: for (int k = 0; k < 3; ++k) lv[k].fmt.matrix = 2; break;
    case BAD_MATRIX3: for (int k = 0; k < 3; ++k) lv[k].fmt.matrix = 3; break;
    case BAD_INFO_RSV: info.rsv[2] = 1; break;
    case BAD_WINDOW: info.win.offset_lft = 18; info.win.offset_rgt = 18; break;
    case BAD_PLANE: src.cb = NULL; break;
    case BAD_STRIDE: src.stride_y = 70; break;
    case BAD_MIX_MATRIX: lv[1].fmt.matrix = 9; break;
    case BAD_MIX_RANGE: lv[2].fmt.full_range = 1; break;
    case BAD_MIX_LOC: lv[1].fmt.chroma_loc = 2; break;
    case BAD_LOC_INFO: info.chroma_loc = 1; break;                               /* the pyramid's location is not the levels' */
    case BAD_TABLE_NULL: size = 17; peak = 255; break;
    case BAD_TABLE_SIZE: size = 16; peak = 255; tab = table; break;
    case BAD_PEAK: size = 17; peak = 65536; tab = table; break;
    case BAD_PEAK_U8: size = 17; peak = 256; tab = table; break;                 /* level 1 is U8 */
    case BAD_ENTRY: size = 17; peak = 255; tab = table; table[3 * 17 * 17 * 17 - 1] = 256; break;
    }
    const int r = ovhip_rgb_pyramid_host(&src, &info, lv, n, size, peak, tab);
    int bad = r != want;
    for (int k = 0; k < 3 && !bad; ++k)
        for (size_t i = 0; i < bytes[k] && !bad; ++i) bad = mem[k][i] != FILL;
    if (bad) fprintf(stderr, "refusal %d: %d (wanted %d), or something was written\n", spoil, r, want);
    for (int k = 0; k < 3; ++k) free(mem[k]);
    for (int c = 0; c < 3; ++c) free(sp[c]);
    free(table);
    ++n_refused;
    return bad;
}

int
main(void)
{
    enum { U8 = OVHIP_RGB_U8, U16 = OVHIP_RGB_U16, F16 = OVHIP_RGB_F16, F32 = OVHIP_RGB_F32, CHW = OVHIP_RGB_PLANAR, HWC = OVHIP_RGB_PACKED };
    static const ovhip_window none = { 0, 0, 0, 0 }, win = { 1, 3, 2, 2 };
    /* every dtype in both layouts: eight levels, a U8 and a U16 one -- two coefficient sets -- among them */
    static const level_spec a[] = { { 272, 48, F16, CHW }, { 204, 36, F16, HWC }, { 136, 24, U8, CHW }, { 136, 24, U8, HWC }, { 68, 12, U16, CHW }, { 100, 20, U16, HWC },
                                    { 36, 8, F32, CHW }, { 36, 8, F32, HWC } };
    static const level_spec b[] = { { 48, 24, U16, HWC }, { 36, 20, F32, CHW }, { 24, 8, F16, HWC }, { 72, 20, U16, CHW } };      /* no U8: any peak */
    static const level_spec d[] = { { 32, 32, U8, CHW }, { 16, 16, F16, CHW }, { 8, 8, U8, HWC }, { 64, 8, F32, HWC } };
    static const level_spec f[] = { { 72, 40, U8, HWC }, { 48, 24, F16, CHW }, { 36, 20, U16, CHW } };
    for (int loc = 0; loc < 6; ++loc)
        if (one(272, 48, none, a, OVHIP_PYRAMID_MAX_LEVELS, 1, 0, loc, 0, 0, -1) || one(272, 48, none, a, OVHIP_PYRAMID_MAX_LEVELS, 9, 1, loc, 17, 255, -1)
            || one(72, 40, none, b, 4, 9, 0, loc, 33, 4095, -1))
            return 1;
    if (one(64, 64, none, d, 4, 5, 0, 3, 65, 255, -1) || one(64, 64, none, d, 4, 6, 1, 3, 0, 0, -1) || one(72, 40, none, b, 4, 9, 0, 2, 17, 65535, 1023)
        || one(72, 40, none, b, 4, 9, 0, 2, 65, 1023, -1) || one(80, 48, win, f, 3, 1, 0, 1, 0, 0, -1) || one(80, 48, win, f, 3, 9, 0, 5, 17, 1, -1))
        return 1;
    static const int want[N_BAD] = { OVHIP_EUNSUP, OVHIP_EUNSUP, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL,
                                     OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EUNSUP, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL,
                                     OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL,
                                     OVHIP_EINVAL };
    for (int s = 0; s < N_BAD; ++s)
        if (refused(s, want[s])) return 1;
    printf("check_rgb_pyramid: %ld pyramids (%ld levels, %ld bytes) equal rgb(reduce()) and rgb_lut(reduce()), %ld refusals wrote nothing\n", n_pyramids, n_levels,
           n_bytes, n_refused);
    return 0;
}
