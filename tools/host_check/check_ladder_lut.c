/* tools/host_check -- the host half of the output ladder through a colour table (openvvc_amd/csrc/ovvc_ladder_lut.c) as a stand-alone
 * program: ovhip_ladder_lut_host over ladders of tests/spec_ladder_lut.py's kind, every plane of the source, the table and every rung's
 * surface in a heap block of exactly its size (source strides equal to the widths; the surface's block is ovhip_surface_bytes long), so
 * that a read or a write one byte outside is the sanitizer's to see; every rung against ovhip_surface_lut_host of
 * ovhip_output_reduce_host into blocks of their own -- the two definitions the ladder composes, which check_reduce and
 * check_surface_lut hold against theirs --, byte for byte, the gaps of a loose layout holding the sentinel; and the refusals, which
 * must write nothing.  `make asan`.  Host code only. */
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

typedef struct { int w, h, format, rounding, loose; } rung_spec;

/* tests/spec_surface.py, loose_layout */
static ovhip_surface_format
format_of(const rung_spec *g)
{
    ovhip_surface_format f;
    memset(&f, 0, sizeof(f));
    f.format = (uint8_t)g->format; f.rounding = (uint8_t)g->rounding;
    if (g->loose) {
        const int es = g->format == OVHIP_SURF_P010 || g->format == OVHIP_SURF_I010 ? 2 : 1;
        const int semi = g->format == OVHIP_SURF_NV12 || g->format == OVHIP_SURF_P010;
        f.pitch_y = (uint32_t)((g->w + 1) * es);
        f.pitch_c = (uint32_t)(((semi ? g->w : g->w / 2) + 3) * es);
        f.offset_c[0] = (uint64_t)f.pitch_y * (uint64_t)g->h + 64;
        f.offset_c[1] = semi ? 0 : f.offset_c[0] + (uint64_t)f.pitch_c * (uint64_t)(g->h / 2) + 32;
    }
    return f;
}

static long n_ladders, n_rungs, n_bytes, n_refused;

static int
one(int w, int h, ovhip_window win, const rung_spec *spec, int n, int sloc, int dloc, int size, int peak, int fill)
{
    uint16_t *sp[3] = { plane(w, h, fill), plane(w / 2, h / 2, fill), plane(w / 2, h / 2, fill) };
    uint16_t *table = table_of(size, peak);
    const ovhip_pic src = { sp[0], sp[1], sp[2], w, h, w, w / 2 };
    const ovhip_surface_conv conv = { 9, 0, (uint8_t)sloc, 1, 0, (uint8_t)dloc, { 0, 0 } };
    ovhip_reduce_info info;
    memset(&info, 0, sizeof(info));
    info.win = win; info.chroma_loc = (uint8_t)sloc;
    ovhip_ladder_rung rungs[OVHIP_LADDER_MAX_RUNGS];
    int32_t ratio[OVHIP_LADDER_MAX_RUNGS][4];
    for (int k = 0; k < n; ++k) {
        rungs[k].out_w = spec[k].w; rungs[k].out_h = spec[k].h; rungs[k].fmt = format_of(&spec[k]);
        rungs[k].dst_bytes = ovhip_surface_bytes(spec[k].w, spec[k].h, NULL, &rungs[k].fmt);
        rungs[k].dst = block(rungs[k].dst_bytes);
    }
    int r = ovhip_ladder_lut_check(w, h, &info, rungs, n, &conv, size, peak, ratio);
    if (r == OVHIP_OK) r = ovhip_ladder_lut_host(&src, &info, rungs, n, &conv, size, peak, table);
    int bad = r != OVHIP_OK;
    if (bad) fprintf(stderr, "%dx%d, %d rungs: %d\n", w, h, n, r);
    for (int k = 0; k < n && !bad; ++k) {
        const int W = spec[k].w, H = spec[k].h;
        uint16_t *rp[3] = { plane(W, H, 0), plane(W / 2, H / 2, 0), plane(W / 2, H / 2, 0) };
        const ovhip_pic red = { rp[0], rp[1], rp[2], W, H, W, W / 2 };
        uint8_t *want = block(rungs[k].dst_bytes);
        int32_t one_ratio[4];
        bad = ovhip_output_reduce_check(w, h, &info, W, H, one_ratio) != OVHIP_OK || memcmp(one_ratio, ratio[k], sizeof(one_ratio)) != 0
              || ovhip_output_reduce_host(&src, &info, &red) != OVHIP_OK
              || ovhip_surface_lut_host(rp[0], rp[1], rp[2], W, H, W, W / 2, NULL, &conv, &rungs[k].fmt, size, peak, table, want, rungs[k].dst_bytes) != OVHIP_OK
              || memcmp(want, rungs[k].dst, rungs[k].dst_bytes) != 0;
        if (bad) fprintf(stderr, "%dx%d locations %d -> %d rung %d (%dx%d, format %d): differs from surface_lut(reduce())\n", w, h, sloc, dloc, k, W, H, spec[k].format);
        n_bytes += (long)rungs[k].dst_bytes; ++n_rungs;
        for (int c = 0; c < 3; ++c) free(rp[c]);
        free(want);
    }
    for (int k = 0; k < n; ++k) free(rungs[k].dst);
    for (int c = 0; c < 3; ++c) free(sp[c]);
    free(table);
    ++n_ladders;
    return bad;
}

/* a ladder of three rungs over 72x40 of which `spoil` makes one thing wrong: `want` comes back and every destination keeps the sentinel */
enum { BAD_RATIO, BAD_UP, BAD_SIZE, BAD_N0, BAD_N9, BAD_SMALL, BAD_NULL, BAD_OVERLAP, BAD_PICTURE, BAD_FORMAT, BAD_INFO_RSV, BAD_WINDOW, BAD_PLANE,
       BAD_CONV_NULL, BAD_CONV_RSV, BAD_SRC_MATRIX, BAD_DST_MATRIX, BAD_DST_LOC4, BAD_DST_LOC6, BAD_TABLE_NULL, BAD_TABLE_SIZE, BAD_PEAK, BAD_ENTRY, BAD_LOC_INFO,
       BAD_LOC_CONV, N_BAD };
static int
refused(int spoil, int want)
{
    static const rung_spec spec[3] = { { 48, 24, OVHIP_SURF_P010, 0, 0 }, { 36, 20, OVHIP_SURF_NV12, 1, 1 }, { 72, 40, OVHIP_SURF_I420, 0, 0 } };
    uint16_t *sp[3] = { plane(72, 40, -1), plane(36, 20, -1), plane(36, 20, -1) };
    uint16_t *table = table_of(17, 1023);
    const uint16_t *tab = table;
    ovhip_pic src = { sp[0], sp[1], sp[2], 72, 40, 72, 36 };
    ovhip_surface_conv conv = { 9, 0, 0, 1, 0, 0, { 0, 0 } };
    const ovhip_surface_conv *cv = &conv;
    ovhip_reduce_info info;
    memset(&info, 0, sizeof(info));
    ovhip_ladder_rung rungs[OVHIP_LADDER_MAX_RUNGS + 1];
    uint8_t *mem[3];
    size_t bytes[3];
    for (int k = 0; k < 3; ++k) {
        rungs[k].out_w = spec[k].w; rungs[k].out_h = spec[k].h; rungs[k].fmt = format_of(&spec[k]);
        rungs[k].dst_bytes = bytes[k] = ovhip_surface_bytes(spec[k].w, spec[k].h, NULL, &rungs[k].fmt);
        rungs[k].dst = mem[k] = block(bytes[k]);
    }
    for (int k = 3; k <= OVHIP_LADDER_MAX_RUNGS; ++k) rungs[k] = rungs[0];
    int n = 3, size = 17, peak = 1023;
    switch (spoil) {
    case BAD_RATIO: rungs[2].out_w = 8; break;                                   /* 9/1, in the last position */
    case BAD_UP: rungs[2].out_w = 144; break;
    case BAD_SIZE: rungs[2].out_w = 34; break;
    case BAD_N0: n = 0; break;
    case BAD_N9: n = OVHIP_LADDER_MAX_RUNGS + 1; break;
    case BAD_SMALL: rungs[2].dst_bytes -= 1; break;
    case BAD_NULL: rungs[1].dst = NULL; break;
    case BAD_OVERLAP: rungs[1].dst = mem[0] + bytes[0] - 1; break;
    case BAD_PICTURE: rungs[2].dst = (uint8_t *)sp[1] + 36 * 20 * 2 - 1; break;
    case BAD_FORMAT: rungs[0].fmt.rounding = 1; break;                           /* P010 takes rounding 0 only */
    case BAD_INFO_RSV: info.rsv[2] = 1; break;
    case BAD_WINDOW: info.win.offset_lft = 18; info.win.offset_rgt = 18; break;
    case BAD_PLANE: src.cb = NULL; break;
    case BAD_CONV_NULL: cv = NULL; break;
    case BAD_CONV_RSV: conv.rsv[0] = 1; break;
    case BAD_SRC_MATRIX: conv.src_matrix = 0; break;
    case BAD_DST_MATRIX: conv.dst_matrix = 2; break;
    case BAD_DST_LOC4: conv.dst_chroma_loc = 4; break;
    case BAD_DST_LOC6: conv.dst_chroma_loc = 6; break;
    case BAD_TABLE_NULL: tab = NULL; break;
    case BAD_TABLE_SIZE: size = 16; break;
    case BAD_PEAK: peak = 65536; break;
    case BAD_ENTRY: table[3 * 17 * 17 * 17 - 1] = 1024; break;
    case BAD_LOC_INFO: info.chroma_loc = 1; break;                               /* the ladder's location is not the conversion's */
    case BAD_LOC_CONV: conv.src_chroma_loc = 2; break;
    }
    const int r = ovhip_ladder_lut_host(&src, &info, rungs, n, cv, size, peak, tab);
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
    enum { NV12 = OVHIP_SURF_NV12, P010 = OVHIP_SURF_P010, I420 = OVHIP_SURF_I420, I010 = OVHIP_SURF_I010 };
    static const ovhip_window none = { 0, 0, 0, 0 }, win = { 1, 3, 2, 2 };
    static const rung_spec a[] = { { 272, 48, I010, 0, 0 }, { 136, 24, NV12, 0, 0 }, { 204, 36, P010, 0, 0 }, { 68, 12, I420, 1, 0 }, { 36, 8, NV12, 1, 0 } };
    static const rung_spec b[] = { { 48, 24, P010, 0, 1 }, { 36, 20, I420, 1, 1 }, { 24, 8, NV12, 0, 1 }, { 72, 20, I010, 0, 1 } };
    static const rung_spec d[] = { { 32, 32, NV12, 1, 0 }, { 16, 16, NV12, 1, 0 }, { 8, 8, NV12, 1, 0 }, { 64, 8, NV12, 1, 0 } };
    static const rung_spec e[] = { { 132, 132, NV12, 0, 0 }, { 512, 512, P010, 0, 0 } };
    static const rung_spec f[] = { { 72, 40, NV12, 0, 0 }, { 48, 24, I010, 0, 0 }, { 36, 20, P010, 0, 0 } };
    static const rung_spec m[] = { { 72, 40, I010, 0, 0 }, { 48, 24, NV12, 0, 0 }, { 36, 20, P010, 0, 0 }, { 24, 8, I420, 1, 0 }, { 72, 20, NV12, 1, 0 },
                                   { 36, 40, I420, 0, 0 }, { 48, 24, P010, 0, 1 }, { 36, 20, I010, 0, 1 } };
    for (int sloc = 0; sloc < 6; ++sloc)
        for (int dloc = 0; dloc < 4; ++dloc)
            if (one(272, 48, none, a, 5, sloc, dloc, 17, 1023, -1) || one(72, 40, none, b, 4, sloc, dloc, 33, 4095, -1)) return 1;
    if (one(64, 64, none, d, 4, 0, 3, 65, 255, -1) || one(1024, 1024, none, e, 2, 0, 2, 17, 1023, -1) || one(1024, 1024, none, e, 2, 0, 2, 17, 65535, 1023)
        || one(80, 48, win, f, 3, 0, 1, 65, 255, -1) || one(80, 48, win, f, 3, 5, 2, 17, 1, -1) || one(72, 40, none, m, OVHIP_LADDER_MAX_RUNGS, 0, 0, 33, 1023, -1))
        return 1;
    static const int want[N_BAD] = { OVHIP_EUNSUP, OVHIP_EUNSUP, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL,
                                     OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL,
                                     OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EUNSUP, OVHIP_EINVAL, OVHIP_EUNSUP, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL,
                                     OVHIP_EINVAL, OVHIP_EINVAL, OVHIP_EINVAL };
    for (int s = 0; s < N_BAD; ++s)
        if (refused(s, want[s])) return 1;
    printf("check_ladder_lut: %ld ladders (%ld rungs, %ld bytes) equal surface_lut(reduce()), %ld refusals wrote nothing\n", n_ladders, n_rungs, n_bytes, n_refused);
    return 0;
}
