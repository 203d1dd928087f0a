/* tools/host_check -- the host half of the surface output through a colour table (openvvc_amd/csrc/ovvc_surface_lut.c, on top of
 * ovvc_rgb.c, ovvc_rgb_lut.c and ovvc_surface.c) as a stand-alone program: ovhip_surface_lut_host over a few small pictures and
 * windows, the three table sizes, the four formats, the four destination chroma locations, tight and with a pitch with gaps -- every
 * plane, every table and every destination in a heap block of exactly its size, so that a read or a write one element outside is the
 * sanitizer's to see (the halo column and row of the destination's filter at every edge of the window among them); the two corners of
 * the table (a picture that clips to 1023 in every channel reads the table's last entry and nothing behind it); the coefficients'
 * sums; every refusal, which must write nothing; and a picture mapped just above an address inside this program's own image, which
 * must be accepted like any other (the plan has no destination but the surface's to hold against the picture).  With the argument
 * `divisions` it checks the normalising division for EVERY o <= P <= 65535 (2.1e9 cases, seconds) and nothing else.  `make asan`.
 * Host code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include "ovvc_hip.h"
#include "ovvc_surface_lut_priv.h"

static uint32_t rng = 97531;
static uint32_t next(void) { rng = rng * 1664525u + 1013904223u; return rng >> 12; }

static uint16_t *
block(size_t n, uint32_t mod, int fixed)
{
    uint16_t *p = (uint16_t *)malloc(n * 2);
    if (!p) exit(2);
    for (size_t i = 0; i < n; ++i) p[i] = (uint16_t)(fixed >= 0 ? (uint32_t)fixed : next() % mod);
    return p;
}

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); return 1; } while (0)

static int
refusals(void)
{
    enum { W = 24, H = 8 };
    uint16_t *y = block(W * H, 1024, -1), *cb = block(W * H / 4, 1024, -1), *cr = block(W * H / 4, 1024, -1);
    uint16_t *table = block((size_t)3 * 17 * 17 * 17, 1024, -1), *above = block((size_t)3 * 17 * 17 * 17, 1024, -1);
    above[3 * 17 * 17 * 17 - 1] = 1024;
    const ovhip_surface_conv ok = { 9, 0, 2, 1, 0, 0, { 0, 0 } }, rsv = { 9, 0, 2, 1, 0, 0, { 0, 1 } }, src2 = { 2, 0, 2, 1, 0, 0, { 0, 0 } },
                             src0 = { 0, 0, 2, 1, 0, 0, { 0, 0 } }, sloc = { 9, 0, 6, 1, 0, 0, { 0, 0 } }, dst2 = { 9, 0, 2, 2, 0, 0, { 0, 0 } },
                             dst0 = { 9, 0, 2, 0, 0, 0, { 0, 0 } }, dloc4 = { 9, 0, 2, 1, 0, 4, { 0, 0 } }, dloc6 = { 9, 0, 2, 1, 0, 6, { 0, 0 } },
                             drange = { 9, 0, 2, 1, 2, 0, { 0, 0 } };
    ovhip_surface_format fmt, dither16, low_pitch;
    memset(&fmt, 0, sizeof(fmt));
    fmt.format = OVHIP_SURF_P010;
    dither16 = fmt; dither16.rounding = OVHIP_SURF_DITHER;
    low_pitch = fmt; low_pitch.pitch_y = 2 * W - 2;
    const ovhip_window none = { 6, 6, 0, 0 };
    const size_t n = ovhip_surface_bytes(W, H, NULL, &fmt);
    uint8_t *dst = (uint8_t *)malloc(n);
    if (!dst) return 2;
    memset(dst, 0xA5, n);
#define CALL(y_, cb_, w_, sy_, win_, conv_, fmt_, s_, p_, t_, d_, n_) ovhip_surface_lut_host(y_, cb_, cr, w_, H, sy_, W / 2, win_, conv_, fmt_, s_, p_, t_, d_, n_)
    struct { const char *what; int got, want; } c[] = {
        { "null conversion", CALL(y, cb, W, W, NULL, NULL, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "conv rsv", CALL(y, cb, W, W, NULL, &rsv, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "source matrix unspecified", CALL(y, cb, W, W, NULL, &src2, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "source matrix not built", CALL(y, cb, W, W, NULL, &src0, &fmt, 17, 1023, table, dst, n), OVHIP_EUNSUP },
        { "source chroma location", CALL(y, cb, W, W, NULL, &sloc, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "destination matrix unspecified", CALL(y, cb, W, W, NULL, &dst2, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "destination matrix not built", CALL(y, cb, W, W, NULL, &dst0, &fmt, 17, 1023, table, dst, n), OVHIP_EUNSUP },
        { "destination chroma location 4", CALL(y, cb, W, W, NULL, &dloc4, &fmt, 17, 1023, table, dst, n), OVHIP_EUNSUP },
        { "destination chroma location 6", CALL(y, cb, W, W, NULL, &dloc6, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "destination range", CALL(y, cb, W, W, NULL, &drange, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "null table", CALL(y, cb, W, W, NULL, &ok, &fmt, 17, 1023, NULL, dst, n), OVHIP_EINVAL },
        { "size 16", CALL(y, cb, W, W, NULL, &ok, &fmt, 16, 1023, table, dst, n), OVHIP_EINVAL },
        { "peak 0", CALL(y, cb, W, W, NULL, &ok, &fmt, 17, 0, table, dst, n), OVHIP_EINVAL },
        { "peak 65536", CALL(y, cb, W, W, NULL, &ok, &fmt, 17, 65536, table, dst, n), OVHIP_EINVAL },
        { "entry above the peak", CALL(y, cb, W, W, NULL, &ok, &fmt, 17, 1023, above, dst, n), OVHIP_EINVAL },
        { "null format", CALL(y, cb, W, W, NULL, &ok, NULL, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "dither on a 16-bit format", CALL(y, cb, W, W, NULL, &ok, &dither16, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "pitch below the row", CALL(y, cb, W, W, NULL, &ok, &low_pitch, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "null destination", CALL(y, cb, W, W, NULL, &ok, &fmt, 17, 1023, table, NULL, n), OVHIP_EINVAL },
        { "destination too small", CALL(y, cb, W, W, NULL, &ok, &fmt, 17, 1023, table, dst, n - 1), OVHIP_EINVAL },
        { "misaligned destination", CALL(y, cb, W, W, NULL, &ok, &fmt, 17, 1023, table, dst + 1, n - 1), OVHIP_EINVAL },
        { "overlapping destination", CALL(y, cb, W, W, NULL, &ok, &fmt, 17, 1023, table, y, 1 << 20), OVHIP_EINVAL },
        { "window leaves nothing", CALL(y, cb, W, W, &none, &ok, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "missing plane", CALL(y, NULL, W, W, NULL, &ok, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "stride below the width", CALL(y, cb, W, W - 1, NULL, &ok, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "width no multiple of 4", CALL(y, cb, W - 2, W, NULL, &ok, &fmt, 17, 1023, table, dst, n), OVHIP_EINVAL },
    };
#undef CALL
    for (unsigned i = 0; i < sizeof(c) / sizeof(c[0]); ++i) if (c[i].got != c[i].want) FAIL("refusal \"%s\": %d, not %d", c[i].what, c[i].got, c[i].want);
    for (size_t i = 0; i < n; ++i) if (dst[i] != 0xA5) FAIL("a refusal wrote");
    if (ovhip_surface_lut_check(&ok, &fmt, 17, 1023) != OVHIP_OK || ovhip_surface_lut_check(&dloc4, &fmt, 17, 1023) != OVHIP_EUNSUP ||
        ovhip_surface_lut_check(&ok, &dither16, 17, 1023) != OVHIP_EINVAL || ovhip_surface_lut_check(&ok, &fmt, 34, 1023) != OVHIP_EINVAL) FAIL("check");
    free(dst); free(above); free(table); free(y); free(cb); free(cr);
    printf("%u refusals\n", (unsigned)(sizeof(c) / sizeof(c[0])));
    return 0;
}

static int
coefficients(void)
{
    static const uint8_t m[] = { 1, 5, 6, 9 };
    for (unsigned k = 0; k < 4; ++k) for (uint8_t full = 0; full < 2; ++full) {
        const ovhip_surface_conv cv = { 9, 0, 0, m[k], full, 0, { 0, 0 } };
        int32_t c[9], yoff;
        if (ovhip_surface_lut_coefs(&cv, c, &yoff) != OVHIP_OK) FAIL("coefs %u %u", m[k], full);
        if (c[3] + c[4] + c[5] || c[6] + c[7] + c[8] || c[0] + c[1] + c[2] != (full ? 16384 : 14030) || yoff != (full ? 0 : 64)) FAIL("coefficient sums %u %u", m[k], full);
    }
    /* the normalising division against the plain one, at the peaks' ends and around the estimate's worst cases */
    static const uint32_t P[] = { 1, 2, 3, 255, 1023, 4000, 16368, 32767, 65534, 65535 };
    for (unsigned k = 0; k < sizeof(P) / sizeof(P[0]); ++k) {
        const float rcp = 1.0f / (float)P[k];
        for (uint32_t o = 0; o <= P[k]; ++o)
            if ((uint32_t)ovhip_surface_lut_norm_(o, P[k], rcp) != (16368u * o + P[k] / 2) / P[k]) FAIL("division %u / %u", o, P[k]);
    }
    return 0;
}

/* a picture whose planes lie a little above an address inside this program's image: no range but the surface's own is held against
 * the picture, so where the planes lie relative to the library's statics must not matter.  The mapping is asked for at a hint (not
 * forced: nothing of the process is replaced); where the kernel puts it elsewhere the next distance is tried, and the case says how
 * near it got. */
static int
near_the_image(void)
{
    enum { W = 1024, H = 512 };
    static char anchor[64];
    const size_t ny = (size_t)W * H, nc = ny / 4, bytes = (ny + 2 * nc) * 2, reach = 6 * ny;      /* reach: the bytes of an RGB picture of 16-bit elements */
    uint16_t *table = block((size_t)3 * 17 * 17 * 17, 1024, -1);
    ovhip_surface_format fmt;
    memset(&fmt, 0, sizeof(fmt));
    const ovhip_surface_conv cv = { 9, 0, 2, 1, 0, 0, { 0, 0 } };
    const size_t n = ovhip_surface_bytes(W, H, NULL, &fmt);
    uint8_t *dst = (uint8_t *)malloc(n);
    if (!dst) return 2;
    int placed = 0;
    for (size_t mb = 1; mb <= 2 && !placed; ++mb) {
        const uintptr_t hint = (((uintptr_t)anchor + (mb << 20)) + 4095) & ~(uintptr_t)4095;
        void *m = mmap((void *)hint, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) continue;
        uint16_t *y = (uint16_t *)m, *cb = y + ny, *cr = cb + nc;
        for (size_t i = 0; i < ny + 2 * nc; ++i) y[i] = (uint16_t)(next() % 1024);
        placed = (uintptr_t)m > (uintptr_t)anchor && (uintptr_t)m - (uintptr_t)anchor < reach;
        const int r = ovhip_surface_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &cv, &fmt, 17, 1023, table, dst, n);
        munmap(m, bytes);
        if (r != OVHIP_OK) FAIL("a picture %zu bytes above the image: %d", (size_t)((uintptr_t)m - (uintptr_t)anchor), r);
    }
    free(dst); free(table);
    printf("a picture near the image: accepted%s\n", placed ? "" : " (the mapping was not granted near the image: not seen this time)");
    return 0;
}

static int
all_divisions(void)
{
    for (uint32_t P = 1; P <= 65535; ++P) {
        const float rcp = 1.0f / (float)P;
        for (uint32_t o = 0; o <= P; ++o)
            if ((uint32_t)ovhip_surface_lut_norm_(o, P, rcp) != (16368u * o + P / 2) / P) FAIL("division %u / %u", o, P);
    }
    printf("every division o <= P <= 65535 exact\n");
    return 0;
}

int
main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "divisions")) return all_divisions();
    if (refusals() || coefficients() || near_the_image()) return 1;
    static const int sizes[][2] = { { 8, 8 }, { 20, 12 }, { 72, 40 } };
    static const ovhip_window wins[] = { { 0, 0, 0, 0 }, { 1, 0, 0, 1 }, { 1, 1, 1, 1 } };
    static const int S[] = { 17, 33, 65 };
    static const int peaks[] = { 255, 65535, 4000 };
    long n_ok = 0;
    uint64_t sum = 0;
    for (unsigned si = 0; si < 3; ++si) {
        const int sz = S[si], peak = peaks[si];
        const size_t cells = (size_t)sz * sz * sz;
        uint16_t *table = block(3 * cells, (uint32_t)peak + 1, -1);
        for (unsigned s = 0; s < 3; ++s) {
            const int w = sizes[s][0], h = sizes[s][1];
            /* pass 0: random planes; pass 1: every pixel clips to (1023, 1023, 1023): the table's last entry; pass 2: to (0, 0, 0) */
            for (int pass = 0; pass < 3; ++pass) {
                uint16_t *y = block((size_t)w * h, 1024, pass == 0 ? -1 : (pass == 1 ? 1023 : 0));
                uint16_t *cb = block((size_t)w * h / 4, 1024, pass == 0 ? -1 : 512), *cr = block((size_t)w * h / 4, 1024, pass == 0 ? -1 : 512);
                for (int f = 0; f < 4; ++f) for (uint8_t dloc = 0; dloc < 4; ++dloc) for (unsigned k = 0; k < 3; ++k) for (int gaps = 0; gaps < 2; ++gaps) {
                    const int W = w - 2 * (wins[k].offset_lft + wins[k].offset_rgt), H = h - 2 * (wins[k].offset_abv + wins[k].offset_blw);
                    const int es = (f == OVHIP_SURF_P010 || f == OVHIP_SURF_I010) ? 2 : 1, semi = f == OVHIP_SURF_NV12 || f == OVHIP_SURF_P010;
                    const ovhip_surface_conv cv = { 9, 0, (uint8_t)(k ? 2 : 1), (uint8_t)(dloc & 1 ? 1 : 9), (uint8_t)(dloc >> 1), dloc, { 0, 0 } };
                    ovhip_surface_format fmt;
                    memset(&fmt, 0, sizeof(fmt));
                    fmt.format = (uint8_t)f;
                    fmt.rounding = (uint8_t)(es == 1 && (dloc & 1));
                    if (gaps) {
                        fmt.pitch_y = (uint32_t)((W + 1) * es); fmt.pitch_c = (uint32_t)(((semi ? W : W / 2) + 3) * es);
                        fmt.offset_c[0] = (uint64_t)fmt.pitch_y * H + 64;
                        if (!semi) fmt.offset_c[1] = fmt.offset_c[0] + (uint64_t)fmt.pitch_c * (H / 2) + 32;
                    }
                    const size_t n = ovhip_surface_bytes(w, h, &wins[k], &fmt);
                    if (!n) { fprintf(stderr, "no size for %dx%d window %u\n", w, h, k); return 1; }
                    uint8_t *dst = (uint8_t *)malloc(n);
                    if (!dst) return 2;
                    memset(dst, 0xA5, n);
                    const int r = ovhip_surface_lut_host(y, cb, cr, w, h, w, w / 2, &wins[k], &cv, &fmt, sz, peak, table, dst, n);
                    if (r != OVHIP_OK) { fprintf(stderr, "ovhip_surface_lut_host: %d\n", r); return 1; }
                    if (pass && f == OVHIP_SURF_I010 && !gaps) {
                        /* a flat picture through one table entry: the surface is flat per plane, and what it holds is the forward matrix of that entry */
                        const uint16_t *e = table + (pass == 1 ? 3 * (cells - 1) : 0);
                        int32_t c[9], yoff, q[3];
                        (void)ovhip_surface_lut_coefs(&cv, c, &yoff);
                        for (int ch = 0; ch < 3; ++ch) q[ch] = (int32_t)((16368u * e[ch] + (uint32_t)peak / 2) / (uint32_t)peak);
                        int32_t want[3];
                        want[0] = (16 * yoff + ((c[0] * q[0] + c[1] * q[1] + c[2] * q[2] + 8192) >> 14) + 8) >> 4;
                        for (int p = 1; p < 3; ++p) {
                            const int32_t c14 = 8192 + ((c[3 * p] * q[0] + c[3 * p + 1] * q[1] + c[3 * p + 2] * q[2] + 8192) >> 14);
                            want[p] = (16 * c14 + 128) >> 8;
                            if (want[p] > 1023) want[p] = 1023;
                        }
                        const uint16_t *d16 = (const uint16_t *)dst;
                        const size_t ny = (size_t)W * H, nc = ny / 4;
                        for (size_t i = 0; i < ny + 2 * nc; ++i)
                            if (d16[i] != want[i < ny ? 0 : (i < ny + nc ? 1 : 2)]) { fprintf(stderr, "the %s corner: S %d, %dx%d, element %zu\n", pass == 1 ? "far" : "near", sz, w, h, i); return 1; }
                    }
                    for (size_t i = 0; i < n; ++i) sum = sum * 31 + dst[i];
                    free(dst);
                    ++n_ok;
                }
                free(y); free(cb); free(cr);
            }
        }
        free(table);
    }
    printf("%ld conversions, checksum %016llx\n", n_ok, (unsigned long long)sum);
    return 0;
}
