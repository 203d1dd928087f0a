/* tools/host_check -- the host half of the RGB output through a colour table (openvvc_amd/csrc/ovvc_rgb_lut.c, on top of ovvc_rgb.c's
 * plan) as a stand-alone program: ovhip_rgb_lut_host over a few small pictures, the three table sizes, dtypes and layouts, every plane,
 * every table and every destination in a heap block of exactly its size, so that a read or a write one element outside is the
 * sanitizer's to see; the v = 1023 edge at every size (a picture that clips to 1023 in every channel reads the table's last entry and
 * nothing behind it); the texel repack and the entry check; and every refusal, which must write nothing.  `make asan`.  Host code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_rgb_lut_priv.h"

static uint32_t rng = 2468;
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
    const ovhip_rgb_format ok = { 1, 0, 0, OVHIP_RGB_U16, OVHIP_RGB_PLANAR, { 0, 0, 0 } }, u8 = { 1, 0, 0, OVHIP_RGB_U8, OVHIP_RGB_PLANAR, { 0, 0, 0 } };
    const ovhip_rgb_format bad_dt = { 1, 0, 0, 4, 0, { 0, 0, 0 } }, unspec = { 2, 0, 0, 1, 0, { 0, 0, 0 } }, unbuilt = { 0, 0, 0, 1, 0, { 0, 0, 0 } };
    const ovhip_window none = { 6, 6, 0, 0 };
    const size_t n = ovhip_rgb_bytes(W, H, NULL, &ok);
    uint8_t *dst = (uint8_t *)malloc(n);
    if (!dst) return 2;
    memset(dst, 0xA5, n);
    struct { const char *what; int got, want; } c[] = {
        { "null table", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &ok, 17, 1023, NULL, dst, n), OVHIP_EINVAL },
        { "size 16", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &ok, 16, 1023, table, dst, n), OVHIP_EINVAL },
        { "size 129", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &ok, 129, 1023, table, dst, n), OVHIP_EINVAL },
        { "peak 0", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &ok, 17, 0, table, dst, n), OVHIP_EINVAL },
        { "peak 65536", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &ok, 17, 65536, table, dst, n), OVHIP_EINVAL },
        { "U8 with peak 1023", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &u8, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "entry above the peak", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &ok, 17, 1023, above, dst, n), OVHIP_EINVAL },
        { "null destination", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &ok, 17, 1023, table, NULL, n), OVHIP_EINVAL },
        { "destination too small", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &ok, 17, 1023, table, dst, n - 1), OVHIP_EINVAL },
        { "misaligned destination", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &ok, 17, 1023, table, dst + 1, n - 1), OVHIP_EINVAL },
        { "overlapping destination", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &ok, 17, 1023, table, y, 1 << 20), OVHIP_EINVAL },
        { "window leaves nothing", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, &none, &ok, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "missing plane", ovhip_rgb_lut_host(y, NULL, cr, W, H, W, W / 2, NULL, &ok, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "stride below the width", ovhip_rgb_lut_host(y, cb, cr, W, H, W - 1, W / 2, NULL, &ok, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "width no multiple of 4", ovhip_rgb_lut_host(y, cb, cr, W - 2, H, W, W / 2, NULL, &ok, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "bad dtype", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &bad_dt, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "matrix unspecified", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &unspec, 17, 1023, table, dst, n), OVHIP_EINVAL },
        { "matrix not built", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, &unbuilt, 17, 1023, table, dst, n), OVHIP_EUNSUP },
        { "null format", ovhip_rgb_lut_host(y, cb, cr, W, H, W, W / 2, NULL, NULL, 17, 1023, table, dst, n), OVHIP_EINVAL },
    };
    for (unsigned i = 0; i < sizeof(c) / sizeof(c[0]); ++i) if (c[i].got != c[i].want) FAIL("refusal \"%s\": %d, not %d", c[i].what, c[i].got, c[i].want);
    for (size_t i = 0; i < n; ++i) if (dst[i] != 0xA5) FAIL("a refusal wrote");
    if (ovhip_rgb_lut_first_above_(17, 1023, above) != (int64_t)3 * 17 * 17 * 17 - 1 || ovhip_rgb_lut_first_above_(17, 1023, table) != -1) FAIL("first_above");
    if (ovhip_rgb_lut_check(17, 255, &u8) != OVHIP_OK || ovhip_rgb_lut_check(17, 256, &u8) != OVHIP_EINVAL || ovhip_rgb_lut_check(34, 255, NULL) != OVHIP_EINVAL) FAIL("check");
    free(dst); free(above); free(table); free(y); free(cb); free(cr);
    printf("%u refusals\n", (unsigned)(sizeof(c) / sizeof(c[0])));
    return 0;
}

int
main(void)
{
    if (refusals()) return 1;
    static const int sizes[][2] = { { 8, 8 }, { 20, 12 }, { 72, 40 } };
    static const ovhip_window wins[] = { { 0, 0, 0, 0 }, { 1, 0, 0, 1 } };
    static const int S[] = { 17, 33, 65 };
    long n_ok = 0;
    uint64_t sum = 0;
    for (unsigned si = 0; si < 3; ++si) {
        const int sz = S[si];
        const size_t cells = (size_t)sz * sz * sz;
        uint16_t *table = block(3 * cells, 256, -1);
        /* the repack, into a block of exactly 8 bytes per texel */
        uint16_t *texels = (uint16_t *)malloc(cells * 8);
        if (!texels) return 2;
        ovhip_rgb_lut_repack_(sz, table, texels);
        for (size_t i = 0; i < cells; ++i)
            if (texels[4 * i] != table[3 * i] || texels[4 * i + 1] != table[3 * i + 1] || texels[4 * i + 2] != table[3 * i + 2] || texels[4 * i + 3]) { fprintf(stderr, "repack at %zu\n", i); return 1; }
        free(texels);
        for (unsigned s = 0; s < 3; ++s) {
            const int w = sizes[s][0], h = sizes[s][1];
            /* pass 0: random planes; pass 1: every pixel clips to (1023, 1023, 1023): the v = 1023 edge in all three channels;
             * pass 2: to (0, 0, 0) */
            for (int pass = 0; pass < 3; ++pass) {
                uint16_t *y = block((size_t)w * h, 1024, pass == 0 ? -1 : (pass == 1 ? 1023 : 0));
                uint16_t *cb = block((size_t)w * h / 4, 1024, pass == 0 ? -1 : 512), *cr = block((size_t)w * h / 4, 1024, pass == 0 ? -1 : 512);
                for (int dt = 0; dt < 4; ++dt) for (int lay = 0; lay < 2; ++lay) for (unsigned k = 0; k < 2; ++k) {
                    const ovhip_rgb_format fmt = { 9, 0, (uint8_t)(k ? 2 : 0), (uint8_t)dt, (uint8_t)lay, { 0, 0, 0 } };
                    const size_t n = ovhip_rgb_bytes(w, h, &wins[k], &fmt);
                    if (!n) { fprintf(stderr, "no size for %dx%d window %u\n", w, h, k); return 1; }
                    uint8_t *dst = (uint8_t *)malloc(n);
                    if (!dst) return 2;
                    const int r = ovhip_rgb_lut_host(y, cb, cr, w, h, w, w / 2, &wins[k], &fmt, sz, 255, table, dst, n);
                    if (r != OVHIP_OK) { fprintf(stderr, "ovhip_rgb_lut_host: %d\n", r); return 1; }
                    if (pass && dt == OVHIP_RGB_U8) {
                        const uint16_t *e = table + (pass == 1 ? 3 * (cells - 1) : 0);          /* the last entry / the first */
                        const size_t px = n / 3;
                        for (size_t i = 0; i < px; ++i) for (int c = 0; c < 3; ++c)
                            if (dst[lay ? 3 * i + c : c * px + i] != e[c]) { fprintf(stderr, "the %s corner: S %d, %dx%d\n", pass == 1 ? "far" : "near", sz, w, h); return 1; }
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
