/* tools/host_check -- the host half of the RGB output (openvvc_amd/csrc/ovvc_rgb.c) as a stand-alone program: ovhip_rgb_host over the
 * sizes, windows, chroma locations, dtypes and layouts of tests/test_rgb_cpu.py, every plane and every destination in a heap block of
 * exactly its size (strides equal to the widths), so that a read or a write one sample outside is the sanitizer's to see; and the
 * refusals, which must write nothing; and of a destination with two faults at once, which of them the plan names.  `make asan`.  Host
 * code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_dpb_priv.h"

static uint32_t rng = 12345;
static uint16_t next10(void) { rng = rng * 1664525u + 1013904223u; return (uint16_t)((rng >> 12) & 1023); }

static uint16_t *
plane(int w, int h)
{
    uint16_t *p = (uint16_t *)malloc((size_t)w * h * 2);
    if (!p) exit(2);
    for (int i = 0; i < w * h; ++i) p[i] = next10();
    return p;
}

/* a destination both too small and not aligned to its element: the RGB plan names the size (the surface plan the alignment) */
static int
two_faults(void)
{
    static uint16_t y[8 * 8], c[4 * 4], buf[3 * 8 * 8 + 1];
    const ovhip_pic pic = { y, c, c, 8, 8, 8, 4 };
    const ovhip_rgb_format fmt = { 1, 0, 0, OVHIP_RGB_U16, OVHIP_RGB_PLANAR, { 0, 0, 0 } };
    const size_t n = ovhip_rgb_bytes(8, 8, NULL, &fmt);
    ovhip_rgb_plan_ plan;
    const char *why = NULL;
    const int r = ovhip_rgb_plan_make_(&pic, NULL, &fmt, (char *)buf + 1, n - 1, &plan, &why);
    if (r != OVHIP_EINVAL || !why || strcmp(why, "destination too small")) { fprintf(stderr, "two faults: %d, \"%s\"\n", r, why ? why : "(null)"); return 1; }
    return 0;
}

int
main(void)
{
    if (two_faults()) return 1;
    static const int sizes[][2] = { { 8, 8 }, { 20, 12 }, { 24, 8 }, { 72, 40 } };
    static const ovhip_window wins[] = { { 0, 0, 0, 0 }, { 1, 0, 0, 1 }, { 0, 3, 2, 0 } };
    static const int matrices[] = { 1, 5, 6, 9 };
    long n_ok = 0, n_refused = 0;
    uint64_t sum = 0;
    for (unsigned s = 0; s < sizeof(sizes) / sizeof(sizes[0]); ++s) {
        const int w = sizes[s][0], h = sizes[s][1];
        uint16_t *y = plane(w, h), *cb = plane(w / 2, h / 2), *cr = plane(w / 2, h / 2);
        for (unsigned m = 0; m < 4; ++m) for (int full = 0; full < 2; ++full) for (int loc = 0; loc < 6; ++loc)
        for (int dt = 0; dt < 4; ++dt) for (int lay = 0; lay < 2; ++lay) for (unsigned k = 0; k < 3; ++k) {
            const ovhip_rgb_format fmt = { (uint8_t)matrices[m], (uint8_t)full, (uint8_t)loc, (uint8_t)dt, (uint8_t)lay, { 0, 0, 0 } };
            const size_t n = ovhip_rgb_bytes(w, h, &wins[k], &fmt);
            if (!n) { fprintf(stderr, "no size for %dx%d window %u\n", w, h, k); return 1; }
            uint8_t *dst = (uint8_t *)malloc(n);
            if (!dst) return 2;
            const int r = ovhip_rgb_host(y, cb, cr, w, h, w, w / 2, &wins[k], &fmt, dst, n);
            if (r != OVHIP_OK) { fprintf(stderr, "ovhip_rgb_host: %d\n", r); return 1; }
            for (size_t i = 0; i < n; ++i) sum = sum * 31 + dst[i];
            /* one byte short: refused, nothing written (the block is one byte short too) */
            uint8_t *small = (uint8_t *)malloc(n - 1);
            if (!small) return 2;
            memset(small, 0xA5, n - 1);
            if (ovhip_rgb_host(y, cb, cr, w, h, w, w / 2, &wins[k], &fmt, small, n - 1) != OVHIP_EINVAL) { fprintf(stderr, "a short destination was taken\n"); return 1; }
            for (size_t i = 0; i + 1 < n; ++i) if (small[i] != 0xA5) { fprintf(stderr, "a refusal wrote\n"); return 1; }
            free(small); free(dst);
            ++n_ok; ++n_refused;
        }
        free(y); free(cb); free(cr);
    }
    printf("%ld conversions, %ld refusals, checksum %016llx\n", n_ok, n_refused, (unsigned long long)sum);
    return 0;
}
