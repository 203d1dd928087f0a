/* tools/host_check -- the host half of the surface output (openvvc_amd/csrc/ovvc_surface.c) as a stand-alone program:
 * ovhip_surface_host over the sizes, windows, formats, roundings and layouts (tight, and with gaps) of tests/test_surface_cpu.py,
 * every plane and every destination in a heap block of exactly its size (strides equal to the widths), so that a read or a write one
 * sample outside is the sanitizer's to see; the gaps of a layout must stay as they were; the refusals, which must write nothing; and of
 * a destination with two faults at once, which of them the plan names.  `make asan`.  Host code only. */
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
    static const uint16_t ends[8] = { 0, 1, 2, 3, 1020, 1021, 1022, 1023 };
    uint16_t *p = (uint16_t *)malloc((size_t)w * h * 2);
    if (!p) exit(2);
    for (int i = 0; i < w * h; ++i) p[i] = next10();
    for (int r = 0; r < h; ++r) { p[r * w] = ends[r % 8]; p[r * w + w - 1] = ends[(r + 4) % 8]; }
    return p;
}

static int is16(int f) { return f == OVHIP_SURF_P010 || f == OVHIP_SURF_I010; }
static int semi(int f) { return f == OVHIP_SURF_NV12 || f == OVHIP_SURF_P010; }

/* a destination both too small and not aligned to its element: the surface plan names the alignment (the RGB plan the size), and
 * quotes no size for it */
static int
two_faults(void)
{
    static uint16_t y[8 * 8], c[4 * 4], buf[8 * 8 + 8 * 4 + 1];
    const ovhip_pic pic = { y, c, c, 8, 8, 8, 4 };
    ovhip_surface_format fmt;
    memset(&fmt, 0, sizeof(fmt));
    fmt.format = OVHIP_SURF_P010;
    const size_t n = ovhip_surface_bytes(8, 8, NULL, &fmt);
    ovhip_surface_plan_ plan;
    const char *why = NULL;
    const int r = ovhip_surface_plan_make_(&pic, NULL, &fmt, (char *)buf + 1, n - 1, &plan, &why);
    if (r != OVHIP_EINVAL || !why || strcmp(why, "destination not aligned to its element") || plan.bytes) {
        fprintf(stderr, "two faults: %d, \"%s\", %zu bytes\n", r, why ? why : "(null)", plan.bytes); return 1;
    }
    return 0;
}

int
main(void)
{
    if (two_faults()) return 1;
    static const int sizes[][2] = { { 8, 8 }, { 16, 8 }, { 20, 12 }, { 34, 18 }, { 72, 40 }, { 136, 72 }, { 264, 136 } };
    static const ovhip_window wins[] = { { 0, 0, 0, 0 }, { 1, 0, 0, 1 }, { 0, 1, 1, 0 }, { 1, 1, 1, 1 } };
    static const int modes[][2] = { { OVHIP_SURF_NV12, 0 }, { OVHIP_SURF_NV12, 1 }, { OVHIP_SURF_P010, 0 }, { OVHIP_SURF_I420, 0 }, { OVHIP_SURF_I420, 1 }, { OVHIP_SURF_I010, 0 } };
    long n_ok = 0, n_refused = 0;
    uint64_t sum = 0;
    for (unsigned s = 0; s < sizeof(sizes) / sizeof(sizes[0]); ++s) {
        const int w = sizes[s][0], h = sizes[s][1];
        uint16_t *y = plane(w, h), *cb = plane(w / 2, h / 2), *cr = plane(w / 2, h / 2);
        for (unsigned m = 0; m < 6; ++m) for (unsigned k = 0; k < 4; ++k) for (int loose = 0; loose < 2; ++loose) {
            const int f = modes[m][0], es = is16(f) ? 2 : 1;
            const int W = w - 2 * (wins[k].offset_lft + wins[k].offset_rgt), H = h - 2 * (wins[k].offset_abv + wins[k].offset_blw);
            const int cw = semi(f) ? W : W / 2;
            ovhip_surface_format fmt;
            memset(&fmt, 0, sizeof(fmt));
            fmt.format = (uint8_t)f; fmt.rounding = (uint8_t)modes[m][1];
            if (loose) {
                fmt.pitch_y = (uint32_t)((W + 1) * es); fmt.pitch_c = (uint32_t)((cw + 3) * es);
                fmt.offset_c[0] = (uint64_t)fmt.pitch_y * H + 64;
                if (!semi(f)) fmt.offset_c[1] = fmt.offset_c[0] + (uint64_t)fmt.pitch_c * (H / 2) + 32;
            }
            const size_t n = ovhip_surface_bytes(w, h, &wins[k], &fmt);
            if (!n) { fprintf(stderr, "no size for %dx%d window %u format %d\n", w, h, k, f); return 1; }
            uint8_t *dst = (uint8_t *)malloc(n);
            if (!dst) return 2;
            memset(dst, 0xA5, n);
            const int r = ovhip_surface_host(y, cb, cr, w, h, w, w / 2, &wins[k], &fmt, dst, n);
            if (r != OVHIP_OK) { fprintf(stderr, "ovhip_surface_host: %d\n", r); return 1; }
            for (size_t i = 0; i < n; ++i) sum = sum * 31 + dst[i];
            if (loose) {
                /* the bytes between the luma rows and between the planes */
                for (int row = 0; row + 1 < H; ++row)
                    for (int b = W * es; b < (int)fmt.pitch_y; ++b)
                        if (dst[(size_t)row * fmt.pitch_y + b] != 0xA5) { fprintf(stderr, "a gap between rows was written\n"); return 1; }
                for (size_t i = (size_t)(H - 1) * fmt.pitch_y + (size_t)W * es; i < fmt.offset_c[0]; ++i)
                    if (dst[i] != 0xA5) { fprintf(stderr, "the gap between planes was written\n"); return 1; }
            }
            /* one byte short: refused, nothing written (the block is one byte short too) */
            uint8_t *small = (uint8_t *)malloc(n - 1);
            if (!small) return 2;
            memset(small, 0xA5, n - 1);
            if (ovhip_surface_host(y, cb, cr, w, h, w, w / 2, &wins[k], &fmt, small, n - 1) != OVHIP_EINVAL) { fprintf(stderr, "a short destination was taken\n"); return 1; }
            for (size_t i = 0; i + 1 < n; ++i) if (small[i] != 0xA5) { fprintf(stderr, "a refusal wrote\n"); return 1; }
            free(small); free(dst);
            ++n_ok; ++n_refused;
        }
        free(y); free(cb); free(cr);
    }
    printf("%ld surfaces, %ld refusals, checksum %016llx\n", n_ok, n_refused, (unsigned long long)sum);
    return 0;
}
