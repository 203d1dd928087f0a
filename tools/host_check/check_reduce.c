/* tools/host_check -- the host half of the reduced-size output (openvvc_amd/csrc/ovvc_reduce.c) as a stand-alone program:
 * ovhip_output_reduce_host over the census of tests/spec_reduce.py (every chroma location where the census runs them, a window, the
 * int32 ceiling filled with 1023 and random), every plane of the source and of the destination in a heap block of exactly its size
 * (strides equal to the widths), so that a read or a write one sample outside is the sanitizer's to see; against the definition
 * written out again here, interval by interval; the refusals, which must write nothing; and the kernel's division
 * (ovhip_reduce_div_, ovvc_reduce_priv.h) at every rounding boundary of every n of the census.  `make asan`.  Host code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_reduce_priv.h"

static uint32_t rng = 2463534242u;
static uint16_t next10(void) { rng = rng * 1664525u + 1013904223u; return (uint16_t)((rng >> 12) & 1023); }

static uint16_t *
plane(int w, int h, int fill)
{
    uint16_t *p = (uint16_t *)malloc((size_t)w * h * 2);
    if (!p) exit(2);
    for (int i = 0; i < w * h; ++i) p[i] = fill >= 0 ? (uint16_t)fill : next10();
    return p;
}

static long fdiv(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

/* the definition, sample by sample: output (kx, ky) of a plane of Sw x Sh samples */
static int
defined(const uint16_t *s, int Sw, int Sh, int kx, int ky, int px, int qx, int py, int qy, int sgx, int sgy)
{
    const long Ax = 4L * px * kx - sgx, Bx = Ax + 4L * px, Ay = 4L * py * ky - sgy, By = Ay + 4L * py;
    long long V = 0;
    for (long jy = fdiv(Ay, 4L * qy); jy <= fdiv(By - 1, 4L * qy); ++jy) {
        const long hi_y = By < 4L * qy * (jy + 1) ? By : 4L * qy * (jy + 1), lo_y = Ay > 4L * qy * jy ? Ay : 4L * qy * jy;
        const long cy = jy < 0 ? 0 : (jy > Sh - 1 ? Sh - 1 : jy);
        long long h = 0;
        for (long jx = fdiv(Ax, 4L * qx); jx <= fdiv(Bx - 1, 4L * qx); ++jx) {
            const long hi_x = Bx < 4L * qx * (jx + 1) ? Bx : 4L * qx * (jx + 1), lo_x = Ax > 4L * qx * jx ? Ax : 4L * qx * jx;
            const long cx = jx < 0 ? 0 : (jx > Sw - 1 ? Sw - 1 : jx);
            h += (hi_x - lo_x) * s[cy * Sw + cx];
        }
        V += (hi_y - lo_y) * h;
    }
    const long long n = 16LL * px * py;
    return (int)((V + n / 2) / n);
}

static long n_pictures, n_samples, n_refused, n_div;

/* one picture of the census: w x h (filled with `fill`, or random for -1) under win -> Wd x Hd at chroma location loc */
static int
one(int w, int h, ovhip_window win, int Wd, int Hd, int loc, int fill)
{
    uint16_t *sp[3] = { plane(w, h, fill), plane(w / 2, h / 2, fill), plane(w / 2, h / 2, fill) };
    uint16_t *dp[3] = { plane(Wd, Hd, 0xA5A5), plane(Wd / 2, Hd / 2, 0xA5A5), plane(Wd / 2, Hd / 2, 0xA5A5) };
    const ovhip_pic src = { sp[0], sp[1], sp[2], w, h, w, w / 2 }, dst = { dp[0], dp[1], dp[2], Wd, Hd, Wd, Wd / 2 };
    ovhip_reduce_info info;
    memset(&info, 0, sizeof(info));
    info.win = win; info.chroma_loc = (uint8_t)loc;
    int32_t ratio[4];
    int r = ovhip_output_reduce_check(w, h, &info, Wd, Hd, ratio);
    if (r == OVHIP_OK) r = ovhip_output_reduce_host(&src, &info, &dst);
    if (r != OVHIP_OK) { fprintf(stderr, "%dx%d -> %dx%d: %d\n", w, h, Wd, Hd, r); return 1; }
    const int Ws = w - 2 * (win.offset_lft + win.offset_rgt), Hs = h - 2 * (win.offset_abv + win.offset_blw);
    const int a = loc & 1, b = loc < 2 ? 1 : (loc < 4 ? 0 : 2);
    int bad = 0;
    for (int c = 0; c < 3 && !bad; ++c) {
        const int sh = c != 0, Sw = Ws >> sh, Sh = Hs >> sh, Dw = Wd >> sh, Dh = Hd >> sh, pw = w >> sh;
        /* the region as a tight block of its own: the definition above never sees the picture around it */
        uint16_t *reg = plane(Sw, Sh, 0);
        for (int y = 0; y < Sh; ++y)
            memcpy(reg + (size_t)y * Sw, sp[c] + (size_t)(y + ((2 * win.offset_abv) >> sh)) * pw + ((2 * win.offset_lft) >> sh), (size_t)Sw * 2);
        const int sgx = c ? (ratio[0] - ratio[1]) * (1 - a) : 0, sgy = c ? (ratio[2] - ratio[3]) * (1 - b) : 0;
        for (int ky = 0; ky < Dh && !bad; ++ky)
            for (int kx = 0; kx < Dw; ++kx) {
                const int want = defined(reg, Sw, Sh, kx, ky, ratio[0], ratio[1], ratio[2], ratio[3], sgx, sgy);
                if (dp[c][(size_t)ky * Dw + kx] != want || (fill >= 0 && want != fill)) {
                    fprintf(stderr, "%dx%d -> %dx%d loc %d plane %d (%d, %d): %d, defined %d\n", w, h, Wd, Hd, loc, c, kx, ky, dp[c][(size_t)ky * Dw + kx], want);
                    bad = 1; break;
                }
                ++n_samples;
            }
        free(reg);
    }
    for (int c = 0; c < 3; ++c) { free(sp[c]); free(dp[c]); }
    ++n_pictures;
    return bad;
}

static int
refused(int w, int h, ovhip_window win, int Wd, int Hd, int loc, int rsv, int want, int want_px)
{
    /* the destination is allocated at the size asked for where that is a size at all */
    const int dw = Wd > 0 ? Wd : 4, dh = Hd > 0 ? Hd : 4, sw = w > 0 ? w : 4, sh = h > 0 ? h : 4;
    uint16_t *sp[3] = { plane(sw, sh, -1), plane(sw / 2 + 1, sh / 2 + 1, -1), plane(sw / 2 + 1, sh / 2 + 1, -1) };
    uint16_t *dp[3] = { plane(dw, dh, 0xA5A5), plane(dw / 2 + 1, dh / 2 + 1, 0xA5A5), plane(dw / 2 + 1, dh / 2 + 1, 0xA5A5) };
    const ovhip_pic src = { sp[0], sp[1], sp[2], w, h, sw, sw / 2 + 1 }, dst = { dp[0], dp[1], dp[2], Wd, Hd, dw, dw / 2 + 1 };
    ovhip_reduce_info info;
    memset(&info, 0, sizeof(info));
    info.win = win; info.chroma_loc = (uint8_t)loc; info.rsv[1] = (uint8_t)rsv;
    int32_t ratio[4] = { -1, -1, -1, -1 };
    const int r0 = ovhip_output_reduce_check(w, h, &info, Wd, Hd, ratio), r1 = ovhip_output_reduce_host(&src, &info, &dst);
    int bad = r0 != want || r1 != want || ratio[0] != want_px;
    for (int i = 0; i < dw * dh && !bad; ++i) bad = dp[0][i] != 0xA5A5;
    for (int i = 0; i < (dw / 2 + 1) * (dh / 2 + 1) && !bad; ++i) bad = dp[1][i] != 0xA5A5 || dp[2][i] != 0xA5A5;
    if (bad) fprintf(stderr, "refusal %dx%d -> %dx%d: %d, %d (wanted %d), p_x %d (wanted %d), or something was written\n", w, h, Wd, Hd, r0, r1, want, ratio[0], want_px);
    for (int c = 0; c < 3; ++c) { free(sp[c]); free(dp[c]); }
    ++n_refused;
    return bad;
}

/* (V + n/2) div n either side of every step, for V = m n - n/2 - 1, m n - n/2, m n - n/2 + 1 up to the numerator's maximum */
static int
division(uint32_t n)
{
    const float rcp = 1.0f / (float)n;
    for (uint32_t m = 1; m <= 1023; ++m)
        for (int d = -1; d <= 1; ++d) {
            const int64_t V = (int64_t)m * n - n / 2 + d;
            if (V < 0 || V > 1023LL * n) continue;
            const uint32_t num = (uint32_t)(V + n / 2);
            if (ovhip_reduce_div_(num, n, rcp) != num / n || ovhip_output_reduce_divide(num, n) != num / n) {
                fprintf(stderr, "division: %u / %u: %u\n", num, n, ovhip_reduce_div_(num, n, rcp)); return 1;
            }
            ++n_div;
        }
    return 0;
}

int
main(void)
{
    static const ovhip_window none = { 0, 0, 0, 0 };
    static const struct { int w, h, Wd, Hd, all_locs; } census[] = {
        { 104, 56, 52, 28, 1 }, { 72, 40, 48, 24, 1 }, { 96, 48, 32, 16, 0 }, { 64, 64, 8, 8, 1 }, { 72, 40, 72, 20, 0 }, { 72, 40, 36, 40, 0 },
        { 72, 40, 72, 40, 0 }, { 100, 52, 52, 28, 0 }, { 200, 20, 136, 12, 0 }, { 1024, 1024, 132, 132, 0 } };
    for (unsigned k = 0; k < sizeof(census) / sizeof(census[0]); ++k) {
        for (int loc = 0; loc < (census[k].all_locs ? 6 : 1); ++loc)
            if (one(census[k].w, census[k].h, none, census[k].Wd, census[k].Hd, loc, -1)) return 1;
        int32_t ratio[4];
        ovhip_reduce_info info;
        memset(&info, 0, sizeof(info));
        if (ovhip_output_reduce_check(census[k].w, census[k].h, &info, census[k].Wd, census[k].Hd, ratio) != OVHIP_OK) return 1;
        if (division(16u * (uint32_t)ratio[0] * (uint32_t)ratio[2])) return 1;
    }
    if (one(1024, 1024, none, 132, 132, 0, 1023) || one(64, 64, none, 8, 8, 4, 1023) || one(72, 40, none, 72, 40, 3, 0)) return 1;
    static const ovhip_window win = { 1, 3, 2, 2 };
    for (int loc = 0; loc < 6; ++loc) if (one(80, 48, win, 48, 24, loc, -1)) return 1;
    static const ovhip_window nothing = { 18, 18, 0, 0 }, odd = { 1, 0, 0, 0 };
    if (refused(1028, 64, none, 132, 64, 0, 0, OVHIP_EUNSUP, 257) || refused(72, 40, none, 8, 40, 0, 0, OVHIP_EUNSUP, 9)
        || refused(72, 40, none, 144, 40, 0, 0, OVHIP_EUNSUP, 1) || refused(70, 40, none, 36, 20, 0, 0, OVHIP_EINVAL, 0)
        || refused(72, 40, none, 34, 20, 0, 0, OVHIP_EINVAL, 0) || refused(72, 40, nothing, 36, 20, 0, 0, OVHIP_EINVAL, 0)
        || refused(72, 40, odd, 36, 20, 0, 0, OVHIP_EINVAL, 0) || refused(72, 40, none, 36, 20, 6, 0, OVHIP_EINVAL, 0)
        || refused(72, 40, none, 36, 20, 0, 1, OVHIP_EINVAL, 0) || refused(16388, 4, none, 8192, 4, 0, 0, OVHIP_EINVAL, 0))
        return 1;
    printf("check_reduce: %ld pictures (%ld samples) equal the definition, %ld refusals wrote nothing, %ld divisions exact\n",
           n_pictures, n_samples, n_refused, n_div);
    return 0;
}
