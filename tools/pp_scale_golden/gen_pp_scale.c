/* gen_pp_scale.c -- TEST INFRASTRUCTURE (run where the reference sources are present; not part of build()).
 *
 * Writes tests/golden/pp_scale/pp_scale.ovg and pp_scale_large.ovg: what the reference's output resampler pp_sample_rate_conv
 * (pp_pic_scale.c:250-377, called once per plane by pp_process_frame, post_proc.c:116-126) produces for a set of up-sampling and
 * equal-size cases.  The reference's pp_pic_scale.c is a compiler input of this program (see the Makefile), nothing of it is
 * copied; the two allocator entry points it calls are supplied here because the reference's ovmem.c needs its build system.
 *
 * Every case runs twice over destinations poisoned with two different patterns (both above the 10-bit range); the results have
 * to be equal and every sample written.  Every case has to be up-sampling in the reference's own sense (neither factor above
 * 1 << scale_bits) for luma AND chroma: down-sampling switches to 12-tap filters and, for chroma phases >= 16, indexes past them.
 *
 * Per case k the files hold c<k>_geom (u32[10]: src_w, src_h, dst_w, dst_h, window left / right / top / bottom, chroma_hor_col,
 * chroma_ver_col), the source planes c<k>_sy / _scb / _scr and the results c<k>_dy / _dcb / _dcr (u16, [h][w]).  The two largest
 * cases go to the second file so that each file stays below 1 MiB.
 *
 *     gen_pp_scale <dir>        the fixture
 *     gen_pp_scale --time       host time of the function at 1920x1080 -> 3840x2160, per plane
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <time.h>
#include "ovdpb.h"
#include "dec_structures.h"

void pp_sample_rate_conv(uint16_t *scaled_dst, uint16_t scaled_stride, int scaledWidth, int scaledHeight, uint16_t *orgSrc, uint16_t org_stride,
                         int orgWidth, int orgHeight, const struct ScalingInfo *const scale_info, uint8_t luma_flag);

/* ovmem.h */
void *ov_mallocz(size_t n) { return calloc(1, n ? n : 1); }
void ov_freep(void *ref) { void **p = (void **)ref; free(*p); *p = NULL; }

static uint32_t g_seed = 0x5053;
static uint32_t rnd32(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

/* ---- "OVG1" container (tests/golden_io.py) ---- */
typedef struct { FILE *f; uint32_t n; } gfile;
static gfile
gfile_open(const char *dir, const char *name)
{
    char path[1024];
    gfile g;
    snprintf(path, sizeof(path), "%s/%s", dir, name);
    g.f = fopen(path, "wb");
    if (!g.f) { perror(path); exit(1); }
    g.n = 0;
    uint32_t hdr[2] = { 0x3147564f, 0 };
    fwrite(hdr, 4, 2, g.f);
    return g;
}
static void
gfile_array(gfile *g, const char *name, int type, int esize, const void *data, int ndim, const uint32_t *dims)
{
    char nm[32] = { 0 };
    uint32_t hdr[6] = { (uint32_t)type, (uint32_t)ndim, 1, 1, 1, 1 };
    size_t total = 1;
    strncpy(nm, name, 31);
    for (int i = 0; i < ndim; ++i) { hdr[2 + i] = dims[i]; total *= dims[i]; }
    fwrite(nm, 1, 32, g->f);
    fwrite(hdr, 4, 6, g->f);
    fwrite(data, (size_t)esize, total, g->f);
    g->n++;
}
static void gfile_close(gfile *g) { fseek(g->f, 4, SEEK_SET); fwrite(&g->n, 4, 1, g->f); fclose(g->f); }
enum { T_U16 = 2, T_U32 = 4 };

enum { RANDOM = 0, ALL_MAX = 1, CHECKER = 2 };
struct scase { int sw, sh, dw, dh, win[4], col[2], content, large; };
static const struct scase cases[] = {
    {  64,  48, 128,  96, { 0, 0, 0, 0 }, { 0, 0 }, RANDOM,  0 },
    {  96,  64, 144,  96, { 0, 0, 0, 0 }, { 1, 0 }, RANDOM,  0 },
    {  80,  48, 104,  72, { 0, 0, 0, 0 }, { 0, 1 }, RANDOM,  0 },
    { 176, 144, 352, 288, { 0, 0, 0, 0 }, { 1, 1 }, RANDOM,  1 },
    {  72,  40,  72,  40, { 0, 0, 0, 0 }, { 0, 0 }, RANDOM,  0 },
    {  64,  64, 128,  64, { 0, 0, 0, 0 }, { 1, 0 }, ALL_MAX, 0 },
    {  64,  64,  64,  96, { 0, 0, 0, 0 }, { 0, 1 }, CHECKER, 0 },
    {  96,  80, 160, 136, { 1, 2, 1, 0 }, { 1, 1 }, RANDOM,  0 },
    { 120,  72, 128,  80, { 2, 0, 0, 1 }, { 0, 0 }, RANDOM,  0 },
    {   8,   8,  16,  16, { 0, 0, 0, 0 }, { 0, 1 }, RANDOM,  0 },
    { 208, 120, 416, 240, { 0, 0, 0, 0 }, { 1, 0 }, RANDOM,  1 },
};
#define N_CASES ((int)(sizeof(cases) / sizeof(cases[0])))

static void
fill(uint16_t *p, int w, int h, int content)
{
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            p[y * w + x] = (uint16_t)(content == ALL_MAX ? 1023 : content == CHECKER ? (((x ^ y) & 1) ? 1023 : 0) : rnd32() & 1023);
}

/* up-sampling (or equal size) in the reference's own sense, pp_pic_scale.c:254-264 */
static int
is_upsampling(int ow, int oh, int sw, int sh, const struct ScalingInfo *si, int luma)
{
    uint16_t extra_w = (uint16_t)((si->scaling_win_left + si->scaling_win_right) << 1);
    uint16_t extra_h = (uint16_t)((si->scaling_win_top + si->scaling_win_bottom) << 1);
    if (luma) { extra_w = (uint16_t)(extra_w << 1); extra_h = (uint16_t)(extra_h << 1); }
    const int bits = luma ? RPR_SCALE_BITS - 1 : RPR_SCALE_BITS;
    const int scale_hor = ((ow - extra_w) << bits) / sw, scale_ver = ((oh - extra_h) << bits) / sh;
    return ow - extra_w > 0 && oh - extra_h > 0 && scale_hor <= (1 << bits) && scale_ver <= (1 << bits);
}

static uint16_t *
run_plane(uint16_t *src, int ow, int oh, int sw, int sh, const struct ScalingInfo *si, int luma)
{
    static const uint16_t poison[2] = { 0xABAB, 0x5C5C };
    uint16_t *out[2];
    if (!is_upsampling(ow, oh, sw, sh, si, luma)) { fprintf(stderr, "%dx%d -> %dx%d (%s) is not up-sampling\n", ow, oh, sw, sh, luma ? "luma" : "chroma"); exit(1); }
    for (int k = 0; k < 2; ++k) {
        out[k] = (uint16_t *)malloc((size_t)sw * sh * 2);
        for (int i = 0; i < sw * sh; ++i) out[k][i] = poison[k];
        pp_sample_rate_conv(out[k], (uint16_t)sw, sw, sh, src, (uint16_t)ow, ow, oh, si, (uint8_t)luma);
    }
    for (int i = 0; i < sw * sh; ++i)
        if (out[0][i] != out[1][i] || out[0][i] > 1023) { fprintf(stderr, "%dx%d -> %dx%d: sample %d unstable or not written\n", ow, oh, sw, sh, i); exit(1); }
    free(out[1]);
    return out[0];
}

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

static int
time_it(void)
{
    const int ow = 1920, oh = 1080, sw = 3840, sh = 2160;
    struct ScalingInfo si;
    memset(&si, 0, sizeof(si));
    double total = 0;
    for (int p = 0; p < 3; ++p) {
        const int d = p ? 2 : 1;
        uint16_t *src = (uint16_t *)malloc((size_t)(ow / d) * (oh / d) * 2), *dst = (uint16_t *)malloc((size_t)(sw / d) * (sh / d) * 2);
        fill(src, ow / d, oh / d, RANDOM);
        double best = 1e30;
        for (int rep = 0; rep < 3; ++rep) {
            const double t0 = now_s();
            pp_sample_rate_conv(dst, (uint16_t)(sw / d), sw / d, sh / d, src, (uint16_t)(ow / d), ow / d, oh / d, &si, p == 0);
            const double dt = now_s() - t0;
            if (dt < best) best = dt;
        }
        printf("%s %dx%d -> %dx%d: %.1f ms (best of 3, one core)\n", p == 0 ? "Y " : p == 1 ? "Cb" : "Cr", ow / d, oh / d, sw / d, sh / d, 1e3 * best);
        total += best;
        free(src); free(dst);
    }
    printf("picture: %.1f ms\n", 1e3 * total);
    return 0;
}

int
main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--time")) return time_it();
    const char *dir = argc > 1 ? argv[1] : "tests/golden/pp_scale";
    gfile g[2] = { gfile_open(dir, "pp_scale.ovg"), gfile_open(dir, "pp_scale_large.ovg") };
    size_t samples = 0;
    for (int k = 0; k < N_CASES; ++k) {
        const struct scase *c = &cases[k];
        struct ScalingInfo si;
        memset(&si, 0, sizeof(si));
        si.scaling_win_left = (uint16_t)c->win[0]; si.scaling_win_right = (uint16_t)c->win[1];
        si.scaling_win_top = (uint16_t)c->win[2]; si.scaling_win_bottom = (uint16_t)c->win[3];
        si.chroma_hor_col_flag = (uint8_t)c->col[0]; si.chroma_ver_col_flag = (uint8_t)c->col[1];
        gfile *f = &g[c->large];
        char name[32];
        const uint32_t geom[10] = { (uint32_t)c->sw, (uint32_t)c->sh, (uint32_t)c->dw, (uint32_t)c->dh, (uint32_t)c->win[0], (uint32_t)c->win[1],
                                    (uint32_t)c->win[2], (uint32_t)c->win[3], (uint32_t)c->col[0], (uint32_t)c->col[1] };
        const uint32_t d1 = 10;
        snprintf(name, sizeof(name), "c%d_geom", k); gfile_array(f, name, T_U32, 4, geom, 1, &d1);
        static const char *pn[3] = { "y", "cb", "cr" };
        for (int p = 0; p < 3; ++p) {
            const int d = p ? 2 : 1, ow = c->sw / d, oh = c->sh / d, sw = c->dw / d, sh = c->dh / d;
            uint16_t *src = (uint16_t *)malloc((size_t)ow * oh * 2);
            fill(src, ow, oh, c->content);
            uint16_t *dst = run_plane(src, ow, oh, sw, sh, &si, p == 0);
            const uint32_t ds[2] = { (uint32_t)oh, (uint32_t)ow }, dd[2] = { (uint32_t)sh, (uint32_t)sw };
            snprintf(name, sizeof(name), "c%d_s%s", k, pn[p]); gfile_array(f, name, T_U16, 2, src, 2, ds);
            snprintf(name, sizeof(name), "c%d_d%s", k, pn[p]); gfile_array(f, name, T_U16, 2, dst, 2, dd);
            samples += (size_t)ow * oh + (size_t)sw * sh;
            free(src); free(dst);
        }
    }
    gfile_close(&g[0]); gfile_close(&g[1]);
    fprintf(stderr, "pp_scale: %d cases, %zu samples\n", N_CASES, samples);
    return 0;
}
