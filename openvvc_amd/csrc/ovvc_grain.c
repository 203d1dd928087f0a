/* ovvc_grain.c -- film grain synthesis, host side (no device needed): the model derivation of one call of the reference's
 * fg_grain_apply_pic (pp_film_grain.c:768-807, :863-865), the grain database (:666-765) and the per-picture seed (:883-885, :635-641).
 * include/ovvc_hip.h ("Film grain synthesis") has the semantics and the places where the reference is undefined. */
#include <pthread.h>
#include <string.h>
#include "ovvc_hip.h"
#include "vvc_fg_tables.h"

#define FG_CELLS 13
#define FG_N     64

uint32_t
ovhip_fg_prng(uint32_t x)
{
    return (x << 1) + (1u ^ ((x >> 2) & 1u) ^ ((x >> 30) & 1u));
}

uint32_t
ovhip_fg_seed(int32_t poc, int32_t idr_offset, int c)
{
    static const uint32_t colour_offset[3] = { 0, 85, 170 };
    return ovt_fg_seed[((uint32_t)poc + ((uint32_t)idr_offset << 5) + colour_offset[c]) & 255u];
}

/* The register's start value for every stripe of a plane: it is stepped once per 16x16 block in raster order and never reset, so stripe
 * k starts n * k steps after the picture's seed (n blocks per stripe: 32 400 steps for the luma of a 4K picture).  One step is affine
 * over GF(2) -- a shift, and a feedback bit that is an xor of two state bits and 1 -- so n steps are too: F^n(x) = c ^ xor of col[i]
 * over the set bits i of x, with c = F^n(0) and col[i] = F^n(1 << i) ^ c.  The 33 images cost 33 n steps once per thread and n (the
 * two most recent n are kept: a picture's luma and chroma widths); after that a stripe costs one xor per set bit. */
typedef struct fg_jump { int n; uint32_t c, col[32]; } fg_jump;

static const fg_jump *
fg_jump_for(int n)
{
    static __thread fg_jump cache[2];
    static __thread int victim;
    for (int k = 0; k < 2; ++k) if (cache[k].n == n) return &cache[k];
    fg_jump *j = &cache[victim];
    victim ^= 1;
    uint32_t z = 0;
    for (int s = 0; s < n; ++s) z = ovhip_fg_prng(z);
    for (int i = 0; i < 32; ++i) {
        uint32_t x = 1u << i;
        for (int s = 0; s < n; ++s) x = ovhip_fg_prng(x);
        j->col[i] = x ^ z;
    }
    j->c = z; j->n = n;
    return j;
}

void
ovhip_fg_stripe_seeds(uint32_t start, int32_t blocks_per_stripe, int32_t n_stripes, uint32_t *out)
{
    if (!out || n_stripes <= 0 || blocks_per_stripe <= 0) return;
    out[0] = start;
    if (n_stripes < 4) {                   /* (not worth a table) */
        for (int k = 1; k < n_stripes; ++k) {
            uint32_t x = out[k - 1];
            for (int s = 0; s < blocks_per_stripe; ++s) x = ovhip_fg_prng(x);
            out[k] = x;
        }
        return;
    }
    const fg_jump *j = fg_jump_for(blocks_per_stripe);
    for (int k = 1; k < n_stripes; ++k) {
        uint32_t x = out[k - 1], y = j->c;
        while (x) { y ^= j->col[__builtin_ctz(x)]; x &= x - 1; }
        out[k] = y;
    }
}

int
ovhip_fg_derive(const ovhip_fg_params *in, ovhip_fg_model *model, ovhip_fg_params *after)
{
    if (!in || !model) return OVHIP_EINVAL;
    if (in->model_id != 0 || in->blending_mode != 0) return OVHIP_EUNSUP;
    ovhip_fg_params p = *in;
    ovhip_fg_model m;
    memset(&m, 0, sizeof(m));
    m.log2_scale = p.log2_scale;
    for (int c = 0; c < 3; ++c) {
        ovhip_fg_comp *k = &p.comp[c];
        if (!k->present) continue;
        int8_t interval[256];
        memset(interval, -1, sizeof(interval));
        for (int i = 0; i < 8; ++i) {
            for (int a = k->lower[i]; a <= k->upper[i]; ++a) interval[a] = (int8_t)i;
            int16_t *v = k->value[i];
            if (k->num_model_values == 1) v[1] = v[2] = 8;
            else if (k->num_model_values == 2) v[2] = v[1];
            if (c > 0) {
                v[0] >>= 1;
                for (int n = 1; n < 3; ++n) {
                    const int d = v[n] << 1;
                    v[n] = (int16_t)(d < 2 ? 2 : d > 14 ? 14 : d);
                }
            }
        }
        /* a cancelled SEI is derived (the reference mutates it all the same) but leaves the picture as decoded */
        if (p.cancel) continue;
        m.present[c] = 1;
        for (int a = 0; a < 256; ++a) {
            if (interval[a] < 0) continue;
            const int16_t *v = k->value[interval[a]];
            if (v[0] == 0) { m.entry[c][a] = OVHIP_FG_ENTRY(0, 0, 0); continue; }
            if (v[1] < 2 || v[1] > 14 || v[2] < 2 || v[2] > 14) return OVHIP_EINVAL;
            m.entry[c][a] = OVHIP_FG_ENTRY(v[0], v[1] - 2, v[2] - 2);
        }
    }
    *model = m;
    if (after) *after = p;
    return OVHIP_OK;
}

/* ---- the database: per cell a 64x64 block of Gaussian noise, low-passed at the cell's cut-offs, through two integer passes of the
 * 64-point inverse transform ---- */
static int8_t fg_db[OVHIP_FG_DB_BYTES];
static pthread_once_t fg_db_once = PTHREAD_ONCE_INIT;

static void
fg_db_build(void)
{
    static int32_t b[FG_N][FG_N], t[FG_N][FG_N];        /* only ever touched under the once */
    for (int h = 0; h < FG_CELLS; ++h) {
        for (int v = 0; v < FG_CELLS; ++v) {
            int8_t *cell = fg_db + (size_t)(h * FG_CELLS + v) * FG_N * FG_N;
            const int fh = ((h + 3) << 2) - 1, fv = ((v + 3) << 2) - 1;
            uint32_t seed = ovt_fg_seed[h + v * FG_CELLS];
            memset(b, 0, sizeof(b));
            for (int l = 0; l <= fv; ++l)
                for (int k = 0; k <= fh; k += 4) {
                    for (int n = 0; n < 4; ++n) b[k + n][l] = ovt_fg_gauss[(seed + (uint32_t)n) & 2047u];
                    seed = ovhip_fg_prng(seed);
                }
            b[0][0] = 0;
            for (int i = 0; i < FG_N; ++i)
                for (int j = 0; j <= fv; ++j) {             /* columns above the vertical cut-off are 0 + 128 >> 8 = 0 */
                    int32_t s = 0;
                    for (int k = 0; k <= fh; ++k) s += ovt_fg_idct64[k][i] * b[k][j];
                    t[i][j] = (s + 128) >> 8;
                }
            for (int j = 0; j < FG_N; ++j)
                for (int i = 0; i < FG_N; ++i) {
                    int32_t s = 0;
                    for (int k = 0; k <= fv; ++k) s += t[i][k] * ovt_fg_idct64[k][j];
                    s = (s + 128) >> 8;
                    cell[j * FG_N + i] = (int8_t)(s < -127 ? -127 : s > 127 ? 127 : s);    /* the reference's signed clip is symmetric */
                }
            /* horizontal 8x8 edges: the first and the last row of every 8 rows are attenuated */
            for (int l = 0; l < FG_N; l += 8)
                for (int k = 0; k < FG_N; ++k) {
                    cell[l * FG_N + k] = (int8_t)((cell[l * FG_N + k] * (int32_t)ovt_fg_deblock[v]) >> 7);
                    cell[(l + 7) * FG_N + k] = (int8_t)((cell[(l + 7) * FG_N + k] * (int32_t)ovt_fg_deblock[v]) >> 7);
                }
        }
    }
}

const int8_t *
ovhip_fg_database(void)
{
    pthread_once(&fg_db_once, fg_db_build);
    return fg_db;
}
