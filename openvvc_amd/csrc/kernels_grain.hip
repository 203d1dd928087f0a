// kernels_grain.hip -- film grain synthesis on the output path: fg_grain_apply_pic (pp_film_grain.c:814-978) as pp_process_frame calls
// it (post_proc.c:106-108), one launch over the luma and both chroma planes.  include/ovvc_hip.h ("Film grain synthesis") has the
// semantics; ovvc_grain.c the host side (model derivation, database, seeds).
//
// Mapping.  A lane owns one row of one 8x8 block: a 16-byte source load, 8 bytes of the database (two dwords: the pattern offset is
// a multiple of 4), a 16-byte store.  The 8 lanes of a block are neighbours in the wave, so the block sum is three xor-shuffles; the
// 8 blocks of a wave lie side by side (64 columns x 8 rows), so the two grain samples the edge smoothing needs from the blocks
// left and right come from lanes +-8.  A 256-thread workgroup is 2 x 2 waves: 128 columns x the 16 rows of a stripe.
//
// Borders between waves: the first and the last block of a wave RECOMPUTE the one grain column they need of the block outside (its
// 8 rows are loaded by the 8 lanes of the border block, summed the same way, and one database byte is read).  That is 2 extra block
// reads per 8 -- a quarter more load instructions, nearly all of them hits in the L2 the neighbouring wave filled -- against a first
// launch that would write a descriptor per block and a second that reads it: no LDS, no barrier, no buffer of 4 bytes per block.
//
// Seeds.  The 31-bit shift register is stepped once per 16x16 block in raster order.  The host jumps it to every stripe's start
// (ovhip_fg_stripe_seeds: one word per stripe, at most 2048 words); a small launch before the main one (k_film_grain_seeds, a lane per
// workgroup of the main grid) steps from there to the block before each workgroup's first, so that a wave of the main kernel has at
// most 5 steps left.  (The first version stepped in the main kernel, with scalar instructions, up to 236 times per wave, and took three
// times as long: the scalar unit is shared by the four SIMDs of a compute unit.  LABBOOK 21.)
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"

namespace {

constexpr int FG_NT = 256;
constexpr int FG_TW = 128, FG_TH = 16;
constexpr int FG_MAX_DIM = 16384;
constexpr int FG_MAX_STRIPES = FG_MAX_DIM / 16 + 2 * (FG_MAX_DIM / 32);
constexpr int FG_SLOTS = OV_FG_SLOTS;
constexpr size_t FG_MODEL_BYTES = 3 * 256 * sizeof(uint32_t);
constexpr size_t FG_SLOT_BYTES = FG_MODEL_BYTES + (size_t)FG_MAX_STRIPES * sizeof(uint32_t);          // what travels from the host per launch
constexpr int FG_MAX_GROUPS = (FG_MAX_DIM / FG_TW) * (FG_MAX_DIM / FG_TH) + 2 * (FG_MAX_DIM / 2 / FG_TW) * (FG_MAX_DIM / 2 / FG_TH);
constexpr size_t FG_DEV_SLOT_BYTES = FG_SLOT_BYTES + (size_t)FG_MAX_GROUPS * sizeof(uint32_t);        // + the device-made seed per workgroup

struct FgPlane {
    const uint16_t *src; uint16_t *dst;
    int w, h, sstride, dstride;
    int ntx;                       // workgroups per stripe
    int seed0;                     // the plane's first word in the seed table
    int present, src_vec, dst_vec;
};
struct FgArgs {
    FgPlane p[3]; int first[3];
    const int8_t *db; const uint32_t *model; const uint32_t *seeds;
    uint32_t *group_seeds;         // per workgroup of the main grid: the register at the block before its first (at its first for tx = 0)
    int n_groups;
    int shift;                     // log2_scale + 6
};

__device__ __forceinline__ uint32_t fg_prng(uint32_t x) { return (x << 1) + (1u ^ ((x >> 2) & 1u) ^ ((x >> 30) & 1u)); }

// what a 16x16 block's seed decides: pattern column | pattern row << 8 | sign << 16
__device__ __forceinline__ uint32_t fg_offsets(uint32_t seed)
{
    return (((seed >> 16) % 52u) & ~3u) | ((((seed & 0xFFFFu) % 56u) & ~7u) << 8) | ((seed & 1u) << 16);
}

__device__ __forceinline__ int fg_sum8(int v)
{
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
    return v;
}

// the model's entry for a block of n samples that sum to `sum`; 0 (grain 0) for a block outside the plane
__device__ __forceinline__ uint32_t fg_entry(const uint32_t *model, int sum, int n)
{
    if (n == 0) return 0;
    const uint32_t avg = (n == 64 ? (uint32_t)sum >> 6 : (uint32_t)sum / (uint32_t)n) >> 2;
    return model[min(avg, 255u)];
}

// the address of row r of the block's 8x8 pattern, and its signed scale.  An entry without an interval is 0: scale 0 in cell 0.
__device__ __forceinline__ const int8_t *fg_pattern(const int8_t *db, uint32_t entry, uint32_t off, int x, int yb, int r, int &scale)
{
    const int s = (int)(int16_t)(entry & 0xFFFFu);
    scale = (off >> 16) ? -s : s;
    const int cell = (int)((entry >> 16) & 15u) * 13 + (int)((entry >> 20) & 15u);
    const int k = (int)(off & 0xFFu) + (x & 8), l = (int)((off >> 8) & 0xFFu) + (yb & 8) + r;
    return db + cell * 4096 + l * 64 + k;
}

__device__ __forceinline__ void fg_load_row(const FgPlane &p, int x, int y, int xs, int s[8])
{
    const uint16_t *q = p.src + (size_t)ov_rowoff(y, p.sstride) + x;
    if (p.src_vec && xs == 8) {
        const uint4 v = *reinterpret_cast<const uint4 *>(q);
        s[0] = (int)(v.x & 0xFFFFu); s[1] = (int)(v.x >> 16); s[2] = (int)(v.y & 0xFFFFu); s[3] = (int)(v.y >> 16);
        s[4] = (int)(v.z & 0xFFFFu); s[5] = (int)(v.z >> 16); s[6] = (int)(v.w & 0xFFFFu); s[7] = (int)(v.w >> 16);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = k < xs ? (int)q[k] : 0;
    }
}

// one lane per workgroup of the main grid: from the stripe's start to the block before the workgroup's first
__global__ __launch_bounds__(64) void k_film_grain_seeds(FgArgs a)
{
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= a.n_groups) return;
    const int pl = ov_tile_plane(a, b);
    const FgPlane p = pl == 0 ? a.p[0] : (pl == 1 ? a.p[1] : a.p[2]);
    if (!p.present) return;
    const int t = ov_tile_index(a, b, pl);
    const int ty = t / p.ntx, tx = t - ty * p.ntx;
    uint32_t sd = a.seeds[p.seed0 + ty];
    for (int i = 0; i < tx * (FG_TW / 16) - 1; ++i) sd = fg_prng(sd);
    a.group_seeds[b] = sd;
}

__global__ __launch_bounds__(FG_NT) void k_film_grain(FgArgs a)
{
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int pl = ov_tile_plane(a, b);
    const FgPlane p = pl == 0 ? a.p[0] : (pl == 1 ? a.p[1] : a.p[2]);
    const int t = ov_tile_index(a, b, pl);
    const int ty = t / p.ntx, tx = t - ty * p.ntx;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int bx = lane >> 3, r = lane & 7;
    const int x0 = tx * FG_TW + (wave & 1) * 64;             // the wave's first column
    const int yb = ty * FG_TH + (wave >> 1) * 8;             // the wave's block row
    if (x0 >= p.w || yb >= p.h) return;                      // wave-uniform
    const int x = x0 + bx * 8, y = yb + r;
    const int xs = min(max(p.w - x, 0), 8), ys = min(p.h - yb, 8);
    const bool row = y < p.h && xs > 0;

    int s[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (row) fg_load_row(p, x, y, xs, s);

    int o[8];
    if (!p.present) {                                        // a component without a model is copied
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = s[k];
    } else {
        // seeds of the 16x16 blocks before, under and after the wave
        uint32_t sd = a.group_seeds[b], before = 0;
        const int steps = (tx > 0) + (wave & 1) * 4;
        for (int i = 0; i < steps; ++i) { before = sd; sd = fg_prng(sd); }
        const uint32_t sd1 = fg_prng(sd), sd2 = fg_prng(sd1), sd3 = fg_prng(sd2), after = fg_prng(sd3);
        const uint32_t f0 = fg_offsets(sd), f1 = fg_offsets(sd1), f2 = fg_offsets(sd2), f3 = fg_offsets(sd3);
        const uint32_t off = bx < 4 ? (bx < 2 ? f0 : f1) : (bx < 6 ? f2 : f3);
        const uint32_t *model = a.model + pl * 256;

        // the lane's own block
        const int sum = fg_sum8(s[0] + s[1] + s[2] + s[3] + s[4] + s[5] + s[6] + s[7]);
        int scale;
        const int8_t *pat = fg_pattern(a.db, fg_entry(model, sum, xs * ys), off, x, yb, r, scale);
        const uint32_t lo = *reinterpret_cast<const uint32_t *>(pat), hi = *reinterpret_cast<const uint32_t *>(pat + 4);
        int g[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int d = (int)(int8_t)(((k < 4 ? lo : hi) >> (8 * (k & 3))) & 0xFFu);
            g[k] = k < xs ? (scale * d) >> a.shift : 0;
        }

        // the grain either side: column 7 of the block to the left, column 0 of the block to the right
        int left = __shfl(g[7], (lane + 56) & 63), right = __shfl(g[0], (lane + 8) & 63);
        const bool has_left = x >= 8, has_right = x + 8 < p.w;
        const bool halo = (bx == 0 && has_left) || (bx == 7 && has_right);
        const int hx = bx == 0 ? x - 8 : x + 8;
        const int hxs = halo ? min(p.w - hx, 8) : 0;
        int hs[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (halo && y < p.h) fg_load_row(p, hx, y, hxs, hs);
        const int hsum = fg_sum8(hs[0] + hs[1] + hs[2] + hs[3] + hs[4] + hs[5] + hs[6] + hs[7]);
        if (halo) {
            int hscale;
            const int8_t *hp = fg_pattern(a.db, fg_entry(model, hsum, hxs * ys), fg_offsets(bx == 0 ? before : after), hx, yb, r, hscale);
            const int hg = (hscale * (int)hp[bx == 0 ? 7 : 0]) >> a.shift;
            if (bx == 0) left = hg; else right = hg;
        }
        const int g0 = has_left ? (left + 2 * g[0] + g[1]) >> 2 : g[0];
        const int g7 = has_right ? (g[6] + 2 * g[7] + right) >> 2 : g[7];
        g[0] = g0; g[7] = g7;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = ov_clip_bd(s[k] + (g[k] << 2));
    }

    if (!row) return;
    uint16_t *d = p.dst + (size_t)ov_rowoff(y, p.dstride) + x;
    if (p.dst_vec && xs == 8) {
        *reinterpret_cast<uint4 *>(d) = make_uint4((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16),
                                                   (uint32_t)o[4] | ((uint32_t)o[5] << 16), (uint32_t)o[6] | ((uint32_t)o[7] << 16));
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) if (k < xs) d[k] = (uint16_t)o[k];
    }
}

// ---- host ----
// first grain launch of a context: the database on the device, and a ring of FG_SLOTS page-locked slots (model + stripe seeds of one
// launch) with their device copies.  A slot is written again only after the launch that read it has completed (its event).
int fg_prepare(ovhip_ctx *ctx)
{
    if (ctx->fg_d) return OVHIP_OK;
    void *d = nullptr, *h = nullptr;
    hipError_t e = hipMalloc(&d, OVHIP_FG_DB_BYTES + FG_SLOTS * FG_DEV_SLOT_BYTES);
    if (e != hipSuccess) return ov_fail(ctx, OVHIP_ENOMEM, "hipMalloc(film grain database)", e);
    e = hipHostMalloc(&h, FG_SLOTS * FG_SLOT_BYTES, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemcpyAsync(d, ovhip_fg_database(), OVHIP_FG_DB_BYTES, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // once per context: the database is pageable host memory
    for (int i = 0; i < FG_SLOTS && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ctx->fg_ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        for (int i = 0; i < FG_SLOTS; ++i) if (ctx->fg_ev[i]) { (void)hipEventDestroy(ctx->fg_ev[i]); ctx->fg_ev[i] = nullptr; }
        if (h) (void)hipHostFree(h);
        (void)hipFree(d);
        return ov_fail(ctx, OVHIP_ENOMEM, "film grain set-up", e);
    }
    ctx->fg_d = d; ctx->fg_h = h;
    ctx->fg_d_cap = OVHIP_FG_DB_BYTES + FG_SLOTS * FG_DEV_SLOT_BYTES; ctx->fg_h_cap = FG_SLOTS * FG_SLOT_BYTES;
    return OVHIP_OK;
}

} // namespace

// library-internal (ovvc_dpb_priv.h): the checker
extern "C" int ovhip_grain_refusal_(ovhip_ctx *ctx, const char *who, const ovhip_pic *pic, const ovhip_fg_model *model)
{
    if (pic->w <= 0 || pic->h <= 0 || ((pic->w | pic->h) & 3) || pic->w > FG_MAX_DIM || pic->h > FG_MAX_DIM) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: %dx%d: sizes have to be multiples of 4 (at most %d)", who, pic->w, pic->h, FG_MAX_DIM);
        return OVHIP_EINVAL;
    }
    if (model->log2_scale > 15) return ov_fail(ctx, OVHIP_EINVAL, "film grain: log2 scale above 15", hipSuccess);
    for (int c = 0; c < 3; ++c)
        for (int a = 0; a < 256 && model->present[c]; ++a) {
            const uint32_t e = model->entry[c][a];
            if (e && (!(e & OVHIP_FG_VALID) || (e >> 25) || ((e >> 16) & 15u) > 12 || ((e >> 20) & 15u) > 12))
                return ov_fail(ctx, OVHIP_EINVAL, "film grain: a model entry points outside the database", hipSuccess);
        }
    return OVHIP_OK;
}

extern "C" int ovhip_film_grain_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_fg_model *model, int32_t poc, int32_t idr_offset,
                                       const ovhip_pic *dst)
{
    if (!ctx || !src || !model || !dst) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    int r = ov_src_dst_check(ctx, "ovhip_film_grain_launch", src, dst);
    if (r != OVHIP_OK) return r;
    if (src->w != dst->w || src->h != dst->h) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_film_grain_launch: src and dst differ in size", hipSuccess);
    if ((r = ovhip_grain_refusal_(ctx, "ovhip_film_grain_launch", src, model)) != OVHIP_OK) return r;
    if ((r = fg_prepare(ctx)) != OVHIP_OK) return r;
    const uint16_t *sp[3] = { src->y, src->cb, src->cr };
    uint16_t *dp[3] = { dst->y, dst->cb, dst->cr };

    const int slot = ctx->fg_next;
    ctx->fg_next = (slot + 1) % FG_SLOTS;
    if (ctx->fg_busy[slot]) OV_HIP(ctx, hipEventSynchronize(ctx->fg_ev[slot]));
    uint32_t *h_slot = (uint32_t *)((char *)ctx->fg_h + (size_t)slot * FG_SLOT_BYTES);
    uint32_t *d_slot = (uint32_t *)((char *)ctx->fg_d + OVHIP_FG_DB_BYTES + (size_t)slot * FG_DEV_SLOT_BYTES);
    memcpy(h_slot, model->entry, FG_MODEL_BYTES);
    uint32_t *seeds = h_slot + 3 * 256;

    FgArgs a;
    int n = 0, n_seeds = 0;
    for (int i = 0; i < 3; ++i) {
        FgPlane &p = a.p[i];
        p.src = sp[i]; p.dst = dp[i];
        p.w = i ? src->w / 2 : src->w; p.h = i ? src->h / 2 : src->h;
        p.sstride = i ? src->stride_c : src->stride_y; p.dstride = i ? dst->stride_c : dst->stride_y;
        p.ntx = (p.w + FG_TW - 1) / FG_TW;
        p.present = model->present[i] != 0;
        p.src_vec = !(((uintptr_t)p.src | ((size_t)p.sstride * 2)) & 15);
        p.dst_vec = !(((uintptr_t)p.dst | ((size_t)p.dstride * 2)) & 15);
        p.seed0 = n_seeds;
        const int stripes = (p.h + FG_TH - 1) / FG_TH, per_stripe = (p.w + 15) / 16;
        if (p.present) ovhip_fg_stripe_seeds(ovhip_fg_seed(poc, idr_offset, i), per_stripe, stripes, seeds + n_seeds);
        n_seeds += stripes;
        a.first[i] = n;
        n += p.ntx * stripes;
    }
    a.db = (const int8_t *)ctx->fg_d; a.model = d_slot; a.seeds = d_slot + 3 * 256;
    a.group_seeds = d_slot + FG_SLOT_BYTES / sizeof(uint32_t); a.n_groups = n;
    a.shift = model->log2_scale + 6;
    OV_HIP(ctx, hipMemcpyAsync(d_slot, h_slot, FG_MODEL_BYTES + (size_t)n_seeds * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_film_grain_seeds, dim3((unsigned)(n + 63) / 64), dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_film_grain, dim3((unsigned)n), dim3(FG_NT), 0, ctx->stream, a);
    OV_LAUNCH_CHECK(ctx, "k_film_grain");
    OV_HIP(ctx, hipEventRecord(ctx->fg_ev[slot], ctx->stream));
    ctx->fg_busy[slot] = 1;
    return OVHIP_OK;
}
