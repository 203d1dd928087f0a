// kernels_scale.hip -- output resampling on gfx950: a decoded picture of one size leaves the device at another (the output
// half of reference picture resampling).  Replaces pp_sample_rate_conv (pp_pic_scale.c:250-377), which pp_process_frame
// (post_proc.c:116-126) calls once per plane when the decoder's `upscale` option is on (ovdec.c:562), for up-sampling and
// equal size; down-sampling (the reference's 12-tap tables) is refused.
//
// One launch for the luma tiles and both chroma planes' tiles, as k_alf.  A workgroup of 256 owns a 64 x 32 destination
// tile: the source window the tile reads (at most 32 + taps - 1 rows of 64 + taps - 1 columns when up-sampling) is staged
// into LDS with aligned 8-byte loads, coordinates clamped there (no padded picture); the horizontal pass runs from LDS into
// an int32 LDS tile (no shift, no clip: intermediates reach 2^17), the vertical pass from that tile into registers, 8
// neighbouring samples per lane, one 16-byte store.  Integer position and phase vary per column / row, so every lane
// holds the tap row of ITS column (horizontal pass) or row (vertical pass) in registers, fetched once per pass.
// Products are 24-bit (v_mad_i32_i24): taps < 2^7, samples < 2^10, intermediates < 2^17.  wave64, no MFMA.
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "vvc_mc_taps.h"

namespace {

#define SC_TW   64                 /* destination tile */
#define SC_TH   32
#define SC_NT   256
#define SC_ROWS (SC_TH + 7)        /* source rows of a tile: the vertical positions of 32 rows span <= 32 rows, + 8 taps - 1 */
#define SC_SRCW 80                 /* staged source columns: 64 + 7, begun at a multiple of 4, in groups of 4 */
#define SC_TMPS (SC_TW + 4)        /* row stride of the int32 tile (dwords): 16-byte aligned rows that do not start on one bank */
#define SC_MAX_DIM 16384           /* positions (index * scale) and the scale's numerator stay far inside int32 */

struct ScaleTaps { int8_t l[16][8]; int8_t c[32][4]; };
constexpr ScaleTaps build_scale_taps()
{
    ScaleTaps t{};
    for (int p = 0; p < 16; ++p) for (int k = 0; k < 8; ++k) t.l[p][k] = ovt_mc_luma[p][k];
    for (int p = 0; p < 32; ++p) for (int k = 0; k < 4; ++k) t.c[p][k] = ovt_mc_chroma[p][k];
    return t;
}
__device__ const ScaleTaps __attribute__((aligned(16))) g_scale_taps = build_scale_taps();

struct ScalePlane {
    const uint16_t *src; uint16_t *dst;
    int ow, oh, sstride;           // source plane
    int sw, sh, dstride;           // destination plane
    int scale_hor, scale_ver, add_x, add_y;
    int ntx;                       // tiles per tile row
    int src_vec, dst_vec;          // 8-byte source loads / 16-byte destination stores are aligned for this plane
};
struct ScaleArgs { ScalePlane p[3]; int first[3]; };

// Integer position and phase of destination index i along one axis.  THE one place the phase is derived: it is the LOW
// bits of the fixed-point position (ref & mask), not the bits below the integer part -- what the reference computes
// (pp_pic_scale.c:333-335, :356-358) and therefore what its output file holds.
template <int BITS, int MASK>
__device__ __forceinline__ void scale_pos(int i, int scale, int add, int &ip, int &ph)
{
    const int ref = __mul24(i, scale) + add;
    ip = ref >> BITS;              // arithmetic: chroma positions may start below 0
    ph = ref & MASK;
}

template <int NT>
__device__ __forceinline__ void load_taps(int ph, int f[NT])
{
    if (NT == 8) {
        const uint2 v = *reinterpret_cast<const uint2 *>(g_scale_taps.l[ph]);
#pragma unroll
        for (int k = 0; k < 4; ++k) { f[k] = (int)(int8_t)(v.x >> (8 * k)); f[4 + k] = (int)(int8_t)(v.y >> (8 * k)); }
    } else {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(g_scale_taps.c[ph]);
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = (int)(int8_t)(v >> (8 * k));
    }
}

// One destination tile of one plane.  NT: 8 (luma: 13 fractional bits, 16 phases) or 4 (chroma: 14 bits, 32 phases).
template <int NT>
__device__ __forceinline__ void scale_tile(const ScalePlane &p, int tx, int ty, uint16_t *s_src, int *s_tmp, int tid)
{
    constexpr int BITS = NT == 8 ? 13 : 14, MASK = NT == 8 ? 15 : 31, B = NT / 2 - 1;
    const int i0 = tx * SC_TW, j0 = ty * SC_TH;
    const int i1 = min(i0 + SC_TW, p.sw) - 1, j1 = min(j0 + SC_TH, p.sh) - 1;
    int x_first, x_last, y_first, y_last, ph;
    scale_pos<BITS, MASK>(i0, p.scale_hor, p.add_x, x_first, ph);
    scale_pos<BITS, MASK>(i1, p.scale_hor, p.add_x, x_last, ph);
    scale_pos<BITS, MASK>(j0, p.scale_ver, p.add_y, y_first, ph);
    scale_pos<BITS, MASK>(j1, p.scale_ver, p.add_y, y_last, ph);
    // the window: rows rb .. rb + nrows - 1, columns gx0 .. gx0 + 4 * ncolg - 1 (both may leave the plane: clamped below)
    const int rb = y_first - B;
    const int nrows = min(y_last - y_first + NT, SC_ROWS);
    const int gx0 = (x_first - B) & ~3;
    const int ncolg = min(((x_last + NT / 2 - gx0) >> 2) + 1, SC_SRCW / 4);

    // stage: 32 slots per row, a lane takes one group of 4 columns
    for (int t = tid; t < nrows * 32; t += SC_NT) {
        const int r = t >> 5, g = t & 31;
        if (g >= ncolg) continue;
        const int x = gx0 + 4 * g;
        const uint16_t *row = p.src + (size_t)ov_rowoff(ov_clip3(rb + r, 0, p.oh - 1), p.sstride);
        uint2 v;
        if (p.src_vec && x >= 0 && x + 4 <= p.ow) {
            v = *reinterpret_cast<const uint2 *>(row + x);
        } else {
            const uint32_t a = row[ov_clip3(x, 0, p.ow - 1)], b = row[ov_clip3(x + 1, 0, p.ow - 1)];
            const uint32_t c = row[ov_clip3(x + 2, 0, p.ow - 1)], d = row[ov_clip3(x + 3, 0, p.ow - 1)];
            v.x = a | (b << 16); v.y = c | (d << 16);
        }
        *reinterpret_cast<uint2 *>(s_src + r * SC_SRCW + 4 * g) = v;
    }
    __syncthreads();

    {   // horizontal: a lane keeps one destination column and walks down the window's rows
        const int c = tid & (SC_TW - 1);
        int xi, phx, f[NT];
        scale_pos<BITS, MASK>(min(i0 + c, p.sw - 1), p.scale_hor, p.add_x, xi, phx);
        load_taps<NT>(phx, f);
        const int xo = ov_clip3(xi - B - gx0, 0, SC_SRCW - NT);
        for (int r = tid >> 6; r < nrows; r += SC_NT / SC_TW) {
            const uint16_t *s = s_src + r * SC_SRCW + xo;
            int acc = 0;
#pragma unroll
            for (int k = 0; k < NT; ++k) acc += __mul24(f[k], (int)s[k]);
            s_tmp[r * SC_TMPS + c] = acc;
        }
    }
    __syncthreads();

    {   // vertical: a lane owns 8 neighbouring samples of one destination row
        const int j = j0 + (tid >> 3), cg = (tid & 7) * 8;
        if (j > j1 || i0 + cg > i1) return;
        int yi, phy, f[NT];
        scale_pos<BITS, MASK>(j, p.scale_ver, p.add_y, yi, phy);
        load_taps<NT>(phy, f);
        const int r0 = ov_clip3(yi - y_first, 0, SC_ROWS - NT);          // = (yi - B) - rb
        int acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const int4 *q = reinterpret_cast<const int4 *>(s_tmp + (r0 + k) * SC_TMPS + cg);
            const int4 a = q[0], b = q[1];
            acc[0] += __mul24(f[k], a.x); acc[1] += __mul24(f[k], a.y); acc[2] += __mul24(f[k], a.z); acc[3] += __mul24(f[k], a.w);
            acc[4] += __mul24(f[k], b.x); acc[5] += __mul24(f[k], b.y); acc[6] += __mul24(f[k], b.z); acc[7] += __mul24(f[k], b.w);
        }
        uint32_t o[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) o[n] = (uint32_t)ov_clip_bd((acc[n] + 2048) >> 12);
        uint16_t *d = p.dst + (size_t)ov_rowoff(j, p.dstride) + i0 + cg;
        if (p.dst_vec && i0 + cg + 8 <= p.sw) {
            *reinterpret_cast<uint4 *>(d) = make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
        } else {
#pragma unroll
            for (int n = 0; n < 8; ++n) if (i0 + cg + n < p.sw) d[n] = (uint16_t)o[n];
        }
    }
}

__global__ __launch_bounds__(SC_NT) void k_output_scale(ScaleArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_src[SC_ROWS * SC_SRCW];
    __shared__ __attribute__((aligned(16))) int s_tmp[SC_ROWS * SC_TMPS];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int pl = ov_tile_plane(a, b);
    const ScalePlane p = pl == 0 ? a.p[0] : (pl == 1 ? a.p[1] : a.p[2]);
    const int t = ov_tile_index(a, b, pl);
    const int ty = t / p.ntx, tx = t - ty * p.ntx;
    if (pl == 0) scale_tile<8>(p, tx, ty, s_src, s_tmp, tid);
    else         scale_tile<4>(p, tx, ty, s_src, s_tmp, tid);
}

// ---- host ----
struct PlaneScale { int scale_hor, scale_ver, add_x, add_y; };

// pp_pic_scale.c:254-274 for one plane type; 0, or OVHIP_EINVAL when the scaling window leaves nothing
int plane_scale(int ow, int oh, int sw, int sh, const ovhip_scale_info *si, int luma, PlaneScale &ps)
{
    uint16_t extra_w = (uint16_t)((si->win_left + si->win_right) << 1), extra_h = (uint16_t)((si->win_top + si->win_bottom) << 1);
    if (luma) { extra_w = (uint16_t)(extra_w << 1); extra_h = (uint16_t)(extra_h << 1); }
    const int bits = luma ? 13 : 14;
    if (ow - extra_w <= 0 || oh - extra_h <= 0) return OVHIP_EINVAL;
    ps.scale_hor = ((ow - extra_w) << bits) / sw;
    ps.scale_ver = ((oh - extra_h) << bits) / sh;
    ps.add_x = ps.add_y = 0;
    if (!luma) {
        ps.add_x = ((1 - (si->chroma_hor_col != 0)) * 8 * (ps.scale_hor - (1 << bits)) + (1 << (bits - 1))) >> bits;
        ps.add_y = ((1 - (si->chroma_ver_col != 0)) * 8 * (ps.scale_ver - (1 << bits)) + (1 << (bits - 1))) >> bits;
    }
    return OVHIP_OK;
}

int scale_check(int32_t src_w, int32_t src_h, const ovhip_scale_info *info, int32_t dst_w, int32_t dst_h, PlaneScale ps[2])
{
    if (src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0 || ((src_w | src_h | dst_w | dst_h) & 3)
        || src_w > SC_MAX_DIM || src_h > SC_MAX_DIM || dst_w > SC_MAX_DIM || dst_h > SC_MAX_DIM) return OVHIP_EINVAL;
    if (plane_scale(src_w, src_h, dst_w, dst_h, info, 1, ps[0]) || plane_scale(src_w / 2, src_h / 2, dst_w / 2, dst_h / 2, info, 0, ps[1]))
        return OVHIP_EINVAL;
    if (ps[0].scale_hor > (1 << 13) || ps[0].scale_ver > (1 << 13) || ps[1].scale_hor > (1 << 14) || ps[1].scale_ver > (1 << 14))
        return OVHIP_EUNSUP;
    return OVHIP_OK;
}

// scale_check with the reason of a refusal in the context's error text
int scale_check_said(ovhip_ctx *ctx, const char *who, const ovhip_pic *src, const ovhip_scale_info *info, int32_t dst_w, int32_t dst_h, PlaneScale ps[2])
{
    const int r = scale_check(src->w, src->h, info, dst_w, dst_h, ps);
    if (r == OVHIP_EUNSUP)
        snprintf(ctx->err, sizeof(ctx->err), "%s: %dx%d -> %dx%d is down-sampling (luma factors %d, %d of %d; chroma %d, %d of %d): the reference's 12-tap "
                 "path is not supported", who, src->w, src->h, dst_w, dst_h, ps[0].scale_hor, ps[0].scale_ver, 1 << 13, ps[1].scale_hor, ps[1].scale_ver, 1 << 14);
    else if (r != OVHIP_OK)
        snprintf(ctx->err, sizeof(ctx->err), "%s: %dx%d -> %dx%d: sizes have to be multiples of 4 (at most %d) and the scaling window has to leave samples",
                 who, src->w, src->h, dst_w, dst_h, SC_MAX_DIM);
    return r;
}

} // namespace

extern "C" int ovhip_output_scale_check(int32_t src_w, int32_t src_h, const ovhip_scale_info *info, int32_t dst_w, int32_t dst_h, int32_t scale[4])
{
    if (!info || !scale) return OVHIP_EINVAL;
    PlaneScale ps[2] = {};
    const int r = scale_check(src_w, src_h, info, dst_w, dst_h, ps);
    scale[0] = ps[0].scale_hor; scale[1] = ps[0].scale_ver; scale[2] = ps[1].scale_hor; scale[3] = ps[1].scale_ver;
    return r;
}

// library-internal (ovvc_dpb_priv.h)
extern "C" int ovhip_scale_refusal_(ovhip_ctx *ctx, const char *who, const ovhip_pic *src, const ovhip_scale_info *info, int32_t dst_w, int32_t dst_h)
{
    PlaneScale ps[2] = {};
    return scale_check_said(ctx, who, src, info, dst_w, dst_h, ps);
}

extern "C" int ovhip_output_scale_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_scale_info *info, const ovhip_pic *dst)
{
    if (!ctx || !src || !info || !dst) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    PlaneScale ps[2] = {};
    int r = ov_src_dst_check(ctx, "ovhip_output_scale_launch", src, dst);
    if (r == OVHIP_OK) r = scale_check_said(ctx, "ovhip_output_scale_launch", src, info, dst->w, dst->h, ps);
    if (r != OVHIP_OK) return r;
    const uint16_t *sp[3] = { src->y, src->cb, src->cr };
    uint16_t *dp[3] = { dst->y, dst->cb, dst->cr };
    ScaleArgs a;
    int n = 0;
    for (int i = 0; i < 3; ++i) {
        ScalePlane &p = a.p[i];
        const PlaneScale &s = ps[i != 0];
        p.src = sp[i]; p.dst = dp[i];
        p.ow = i ? src->w / 2 : src->w; p.oh = i ? src->h / 2 : src->h; p.sstride = i ? src->stride_c : src->stride_y;
        p.sw = i ? dst->w / 2 : dst->w; p.sh = i ? dst->h / 2 : dst->h; p.dstride = i ? dst->stride_c : dst->stride_y;
        p.scale_hor = s.scale_hor; p.scale_ver = s.scale_ver; p.add_x = s.add_x; p.add_y = s.add_y;
        p.ntx = (p.sw + SC_TW - 1) / SC_TW;
        p.src_vec = !(((uintptr_t)p.src | ((size_t)p.sstride * 2)) & 7) && !(p.ow & 3);
        p.dst_vec = !(((uintptr_t)p.dst | ((size_t)p.dstride * 2)) & 15);
        a.first[i] = n;
        n += p.ntx * ((p.sh + SC_TH - 1) / SC_TH);
    }
    hipLaunchKernelGGL(k_output_scale, dim3((unsigned)n), dim3(SC_NT), 0, ctx->stream, a);
    OV_LAUNCH_CHECK(ctx, "k_output_scale");
    return OVHIP_OK;
}
