// Motion field output on the device (include/ovvc_hip.h, "Motion field output on the device"): the motion of a decoded picture as a
// dense field on the 4x4 luma grid in device memory -- four vector channels and one info word per cell.  The refusals, the sizes and
// what one unit says about its cells are the host twin's (ovvc_mvfield.c, ovvc_mvfield_priv.h).
//
// Two launches in order on the context's stream.  k_mvfield_clear writes the empty cell into every byte of the wanted destinations: a
// lane owns one 16-byte line of a destination and stores it whole where the line lies inside, 2 bytes at a time at a destination's two
// ends.  k_mvfield then scatters the units of all five lists in one grid: a lane owns one row of a unit's cells (1..4 cells: a unit is at
// most 16 luma samples wide).  It reads its unit (32 to 64 bytes, the same for the up to four lanes of a unit: one cache line), an affine
// row its cells' side words with one 16-byte load per cell, and stores the row's info words as one run, its vectors as one run per
// channel (planar) or per cell (cells).  A run leaves in 16-, 8- or 4-byte stores, whichever its address allows -- a planar row of a
// grid whose width is no multiple of 4 cells starts on 8- or 4-byte boundaries, a destination that is only element-aligned on 2-byte
// ones (F16) -- and the choice depends on the address and the run's length alone, never on the data.  Units never overlap, so no two
// lanes write the same byte: no LDS, no atomics.  Consecutive lanes write consecutive rows of one unit, then the next unit in
// recorder (= raster-of-CTU) order: stores of a wave fall into a few hundred bytes of a handful of rows (scatter, but a local one).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_mvfield_priv.h"

namespace {

#define MVF_NT 256

struct MvfArgs {
    ovhip_mvfield_src s;
    unsigned first[6];        // the first item of each list (4 items per unit: its rows); [5]: the item count
    int W4, H4;
    int refined;              // OVHIP_MVF_REFINED
    char *vec; uint32_t *info;
};

struct ClearArgs {
    char *dst[2];             // vectors (cleared to 0), info (cleared to OVHIP_MVF_EMPTY); nullptr: not wanted
    size_t bytes[2];
    unsigned lines0, n_lines; // 16-byte lines of dst[0] / of both
};

__global__ __launch_bounds__(MVF_NT) void k_mvfield_clear(ClearArgs a)
{
    unsigned i = blockIdx.x * MVF_NT + threadIdx.x;
    if (i >= a.n_lines) return;
    const int k = i >= a.lines0;
    if (k) i -= a.lines0;
    const uintptr_t base = (uintptr_t)(k ? a.dst[1] : a.dst[0]), end = base + (k ? a.bytes[1] : a.bytes[0]);
    const uintptr_t line = (base & ~(uintptr_t)15) + (uintptr_t)i * 16;
    const uint32_t word = k ? OVHIP_MVF_EMPTY : 0u;
    if (line >= base && line + 16 <= end) {
        // (an info destination is 4-byte aligned, so a word of the pattern never straddles a line)
        *reinterpret_cast<uint4 *>(line) = make_uint4(word, word, word, word);
        return;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uintptr_t p = line + 2 * q;
        if (p >= base && p + 2 <= end) *reinterpret_cast<uint16_t *>(p) = (uint16_t)(((p - base) & 2) ? word >> 16 : word);
    }
}

__device__ __forceinline__ void st1(char *p, uint32_t a) { *reinterpret_cast<uint32_t *>(p) = a; }
__device__ __forceinline__ void st2(char *p, uint32_t a, uint32_t b) { *reinterpret_cast<uint2 *>(p) = make_uint2(a, b); }
__device__ __forceinline__ void sth(char *p, uint32_t a) { *reinterpret_cast<uint16_t *>(p) = (uint16_t)a; }

// the first n (1..4) of four words to p, a multiple of 4
__device__ __forceinline__ void run_words(char *p, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int n)
{
    const uintptr_t ad = (uintptr_t)p;
    if (n == 4 && (ad & 15) == 0) { *reinterpret_cast<uint4 *>(p) = make_uint4(w0, w1, w2, w3); return; }
    if ((ad & 7) == 0) {
        if (n >= 2) st2(p, w0, w1); else st1(p, w0);
        if (n == 4) st2(p + 8, w2, w3); else if (n == 3) st1(p + 8, w2);
    } else {
        st1(p, w0);
        if (n >= 3) st2(p + 4, w1, w2); else if (n == 2) st1(p + 4, w1);
        if (n == 4) st1(p + 12, w3);
    }
}

// the first n (1..4) of four 16-bit values, two to a word, to p, a multiple of 2
__device__ __forceinline__ void run_halfs(char *p, uint32_t w0, uint32_t w1, int n)
{
    const uintptr_t ad = (uintptr_t)p;
    if ((ad & 3) == 0) {
        if (n == 4 && (ad & 7) == 0) { st2(p, w0, w1); return; }
        if (n >= 2) st1(p, w0); else sth(p, w0);
        if (n == 4) st1(p + 4, w1); else if (n == 3) sth(p + 4, w1);
    } else {
        sth(p, w0);
        if (n >= 3) st1(p + 2, (w0 >> 16) | (w1 << 16)); else if (n == 2) sth(p + 2, w0 >> 16);
        if (n == 4) sth(p + 6, w1 >> 16);
    }
}

template <int DT> __device__ __forceinline__ uint32_t mvf_elem(int32_t v)
{
    if constexpr (DT == OVHIP_MVF_I32) return (uint32_t)v;
    else if constexpr (DT == OVHIP_MVF_F32) return __float_as_uint((float)v * 0.0625f);
    else return (uint32_t)__half_as_ushort(__float2half_rn((float)v * 0.0625f));
}

template <int DT, int LAYOUT>
__global__ __launch_bounds__(MVF_NT) void k_mvfield(MvfArgs a)
{
    constexpr int ES = DT == OVHIP_MVF_F16 ? 2 : 4;
    const unsigned item = blockIdx.x * MVF_NT + threadIdx.x;
    if (item >= a.first[5]) return;
    const int list = (item >= a.first[1]) + (item >= a.first[2]) + (item >= a.first[3]) + (item >= a.first[4]);
    // (selects, not an index that differs from lane to lane: the arguments stay in scalar registers)
    const unsigned f = list == 0 ? a.first[0] : list == 1 ? a.first[1] : list == 2 ? a.first[2] : list == 3 ? a.first[3] : a.first[4];
    const unsigned k = (item - f) >> 2;
    const int row = (int)((item - f) & 3);
    mvf_unit_ u;
    int live;
    if (list == 0) live = mvf_from_mc_(&a.s.mc[k], 0, nullptr, &u);
    else if (list == 1) live = mvf_from_mc_(&a.s.mcx[k], 1, a.refined ? a.s.refined + 4 * (size_t)k : nullptr, &u);
    else if (list == 2) live = mvf_from_aff_(&a.s.aff[k], &u);
    else if (list == 3) live = mvf_from_rpr_(&a.s.rpr[k], &u);
    else live = mvf_from_affr_(&a.s.affr[k], &u);
    const int cx0 = u.x >> 2, cy = (u.y >> 2) + row, uw4 = u.w >> 2;
    const int n = min(min(uw4, 4), a.W4 - cx0);               // the row's cells inside the grid (a unit is at most 16 samples wide)
    if (!live || row >= (u.h >> 2) || cy >= a.H4 || n <= 0) return;
    const size_t cell0 = (size_t)cy * (size_t)a.W4 + (size_t)cx0;
    if (a.info) run_words((char *)(a.info + cell0), u.info, u.info, u.info, u.info, n);
    if (!a.vec) return;

    uint32_t e[4][4];                                         // [cell][channel], as stored
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int32_t v0 = u.v[0], v1 = u.v[1], v2 = u.v[2], v3 = u.v[3];
        if (u.aff && c < n) {
            const int32_t *sw = a.s.side + u.side_off + 4 * (size_t)(row * uw4 + c);
            int32_t s0, s1, s2, s3;
            if (((uintptr_t)sw & 15) == 0) { const int4 q = *reinterpret_cast<const int4 *>(sw); s0 = q.x; s1 = q.y; s2 = q.z; s3 = q.w; }
            else { s0 = sw[0]; s1 = sw[1]; s2 = sw[2]; s3 = sw[3]; }
            v0 = (u.use & 1) ? s0 : 0; v1 = (u.use & 1) ? s1 : 0; v2 = (u.use & 2) ? s2 : 0; v3 = (u.use & 2) ? s3 : 0;
        }
        e[c][0] = mvf_elem<DT>(v0); e[c][1] = mvf_elem<DT>(v1); e[c][2] = mvf_elem<DT>(v2); e[c][3] = mvf_elem<DT>(v3);
    }

    if constexpr (LAYOUT == OVHIP_MVF_PLANAR) {
        const size_t plane = (size_t)a.W4 * (size_t)a.H4;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            char *p = a.vec + ((size_t)ch * plane + cell0) * ES;
            if constexpr (ES == 4) run_words(p, e[0][ch], e[1][ch], e[2][ch], e[3][ch], n);
            else run_halfs(p, e[0][ch] | (e[1][ch] << 16), e[2][ch] | (e[3][ch] << 16), n);
        }
    } else {
        char *p = a.vec + cell0 * 4 * ES;
        if constexpr (ES == 4) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < n) run_words(p + 16 * c, e[c][0], e[c][1], e[c][2], e[c][3], 4);
        } else if (((uintptr_t)p & 3) == 0) {
            // two cells (8 halves) to four words
#pragma unroll
            for (int c = 0; c < 4; c += 2)
                if (c < n)
                    run_words(p + 8 * c, e[c][0] | (e[c][1] << 16), e[c][2] | (e[c][3] << 16), e[c + 1][0] | (e[c + 1][1] << 16), e[c + 1][2] | (e[c + 1][3] << 16),
                              c + 1 < n ? 4 : 2);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < n) run_halfs(p + 8 * c, e[c][0] | (e[c][1] << 16), e[c][2] | (e[c][3] << 16), 4);
        }
    }
}

template <int DT> int mvf_launch_l(const MvfArgs &a, int layout, hipStream_t st)
{
    const dim3 grid((a.first[5] + MVF_NT - 1) / MVF_NT), block(MVF_NT);
    if (layout == OVHIP_MVF_PLANAR) hipLaunchKernelGGL((k_mvfield<DT, OVHIP_MVF_PLANAR>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_mvfield<DT, OVHIP_MVF_CELLS>), grid, block, 0, st, a);
    return 0;
}

} // namespace

extern "C" int ovhip_mvfield_launch(ovhip_ctx *ctx, int32_t w, int32_t h, const ovhip_mvfield_src *d_src, const ovhip_mvfield_format *fmt,
                                    void *d_vec, size_t vec_bytes, void *d_info, size_t info_bytes)
{
    if (!ctx) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    ovhip_mvfield_plan_ p;
    const char *why = "";
    const int r = ovhip_mvfield_plan_make_(w, h, d_src, fmt, d_vec, vec_bytes, d_info, info_bytes, &p, &why);
    if (r != OVHIP_OK) {
        if (p.need) snprintf(ctx->err, sizeof(ctx->err), "ovhip_mvfield_launch: %s: %zu bytes given, the field needs %zu: invalid argument", why, p.given, p.need);
        else snprintf(ctx->err, sizeof(ctx->err), "ovhip_mvfield_launch: %s: invalid argument", why);
        return r;
    }
    const uint64_t units = (uint64_t)d_src->n_mc + d_src->n_mcx + d_src->n_aff + d_src->n_rpr + d_src->n_affr;
    if (4 * units > 0x7FFFFFFFu) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_mvfield_launch: too many units", hipSuccess);

    ClearArgs c;
    c.dst[0] = (char *)d_vec; c.dst[1] = (char *)d_info;
    c.bytes[0] = d_vec ? p.vec_bytes : 0; c.bytes[1] = d_info ? p.info_bytes : 0;
    unsigned lines[2];
    for (int k = 0; k < 2; ++k) {
        const uintptr_t b = (uintptr_t)c.dst[k];
        lines[k] = c.bytes[k] ? (unsigned)((((b + c.bytes[k] + 15) & ~(uintptr_t)15) - (b & ~(uintptr_t)15)) / 16) : 0u;
    }
    c.lines0 = lines[0]; c.n_lines = lines[0] + lines[1];
    hipLaunchKernelGGL(k_mvfield_clear, dim3((c.n_lines + MVF_NT - 1) / MVF_NT), dim3(MVF_NT), 0, ctx->stream, c);
    OV_LAUNCH_CHECK(ctx, "k_mvfield_clear");
    if (!units) return OVHIP_OK;

    MvfArgs a;
    a.s = *d_src;
    const uint32_t n[5] = { d_src->n_mc, d_src->n_mcx, d_src->n_aff, d_src->n_rpr, d_src->n_affr };
    a.first[0] = 0;
    for (int k = 0; k < 5; ++k) a.first[k + 1] = a.first[k] + 4 * n[k];
    a.W4 = p.W4; a.H4 = p.H4; a.refined = fmt->vectors == OVHIP_MVF_REFINED;
    a.vec = (char *)d_vec; a.info = (uint32_t *)d_info;
    switch (fmt->dtype) {
    case OVHIP_MVF_I32: mvf_launch_l<OVHIP_MVF_I32>(a, fmt->layout, ctx->stream); break;
    case OVHIP_MVF_F32: mvf_launch_l<OVHIP_MVF_F32>(a, fmt->layout, ctx->stream); break;
    default:            mvf_launch_l<OVHIP_MVF_F16>(a, fmt->layout, ctx->stream); break;
    }
    OV_LAUNCH_CHECK(ctx, "k_mvfield");
    return OVHIP_OK;
}
