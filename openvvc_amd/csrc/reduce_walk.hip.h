// reduce_walk.hip.h -- the walk of the reduced-size output over one tile of one plane, shared by k_output_reduce (kernels_reduce.hip:
// the tile leaves as 16-bit samples of a picture), k_output_ladder (kernels_ladder.hip: the tile leaves as a surface's elements) and
// k_ladder_lut (kernels_ladder_lut.hip: the tiles of a rung's Y, Cb and Cr stay in LDS for the colour conversion).
// Definition: include/ovvc_hip.h, "Reduced-size output on the device"; the arithmetic both sides of the library agree on:
// ovvc_reduce_priv.h.
//
// A workgroup is ONE wave: it owns 64 destination columns by a band of RD_BAND destination rows and walks down the source rows under the
// band once, a GROUP of rows at a time: as many rows as fill the wave's 128 chunk slots (7 rows at 2:1, 1 row at 8:1), so that a wave
// has all its lanes' loads in flight at every ratio.  A group's row segments (at most 64 * 8 + 2 samples each) are staged into LDS,
// double-buffered -- the next group's loads fly while this group is summed --, with 16-byte loads on the chunks that the row's ADDRESS
// puts on 16-byte boundaries and that lie inside the region, element loads on the chunks at the region's edge; nothing outside the
// region is read.  A lane keeps the first sample and the (at most 9) weights of ITS column in registers -- closed form, no table, no
// upload --, sums each row horizontally from LDS and adds that into the two running vertical sums a source row can meet (a footprint is
// at least a sample long).  A footprint that ends is divided (reciprocal estimate and one correction: exact) into an LDS tile of the
// band; what becomes of the tile is the EPILOGUE's business, the walk's template parameter.  wave64, no MFMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ovvc_reduce_priv.h"

namespace {

#define RD_TW    64                 /* destination columns of a wave */
#define RD_BAND  8                  /* destination rows of a wave */
#define RD_NT    64
#define RD_TAPS  OVHIP_REDUCE_MAX_TAPS
#define RD_CHUNK 8                  /* samples of a 16-byte chunk */
#define RD_NCH   2                  /* chunk slots of a lane per group: 128 of a wave */
#define RD_SLOTS (RD_NCH * RD_NT)
#define RD_ROWS  8                  /* rows of a group at most */
#define RD_SLACK (2 * RD_CHUNK)     /* behind a staged row: the reach of a lane whose trailing weights are zero */
// chunks of a row at most: the segment (<= 64 * 8 + 2 samples) begun up to 7 samples early (the address's phase), in whole chunks
#define RD_MAXCPR ((RD_TW * OVHIP_REDUCE_MAX_RATIO + 2 + 7 + 7) / RD_CHUNK)
// samples of a staged group: rows * cpr <= max(RD_SLOTS, RD_MAXCPR) chunks, and every row's slack
#define RD_LDS   (RD_SLOTS * RD_CHUNK + RD_ROWS * RD_SLACK)

// one tile's walk: the plane's region (src: its first sample) and destination size in this plane's samples, the ratios of the plan,
// and what the launcher derives of them (rd_shape)
struct RdTile {
    const uint16_t *src; int sstride;
    int sw, sh, dw, dh, sgx, sgy;
    int px, qx, py, qy, ntap, cpr, rows; uint32_t n; float rcp;
    int tx, ty;                                // the tile: 64 columns by RD_BAND rows of the destination
};

// what a launcher derives of a plan's ratios.  ntap: samples under a footprint; cpr: chunks a staged row takes at most -- a row's
// segment is at most ceil(64 p / q) + 2 samples, begun up to 7 samples early and ended in a whole chunk --; rows: rows of a group,
// rows * cpr <= RD_SLOTS
static inline void rd_shape(const ovhip_reduce_plan_ &pl, int *ntap, int *cpr, int *rows)
{
    *ntap = (pl.px + pl.qx - 1) / pl.qx + 1;
    if (*ntap > RD_TAPS) *ntap = RD_TAPS;
    *cpr = ((RD_TW * pl.px + pl.qx - 1) / pl.qx + 2 + 7 + 7) / RD_CHUNK;
    *rows = RD_SLOTS / *cpr < 1 ? 1 : (RD_SLOTS / *cpr > RD_ROWS ? RD_ROWS : RD_SLOTS / *cpr);
}

// What the launchers of the one-launch outputs (k_output_ladder, k_ladder_lut, k_rgb_pyramid) fill alike in their argument structs, by the
// members' names -- the structs themselves stay apart.  rd_src_fill: the source region of plan p0 (the same in every rung or level);
// rd_level_fill: a rung's or a level's ratios, shape and size
template <class Args> static inline void rd_src_fill(Args &a, const ovhip_pic *src, const ovhip_reduce_plan_ &p0)
{
    const uint16_t *sp[3] = { src->y, src->cb, src->cr };
    for (int i = 0; i < 3; ++i) {
        const int c = i != 0, stride = c ? src->stride_c : src->stride_y;
        a.src[i] = sp[i] + (size_t)(p0.y0 >> c) * (size_t)stride + (size_t)(p0.x0 >> c);
    }
    a.sstride[0] = src->stride_y; a.sstride[1] = src->stride_c;
    a.sw = p0.Ws; a.sh = p0.Hs;
}
template <class Level> static inline void rd_level_fill(Level &g, const ovhip_reduce_plan_ &rp)
{
    g.px = rp.px; g.qx = rp.qx; g.py = rp.py; g.qy = rp.qy;
    g.n = rp.n; g.rcp = 1.0f / (float)rp.n;
    rd_shape(rp, &g.ntap, &g.cpr, &g.rows);
    g.sgx = rp.sgx; g.sgy = rp.sgy;
    g.dw = rp.Wd; g.dh = rp.Hd;
}

// the first staged sample of a row whose segment begins at sample xs: back to the 16-byte boundary at or below its address
__device__ __forceinline__ int stage_base(const uint16_t *row, int xs)
{
    return xs - (int)(((uintptr_t)(row + xs) >> 1) & (RD_CHUNK - 1));
}

// chunk `ch` of row `row` (valid: the row exists and the slot is used), whose segment is samples xs .. xe; samples outside 0 .. sw-1
// are not read (they carry no weight: 0 stands in)
__device__ __forceinline__ uint4 stage_load(const uint16_t *row, bool valid, int ch, int xs, int xe, int sw)
{
    uint4 v = make_uint4(0, 0, 0, 0);
    if (!valid) return v;
    const int x = stage_base(row, xs) + RD_CHUNK * ch;
    if (x > xe) return v;
    if (x >= 0 && x + RD_CHUNK <= sw) return *reinterpret_cast<const uint4 *>(row + x);
    uint32_t e[RD_CHUNK];
#pragma unroll
    for (int i = 0; i < RD_CHUNK; ++i) e[i] = (x + i >= 0 && x + i < sw) ? (uint32_t)row[x + i] : 0u;
    return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

// where a walk's columns and rows lie in the destination plane, and who walks.  RdGrid: tile (t.tx, t.ty) of the grid of 64 x RD_BAND
// tiles, by a workgroup of one wave.  RdAt: columns k0 .. k1 (at most RD_TW of them) and rows ka .. kb - 1 (at most RD_BAND) wherever the
// caller puts them -- k_ladder_lut's tiles carry a halo, so their origins are no multiples of the tile; t.tx and t.ty are not read
// then --, by ONE WAVE of a larger workgroup, with s_row and s_out of its own: its lanes wait for one another only (the fences order its
// LDS writes and reads as __syncthreads' do, without the workgroup's barrier), so the waves of a workgroup walk different tiles at once.
struct RdGrid {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ int k0(const RdTile &t) const { return t.tx * RD_TW; }
    __device__ __forceinline__ int k1(const RdTile &t, int k0) const { return min(k0 + RD_TW, t.dw) - 1; }
    __device__ __forceinline__ int ka(const RdTile &t) const { return t.ty * RD_BAND; }
    __device__ __forceinline__ int kb(const RdTile &t, int ka) const { return min(ka + RD_BAND, t.dh); }
};
struct RdAt {
    int c0, c1, ra, rb;
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x & (RD_NT - 1); }
    __device__ __forceinline__ void sync() const
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    __device__ __forceinline__ int k0(const RdTile &) const { return c0; }
    __device__ __forceinline__ int k1(const RdTile &, int) const { return c1; }
    __device__ __forceinline__ int ka(const RdTile &) const { return ra; }
    __device__ __forceinline__ int kb(const RdTile &, int) const { return rb; }
};

// The columns and rows `at` names into s_out (every lane's column: a lane past the last column repeats it), then epi(k0, k1, ka, kb):
// columns k0 .. k1 and rows ka .. kb - 1 of the destination plane, behind at.sync(), so the epilogue may read all of s_out.
// s_row is free again when the epilogue runs.
template <class At, class Epi>
__device__ __forceinline__ void rd_walk_at(const RdTile &t, const At at, uint16_t (*s_row)[RD_LDS], uint16_t (*s_out)[RD_TW], Epi epi)
{
    const int lane = at.lane();
    const int px = t.px, qx = t.qx, py = t.py, qy = t.qy;
    const int rows = t.rows, cpr = t.cpr, rstride = cpr * RD_CHUNK + RD_SLACK;

    // this lane's column: its first sample and its weights (a lane past the plane's width works on the last column and stores nothing)
    const int k0 = at.k0(t), k1 = at.k1(t, k0);
    const int kx = min(k0 + lane, k1);
    const int jb = ovhip_reduce_first_(kx, px, qx, t.sgx, t.sw);
    int w[RD_TAPS];
#pragma unroll
    for (int i = 0; i < RD_TAPS; ++i) w[i] = jb + i < t.sw ? ovhip_reduce_weight_(kx, jb + i, px, qx, t.sgx, t.sw) : 0;
    const int xs = ovhip_reduce_first_(k0, px, qx, t.sgx, t.sw), xe = ovhip_reduce_last_(k1, px, qx, t.sgx, t.sw);

    const int ka = at.ka(t), kb = at.kb(t, ka);
    const int ys = ovhip_reduce_first_(ka, py, qy, t.sgy, t.sh), ye = ovhip_reduce_last_(kb - 1, py, qy, t.sgy, t.sh);

    // this lane's chunk slots: row of the group and chunk of that row, the same for every group
    int sr[RD_NCH], sc[RD_NCH];
#pragma unroll
    for (int c = 0; c < RD_NCH; ++c) { const int s = lane + RD_NT * c; sr[c] = s / cpr; sc[c] = s - sr[c] * cpr; }

    uint4 v[RD_NCH];
#pragma unroll
    for (int c = 0; c < RD_NCH; ++c)
        v[c] = stage_load(t.src + (size_t)(ys + sr[c]) * (size_t)t.sstride, sr[c] < rows && ys + sr[c] <= ye, sc[c], xs, xe, t.sw);

    int cur = ka, last_cur = ovhip_reduce_last_(cur, py, qy, t.sgy, t.sh);
    int acc0 = 0, acc1 = 0, buf = 0;
    const int half = (int)(t.n >> 1);
    for (int jy = ys; jy <= ye; jy += rows) {
        uint16_t *s = s_row[buf];
#pragma unroll
        for (int c = 0; c < RD_NCH; ++c)
            if (sr[c] < rows) *reinterpret_cast<uint4 *>(s + sr[c] * rstride + RD_CHUNK * sc[c]) = v[c];
        at.sync();
#pragma unroll
        for (int c = 0; c < RD_NCH; ++c) {                      // the next group's loads fly while this group is summed
            const int y = jy + rows + sr[c];
            v[c] = stage_load(t.src + (size_t)y * (size_t)t.sstride, sr[c] < rows && y <= ye, sc[c], xs, xe, t.sw);
        }
        const int rend = min(rows, ye + 1 - jy);
        for (int r = 0; r < rend; ++r) {
            const int y = jy + r;
            const uint16_t *mine = s + r * rstride + (jb - stage_base(t.src + (size_t)y * (size_t)t.sstride, xs));
            int h = 0;
#pragma unroll
            for (int i = 0; i < RD_TAPS; ++i)
                if (i < t.ntap) h += __mul24(w[i], (int)mine[i]);   // (a weight of 0 may meet a sample that was not staged: it counts nothing)
            acc0 += __mul24(ovhip_reduce_weight_(cur, y, py, qy, t.sgy, t.sh), h);
            if (cur + 1 < kb) acc1 += __mul24(ovhip_reduce_weight_(cur + 1, y, py, qy, t.sgy, t.sh), h);
            while (cur < kb && y == last_cur) {
                s_out[cur - ka][lane] = (uint16_t)ovhip_reduce_div_((uint32_t)(acc0 + half), t.n, t.rcp);
                acc0 = acc1; acc1 = 0;
                ++cur;
                last_cur = cur < kb ? ovhip_reduce_last_(cur, py, qy, t.sgy, t.sh) : -1;
            }
        }
        buf ^= 1;
    }
    at.sync();
    epi(k0, k1, ka, kb);
}

// the tile (t.tx, t.ty) of the destination plane
template <class Epi>
__device__ __forceinline__ void rd_walk(const RdTile &t, uint16_t (*s_row)[RD_LDS], uint16_t (*s_out)[RD_TW], Epi epi)
{
    rd_walk_at(t, RdGrid{}, s_row, s_out, epi);
}

} // namespace
