// Decoded picture hash SEI (payload type 132) where the picture is: CRC and checksum of the three planes of a decoded picture at its
// coded size, 12 bytes leaving the device (include/ovvc_hip.h, "Decoded picture hash"; the host half is ovvc_pichash.c).
//
// k_pic_hash: one 256-thread workgroup per ROW of a plane (Y rows, then Cb, then Cr); a lane owns runs of 8 samples, one 16-byte load
// each where the plane's rows are 16-byte aligned.  The w & 7 samples behind a row's last full run are lane 0's, sample by sample: a
// 4-wide chroma plane has nothing else, and nothing is read past a row's end.
//   checksum  per lane in uint32, wave reduction, LDS; the row's sum goes to rows[].  (One atomic add per row into the plane's word
//             was the first shape: 4320 adds on three words took 51 us per 4K picture, the adds alone; this one takes as long as the CRC.)
//   CRC       R(A) = A x^16 mod P from a zero register; R(A | B) = R(A) x^|B| + R(B).  The runs of a row are laid RIGHT-aligned on a
//             whole number of 256-lane chunks: the empty slots in front are leading zeros, which leave R alone, and every piece is
//             then followed by a length known at compile time -- x^32768 between a lane's chunks, x^(128 (255 - lane)) behind a lane's
//             runs (a table), after which the lanes, then the waves, combine by exclusive or; x^16 .. x^112 in front of the row's tail.
//             The row's remainder goes to rows[].
// k_pic_hash_rows: one workgroup per plane combines rows[] -- the checksum's by addition; the CRC's the same way as above (the rows
//   right-aligned on 256 threads; the powers of x^(16 w) come from the host), then the start value's term 0xFFFF x^(n + 16) mod P is
//   added.  No atomic, no dependence on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"

namespace {

#define PH_NT 256
#define PH_POLY 0x11021u

// a(x) b(x) mod P
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 15; i >= 0; --i) {
        r <<= 1;
        if (r & 0x10000u) r ^= PH_POLY;
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}
// x^k mod P
__host__ __device__ constexpr uint32_t gf_xpow(uint64_t k)
{
    uint32_t r = 1, b = 2;
    for (; k; k >>= 1) { if (k & 1) r = gf_mul(r, b); b = gf_mul(b, b); }
    return r;
}
// by a power of x known at compile time
template <uint64_t K> __device__ __forceinline__ uint32_t gf_mul_x(uint32_t a)
{
    constexpr uint32_t c = gf_xpow(K);
    return gf_mul(a, c);
}

// x^(128 (255 - lane)) mod P: the bits that follow a lane's run inside a chunk
struct LaneX { uint16_t v[PH_NT]; };
constexpr LaneX lane_x_table()
{
    LaneX t = {};
    for (int i = 0; i < PH_NT; ++i) t.v[i] = (uint16_t)gf_xpow(128 * (uint64_t)(PH_NT - 1 - i));
    return t;
}
__constant__ LaneX c_lane_x = lane_x_table();

// one sample into the register: its low byte, then its high byte (crc' = (crc x^8 + byte x^16) mod P each)
__device__ __forceinline__ uint32_t crc_byte(uint32_t crc, uint32_t b)
{
    uint32_t x = (crc >> 8) ^ b;
    x ^= x >> 4;
    return ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t crc_sample(uint32_t crc, uint32_t s) { return crc_byte(crc_byte(crc, s & 0xFFu), s >> 8); }
__device__ __forceinline__ uint32_t sum_sample(uint32_t s, uint32_t m) { return ((s & 0xFFu) ^ m) + ((s >> 8) ^ m); }

struct HashArgs {
    const uint16_t *src[3]; int stride[3], w[3], h[3];
    int first[3];                     // first row (= workgroup) of each plane in the grid
    int vec[3];                       // the plane's rows are 16-byte aligned
    uint32_t xrow[3];                 // CRC: x^(16 w) mod P, one row's length
    uint32_t xthr[3][8];              //      xrow^(rows per thread << k): between the threads of k_pic_hash_rows
    uint32_t init[3];                 //      0xFFFF x^(n + 16) mod P
};

template <bool CRC>
__global__ __launch_bounds__(PH_NT) void k_pic_hash(HashArgs a, uint32_t *__restrict__ rows)
{
    __shared__ uint32_t s_wave[PH_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int c = ov_tile_plane(a, b), y = ov_tile_index(a, b, c);
    const int w = c == 0 ? a.w[0] : a.w[1], stride = c == 0 ? a.stride[0] : a.stride[1];
    const uint16_t *base = c == 0 ? a.src[0] : (c == 1 ? a.src[1] : a.src[2]);
    const uint16_t *row = base + (size_t)y * stride;
    const bool vec = (c == 0 ? a.vec[0] : (c == 1 ? a.vec[1] : a.vec[2])) != 0;
    const int n_full = w >> 3, n_chunks = (n_full + PH_NT - 1) / PH_NT, lead = n_chunks * PH_NT - n_full;
    const uint32_t my = ((uint32_t)y & 0xFFu) ^ ((uint32_t)y >> 8);
    uint32_t acc = 0;
    for (int k = 0; k < n_chunks; ++k) {
        const int run = k * PH_NT + tid - lead;                   // < 0: an empty slot in front of the row
        uint32_t s[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (run >= 0) {
            if (vec) {
                const uint4 v = reinterpret_cast<const uint4 *>(row)[run];
                s[0] = v.x & 0xFFFFu; s[1] = v.x >> 16; s[2] = v.y & 0xFFFFu; s[3] = v.y >> 16;
                s[4] = v.z & 0xFFFFu; s[5] = v.z >> 16; s[6] = v.w & 0xFFFFu; s[7] = v.w >> 16;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) s[j] = row[8 * run + j];
            }
        }
        if (CRC) {
            uint32_t r = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) r = crc_sample(r, s[j]);
            acc = gf_mul_x<128 * PH_NT>(acc) ^ r;
        } else if (run >= 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t x = (uint32_t)(8 * run + j);
                acc += sum_sample(s[j], my ^ (x & 0xFFu) ^ (x >> 8));
            }
        }
    }
    // the row's tail: fewer than 8 samples, lane 0's
    uint32_t tail = 0;
    const int nt = w & 7;
    if (tid == 0)
        for (int j = 0; j < nt; ++j) {
            const uint32_t x = (uint32_t)(8 * n_full + j), sv = row[x];
            tail = CRC ? crc_sample(tail, sv) : tail + sum_sample(sv, my ^ (x & 0xFFu) ^ (x >> 8));
        }
    // lanes within the wave (lane 0 ends up with the wave's 64 runs), then the waves through LDS; the CRC's pieces are moved to their
    // place in the chunk first, after which they combine by exclusive or
    if (CRC) acc = gf_mul(acc, c_lane_x.v[tid]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) acc = CRC ? acc ^ __shfl_down(acc, d) : acc + __shfl_down(acc, d);
    if ((tid & 63) == 0) s_wave[tid >> 6] = acc;
    __syncthreads();
    if (tid != 0) return;
    if (CRC) {
        uint32_t r = 0;
#pragma unroll
        for (int i = 0; i < PH_NT / 64; ++i) r ^= s_wave[i];
        // nt x 16 bits follow the full runs (x^0 .. x^112: one of eight constants)
        uint32_t xt = 1;
        for (int j = 0; j < nt; ++j) xt = gf_mul_x<16>(xt);
        rows[b] = gf_mul(r, xt) ^ tail;
    } else {
        uint32_t r = tail;
#pragma unroll
        for (int i = 0; i < PH_NT / 64; ++i) r += s_wave[i];
        rows[b] = r;
    }
}

template <bool CRC>
__global__ __launch_bounds__(PH_NT) void k_pic_hash_rows(HashArgs a, const uint32_t *__restrict__ rows, uint32_t *__restrict__ out)
{
    __shared__ uint32_t s_r[PH_NT];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int h = c == 0 ? a.h[0] : a.h[1], first = c == 0 ? a.first[0] : (c == 1 ? a.first[1] : a.first[2]);
    const uint32_t xrow = c == 0 ? a.xrow[0] : a.xrow[1];
    const int per = (h + PH_NT - 1) / PH_NT, lead = per * PH_NT - h;        // rows per thread; empty slots in front
    uint32_t acc = 0;
    for (int j = 0; j < per; ++j) {
        const int r = tid * per + j - lead;
        const uint32_t v = r >= 0 ? rows[first + r] : 0u;
        acc = CRC ? gf_mul(acc, xrow) ^ v : acc + v;
    }
    s_r[tid] = acc;
    for (int k = 0; k < 8; ++k) {
        __syncthreads();
        const int d = 1 << k;
        if ((tid & (2 * d - 1)) == 0) s_r[tid] = CRC ? gf_mul(s_r[tid], c == 0 ? a.xthr[0][k] : a.xthr[1][k]) ^ s_r[tid + d] : s_r[tid] + s_r[tid + d];
    }
    if (tid == 0) out[c] = CRC ? s_r[0] ^ (c == 0 ? a.init[0] : a.init[1]) : s_r[0];
}

// what the launch refuses, and the launch's arguments
static bool hash_args(const ovhip_pic *pic, int n_planes, HashArgs &a)
{
    if (pic->w <= 0 || pic->h <= 0 || (pic->w & 1) || (pic->h & 1) || pic->w > 16384 || pic->h > 16384) return false;
    memset(&a, 0, sizeof(a));
    int first = 0;
    for (int c = 0; c < 3; ++c) {
        const uint16_t *p = c == 0 ? pic->y : (c == 1 ? pic->cb : pic->cr);
        a.w[c] = c ? pic->w / 2 : pic->w; a.h[c] = c ? pic->h / 2 : pic->h; a.stride[c] = c ? pic->stride_c : pic->stride_y;
        a.first[c] = first;
        if (c >= n_planes) { a.src[c] = nullptr; a.vec[c] = 0; continue; }          // (first[] of an absent plane = the grid's end)
        if (!p || a.stride[c] < a.w[c]) return false;
        a.src[c] = p;
        a.vec[c] = ((uintptr_t)p & 15) == 0 && (a.stride[c] & 7) == 0;
        first += a.h[c];
        const int per = (a.h[c] + PH_NT - 1) / PH_NT;
        a.xrow[c] = gf_xpow(16 * (uint64_t)a.w[c]);
        for (int k = 0; k < 8; ++k) a.xthr[c][k] = gf_xpow(16 * (uint64_t)a.w[c] * (uint64_t)per << k);
        a.init[c] = gf_mul(0xFFFFu, gf_xpow(16 * (uint64_t)a.w[c] * (uint64_t)a.h[c] + 16));
    }
    return true;
}

} // namespace

extern "C" int ovhip_pic_hash_launch(ovhip_ctx *ctx, const ovhip_pic *pic, int method, int n_planes, uint32_t *d_out)
{
    if (!ctx || !pic) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    HashArgs a;
    if (!d_out || (method != OVHIP_HASH_CRC && method != OVHIP_HASH_CHECKSUM) || (n_planes != 1 && n_planes != 3) || !hash_args(pic, n_planes, a))
        return ov_fail(ctx, OVHIP_EINVAL, "ovhip_pic_hash_launch: bad method / plane count / picture", hipSuccess);
    const int n_rows = a.h[0] + (n_planes == 3 ? 2 * a.h[1] : 0);
    if ((size_t)n_rows * sizeof(uint32_t) > ctx->hash_d_cap) {
        if (ctx->hash_d) (void)hipFree(ctx->hash_d);               // (waits for the device: a launch that still reads it has ended)
        ctx->hash_d = nullptr; ctx->hash_d_cap = 0;
        const hipError_t e = hipMalloc(&ctx->hash_d, (size_t)n_rows * sizeof(uint32_t));
        if (e != hipSuccess) return ov_fail(ctx, OVHIP_ENOMEM, "hipMalloc(picture hash rows)", e);
        ctx->hash_d_cap = (size_t)n_rows * sizeof(uint32_t);
    }
    // every word of d_out is written by the second launch (nothing accumulates in it: no reset)
    uint32_t *rows = (uint32_t *)ctx->hash_d;
    if (method == OVHIP_HASH_CRC) {
        hipLaunchKernelGGL(k_pic_hash<true>, dim3((unsigned)n_rows), dim3(PH_NT), 0, ctx->stream, a, rows);
        hipLaunchKernelGGL(k_pic_hash_rows<true>, dim3((unsigned)n_planes), dim3(PH_NT), 0, ctx->stream, a, rows, d_out);
    } else {
        hipLaunchKernelGGL(k_pic_hash<false>, dim3((unsigned)n_rows), dim3(PH_NT), 0, ctx->stream, a, rows);
        hipLaunchKernelGGL(k_pic_hash_rows<false>, dim3((unsigned)n_planes), dim3(PH_NT), 0, ctx->stream, a, rows, d_out);
    }
    OV_LAUNCH_CHECK(ctx, "k_pic_hash");
    return OVHIP_OK;
}

extern "C" int ovhip_pic_hash(ovhip_ctx *ctx, const ovhip_pic *pic, int method, int n_planes, ovhip_pic_hash_value *out)
{
    if (!ctx || !pic || !out) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    if (method != OVHIP_HASH_MD5) {
        int r = ov_scratch(ctx, 16, 16);
        if (r) return r;
        uint32_t *d = (uint32_t *)ctx->scratch_d, *hw = (uint32_t *)ctx->scratch_h;
        r = ovhip_pic_hash_launch(ctx, pic, method, n_planes, d);
        if (r) return r;
        if (hipMemcpyAsync(hw, d, (size_t)n_planes * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            return ov_fail(ctx, OVHIP_ENODEV, "ovhip_pic_hash: D2H", hipGetLastError());
        if (ov_sync_stream(ctx) != hipSuccess) return ov_fail(ctx, OVHIP_ELAUNCH, "ovhip_pic_hash", hipGetLastError());
        memset(out, 0, sizeof(*out));
        out->method = (uint8_t)method; out->n_planes = (uint8_t)n_planes;
        for (int c = 0; c < n_planes; ++c) {
            uint8_t *v = out->value[c];
            if (method == OVHIP_HASH_CRC) { v[0] = (uint8_t)(hw[c] >> 8); v[1] = (uint8_t)hw[c]; }
            else { v[0] = (uint8_t)(hw[c] >> 24); v[1] = (uint8_t)(hw[c] >> 16); v[2] = (uint8_t)(hw[c] >> 8); v[3] = (uint8_t)hw[c]; }
        }
        return OVHIP_OK;
    }
    // MD5, the conformance route: the planes, tight, into the page-locked scratch; then the host's hash over them on this thread
    HashArgs a;
    if ((n_planes != 1 && n_planes != 3) || !hash_args(pic, n_planes, a))
        return ov_fail(ctx, OVHIP_EINVAL, "ovhip_pic_hash: bad plane count / picture", hipSuccess);
    const size_t ysz = (size_t)a.w[0] * a.h[0], csz = (size_t)a.w[1] * a.h[1];
    int r = ov_scratch(ctx, 0, (ysz + (n_planes == 3 ? 2 * csz : 0)) * sizeof(uint16_t));
    if (r) return r;
    uint16_t *hp[3] = { (uint16_t *)ctx->scratch_h, (uint16_t *)ctx->scratch_h + ysz, (uint16_t *)ctx->scratch_h + ysz + csz };
    for (int c = 0; c < n_planes; ++c)
        OV_HIP(ctx, hipMemcpy2DAsync(hp[c], (size_t)a.w[c] * 2, a.src[c], (size_t)a.stride[c] * 2, (size_t)a.w[c] * 2, a.h[c], hipMemcpyDeviceToHost, ctx->stream));
    if (ov_sync_stream(ctx) != hipSuccess) return ov_fail(ctx, OVHIP_ELAUNCH, "ovhip_pic_hash: D2H", hipGetLastError());
    return ovhip_pic_hash_host(OVHIP_HASH_MD5, n_planes, hp[0], hp[1], hp[2], pic->w, pic->h, a.w[0], a.w[1], out);
}
