// run_io.hip.h -- a lane's run of a row in registers, shared by the streaming output kernels (kernels_rgb.hip, kernels_surface.hip):
// elements packed into dwords, loaded and stored 16 bytes at a time where the run's address is a multiple of 16, else 8 or 4 at a
// time, else element by element -- the path of a row's tail and of an address that is only element-aligned.  Which path a run takes
// depends on its address alone, never on the data.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// element e (a compile-time index after unrolling) of a run kept as dwords
template <int ES, int NW> __device__ __forceinline__ void run_put(uint32_t (&w)[NW], int e, uint32_t bits)
{
    if constexpr (ES == 4) w[e] = bits;
    else if constexpr (ES == 2) w[e >> 1] |= bits << (16 * (e & 1));
    else w[e >> 2] |= bits << (8 * (e & 3));
}
template <int ES, int NW> __device__ __forceinline__ uint32_t run_get(const uint32_t (&w)[NW], int e)
{
    if constexpr (ES == 4) return w[e];
    else if constexpr (ES == 2) return (w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
    else return (w[e >> 2] >> (8 * (e & 3))) & 0xFFu;
}

// NS samples at p, of which the first n exist (n < NS: a row's tail), two to a dword
template <int NS> __device__ __forceinline__ void run_load(const uint16_t *p, uint32_t (&w)[NS / 2], int n)
{
    constexpr int NW = NS / 2;
    const uintptr_t ad = (uintptr_t)p;
    if (n == NS && (ad & 15) == 0) {
#pragma unroll
        for (int k = 0; k < NW; k += 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p + 2 * k);
            w[k] = v.x; w[k + 1] = v.y; w[k + 2] = v.z; w[k + 3] = v.w;
        }
    } else if (n == NS && (ad & 7) == 0) {
#pragma unroll
        for (int k = 0; k < NW; k += 2) {
            const uint2 v = *reinterpret_cast<const uint2 *>(p + 2 * k);
            w[k] = v.x; w[k + 1] = v.y;
        }
    } else if (n == NS && (ad & 3) == 0) {
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = *reinterpret_cast<const uint32_t *>(p + 2 * k);
    } else {
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const uint32_t lo = 2 * k < n ? p[2 * k] : 0u, hi = 2 * k + 1 < n ? p[2 * k + 1] : 0u;
            w[k] = lo | (hi << 16);
        }
    }
}

// NE elements of ES bytes at p, of which the first n exist (n < NE: a row's tail).  p is a multiple of ES.  The run is a whole number
// of 8-byte pairs of dwords: a plane's 8 / 16 / 32 / 64 bytes, or the 24 / 48 / 96 bytes of 8 packed RGB pixels.
template <int ES, int NE> __device__ __forceinline__ void run_store(char *p, const uint32_t (&w)[NE * ES / 4], int n)
{
    constexpr int NB = NE * ES, NW = NB / 4;
    const uintptr_t ad = (uintptr_t)p;
    if (n == NE && (ad & 15) == 0) {
#pragma unroll
        for (int k = 0; k + 4 <= NW; k += 4) *reinterpret_cast<uint4 *>(p + 4 * k) = make_uint4(w[k], w[k + 1], w[k + 2], w[k + 3]);
        if constexpr (NW & 2) *reinterpret_cast<uint2 *>(p + 4 * (NW & ~3)) = make_uint2(w[NW & ~3], w[(NW & ~3) + 1]);
    } else if (n == NE && (ad & 7) == 0) {
#pragma unroll
        for (int k = 0; k < NW; k += 2) *reinterpret_cast<uint2 *>(p + 4 * k) = make_uint2(w[k], w[k + 1]);
    } else if (n == NE && (ad & 3) == 0) {
#pragma unroll
        for (int k = 0; k < NW; ++k) *reinterpret_cast<uint32_t *>(p + 4 * k) = w[k];
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const uint32_t v = run_get<ES, NW>(w, e);
            if (e < n) {
                if constexpr (ES == 4) *reinterpret_cast<uint32_t *>(p + 4 * e) = v;
                else if constexpr (ES == 2) *reinterpret_cast<uint16_t *>(p + 2 * e) = (uint16_t)v;
                else *reinterpret_cast<uint8_t *>(p + e) = (uint8_t)v;
            }
        }
    }
}

} // namespace
