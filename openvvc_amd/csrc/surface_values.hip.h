// surface_values.hip.h -- the value functions of the surface output (include/ovvc_hip.h, "Surface output on the device", Values),
// shared by the kernels that store a surface's elements: k_surface (kernels_surface.hip) and k_output_ladder (kernels_ladder.hip).
// Samples stay packed two to a dword.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ovvc_hip.h"

namespace {

// the two thresholds of output row `row` of a plane, for an even and an odd column: D[row & 1][0] | D[row & 1][1] << 16 (ROUND: 2 | 2 << 16)
__device__ __forceinline__ uint32_t surf_thr(bool dither, int row)
{
    return dither ? ((row & 1) ? (3u | (1u << 16)) : (0u | (2u << 16))) : (2u | (2u << 16));
}

// the stored values of two samples in one dword; thr: surf_thr of the row
template <int FMT> __device__ __forceinline__ uint32_t surf_pair(uint32_t w, uint32_t thr)
{
    if constexpr (FMT == OVHIP_SURF_I010) return w;
    else if constexpr (FMT == OVHIP_SURF_P010) return w << 6;                  // (s <= 1023: nothing crosses into the upper half)
    else {
        const uint32_t q = ((w + thr) >> 2) & 0x01FF01FFu;                     // s + 3 <= 1026: each half <= 256, no carry between them
        return q - ((q >> 8) & 0x00010001u);                                   // min(255, .): 256 is the only value above
    }
}

// four 8-bit values out of two dwords of two 16-bit values each
__device__ __forceinline__ uint32_t narrow4(uint32_t a, uint32_t b)
{
    return (a & 0xFFu) | ((a >> 8) & 0xFF00u) | ((b & 0xFFu) << 16) | ((b & 0xFF0000u) << 8);
}

// the Cb pair b and the Cr pair r of two neighbouring columns as the four elements Cb Cr Cb Cr of an interleaved row
__device__ __forceinline__ void surf_interleave(uint32_t b, uint32_t r, uint32_t *lo, uint32_t *hi)
{
    *lo = (b & 0xFFFFu) | (r << 16);
    *hi = (b >> 16) | (r & 0xFFFF0000u);
}

} // namespace
