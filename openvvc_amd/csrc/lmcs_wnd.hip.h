// The chroma residual scale of a region from the luma around it (rcn_lmcs_compute_chroma_scale, libovvc/rcn_lmcs.c:204-350): the
// window table as a kernel argument and the arithmetic behind the neighbour sum.  k_lmcs_scale (kernels_lmcs.hip) and region_scale
// (kernels_intra.hip) load and reduce the neighbours in their own way and share what follows.
#pragma once
#include "ovvc_common.hip.h"

struct LmcsWnd { uint16_t bnd[17]; int min_idx, max_idx, crs_offset; };

// luts may be null (a picture without chroma scaling: nothing reads the window)
static inline LmcsWnd lmcs_wnd_of(const ovhip_lmcs_luts *luts)
{
    LmcsWnd wnd;
    memset(&wnd, 0, sizeof(wnd));
    if (luts) { memcpy(wnd.bnd, luts->wnd_bnd, sizeof(wnd.bnd)); wnd.min_idx = luts->min_idx; wnd.max_idx = luts->max_idx; wnd.crs_offset = luts->crs_offset; }
    return wnd;
}

// sum: the 64 samples of every side that exists (padded with its last available sample to 16 units)
__device__ __forceinline__ int lmcs_scale_of_sum(const LmcsWnd &wnd, int sum, bool has_abv, bool has_lft)
{
    const int nb_units = (has_abv ? 16 : 0) + (has_lft ? 16 : 0);
    int log2_nb = 0;
    for (int v = nb_units; v; v >>= 1) ++log2_nb;             // 16 -> 5, 32 -> 6, as the reference counts
    const int avg = log2_nb ? (sum + (1 << log2_nb)) >> (log2_nb + 1) : 512;
    int idx = wnd.min_idx;                                    // get_bwd_idx (rcn_lmcs.c:83-93)
    for (; idx < wnd.max_idx; ++idx)
        if (avg < wnd.bnd[idx + 1]) break;
    idx = min(idx, 15);
    const int wnd_sz = (int)wnd.bnd[idx + 1] - (int)wnd.bnd[idx];
    return wnd_sz == 0 ? 1 << 11 : (1 << (OV_BD - 4 + 11)) / (wnd_sz + wnd.crs_offset);
}
