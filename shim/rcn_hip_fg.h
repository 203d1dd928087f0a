/* rcn_hip_fg.h -- the film grain characteristics SEI as the reference parses it (struct OVSEIFGrain, nvcl_structures.h:115-137) <-> the
 * fields the back-end's film grain synthesis reads (ovhip_fg_params, include/ovvc_hip.h), for an application that post-processes on the
 * device where it would call pp_process_frame.  Header only: the override block's library exports nothing for it.
 * tools/fg_golden/gen_fg.c compiles it against the reference's headers and checks both functions against the reference's own derivation. */
#include <string.h>
#ifndef RCN_HIP_FG_H
#define RCN_HIP_FG_H
#include "nvcl_structures.h"
#include "ovvc_hip.h"

static inline void
hip_fg_params_of(const struct OVSEIFGrain *fg, ovhip_fg_params *p)
{
    memset(p, 0, sizeof(*p));
    p->cancel = fg->fg_characteristics_cancel_flag; p->model_id = fg->fg_model_id;
    p->blending_mode = fg->fg_blending_mode_id; p->log2_scale = fg->fg_log2_scale_factor;
    for (int c = 0; c < 3; ++c) {
        ovhip_fg_comp *k = &p->comp[c];
        k->present = fg->fg_comp_model_present_flag[c];
        k->num_intervals = (uint8_t)(fg->fg_num_intensity_intervals_minus1[c] + 1);
        k->num_model_values = (uint8_t)(fg->fg_num_model_values_minus1[c] + 1);
        for (int i = 0; i < 8; ++i) {
            k->lower[i] = fg->fg_intensity_interval_lower_bound[c][i];
            k->upper[i] = fg->fg_intensity_interval_upper_bound[c][i];
            for (int n = 0; n < 3; ++n) k->value[i][n] = fg->fg_comp_model_value[c][i][n];
        }
    }
}

/* what one call's derivation changes in the caller's struct: the model values (fg_compute_model_values, pp_film_grain.c:768-807) */
static inline void
hip_fg_write_back(const ovhip_fg_params *after, struct OVSEIFGrain *fg)
{
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 8; ++i)
            for (int n = 0; n < 3; ++n) fg->fg_comp_model_value[c][i][n] = after->comp[c].value[i][n];
}
#endif
