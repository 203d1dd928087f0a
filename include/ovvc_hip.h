/* ovvc_hip.h -- C ABI of the MI355X (gfx950) reconstruction back-end for OpenVVC.
 *
 * This is the drop-in boundary: a plain-C shared library (libovvc_hip.so) that a host
 * decoder written in C binds exactly where OpenVVC binds its x86/ARM back-ends -- the
 * `struct RCNFunctions` dispatch table (reference: libovvc/rcn_structures.h:499-694, filled
 * by rcn_init_functions(), libovvc/rcn.c:147-300).  The reference drives reconstruction one
 * block per call, interleaved with CABAC parsing; a GPU cannot be driven that way, so the
 * boundary is split in two layers (INTEGRATION.md shows the reference-side stub):
 *
 *   1. RECORDER  (host, no GPU needed): ovhip_rec_*() take the arguments the reference's
 *      orchestrator slots receive (rcn_tu_st / rcn_mcp_b / ...), run the host-side control
 *      logic those slots contain (transform-type selection, QP -> scale/shift, LFNST kernel
 *      choice, MV clipping, identical-motion test, PU splitting) and append fixed-size
 *      commands to per-picture buffers.
 *   2. ENGINE    (device): ovhip_*_launch() run one frame-resident, stage-parallel HIP kernel
 *      per stage over a whole command buffer (inverse quant + LFNST + inverse transform +
 *      residual add; luma/chroma motion compensation; deblocking; SAO; ALF/CC-ALF).
 *
 * Signatures are plain pointers and sizes; no torch / C++ types.  Every engine entry point
 * returns 0 on success or a negative OVHIP_E* code (the reference slots return void -- see
 * SURVEY.md 8b "Error convention"; the shim latches the first error per picture) and fails
 * loudly (OVHIP_ENODEV) when no HIP device is present: there is no CPU fallback.
 *
 * All sample planes are 16-bit (OVSample = uint16_t for 10-bit, libovvc/bitdepth.h:36-40),
 * 4:2:0, strides in SAMPLES.  10-bit only, like the reference's x86 SIMD path (rcn.c:217).
 */
#ifndef OVVC_HIP_H
#define OVVC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OVHIP_ABI_VERSION 9

/* ---- error codes (negative, in the spirit of libovvc/overror.h:40-45) ---- */
#define OVHIP_OK        0
#define OVHIP_ENODEV   (-1)  /* no HIP device / runtime failure                  */
#define OVHIP_ENOMEM   (-2)
#define OVHIP_EINVAL   (-3)  /* malformed command / argument                      */
#define OVHIP_ELAUNCH  (-4)  /* kernel launch or execution error (see last_error) */
#define OVHIP_EUNSUP   (-5)  /* tool outside the supported hot path (e.g. RPR)    */
#define OVHIP_EREF     (-6)  /* a reference picture failed to decode, or the DPB was shut down while waiting for it */

/* ---- transform types: same numbering as enum DCTType, rcn_structures.h:87-93 ---- */
enum { OVHIP_DST_VII = 0, OVHIP_DCT_VIII = 1, OVHIP_DCT_II = 2 };

/* ------------------------------------------------------------------------------------
 * Picture: three device-resident planes.  Mirrors what the rcn path sees of an OVFrame
 * (libovvc/ovframe.h:84-124: data[3], linesize[3], width, height) -- tight planes, no
 * padding (ovframepool.c set_plane_properties); reference windows that leave the picture
 * are resolved by coordinate clamping on the device instead of emulate_block_border()
 * (rcn_inter.c:148-225).
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_pic {
    uint16_t *y, *cb, *cr;   /* DEVICE pointers                           */
    int32_t   w, h;          /* luma size in samples (chroma = w/2 x h/2) */
    int32_t   stride_y;      /* samples                                   */
    int32_t   stride_c;      /* samples                                   */
} ovhip_pic;

/* ------------------------------------------------------------------------------------
 * Transform-block command: one inverse-quantisation + (LFNST) + 2-pass inverse transform
 * + residual-add.  Produced by ovhip_rec_tu(); replaces one pass through
 * rcn_residual()/rcn_residual_c()/rcn_res_c()/rcn_jcbcr() + ict.add/ict.ict
 * (rcn_transform_tree.c:415-506, :553-628, :720-867, :1228-1301; rcn_residuals.c:46-222).
 * 32 bytes.
 * ---------------------------------------------------------------------------------- */
enum {                        /* ovhip_tb_cmd.kind */
    OVHIP_TB_TR      = 0,     /* dequant -> [LFNST] -> vertical pass (>>7) -> horizontal (>>10) */
    OVHIP_TB_DC      = 1,     /* DC-only shortcut, inverse_dct_ii_dc (rcn_transform.c:576-598)  */
    OVHIP_TB_TS      = 2,     /* transform skip: de-scan + dequant_ts, no transform             */
    OVHIP_TB_TS_RAW  = 3      /* transform skip, coefficients already raster + scaled (memcpy)  */
};
enum {                        /* ovhip_tb_cmd.res_mode: how the residual r is applied (rcn_residuals.c) */
    OVHIP_RES_ADD      = 0,   /*  r        */
    OVHIP_RES_SUB      = 1,   /* -r        */
    OVHIP_RES_ADD_HALF = 2,   /*  r >> 1   */
    OVHIP_RES_SUB_HALF = 3,   /* (-r) >> 1 */
    OVHIP_RES_SCALE    = 4,   /* flag: LMCS chroma residual scaling with c_scale (scale_* variants) */
    OVHIP_RES_SCALE_IDX = 8,  /* flag (with OVHIP_RES_SCALE): c_scale is an INDEX into the launch's table of
                               * device-derived scales (ovhip_lmcs_scale_launch), not the scale itself */
    OVHIP_RES_STORE = 16      /* the block belongs to an ordered task (ovhip_itask): r (after the sign / half variant,
                               * before any chroma scaling) is STORED into the residual picture of the launch, saturated
                               * to int16, instead of being added -- the ordered pass adds it to its prediction */
};
#define OVHIP_TB_FLAG_RASTER 0x80  /* in .kind: coefficients stored raster (2xN / Nx2 chroma TBs) */
#define OVHIP_TB_FLAG_BDPCM  0x40  /* in .kind (with TS / TS_RAW): block DPCM, rcn_bdpcm_tb (rcn_transform_tree.c:631-688):
                                    * the LEVELS are accumulated along rows (tr_h = 0) or columns (tr_h = 1) with int16
                                    * saturation, THEN de-quantised (TS) or taken as they are (TS_RAW)               */

typedef struct ovhip_tb_cmd {
    uint16_t x, y;            /* top-left in samples of `plane`                                 */
    uint8_t  plane;           /* 0 Y, 1 Cb, 2 Cr                                                */
    uint8_t  log2_w, log2_h;  /* 1..6                                                           */
    uint8_t  kind;            /* OVHIP_TB_* | OVHIP_TB_FLAG_RASTER                              */
    uint8_t  tr_h, tr_v;      /* OVHIP_DST_VII / DCT_VIII / DCT_II                              */
    uint8_t  lfnst;           /* bit0 on, bits1-2 kernel set (lfnst_mode_map), bit3 idx, bit4 transpose */
    uint8_t  res_mode;        /* OVHIP_RES_*                                                    */
    uint8_t  plane2;          /* 0xff none; else second destination (JCCR), same x,y            */
    uint8_t  res_mode2;
    uint8_t  dq_shift;        /* |shift| of struct IQScale (rcn_dequant.c:92-158)                */
    uint8_t  dq_neg;          /* 1: c * (scale << shift)   0: (c*scale + add) >> shift          */
    int16_t  dq_scale;
    int16_t  c_scale;         /* LMCS chroma residual scale (1<<11 = none)                      */
    uint32_t coef_off;        /* int16 index into the coefficient arena                         */
    uint64_t sig_sb_map;      /* bit sb_y*8+sb_x; arena holds 16 int16 per SET bit, ascending   */
} ovhip_tb_cmd;

/* ------------------------------------------------------------------------------------
 * Prediction-unit command ("MC unit"): <= 16x16 luma samples (+ the co-located 4:2:0 chroma)
 * predicted from one or two reference pictures.  Produced by ovhip_rec_pu(), which performs
 * clip_mv() (rcn_inter.c:96-109), the identical-motion test (:256-268), half-pel AMVR filter
 * selection (:572-577) and BCW weight lookup (:89, :587-596) on the host, then splits the PU.
 * Replaces rcn_mcp / rcn_mcp_b / rcn_mcp_b_l / rcn_mcp_b_c and the leaf kernels behind
 * mc_l/mc_c.{unidir,bidir0,bidir1,bidir_w} (rcn_inter.c:520-602, :1391-1554, :2750-2966;
 * rcn_mc.c:382-1610).  32 bytes.
 * ---------------------------------------------------------------------------------- */
enum {                        /* ovhip_mc_unit.flags */
    OVHIP_MC_HPEL_FILT = 1,   /* prec_amvr == MV_PRECISION_HALF: frac 8 uses the 6-tap smoothing row */
    OVHIP_MC_FILT_4x4  = 2,   /* the reference call was a 4x4 luma block: ov_mc_filters_4        */
    OVHIP_MC_NO_LUMA   = 4,   /* rcn_mcp_b_c: chroma only                                        */
    OVHIP_MC_NO_CHROMA = 8,   /* rcn_mcp_b_l: luma only                                          */
    OVHIP_MC_LMCS      = 16,  /* forward-reshape the luma prediction (lmcs_reshape_forward)      */
    /* "refined" units: only accepted by ovhip_mcx_launch(); dir == 3, plain average, w,h in {8,16}     */
    OVHIP_MC_BDOF      = 32,  /* luma through bi-directional optical flow: rcn_bdof_mcp_l
                               * (rcn_inter.c:1136-1250; rcn_prof_bdof.c:303-490)                  */
    OVHIP_MC_GPM       = 128, /* geometric partitioning (rcn_gpm_b, rcn_inter.c:3118-3143): dir == 3, ref0/mv0 and
                               * ref1/mv1 are the two uni-predictions, blended with the per-sample weight
                               * w = clip3(0, 8, (K + A*x + B*y) >> 3): (p0*w + p1*(8-w) + 64) >> 7,
                               * put_weighted_gpm_bi_pixels (rcn_mc.c:1630-1655); aux = (K & 0xffff) | (A & 0xff) << 16 | (B & 0xff) << 24,
                               * x, y relative to the unit (chroma samples use 2x, 2y)             */
    OVHIP_MC_DMVR      = 64   /* decoder-side MV refinement first: rcn_dmvr_mv_refine
                               * (rcn_inter.c:872-1126).  mv0/mv1 are then NOT clipped (the device
                               * applies clip_mv for the window anchor only, as the reference does);
                               * with OVHIP_MC_BDOF = its apply_bdof argument                      */
};

typedef struct ovhip_mc_unit {
    uint16_t x, y;            /* luma position in the picture                                    */
    uint8_t  w, h;            /* luma size, 4..16 (chroma w/2 x h/2)                             */
    uint8_t  dir;             /* 1: ref0 only, 2: ref1 only, 3: bi                               */
    uint8_t  flags;           /* OVHIP_MC_*                                                      */
    uint8_t  ref0, ref1;      /* indices into the launch's reference-picture table               */
    int8_t   w0, w1;          /* bi weights (4,4 = plain average path; else BCW, w0+w1 == 8)     */
    int32_t  mv0x, mv0y;      /* 1/16 luma pel, ALREADY clipped (chroma uses the same at 1/32)   */
    int32_t  mv1x, mv1y;
    uint32_t aux;             /* OVHIP_MC_GPM: packed weight plane (see the flag).  Otherwise 0, or the fused CIIP
                               * blend: bits 0-2 wt (1..3), bit 8 = chroma keeps the inter prediction            */
} ovhip_mc_unit;

/* ------------------------------------------------------------------------------------
 * Affine unit: <= 16x16 luma samples of an affine CU, every 4x4 luma sub-block with its own
 * motion vectors and (optionally) prediction refinement with optical flow (PROF); the chroma of
 * the same area as 4x4-chroma blocks with the averaged motion vector.  Produced by
 * ovhip_rec_affine_cu().  Replaces the per-sub-block calls of rcn_affine_mcp_b_l /
 * rcn_affine_prof_mcp_b_l / rcn_affine_mcp_b_c (drv_affine_mvp.c:3264-3411) into
 * rcn_mcp_b_l(2,2) / rcn_prof_mcp_b_l / rcn_mcp_b_c(3,3) and the leaf code behind them:
 * rcn_prof_motion_compensation_b_l, rcn_prof_mcp_l (rcn_inter.c:1252-1386, :1631-1722),
 * extend_prof_buff / compute_prof_grad / rcn_prof (rcn_prof_bdof.c:152-290).  32 bytes.
 *
 * Side arena (int32): at side_off, for each luma sub-block in raster order 4 words
 * {mv0x, mv0y, mv1x, mv1y} (clip_mv() already applied for a 4x4 block), then for each
 * 8x8-luma chroma block 4 words (clip_mv() for the 8x8 block).  At prof_off (CU-wide, only
 * read when OVHIP_AFF_PROF is set): struct PROFInfo = 64 int16 {h0[16], v0[16], h1[16], v1[16]}.
 * ---------------------------------------------------------------------------------- */
enum {                        /* ovhip_aff_unit.flags */
    OVHIP_AFF_PROF      = 1,  /* the CU went through rcn_affine_prof_mcp_b_l                      */
    OVHIP_AFF_LMCS      = 16, /* = OVHIP_MC_LMCS                                                  */
    OVHIP_AFF_NO_CHROMA = 8   /* = OVHIP_MC_NO_CHROMA                                             */
};

typedef struct ovhip_aff_unit {
    uint16_t x, y;            /* luma position in the picture                                    */
    uint8_t  w, h;            /* luma size, multiples of 8, <= 16                                 */
    uint8_t  dir;             /* 1, 2, 3                                                         */
    uint8_t  flags;           /* OVHIP_AFF_*                                                     */
    uint8_t  ref0, ref1;
    int8_t   w0, w1;          /* bi weights as in ovhip_mc_unit                                  */
    uint8_t  prof_dir;        /* bi-prediction: lists refined by PROF (bit0 L0, bit1 L1)         */
    uint8_t  ident_c;         /* per chroma block: identical motion -> uni-prediction from L1    */
    uint16_t ident_l;         /* per luma sub-block (no PROF only): same, rcn_inter.c:256-268    */
    uint32_t side_off;        /* int32 index of the unit's motion vectors in the side arena      */
    uint32_t prof_off;        /* int32 index of the CU's PROFInfo in the side arena              */
    uint32_t pad[2];
} ovhip_aff_unit;

/* ------------------------------------------------------------------------------------
 * Reference picture resampling (RPR): prediction from a reference of another size.  The reference
 * keeps one scale factor per (picture, reference) pair and axis, ((ref_w << 14) + cur_w / 2) / cur_w
 * over the scaling windows (ctudec_compute_refs_scaling, ctudec.c:43-86); 1 << 14 on both axes is
 * "unscaled".  A unit that reads at least one scaled list is an ovhip_rpr_unit instead of an
 * ovhip_mc_unit: a tile of at most 16x16 luma samples of one PU (+ its 4:2:0 chroma) that carries,
 * per list, the PU's anchor AFTER clip_rpr_position and the tile's offset inside the PU, because
 * per-column positions (anchor + ((col * step) << 4) + 8192) >> 14 use the ROUNDED step
 * ((scale + 8) >> 4) << 4 and cannot be re-derived from the tile's own position
 * (rcn_mcp_rpr_l / _bi_l / _c / _bi_c, rcn_inter.c:2009-2512; combined as rcn_mc_rpr_b_l / _c, :2522-2736).
 * 64 bytes.
 * ---------------------------------------------------------------------------------- */
#define OVHIP_RPR_UNSCALED (1 << 14)
typedef struct ovhip_ref_scale {
    int32_t scale_hor, scale_ver;   /* scale_fact_rpl*[ref_idx][0 / 1]: 2048 (1/8) .. 32768 (2)                      */
    int32_t ref_w, ref_h;           /* the reference's luma size (frame->width / height)                              */
    uint8_t chroma_hor_col_flag;    /* sps_chroma_horizontal_collocated_flag (scale_info.chroma_hor_col_flag)         */
    uint8_t chroma_ver_col_flag;    /* sps_chroma_vertical_collocated_flag                                            */
    uint8_t pad[2];
} ovhip_ref_scale;

enum {                        /* ovhip_rpr_unit.flags */
    OVHIP_RPR_S0        = 1,  /* list 0 is scaled (else: regular 14-bit interpolation, rcn_mcp_bidir0_l / _c)     */
    OVHIP_RPR_S1        = 2,  /* list 1 is scaled                                                                  */
    OVHIP_RPR_NO_LUMA   = 4,  /* = OVHIP_MC_NO_LUMA                                                                */
    OVHIP_RPR_NO_CHROMA = 8,  /* = OVHIP_MC_NO_CHROMA                                                              */
    OVHIP_RPR_LMCS      = 16, /* = OVHIP_MC_LMCS                                                                   */
    OVHIP_RPR_HPEL_FILT = 32, /* unscaled side: = OVHIP_MC_HPEL_FILT                                               */
    OVHIP_RPR_GPM       = 128 /* = OVHIP_MC_GPM, aux as there                                                      */
};

typedef struct ovhip_rpr_side {
    int32_t pos_x, pos_y;     /* scaled: clipped luma anchor ref_pos (1/2^18 sample); unscaled: clip_mv()'d MV (1/16) */
    int32_t cpos_x, cpos_y;   /* scaled: clipped chroma anchor (1/2^19 chroma sample); unscaled: 0                    */
    uint16_t step_x, step_y;  /* scaled: ((scale + 8) >> 4) << 4; unscaled: 0                                        */
    uint8_t  filt;            /* scaled: luma filter set, horizontal | vertical << 4 (compute_rpr_filter_idx, 0..5)  */
    uint8_t  filt_c;          /* scaled: chroma filter set, horizontal | vertical << 4 (0..2)                        */
    uint8_t  ref;             /* slot in the launch's reference table                                              */
    uint8_t  pad;
} ovhip_rpr_side;

typedef struct ovhip_rpr_unit {
    uint16_t x, y;            /* luma position of the tile in the picture                                          */
    uint8_t  w, h;            /* luma size, 4..16                                                                  */
    uint8_t  ox, oy;          /* the tile's offset inside its PU (luma; chroma ox / 2, oy / 2)                     */
    uint8_t  dir;             /* 1, 2, 3 as in ovhip_mc_unit                                                       */
    uint8_t  flags;           /* OVHIP_RPR_*                                                                       */
    int8_t   w0, w1;          /* bi weights as in ovhip_mc_unit                                                    */
    uint32_t aux;             /* as ovhip_mc_unit.aux (GPM weight plane or CIIP blend)                             */
    ovhip_rpr_side s[2];
} ovhip_rpr_unit;

/* ------------------------------------------------------------------------------------
 * Affine unit that reads a reference of another size: <= 16x16 luma samples of an affine CU of which at
 * least one used list is scaled -- ovhip_aff_unit's shape with the per-list data of ovhip_rpr_side.  Every
 * 4x4 luma sub-block is a 4x4 PU of its own to the reference (rcn_mcp_b_l(2,2) / rcn_prof_mcp_b_l into
 * rcn_mcp_rpr_l / rcn_mc_rpr_b_l / rcn_mc_rpr_prof_b_l, rcn_inter.c:2815-2918, :2524-2649): its own anchor
 * after clip_rpr_position, the 4x4 filter sets 3..5; every 4x4 chroma block of an 8x8 luma area is
 * rcn_mcp_b_c(3,3) into rcn_mcp_rpr_c / rcn_mc_rpr_b_c (:2920-2966) with sets 0..2.  PROF refines the
 * unscaled side of a mixed bi-prediction only (rcn_prof_mcp_bi_l, :1729-1819).  Produced by
 * ovhip_rec_affine_cu() on a recorder with OVHIP_RPR_TOOL_AFFINE; replaces the same calls of
 * drv_affine_mvp.c:3264-3411 as ovhip_aff_unit.  48 bytes.
 *
 * Side arena (int32, the arena of ovhip_rec_aff_side): at side_off, for each luma sub-block in raster order
 * 4 words {a0, b0, a1, b1}: a scaled list's clipped luma anchor (ref_pos x, y; 1/2^18 sample), an unscaled
 * list's clip_mv()'d vector (4x4 block), an unused list's zeros; then for each 8x8-luma chroma block 4 words:
 * the clipped chroma anchor (1/2^19 chroma sample) or the clip_mv()'d averaged vector (8x8 block).  At
 * prof_off (only read with OVHIP_AFFR_PROF): struct PROFInfo as for ovhip_aff_unit.
 * ---------------------------------------------------------------------------------- */
enum {                        /* ovhip_aff_rpr_unit.flags */
    OVHIP_AFFR_S0        = 1, /* list 0 is scaled                                                 */
    OVHIP_AFFR_S1        = 2, /* list 1 is scaled                                                 */
    OVHIP_AFFR_PROF      = 4, /* the CU went through rcn_affine_prof_mcp_b_l                      */
    OVHIP_AFFR_NO_CHROMA = 8, /* = OVHIP_MC_NO_CHROMA                                             */
    OVHIP_AFFR_LMCS      = 16 /* = OVHIP_MC_LMCS                                                  */
};

typedef struct ovhip_aff_rpr_list {
    uint16_t step_x, step_y;  /* scaled: ((scale + 8) >> 4) << 4; unscaled: 0                          */
    uint8_t  filt;            /* scaled: luma filter set, horizontal | vertical << 4 (3..5: flag_4x4)  */
    uint8_t  filt_c;          /* scaled: chroma filter set, horizontal | vertical << 4 (0..2)          */
    uint8_t  ref;             /* slot in the launch's reference table                                  */
    uint8_t  pad;
} ovhip_aff_rpr_list;

typedef struct ovhip_aff_rpr_unit {
    uint16_t x, y;            /* luma position in the picture                                    */
    uint8_t  w, h;            /* luma size, multiples of 8, <= 16; 4x4 (with OVHIP_AFFR_NO_CHROMA): a lone 4x4 luma PU */
    uint8_t  dir;             /* 1, 2, 3                                                         */
    uint8_t  flags;           /* OVHIP_AFFR_*                                                    */
    int8_t   w0, w1;          /* bi weights as in ovhip_mc_unit                                  */
    uint8_t  prof_dir;        /* bi-prediction: lists PROF is applied to (bit0 L0, bit1 L1): unscaled ones only */
    uint8_t  ident_c;         /* per chroma block: identical motion -> uni-prediction from L1    */
    uint16_t ident_l;         /* per luma sub-block (no PROF only): same                          */
    uint16_t pad0;
    uint32_t side_off;        /* int32 index of the unit's anchors / vectors in the side arena   */
    uint32_t prof_off;        /* int32 index of the CU's PROFInfo in the side arena              */
    ovhip_aff_rpr_list s[2];
    uint32_t pad[2];
} ovhip_aff_rpr_unit;

/* ------------------------------------------------------------------------------------
 * CIIP blend unit: dst = (intra * wt + inter * (4 - wt) + 2) >> 2 over one CU, luma and chroma
 * (put_weighted_ciip_pixels rcn_mc.c:1611-1628 driven by rcn_ciip_weighted_sum rcn_inter.c:2968-3009).
 * The inter prediction is what the MC launch left in `dst` (rcn_ciip / rcn_ciip_b record the PU
 * as usual); the intra (planar) prediction comes from the caller's intra path in a second picture.
 * 8 bytes.
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_ciip_unit {
    uint16_t x, y;            /* luma position in the picture                                    */
    uint8_t  log2_w, log2_h;  /* CU size                                                         */
    uint8_t  wt;              /* 1 + (above CU intra) + (left CU intra)                           */
    uint8_t  chroma_inter;    /* log2_w <= 2: chroma keeps the inter prediction (rcn_inter.c:2998)*/
} ovhip_ciip_unit;

/* ------------------------------------------------------------------------------------
 * LMCS (luma mapping with chroma scaling), rcn_lmcs.c.
 *   ovhip_lmcs_build()      = rcn_init_lmcs -> init_lmcs_lut (rcn_lmcs.c:93-179, :352-370): host, per APS
 *   forward reshape          : fused into the MC kernels (OVHIP_MC_LMCS + fwd LUT)
 *   ovhip_lmcs_scale_launch = rcn_lmcs_compute_chroma_scale (rcn_lmcs.c:204-350) for every 64-aligned CU
 *                             (vcl_coding_unit.c:724-730), on the reshaped-domain reconstruction
 *   ovhip_lmcs_inverse_launch = lmcs_reshape_backward over the picture (slicedec.c:746-750, :799-803)
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_lmcs_data {       /* struct OVLMCSData (nvcl_structures.h:671-680) with the signs applied */
    uint8_t  min_bin_idx;              /* lmcs_min_bin_idx                                                  */
    uint8_t  delta_max_bin_idx;        /* lmcs_delta_max_bin_idx                                            */
    int16_t  crs_offset;               /* +-lmcs_delta_abs_crs                                              */
    int16_t  cw_delta[16];             /* +-lmcs_delta_abs_cw[i]                                            */
} ovhip_lmcs_data;

typedef struct ovhip_lmcs_luts {       /* struct LMCSLUTs + the LMCSInfo scalars (rcn_lmcs.c:75-81, rcn_lmcs.h:40-49) */
    uint16_t fwd_lut[1024];
    uint16_t bwd_lut[1024];
    uint16_t wnd_bnd[17];
    uint8_t  min_idx, max_idx;
    int16_t  crs_offset;
    uint16_t pad;
} ovhip_lmcs_luts;

typedef struct ovhip_lmcs_region {     /* one rcn_lmcs_compute_chroma_scale() call, 8 bytes */
    uint16_t x, y;                     /* luma position of the 64-aligned CU in the picture                 */
    uint8_t  n_abv, n_lft;             /* available 4-sample units above / left (bit length of the masks)    */
    uint8_t  ordered;                  /* 1: luma around the region comes from ordered tasks -- ovhip_lmcs_scale_launch skips
                                        * it, an OVHIP_IT_REGION task derives the scale in the ordered pass  */
    uint8_t  pad;
} ovhip_lmcs_region;

int ovhip_lmcs_build(const ovhip_lmcs_data *data, ovhip_lmcs_luts *out);


/* ------------------------------------------------------------------------------------
 * Deblocking.  The reference filters one CTU per df.rcn_dbf_ctu() call from CTU-local bit maps
 * (struct DBFInfo, libovvc/ctudec.h:130-170) that carry neighbour state between calls
 * (dbf_load_info/dbf_store_info, drv_lines.c:618-761).  The recorder (ovhip_rec_dbf_ctu) runs the
 * edge enumeration, bS / QP lookup and filter-length derivation of vvc_dbf_ctu_hor/_ver and
 * vvc_dbf_chroma_hor/_ver (rcn_df.c:1151-1431, :1876-2167) WITHOUT touching samples and writes one
 * 16-bit parameter word per 4-sample edge segment; the device then filters all vertical edges of
 * the picture, then all horizontal edges, which yields the same samples as the reference's per-CTU
 * V-then-H order.  The decode path filters from the compact edge lists of those
 * words (ovhip_dbf_launch_edges*); ovhip_dbf_launch applies the same filter to the picture-level
 * planes laid out below.
 *
 * luma word   : bits 0-1 bS (0 = edge not filtered), 2-4 max filter length P side (1,2,3,5,7),
 *               5-7 max filter length Q side, 8-15 average QP byte of the two blocks
 *               ((qp_p + qp_q + 1) >> 1 on the uint8 map entries, as the reference computes it).
 * chroma word : bit 0 filtered, bit 1 bS==2, bit 2 "large" (strong filter allowed), bit 3 CTU-top
 *               horizontal edge (is_ctb_b: one P-side line), bits 8-15 average chroma QP byte.
 * Planes are indexed by 4x4-luma-sample unit: luma_v[uy*w4 + ux] = vertical edge at x = 4*ux, rows
 * 4*uy..4*uy+3; luma_h[uy*w4 + ux] = horizontal edge at y = 4*uy, columns 4*ux..+3.  Chroma edges
 * live on the 8-luma-sample grid: c*_v[uy*(w4/2) + ux/2], c*_h[(uy/2)*w4 + ux] (2 chroma samples).
 * ---------------------------------------------------------------------------------- */
#define OVHIP_DBF_LUMA(bs, lp, lq, qp)  ((uint16_t)((bs) | ((lp) << 2) | ((lq) << 5) | ((qp) << 8)))
#define OVHIP_DBF_C_ON     1
#define OVHIP_DBF_C_BS2    2
#define OVHIP_DBF_C_LARGE  4
#define OVHIP_DBF_C_CTB_B  8

typedef struct ovhip_dbf_planes {
    const uint16_t *luma_v, *luma_h;      /* [h4][w4]                      */
    const uint16_t *cb_v, *cr_v;          /* [h4][w4c],  w4c = (w4+1)/2    */
    const uint16_t *cb_h, *cr_h;          /* [h4c][w4],  h4c = (h4+1)/2    */
    int32_t w4, h4;
    int16_t beta_offset, tc_offset;       /* DBFInfo.beta_offset / tc_offset (per slice) */
} ovhip_dbf_planes;

/* What df.rcn_dbf_ctu / df.rcn_dbf_truncated_ctu receive (rcn_structures.h:408-413): a copy of the
 * CTU's struct DBFInfo arrays (same element layout: 16+33 / 33 x uint64 masks, 34x33 QP bytes), after
 * ovhip_rec_dbf_mv_prepass() in P / B slices, plus the call arguments and ctudec->ctu_ngh_flags. */
typedef struct ovhip_dbf_ctu {
    uint64_t ctb_bound_ver[49], ctb_bound_hor[49], ctb_bound_ver_c[49], ctb_bound_hor_c[49];
    uint64_t aff_edg_ver[49], aff_edg_hor[49];
    uint64_t bs2_ver[33], bs2_hor[33], bs2c_ver[33], bs2c_hor[33];
    uint64_t bs1_ver[33], bs1_hor[33], bs1cb_ver[33], bs1cb_hor[33], bs1cr_ver[33], bs1cr_hor[33];
    uint64_t affine_ver[33], affine_hor[33];
    uint8_t  qp_y[34 * 33], qp_cb[34 * 33], qp_cr[34 * 33];
    int16_t  beta_offset, tc_offset;
    uint8_t  disable_v, disable_h;
    uint8_t  log2_ctu_s, last_x, last_y;  /* slot arguments                                    */
    uint8_t  ctu_lft, ctu_abv;            /* ctu_ngh_flags & CTU_LFT_FLG / CTU_UP_FLG           */
    uint8_t  pad;
    uint16_t ctu_w, ctu_h;                /* samples; < 1<<log2_ctu_s selects the truncated slot */
    uint16_t ctb_x, ctb_y;                /* CTU address in the picture                         */
} ovhip_dbf_ctu;

/* The MV-based boundary-strength pre-pass rcn_dbf_ctu runs first in P / B slices (dbf_ctu_preproc_v/_h ->
 * dbf_mv_set_vedges/_hedges -> check_dbf_enabled(_p), mv_threshold_check; rcn_df.c:1512-1874): CU and affine
 * sub-block edges that carry no bS yet get bS 1 when the motion on the two sides differs (different reference
 * pictures, or a vector component >= 8 in 1/16 units apart).  Host work on the CTU's 34x34 motion grids. */
typedef struct ovhip_dbf_mv_ctx {
    uint64_t cu_edge_ver[33], cu_edge_hor[33];           /* dbf_info->cu_edge (dbf_utils.h:60-73)                     */
    uint64_t map0_h[33], map0_v[33];                     /* inter_ctx->mv_ctx0.map.hfield / vfield (ctudec.h:298-302)  */
    uint64_t map1_h[33], map1_v[33];                     /* inter_ctx->mv_ctx1.map                                    */
    uint64_t ibc_h[33], ibc_v[33];                       /* dbf_info->ibc_ctx->ctu_map (all 0 without IBC)             */
    int16_t  dist_ref0[16], dist_ref1[16];               /* inter_ctx->dist_ref_0 / _1                                */
    const void *mvs0, *mvs1;                             /* inter_ctx->mv_ctx0.mvs / mv_ctx1.mvs: OVMV[34 * 34]        */
    int32_t  mv_bytes;                                   /* sizeof(OVMV): x, y int32 at offset 0 / 4, ref_idx int8 at 8 */
} ovhip_dbf_mv_ctx;
/* Updates ctu->bs1_ver / bs1_hor in place (what the slot does to dbf_info->bs1_map); call it before
 * ovhip_rec_dbf_ctu for slices other than I. */
int ovhip_rec_dbf_mv_prepass(ovhip_dbf_ctu *ctu, const ovhip_dbf_mv_ctx *mv);

/* ------------------------------------------------------------------------------------
 * Sample adaptive offset.  One entry per CTU in raster order (index ctb_y * nb_ctu_w + ctb_x,
 * nb_ctu_w = ceil(w / ctu)), a compact copy of what the SAO slots read from SAOParamsCtu
 * (libovvc/dec_structures.h:263-274: type_idx, band_position, eo_class, offset_val).
 * ovhip_sao_launch() reads the deblocked picture `src` and writes every sample of `dst` (copy
 * where SAO is off): the frame-resident equivalent of the reference's filter_region copies
 * (rcn_ctu.c:315-510) -- a sample is always filtered with the parameters of the CTU that
 * contains it and picture-border samples whose neighbour is outside stay unmodified
 * (rcn_sao.c:119-188, :190-293).
 * ---------------------------------------------------------------------------------- */
enum { OVHIP_SAO_OFF = 0, OVHIP_SAO_BAND = 1, OVHIP_SAO_EDGE = 2 };   /* = SAO_NOT_APPLIED / SAO_BAND / SAO_EDGE */
/* Sides of a CTU that are borders of its RECT ENTRY (tile) inside the picture: the reference filters a rect entry on its own
 * (slicedec.c:636-657) -- is_border comes from the entry-local CTU index (rcn_sao.c:211-214, :253-257; rcn_alf.c:1313-1318): SAO
 * leaves a sample whose neighbour lies across such a side unmodified, ALF / CC-ALF pad across it as at the picture border
 * (rcn_extend_filter_region, rcn_ctu.c:361-508).  All zero in a picture of one entry.  ONE_ROW: the entry is a single CTU row
 * high (its first 6-row band is then filtered with the BOTTOM flag set, rcn_sao.c:262). */
#define OVHIP_BORDER_LEFT    1
#define OVHIP_BORDER_RIGHT   2
#define OVHIP_BORDER_UPPER   4
#define OVHIP_BORDER_BOTTOM  8
#define OVHIP_BORDER_ONE_ROW 16
typedef struct ovhip_sao_ctu {
    uint8_t type[3];          /* per component Y, Cb, Cr                                  */
    uint8_t band_position[3]; /* first of the 4 consecutive bands (of 32)                  */
    uint8_t eo_class[3];      /* 0 horizontal, 1 vertical, 2 45 deg (135 in spec), 3 other diagonal */
    uint8_t border;           /* OVHIP_BORDER_*                                            */
    uint8_t pad[2];
    int16_t offset_val[3][5]; /* band: [0..3]; edge: indexed by 2 + sign(c-a) + sign(c-b) */
    uint8_t pad2[2];
} ovhip_sao_ctu;

/* ------------------------------------------------------------------------------------
 * Adaptive loop filter + cross-component ALF.  Per CTU: what alf.rcn_alf_filter_line reads from
 * ALFParamsCtu (dec_structures.h:277-283) and alf_info.ctb_cc_alf_filter_idx (ctudec.h:184-215).
 * Per picture: the coefficient / clip sets exactly as rcn_alf_reconstruct_coeff_APS() expands them
 * on the host (struct RCNALF, rcn_alf.h:60-66: 16 fixed + 8 APS luma sets of 4 transposes x 25
 * classes x 13 taps; 8 chroma alternatives x 7) and the CC-ALF coefficients of the two APS
 * (OVALFData.alf_cc_mapped_coeff[2][4][8], nvcl_structures.h:668).  ovhip_alf_launch() reads the
 * post-SAO picture `src` (clamped at the picture border = the replicate-padded filter_region,
 * rcn_ctu.c:361-508) and writes every sample of `dst`.
 * ---------------------------------------------------------------------------------- */
#define OVHIP_ALF_LUMA_SET_SIZE (4 * 25 * 13)
typedef struct ovhip_alf_ctu {
    uint8_t flags;            /* ctb_alf_flag: bit2 luma, bit1 Cb, bit0 Cr                        */
    uint8_t luma_set;         /* ctb_alf_idx: 0..15 fixed sets, 16.. APS sets                     */
    uint8_t cb_alt, cr_alt;   /* chroma alternative filter index                                  */
    uint8_t cc_cb_idx, cc_cr_idx; /* ctb_cc_alf_filter_idx (0 = off, else filter idx + 1)         */
    uint8_t border;           /* OVHIP_BORDER_* (rect-entry borders inside the picture)            */
    uint8_t pad;
} ovhip_alf_ctu;

typedef struct ovhip_alf_pic {
    const ovhip_alf_ctu *ctus;    /* DEVICE [ceil(w/ctu) * ceil(h/ctu)], raster                    */
    const int16_t *luma_coeff;    /* DEVICE [24][OVHIP_ALF_LUMA_SET_SIZE]  RCNALF.filter_coeff_dec  */
    const int16_t *luma_clip;     /* DEVICE [24][OVHIP_ALF_LUMA_SET_SIZE]  RCNALF.filter_clip_dec   */
    const int16_t *chroma_coeff;  /* DEVICE [8][7]  RCNALF.chroma_coeff_final                      */
    const int16_t *chroma_clip;   /* DEVICE [8][7]  RCNALF.chroma_clip_final                       */
    const int16_t *cc_coeff;      /* DEVICE [2][4][8]  Cb APS / Cr APS alf_cc_mapped_coeff[c]      */
    uint8_t *class_scratch;       /* DEVICE scratch, ceil(w/4) * ceil(h/4) bytes (class | transpose << 5) */
    int32_t log2_ctu_s;
} ovhip_alf_pic;

/* ------------------------------------------------------------------------------------
 * Ordered tasks: everything whose INPUT is reconstructed samples of the same picture -- intra prediction
 * (vvc_intra_pred, vvc_intra_pred_chroma, intra_pred_mrl, rcn_intra_mip, cclm.*: rcn_structures.h:507-524, :558-593;
 * rcn_intra.c:484-1180, rcn_intra_cclm.c, rcn_intra_mip.c, rcn_fill_ref.c), CIIP's planar part (rcn_inter.c:3011-3067), and
 * the chroma-scale regions / chroma residuals that depend on such blocks.  The reference runs them in decoding order,
 * interleaved with everything else; the recorder gives each task a LEVEL = 1 + the highest level among the tasks that
 * produce its inputs (0 = inputs come from inter blocks only), and the device runs level after level, all tasks of a level
 * in one launch, after the stage-parallel prediction / residual launches.  One task = one prediction block (one
 * transform block of an intra CU): predict, add the residual the transform stage STOREd for it, clip, write.  32 bytes.
 * ---------------------------------------------------------------------------------- */
enum { OVHIP_IT_LUMA = 0,     /* luma block                                                                          */
       OVHIP_IT_CHROMA = 1,   /* Cb + Cr block (x, y, size in chroma samples)                                        */
       OVHIP_IT_REGION = 2,   /* rcn_lmcs_compute_chroma_scale of region c_scale (needs ordered luma around it)      */
       OVHIP_IT_RES_C = 3,    /* chroma residual add of an already predicted block whose scale is an ordered region's */
       OVHIP_IT_IBC_L = 4,    /* intra block copy, luma block: the block at (x + pad[0], y + pad[1]) of this picture, before */
       OVHIP_IT_IBC_C = 5 };  /* any loop filter (+ residual); Cb + Cr block likewise, offsets in chroma samples.  Produced */
                              /* by ovhip_rec_tu_ibc only (rcn_ibc_l / rcn_ibc_c, rcn_ibc.c:8-139)                        */
enum {                        /* ovhip_itask.flags */
    OVHIP_IF_CORNER = 1,      /* the above-left neighbour unit is available                                          */
    OVHIP_IF_MIP = 2,         /* matrix-based intra prediction, mode = mip mode; OVHIP_IF_MIP_TR: transposed          */
    OVHIP_IF_MIP_TR = 4,
    OVHIP_IF_BDPCM = 8,       /* block-DPCM CU: pure horizontal copy, OVHIP_IF_BDPCM_VER: vertical                    */
    OVHIP_IF_BDPCM_VER = 16,
    OVHIP_IF_RES_Y = 32, OVHIP_IF_RES_CB = 64, OVHIP_IF_RES_CR = 128,   /* a STOREd residual exists for that plane    */
    OVHIP_IF_RES_SCALE = 256, /* chroma residual is LMCS-scaled with c_scale ...                                     */
    OVHIP_IF_SCALE_IDX = 512, /* ... which is the index of a chroma-scale region                                      */
    OVHIP_IF_IBC_FREE = 4096, /* OVHIP_IT_IBC_*: no unit of the source block is written by an ordered task (its level is 1): the
                               * item waits for nothing                                                                   */
    OVHIP_IF_CORNER_L = 2048, /* ISP only: the corner unit as the LEFT arm's progress map sees it (OVHIP_IF_CORNER: as the above
                               * arm's map sees it; for every other task the two coincide)                                */
    OVHIP_IF_ISP = 1024       /* a prediction call of an intra-sub-partition CU (intra_pred_isp, rcn_intra.c:566-640): the
                               * reference arms are the CODING UNIT's (isp_* fields), shifted by the partition's offset; always
                               * the 4-tap cubic filter, no reference smoothing, wide angles by the CU's shape, PDPC only for
                               * blocks at least 4 samples high                                                           */
};
typedef struct ovhip_itask {
    uint16_t x, y;            /* top-left in samples of the task's plane(s), picture coordinates                      */
    uint8_t  log2_w, log2_h;
    uint8_t  kind;            /* OVHIP_IT_*                                                                           */
    uint8_t  mode;            /* 0 planar, 1 DC, 2..66 angular (before the wide-angle remap); chroma also 67 LM, 68 MDLM
                               * left, 69 MDLM top; OVHIP_IF_MIP: the MIP mode                                        */
    uint16_t flags;           /* OVHIP_IF_*                                                                           */
    uint8_t  avl_lft, avl_abv;/* available neighbour units (4 luma / 2 chroma samples) below / right of the corner, as the
                               * reference counts them: position of the highest available unit (rcn_fill_ref.c: 64 -
                               * clz(avl_map) - 1).  LM modes: 67: 0/1 flags; 68: avl_lft = contiguous units, avl_abv flag;
                               * 69: avl_abv = contiguous units, avl_lft flag (rcn_intra_cclm.c:56-68, :770-776, :843-849) */
    uint8_t  mrl_idx;         /* multi-reference-line index 0..2                                                      */
    uint8_t  ciip_wt;         /* != 0: CIIP CU, the (planar) prediction is blended into the inter prediction with this
                               * weight before the residual (ovhip_ciip_weight)                                        */
    int16_t  c_scale;         /* chroma residual scale, or region index (OVHIP_IF_SCALE_IDX, OVHIP_IT_REGION)          */
    uint16_t level;           /* >= 1                                                                                 */
    uint16_t ctu_deps;        /* set by the recorder: 0x8000 | log2_ctu << 8 | neighbour CTUs (bit 0 left, 1 above-left, 2 above,
                               * 3 above-right) holding ordered tasks whose samples this task reads; 0 = unknown            */
    uint8_t  isp_log2_cb_w, isp_log2_cb_h;   /* OVHIP_IF_ISP: the coding unit's size ...                                       */
    uint8_t  isp_off_x, isp_off_y;           /* ... and this block's offset inside it; avl_abv / avl_lft / the corner flag then
                                              * describe the CU's arms (above arm from (x - off_x - 1, y - 1), 2 cb_w + 1 long;
                                              * left arm from (x - 1, y - off_y - 1), 2 cb_h + 1 long)                         */
    uint8_t  isp_log2_pb;     /* OVHIP_IF_ISP: width of one partition inside this block (vertical partitions narrower than 4 are
                               * predicted 4 columns at a time) and ...                                                  */
    uint8_t  isp_res_mask;    /* ... which of them carry a residual (bit = x >> isp_log2_pb); the others add nothing        */
    uint16_t pad[3];          /* OVHIP_IT_IBC_*: pad[0], pad[1] = (int16_t) offset from the block to its source, in samples of the
                               * task's plane (chroma: the luma vector >> 1, arithmetic: the floor the reference takes, CU
                               * positions being even); else 0                                                            */
} ovhip_itask;
#define OVHIP_ITASK_IBC_DX(t) ((int)(int16_t)(t).pad[0])
#define OVHIP_ITASK_IBC_DY(t) ((int)(int16_t)(t).pad[1])

/* ------------------------------------------------------------------------------------
 * Recorder (host side, pure C, usable without a GPU).
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_recorder ovhip_recorder;

/* Per-slice / per-CU state the reference keeps in OVCTUDec and that rcn_tu_st & co. read
 * implicitly.  The shim snapshots it at slot-call time. */
typedef struct ovhip_tu_state {
    uint8_t qp_y, qp_cb, qp_cr, qp_jcbcr;                 /* ctudec->dequant_*.qp               */
    uint8_t qp_y_skip, qp_cb_skip, qp_cr_skip, qp_jcbcr_skip;
    uint8_t dep_quant;        /* residual_coding_l == residual_coding_dpq (rcn_transform_tree.c:399) */
    uint8_t mts_implicit;     /* ctudec->mts_implicit (:435)                                      */
    uint8_t sh_ts_disabled;   /* ctudec->sh_ts_disabled (:673)                                    */
    uint8_t ict_type;         /* rcn_init_functions(ict_type): selects ict.ict[][] set (rcn_residuals.c:231) */
    uint8_t lmcs_scale_c;     /* lmcs_info.scale_c_flag: 1 = lmcs_chroma_scale below is the value;
                               * 2 = use the scale of the last ovhip_rec_lmcs_region() (derived on the device) */
    uint8_t pad[3];
    int16_t lmcs_chroma_scale;/* lmcs_info.lmcs_chroma_scale                                      */
    int8_t  intra_mode;       /* ctudec->intra_mode (luma LFNST kernel choice, :461)              */
    int8_t  lfnst_mode_c;     /* chroma: intra mode after derive_lfnst_mode_c's DM/LM substitution */
} ovhip_tu_state;

/* One transform unit as handed to tmp.rcn_tu_st / rcn_tu_l / rcn_tu_c (rcn_structures.h:475-486)
 * together with its struct TUInfo (rcn_transform_tree.c:56-66). */
typedef struct ovhip_tu_desc {
    uint16_t x0, y0;          /* LUMA sample position in the picture (ctb origin already added)  */
    uint8_t  log2_tb_w, log2_tb_h;  /* luma TU size (tree 2: chroma TU size, x0/y0 chroma units)  */
    uint8_t  tree;            /* 0 single tree (rcn_tu_st), 1 luma (rcn_tu_l), 2 chroma (rcn_tu_c) */
    uint8_t  cbf_mask;        /* 0x10 luma, 0x08 joint CbCr, 0x02 Cb, 0x01 Cr                     */
    uint16_t cu_flags;        /* CUFlags bits (cu_utils.h:44-60)                                  */
    uint8_t  tr_skip_mask;    /* 0x10 luma, 0x02 cb, 0x01 cr                                      */
    uint8_t  cu_mts_flag, cu_mts_idx;
    uint8_t  lfnst_flag, lfnst_idx;
    uint8_t  pad;
    uint16_t last_pos[3];     /* tb_info[0]=Cb/joint, [1]=Cr, [2]=luma   (y<<8 | x)               */
    uint64_t sig_sb_map[3];
    const int16_t *coef[3];   /* host pointers: residual_cb/cr/y + pos_offset, reference layout   */
} ovhip_tu_desc;

/* One coding unit's transform tree as handed to tmp.rcn_transform_tree (rcn_structures.h:464-468;
 * rcn_transform_tree.c:1454-1506): the CU is cut at the maximum transform size (and 128-wide CUs at 64 first) and
 * every leaf goes to rcn_tu_st / rcn_tu_l / rcn_tu_c with its own struct TUInfo out of the caller's array of up to
 * 16.  The reference's walker calls those leaves directly (not through the table), so this is the entry a shim
 * has to override; intra CUs additionally need rcn_intra_tu before every leaf, which is the caller's business. */
typedef struct ovhip_tu_info {   /* struct TUInfo (rcn_transform_tree.c:56-66) without the SBT flag */
    uint8_t  cbf_mask, tr_skip_mask, cu_mts_flag, cu_mts_idx, lfnst_flag, lfnst_idx;
    uint16_t pos_offset;          /* int16 offset of this TU's coefficients in ctudec->residual_y / _cb / _cr */
    uint16_t last_pos[3];         /* tb_info[0] = Cb / joint, [1] = Cr, [2] = luma                             */
    uint16_t pad;
    uint64_t sig_sb_map[3];
} ovhip_tu_info;

typedef struct ovhip_tt_desc {
    uint16_t x0, y0;              /* luma position of the CU in the picture (tree 2: chroma units)             */
    uint8_t  log2_w, log2_h;      /* CU size (tree 2: chroma size)                                             */
    uint8_t  log2_max_tb_s;       /* part_ctx->log2_max_tb_s                                                   */
    uint8_t  tree;                /* ctu_dec->transform_unit: 0 transform_unit_st, 1 _l, 2 _c                  */
    uint16_t cu_flags;
    uint16_t pad;
    const ovhip_tu_info *tu_info; /* the caller's array, indexed as the reference does                          */
    const int16_t *residual[3];   /* ctudec->residual_cb, residual_cr, residual_y (bases, pos_offset not applied) */
} ovhip_tt_desc;

/* One prediction call as handed to rcn_mcp_b (rcn_structures.h:640-646). */
typedef struct ovhip_pu_desc {
    uint16_t x0, y0;          /* luma position in the picture                                    */
    uint8_t  log2_w, log2_h;  /* PU size                                                          */
    uint8_t  inter_dir;       /* 1, 2, 3                                                          */
    uint8_t  ref_idx0, ref_idx1;
    uint8_t  bcw_idx_plus1;   /* OVMV.bcw_idx_plus1 of mv0                                        */
    uint8_t  prec_amvr_half;  /* inter_ctx->prec_amvr == MV_PRECISION_HALF                        */
    uint8_t  planes;          /* 3 both (rcn_mcp_b), 1 luma only (rcn_mcp_b_l), 2 chroma only     */
    uint8_t  lmcs;            /* luma forward reshaping active                                    */
    uint8_t  refine;          /* 0: rcn_mcp_b / _l / _c.  bit0 (OVHIP_PU_BDOF): the caller's bdof_enable,
                               * bit1 (OVHIP_PU_DMVR): its dmvr_enable -- the PU is then the whole CU and is
                               * cut into <=16x16 calls exactly as vcl_coding_unit.c:2450-2472 / :2598-2668 do */
    int32_t  mv0x, mv0y, mv1x, mv1y;
    int32_t  poc0, poc1;      /* rpl0[ref_idx0]->poc, rpl1[ref_idx1]->poc (identical-motion test) */
    uint8_t  ref0, ref1;      /* slots of those pictures in the launch's reference table          */
    uint8_t  gpm_split_dir;   /* OVHIP_PU_GPM: gpm_ctx->split_dir (merge_gpm_partition_idx), 0..63  */
    uint8_t  ciip_wt;         /* 0: not a CIIP CU; 1..3 = ovhip_ciip_weight(): the units of this PU blend the
                               * caller's planar prediction in as they are stored (rcn_ciip / rcn_ciip_b),
                               * no separate ovhip_rec_ciip / ovhip_ciip_launch needed                 */
} ovhip_pu_desc;

/* One affine CU as rcn_affine_mcp_b_l / rcn_affine_prof_mcp_b_l / rcn_affine_mcp_b_c receive it
 * (drv_affine_mvp.c:3264-3411): the sub-block motion field the driver wrote into
 * inter_ctx->mv_ctx0/1 and, when prof_dir != 0, the PROFInfo compute_prof_dmv_scale() derived. */
typedef struct ovhip_affine_desc {
    uint16_t x0, y0;          /* luma position in the picture                                    */
    uint8_t  log2_w, log2_h;  /* CU size, >= 8x8                                                 */
    uint8_t  inter_dir;
    uint8_t  bcw_idx_plus1;
    uint8_t  prof_dir;        /* 0: rcn_affine_mcp_b_l, else rcn_affine_prof_mcp_b_l(prof_dir)    */
    uint8_t  lmcs;
    uint8_t  ref0, ref1;      /* slots in the launch's reference table                           */
    int32_t  poc0, poc1;
    int32_t  mv_stride;       /* in motion vectors (34 in the reference's mv_ctx)                 */
    const int32_t *mv0, *mv1; /* host: (x, y) pairs per 4x4 sub-block, row stride mv_stride      */
    int16_t  dmv_scale[4][16];/* struct PROFInfo: h0, v0, h1, v1                                  */
} ovhip_affine_desc;

#define OVHIP_PU_BDOF 1
#define OVHIP_PU_DMVR 2
#define OVHIP_PU_GPM  4       /* rcn_gpm_b: mv0/ref0 and mv1/ref1 are gpm_ctx->mv0 / mv1 and their pictures */

ovhip_recorder *ovhip_rec_create(int32_t pic_w, int32_t pic_h);
/* The recorder's arrays from a caller-supplied allocator: the engine passes page-locked host memory so that the
 * per-picture flush (ovhip_job_flush) is plain asynchronous DMA out of the arrays the slots wrote. */
typedef struct ovhip_allocator {
    void *(*alloc)(void *user, size_t bytes);
    void  (*free)(void *user, void *p);
    void  *user;
} ovhip_allocator;
ovhip_recorder *ovhip_rec_create_ex(int32_t pic_w, int32_t pic_h, const ovhip_allocator *a);
/* on (default): ovhip_rec_dbf_ctu also maintains the dense edge planes of ovhip_rec_dbf_planes; off: edge lists only */
void  ovhip_rec_set_dense_dbf_planes(ovhip_recorder *rec, int on);
void  ovhip_rec_destroy(ovhip_recorder *rec);
void  ovhip_rec_reset(ovhip_recorder *rec);
/* Append the commands of one TU / PU.  Return number of commands appended or <0. */
int   ovhip_rec_tu(ovhip_recorder *rec, const ovhip_tu_state *st, const ovhip_tu_desc *tu);
/* A TU of a CU that has ordered tasks: intra_l / intra_c (either may be NULL) describe the luma / chroma prediction the
 * reference runs right before the TU's luma / chroma residual (rcn_intra_tu -> rcn_tu_st -> intra_pred_c,
 * rcn_transform_tree.c:1384-1430, :1269-1287; rcn_tu_c :1349-1382): fill x, y, log2_w, log2_h, kind, mode, the OVHIP_IF_CORNER /
 * MIP / BDPCM flags, avl_lft, avl_abv, mrl_idx, ciip_wt.  The recorder computes the level, stores the tasks in decoding
 * order, marks the TU's transform blocks OVHIP_RES_STORE and sets the tasks' OVHIP_IF_RES_* / scale fields.  A chroma
 * block that only needs an ordered chroma scale (inter CU below an ordered region) becomes an OVHIP_IT_RES_C task by itself.
 * Returns the number of transform-block commands appended or <0. */
int   ovhip_rec_tu_intra(ovhip_recorder *rec, const ovhip_tu_state *st, const ovhip_tu_desc *tu, const ovhip_itask *intra_l,
                         const ovhip_itask *intra_c);
/* Intra block copy.  One IBC coding unit as rcn_ibc_l / rcn_ibc_c receive it (the last two slots of struct RCNFunctions,
 * rcn_structures.h; rcn_ibc.c:8-139; callers vcl_coding_unit.c:1032-1066, :1088-1133, :1155-1205, :1257-1311): position and size in luma samples of
 * the picture, the block vector in whole luma samples (IBCMV), the CTU size the reference's ring ctu_buff is laid out for and
 * the left edge of the rect entry / tile the CU lies in.  The reference copies out of a per-CTU-row ring of
 * (256 * 128) >> log2_ctu luma columns (rcn_ctu.c:554-568); the device reads the PICTURE at (x0 + mv_x, y0 + mv_y), which is the
 * same sample exactly when (ovhip_rec_ibc_check)
 *   - the source lies in the CU's CTU row and inside the picture,
 *   - its left edge is not left of win_x0 nor of the ring's oldest CTU ((x0 >> log2_ctu) - (ring CTUs - 1)),
 *   - its right edge is not right of the CU's CTU,
 *   - it does not intersect the CU,
 *   - it is decoded already (the caller's guarantee: the recorder cannot know).
 * H.266 forbids every other vector; for those the reference reads stale ring content and no parity is claimed. */
typedef struct ovhip_ibc_desc {
    uint16_t x0, y0;          /* luma position of the CU in the picture                                                */
    uint8_t  log2_w, log2_h;  /* CU size in luma samples                                                                */
    uint8_t  log2_ctu;        /* 5..7                                                                                  */
    uint8_t  has_chroma;      /* rcn_ibc_c follows rcn_ibc_l (single tree and not `share`); 0: luma only                */
    int16_t  mv_x, mv_y;      /* IBCMV, whole luma samples                                                             */
    uint16_t win_x0;          /* left edge (luma samples) of the rect entry / tile                                     */
    uint16_t pad;
} ovhip_ibc_desc;
/* 0 when the picture holds the sample the reference's ring would deliver for every sample of the CU's source block, else
 * OVHIP_EUNSUP with the violated rule in ovhip_rec_refusal.  Records nothing. */
int   ovhip_rec_ibc_check(ovhip_recorder *rec, const ovhip_ibc_desc *cu);
/* A TU of an IBC CU, shaped like ovhip_rec_tu_intra: what rcn_ibc_l (+ rcn_ibc_c) followed by tmp.rcn_transform_tree do to the
 * TU's blocks.  tu lies inside cu (tree 0: luma + chroma when cu->has_chroma, tree 1: luma only); cu_flags carries flg_ibc_flag and
 * no flg_pred_mode_flag (vcl_transform_unit.c:1826-1959: the inter branch, no LFNST, no SBT).  One OVHIP_IT_IBC_L task per luma
 * block and one OVHIP_IT_IBC_C task per chroma block pair, each with the CU's vector: prediction and residual together, so that
 * every 4x4 unit has ONE ordered writer.  level = 1 + the highest level among the units the source block touches; the TU's
 * transform blocks are marked OVHIP_RES_STORE, the tasks get OVHIP_IF_RES_* / the chroma-scale fields as intra tasks do; a cbf of 0
 * gives a task without residual.  cu is checked first (ovhip_rec_ibc_check): a refusal leaves the recorder as it was.
 * Returns the number of transform-block commands appended or <0. */
int   ovhip_rec_tu_ibc(ovhip_recorder *rec, const ovhip_tu_state *st, const ovhip_tu_desc *tu, const ovhip_ibc_desc *cu);
/* Number of OVHIP_IT_IBC_* tasks recorded since the last reset: pictures without any run the kernels built without the IBC path. */
size_t ovhip_rec_ibc_tasks(const ovhip_recorder *rec);
/* tmp.recon_isp_subtree_v / _h (rcn_structures.h:480-491; rcn_transform_tree.c:1087-1205): an intra-sub-partition CU -- 2 or
 * 4 partitions side by side (vertical) or stacked; prediction and residual alternate partition by partition, so every
 * prediction call becomes an ordered task and every partition's transform block a STORE-mode command.  The partition
 * geometry, the transform types (DST-VII where mts_enabled and the side is 4..16) and the 1xN / 2xN / Nx1 / Nx2 block
 * paths are derived here as the reference derives them.  Vertical partitions narrower than 4 are predicted 4 columns at a
 * time (:1123-1138).  Returns the number of commands appended or <0. */
typedef struct ovhip_isp_desc {
    uint16_t x0, y0;                  /* luma position of the CU in the picture                                          */
    uint8_t  log2_cb_w, log2_cb_h;
    uint8_t  vertical;                /* 1: recon_isp_subtree_v, 0: recon_isp_subtree_h                                    */
    uint8_t  intra_mode;
    uint8_t  cbf_mask;                /* ISPTUInfo.cbf_mask: bit (nb_partitions - 1 - i) = partition i                     */
    uint8_t  lfnst_flag, lfnst_idx;
    uint8_t  mts_enabled;             /* ctudec->mts_enabled (:1110, :1180)                                                */
    /* per PREDICTION call, in call order (vertical: one per 4 columns; horizontal: one per partition): what fill_ref_left_0 /
     * fill_ref_above_0 read out of the progress bit-fields with the CU's geometry (rcn_intra.c:584-594) */
    uint8_t  corner[4];               /* bit 0: the above arm's map, bit 1: the left arm's map                                  */
    uint8_t  avl_abv[4], avl_lft[4];
    uint16_t last_pos[4];             /* ISPTUInfo.tb_info[i]                                                              */
    uint64_t sig_sb_map[4];
    const int16_t *coef;              /* ctudec->residual_y: partition i at i << (log2_tb_w + log2_tb_h)                   */
} ovhip_isp_desc;
int   ovhip_rec_isp_cu(ovhip_recorder *rec, const ovhip_tu_state *st, const ovhip_isp_desc *cu);
/* Number and size of the partitions and of the prediction calls of an ISP CU, as recon_isp_subtree_* derive them. */
void  ovhip_isp_geometry(int32_t log2_cb_w, int32_t log2_cb_h, int32_t vertical, int32_t *log2_pb, int32_t *n_pb, int32_t *log2_pred,
                         int32_t *n_pred);
/* The ordered tasks in decoding order, and sorted by level: level_start[l] .. level_start[l + 1] are the tasks of level
 * l + 1 (n_levels + 1 entries).  Sorting happens in the call. */
const ovhip_itask *ovhip_rec_itasks(const ovhip_recorder *rec, size_t *n);
const ovhip_itask *ovhip_rec_itasks_sorted(ovhip_recorder *rec, size_t *n, const uint32_t **level_start, uint32_t *n_levels);
/* The ordered tasks grouped by the CTU their block lies in (CTUs in raster order, inside a CTU by level, inside a level in
 * decoding order), with one descriptor per CTU that holds any.  deps: bit 0 left, 1 above-left, 2 above, 3 above-right
 * neighbour CTU must have finished its own tasks first: the union of its tasks' ctu_deps when every task carries them for
 * this CTU size, otherwise every such neighbour that holds ordered tasks at all. */
typedef struct ovhip_ictu {
    uint16_t cx, cy;          /* CTU column / row */
    uint32_t first, n;        /* its tasks in the returned array */
    uint32_t deps;
} ovhip_ictu;
/* CTU size (log2, 5..7; 7 when never called) the recorder relates ovhip_itask.ctu_deps to; call before the picture's first TU. */
int   ovhip_rec_set_ctu_size(ovhip_recorder *rec, int32_t log2_ctu_s);
uint32_t ovhip_rec_itask_levels(const ovhip_recorder *rec);      /* highest level recorded so far */
const ovhip_itask *ovhip_rec_itasks_by_ctu(ovhip_recorder *rec, int32_t log2_ctu_s, size_t *n, const ovhip_ictu **ctus, size_t *n_ctus);
/* tmp.rcn_transform_tree: walks the tree and records every leaf with ovhip_rec_tu.  Returns the number of
 * commands appended or <0. */
int   ovhip_rec_transform_tree(ovhip_recorder *rec, const ovhip_tu_state *st, const ovhip_tt_desc *tt);
int   ovhip_rec_pu(ovhip_recorder *rec, const ovhip_pu_desc *pu);
int   ovhip_rec_affine_cu(ovhip_recorder *rec, const ovhip_affine_desc *cu);
/* One inter coding unit in ONE call, whatever its kind (what a recorder-friendly caller hands over per CU, shim/caller.patch):
 * exactly one of pu (rcn_mcp_b; with refine flags the whole BDOF / DMVR coding unit, cut here as vcl_coding_unit.c:2450-2472 / :2598-2668
 * cut it; GPM) and aff (an affine coding unit) is non-NULL.  Returns what ovhip_rec_pu / ovhip_rec_affine_cu return. */
int   ovhip_rec_cu_inter(ovhip_recorder *rec, const ovhip_pu_desc *pu, const ovhip_affine_desc *aff);
/* Reference picture resampling: the scale of reference-table slot `slot` (0..255) for the picture being recorded; NULL
 * restores the default (unscaled, what every slot is after ovhip_rec_create / ovhip_rec_reset).  ovhip_rec_pu and
 * ovhip_rec_cu_inter then emit ovhip_rpr_unit for PUs that read a scaled slot.  Refused with OVHIP_EUNSUP (the
 * reason in ovhip_rec_refusal): DMVR / BDOF with a scaled reference, affine CUs with a scaled reference, 4x4 PUs with a
 * scaled reference (these two unless ovhip_rec_set_rpr_tools opted in), a slot whose scale is 1 but whose size differs from
 * the picture's.  Returns 0 or <0. */
int   ovhip_rec_set_ref_scale(ovhip_recorder *rec, int32_t slot, const ovhip_ref_scale *scale);
/* Opt-in to the prediction tools under reference picture resampling that need arrays a caller of the plain v9 interface does
 * not know (it would leave their CUs unpredicted): a property of the caller, it survives ovhip_rec_reset.  mask = 0 (the
 * default) refuses as described above.
 *   OVHIP_RPR_TOOL_AFFINE  affine CUs with a scaled reference become ovhip_aff_rpr_unit: read with ovhip_rec_aff_rpr_units,
 *                          launched by ovhip_mca_rpr_launch: rcn_affine_mcp_b_l / _prof_mcp_b_l / _mcp_b_c on scaled lists
 *   OVHIP_RPR_TOOL_PU4x4   a 4x4 luma-only PU (planes == 1: rcn_mcp_b_l(2,2), the unpatched caller's affine fallback) with a
 *                          scaled reference becomes an ovhip_rpr_unit with the filter sets 3..5 -- or, where its bi-prediction
 *                          mixes a scaled and an unscaled list, a one-sub-block ovhip_aff_rpr_unit: the reference filters the
 *                          unscaled side of a 4x4 block with the 6-tap set (rcn_mc.c:457), which k_mc_rpr does not hold.
 *                          With chroma it stays refused
 * Returns 0 or <0 (unknown bits). */
#define OVHIP_RPR_TOOL_AFFINE 1u
#define OVHIP_RPR_TOOL_PU4x4  2u
int   ovhip_rec_set_rpr_tools(ovhip_recorder *rec, uint32_t mask);
/* Why the last OVHIP_EUNSUP of this recorder was returned ("" when none since create / reset). */
const char *ovhip_rec_refusal(const ovhip_recorder *rec);
/* rcn_ciip_weighted_sum: mode_abv / mode_lft = part_map.cu_mode_x[x_right >> log2_min_cb] /
 * cu_mode_y[y_bottom >> log2_min_cb] as enum CUMode (cu_utils.h:132-139). */
int   ovhip_rec_ciip(ovhip_recorder *rec, int32_t x0, int32_t y0, int32_t log2_w, int32_t log2_h,
                     int32_t mode_abv, int32_t mode_lft);
/* The CIIP weight 1 + (above CU intra) + (left CU intra) (rcn_inter.c:2977-2981) for ovhip_pu_desc.ciip_wt. */
int   ovhip_ciip_weight(int32_t mode_abv, int32_t mode_lft);
/* rcn_lmcs_compute_chroma_scale(lmcs_info, stride, progress_field, ctu_buff.y, x0, y0): abv_mask / lft_mask are
 * the two 16-bit availability masks it derives from progress_field (rcn_lmcs.c:327-332).  Returns the
 * region index; TUs recorded afterwards with lmcs_scale_c == 2 refer to it. */
int   ovhip_rec_lmcs_region(ovhip_recorder *rec, int32_t x0, int32_t y0, uint32_t abv_mask, uint32_t lft_mask);
/* Compact form of the edge planes: only the 4-sample segments that carry an edge, in raster order, luma
 * first, then Cb, then Cr (8 bytes each).  A lane of the device kernel then always has an edge to filter
 * (in the dense planes ~3/4 of the words are 0).  ux, uy: position in 4-luma-sample units. */
typedef struct ovhip_dbf_edge {
    uint16_t ux, uy;
    uint16_t word;            /* OVHIP_DBF_LUMA(...) or the chroma word, as in the planes          */
    uint8_t  comp;            /* 0 Y, 1 Cb, 2 Cr                                                   */
    uint8_t  pad;             /* offset-pair index, see ovhip_dbf_offsets; ovhip_dbf_compact writes 0 */
} ovhip_dbf_edge;
/* The deblocking offsets are slice-level state (DBFInfo.beta_offset / tc_offset = sh_luma_*_offset_div2 * 2,
 * slicedec.c:1416-1417): ovhip_rec_dbf_ctu gives every distinct pair of a picture an index, which travels in
 * ovhip_dbf_edge.pad.  More than OVHIP_DBF_MAX_OFFSETS distinct pairs in one picture: OVHIP_EUNSUP. */
#define OVHIP_DBF_MAX_OFFSETS 8
typedef struct ovhip_dbf_offsets { int8_t beta[OVHIP_DBF_MAX_OFFSETS], tc[OVHIP_DBF_MAX_OFFSETS]; } ovhip_dbf_offsets;
/* The edge lists ovhip_rec_dbf_ctu emitted so far (CTU by CTU, no sorting needed), dir 0 vertical / 1 horizontal. */
const ovhip_dbf_edge *ovhip_rec_dbf_edges(const ovhip_recorder *rec, int dir, size_t *n, ovhip_dbf_offsets *offsets);
/* dir 0: vertical edges, 1: horizontal.  planes: HOST pointers.  Writes at most cap entries to out (may be
 * NULL to count) and returns the number of edges, or <0. */
int64_t ovhip_dbf_compact(const ovhip_dbf_planes *planes, int dir, ovhip_dbf_edge *out, size_t cap);

/* Convert one CTU's deblocking maps into the picture-level edge planes.  Returns 0 or <0. */
int   ovhip_rec_dbf_ctu(ovhip_recorder *rec, const ovhip_dbf_ctu *ctu);
/* The same for n consecutive CTUs (a CTU row; n = 1 for a caller that keeps ONE struct DBFInfo, as the reference does) with the maps
 * read IN PLACE: ovhip_dbf_view = ovhip_dbf_ctu with every array by pointer -- into the caller's struct DBFInfo (ctudec.h:130-170;
 * same element layout: ctb_bound_* / aff_edg_* 49 words, bs* / affine_* 33 words, qp_* 34 x 33 bytes = struct DBFQPMap.hor) -- instead
 * of a 9 KB descriptor filled and copied per CTU.  ovhip_rec_dbf_mv_prepass_view: the MV-based pre-pass on the caller's
 * own bs1 maps (what the scalar slot does to dbf_info->bs1_map), no write-back copy. */
typedef struct ovhip_dbf_view {
    const uint64_t *ctb_bound_ver, *ctb_bound_hor, *ctb_bound_ver_c, *ctb_bound_hor_c, *aff_edg_ver, *aff_edg_hor;
    const uint64_t *bs2_ver, *bs2_hor, *bs2c_ver, *bs2c_hor, *bs1_ver, *bs1_hor, *bs1cb_ver, *bs1cb_hor, *bs1cr_ver, *bs1cr_hor, *affine_ver, *affine_hor;
    const uint8_t  *qp_y, *qp_cb, *qp_cr;
    int16_t  beta_offset, tc_offset;
    uint8_t  disable_v, disable_h, log2_ctu_s, last_x, last_y, ctu_lft, ctu_abv, pad;
    uint16_t ctu_w, ctu_h, ctb_x, ctb_y;
} ovhip_dbf_view;
int   ovhip_rec_dbf_row(ovhip_recorder *rec, const ovhip_dbf_view *ctus, size_t n);
int   ovhip_rec_dbf_mv_prepass_view(const ovhip_dbf_view *ctu, uint64_t *bs1_ver, uint64_t *bs1_hor, const ovhip_dbf_mv_ctx *mv);
/* Host copies of the edge planes (pointers valid until the next reset/destroy). */
int   ovhip_rec_dbf_planes(const ovhip_recorder *rec, ovhip_dbf_planes *out);
/* Bulk append of already-recorded commands to an EMPTY recorder (replay of a stored command stream). */
enum { OVHIP_REC_TB = 0, OVHIP_REC_COEF, OVHIP_REC_MC, OVHIP_REC_MCX, OVHIP_REC_AFF, OVHIP_REC_SIDE, OVHIP_REC_REGION,
       OVHIP_REC_CIIP, OVHIP_REC_EDGE_V, OVHIP_REC_EDGE_H, OVHIP_REC_ITASK, OVHIP_REC_RPR, OVHIP_REC_AFF_RPR };
int   ovhip_rec_append_raw(ovhip_recorder *rec, int which, const void *data, size_t n);
int   ovhip_rec_set_dbf_offsets(ovhip_recorder *rec, const ovhip_dbf_offsets *offsets, int n);
/* Access to the recorded (host) buffers. */
const ovhip_tb_cmd  *ovhip_rec_tb_cmds(const ovhip_recorder *rec, size_t *n);
/* The same commands reordered into four classes: big luma blocks, small luma blocks, big chroma blocks, small chroma
 * blocks (counts[0..3]); small = at most 256 samples and no side above 32 (16x16, 32x8, 8x32, 32x4, ...).  Luma first because with device-derived
 * chroma scales the chroma commands must run after ovhip_lmcs_scale_launch, which must run after the luma
 * ones; by size because ovhip_itx_launch_classes gives big and small blocks different workgroup shapes. */
const ovhip_tb_cmd  *ovhip_rec_tb_cmds_split(ovhip_recorder *rec, size_t counts[4], size_t *n);
const ovhip_lmcs_region *ovhip_rec_lmcs_regions(const ovhip_recorder *rec, size_t *n);
const int16_t       *ovhip_rec_coefs(const ovhip_recorder *rec, size_t *n_int16);
const ovhip_mc_unit *ovhip_rec_mc_units(const ovhip_recorder *rec, size_t *n);
/* The refined (OVHIP_MC_BDOF / OVHIP_MC_DMVR) units, kept apart so that each list is one launch. */
const ovhip_mc_unit *ovhip_rec_mcx_units(const ovhip_recorder *rec, size_t *n);
const ovhip_aff_unit *ovhip_rec_aff_units(const ovhip_recorder *rec, size_t *n);
const ovhip_rpr_unit *ovhip_rec_rpr_units(const ovhip_recorder *rec, size_t *n);
/* The affine units that read a scaled reference (OVHIP_RPR_TOOL_AFFINE); their side data lies in ovhip_rec_aff_side(). */
const ovhip_aff_rpr_unit *ovhip_rec_aff_rpr_units(const ovhip_recorder *rec, size_t *n);
const ovhip_ciip_unit *ovhip_rec_ciip_units(const ovhip_recorder *rec, size_t *n);
const int32_t        *ovhip_rec_aff_side(const ovhip_recorder *rec, size_t *n_int32);

/* ------------------------------------------------------------------------------------
 * Engine (device side).
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_ctx ovhip_ctx;

int  ovhip_abi_version(void);
/* stream: a hipStream_t the caller owns (e.g. torch's current stream) or NULL to create one. */
int  ovhip_ctx_create(ovhip_ctx **out, int device, void *stream);
void ovhip_ctx_destroy(ovhip_ctx *ctx);
/* 1 if the streams of the two (idle) contexts are served by the same hardware queue, 0 if not (measured: ~2 ms), < 0 error; and a
 * fresh stream for a context whose stream is in the wrong company (see ovvc_engine.hip) */
int  ovhip_ctx_shares_queue(ovhip_ctx *a, ovhip_ctx *b);
int  ovhip_ctx_new_stream(ovhip_ctx *ctx);
int  ovhip_ctx_sync(ovhip_ctx *ctx);
const char *ovhip_last_error(const ovhip_ctx *ctx);
/* Overlap of independent launches inside one stage: route the following launches to side stream k (1..3), or back
 * to the main stream (0); join makes the main stream wait for every side stream used since the last join. */
int  ovhip_ctx_fork(ovhip_ctx *ctx, int k);
int  ovhip_ctx_join(ovhip_ctx *ctx);
void *ovhip_ctx_stream(ovhip_ctx *ctx);

/* device memory helpers (plain hipMalloc/hipMemcpyAsync on the context stream) */
int  ovhip_malloc(ovhip_ctx *ctx, size_t bytes, void **dptr);
int  ovhip_free(ovhip_ctx *ctx, void *dptr);
int  ovhip_h2d(ovhip_ctx *ctx, void *dptr, const void *host, size_t bytes);
int  ovhip_d2h(ovhip_ctx *ctx, void *host, const void *dptr, size_t bytes);
int  ovhip_d2d(ovhip_ctx *ctx, void *dst, const void *src, size_t bytes);     /* synchronous */
/* page-locked host memory (DMA source / target: output frames, recorder arrays); NULL on failure */
void *ovhip_host_alloc(size_t bytes);
void  ovhip_host_free(void *p);
int  ovhip_pic_alloc(ovhip_ctx *ctx, int32_t w, int32_t h, ovhip_pic *pic);   /* three tight planes, zero-filled, complete on return */
int  ovhip_pic_free(ovhip_ctx *ctx, ovhip_pic *pic);
int  ovhip_pic_upload(ovhip_ctx *ctx, const ovhip_pic *pic, const uint16_t *y, const uint16_t *cb,
                      const uint16_t *cr, int32_t host_stride_y, int32_t host_stride_c);
int  ovhip_pic_download(ovhip_ctx *ctx, const ovhip_pic *pic, uint16_t *y, uint16_t *cb,
                        uint16_t *cr, int32_t host_stride_y, int32_t host_stride_c);

/* Stage launches.  cmds / coefs / units are DEVICE pointers; asynchronous on the ctx stream. */
int  ovhip_itx_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_tb_cmd *d_cmds,
                      uint32_t n_cmds, const int16_t *d_coefs, const int16_t *d_lmcs_scales);
/* Same, for a command list sorted by ovhip_rec_tb_cmds_split: the first n_large commands may have any size,
 * the following n_small commands must all be small in the sense of ovhip_rec_tb_cmds_split. */
int  ovhip_itx_launch_classes(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_tb_cmd *d_cmds,
                              uint32_t n_large, uint32_t n_small, const int16_t *d_coefs,
                              const int16_t *d_lmcs_scales);
/* Same for a picture with ordered tasks: the OVHIP_RES_STORE commands write their residual (int16 bits) at the block's position
 * of `res`, a picture of dst's geometry (ovhip_pic_alloc(w, h)); the others add to dst as usual. */
int  ovhip_itx_launch_classes_res(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *res, const ovhip_tb_cmd *d_cmds,
                                  uint32_t n_large, uint32_t n_small, const int16_t *d_coefs, const int16_t *d_lmcs_scales);
/* The CHROMA commands of a picture (same classes) plus, riding in the same launch, the inverse LMCS mapping of the
 * luma plane (= ovhip_lmcs_inverse_launch).  Legal once the luma commands and ovhip_lmcs_scale_launch have run:
 * the commands must not address plane 0. */
int  ovhip_itx_launch_chroma_lmcs(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_tb_cmd *d_cmds,
                                  uint32_t n_large, uint32_t n_small, const int16_t *d_coefs,
                                  const int16_t *d_lmcs_scales, const uint16_t *d_bwd_lut);
/* d_regions, d_scales: DEVICE; d_scales[i] receives lmcs_chroma_scale of region i.  luts: HOST. */
int  ovhip_lmcs_scale_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_lmcs_region *d_regions,
                             uint32_t n_regions, const ovhip_lmcs_luts *luts, int16_t *d_scales);
/* Maps the luma plane through d_bwd_lut (DEVICE, 1024 entries) in place. */
int  ovhip_lmcs_inverse_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const uint16_t *d_bwd_lut);
/* intra: the picture holding the caller's planar prediction for units with a fused CIIP blend, or NULL. */
int  ovhip_mc_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs,
                     const ovhip_mc_unit *d_units, uint32_t n_units, const uint16_t *d_lmcs_fwd_lut,
                     const ovhip_pic *intra);
/* Refined units (OVHIP_MC_BDOF / OVHIP_MC_DMVR).  d_mv_out: DEVICE array of 4 int32 per unit
 * (mv0x, mv0y, mv1x, mv1y finally used), or NULL.  It replaces the `OVMV *mv0, *mv1` in/out
 * arguments of rcn_dmvr_mv_refine (rcn_structures.h:628-632): the caller copies them into its
 * TMVP motion field as vcl_coding_unit.c:2621-2645 does. */
int  ovhip_mcx_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs,
                      const ovhip_mc_unit *d_units, uint32_t n_units, const uint16_t *d_lmcs_fwd_lut,
                      int32_t *d_mv_out);
/* The decoder-side MV refinement of the units that carry OVHIP_MC_DMVR alone: refined vectors to d_mv_out (4 int32 per
 * unit of the list, other units' entries untouched), no sample written.  geom: any picture of the references' size. */
int  ovhip_dmvr_search_launch(ovhip_ctx *ctx, const ovhip_pic *geom, const ovhip_pic *refs, uint32_t n_refs,
                              const ovhip_mc_unit *d_units, uint32_t n_units, int32_t *d_mv_out);
/* Units that read a reference of another size (ovhip_rpr_unit).  Every reference is read with its OWN w / h / strides
 * (coordinates clamped against it: the device form of emulate_block_border); dst and intra have the picture's size. */
int  ovhip_mc_rpr_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs,
                         const ovhip_rpr_unit *d_units, uint32_t n_units, const uint16_t *d_lmcs_fwd_lut,
                         const ovhip_pic *intra);
/* Affine units that read a reference of another size (ovhip_aff_rpr_unit); d_side: the DEVICE copy of ovhip_rec_aff_side().
 * References with their OWN geometry as in ovhip_mc_rpr_launch.  Replaces the per-sub-block calls of rcn_affine_mcp_b_l /
 * rcn_affine_prof_mcp_b_l / rcn_affine_mcp_b_c (drv_affine_mvp.c:3264-3411) where a list is scaled. */
int  ovhip_mca_rpr_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs,
                          const ovhip_aff_rpr_unit *d_units, uint32_t n_units, const int32_t *d_side,
                          const uint16_t *d_lmcs_fwd_lut);
/* CIIP: blends the intra prediction held in `intra` into `dst` (which holds the inter prediction). */
int  ovhip_ciip_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *intra,
                       const ovhip_ciip_unit *d_units, uint32_t n_units);
/* Affine units; d_side: the DEVICE copy of ovhip_rec_aff_side(). */
int  ovhip_mca_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs,
                      const ovhip_aff_unit *d_units, uint32_t n_units, const int32_t *d_side,
                      const uint16_t *d_lmcs_fwd_lut);
/* The refined and the affine units of a picture in ONE launch (they write disjoint blocks and read only the
 * references): equal to ovhip_mcx_launch + ovhip_mca_launch, one kernel boundary and one launch tail cheaper. */
int  ovhip_mcxa_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs,
                       const ovhip_mc_unit *d_xunits, uint32_t n_xunits, int32_t *d_mv_out,
                       const ovhip_aff_unit *d_aunits, uint32_t n_aunits, const int32_t *d_side,
                       const uint16_t *d_lmcs_fwd_lut);
/* One LEVEL of the ordered pass (ovhip_itask): d_tasks = the n tasks of that level (DEVICE), all mutually independent; the
 * launch boundary to the next level makes their stores visible to it.  res: the residual picture the OVHIP_RES_STORE
 * commands wrote; d_regions / luts / d_scales as in ovhip_lmcs_scale_launch (NULL without LMCS chroma scaling): ordered regions
 * write their scale, scaled chroma residuals read it.  geom: the launch geometry (strips of the largest block, one or two
 * colour planes) from ovhip_intra_level_geom() on the HOST copy of the same tasks, or OVHIP_INTRA_GEOM_ANY (always valid,
 * launches up to 8x the workgroups, most of which leave at once). */
#define OVHIP_INTRA_GEOM_ANY 0x12u
#define OVHIP_INTRA_GEOM_IBC 0x20u       /* OR-ed into geom: the tasks may hold OVHIP_IT_IBC_* (ovhip_intra_level_geom sets it) */
uint32_t ovhip_intra_level_geom(const ovhip_itask *tasks, size_t n);
int  ovhip_intra_level_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_pic *res, const ovhip_itask *d_tasks, uint32_t n,
                              const ovhip_lmcs_region *d_regions, const ovhip_lmcs_luts *luts, int16_t *d_scales, int32_t log2_ctu_s,
                              uint32_t geom);
/* The WHOLE ordered pass in one launch: a workgroup per CTU that holds ordered tasks keeps the CTU's samples in LDS and runs
 * its tasks level by level; CTUs wait for their left / above-left / above / above-right neighbours (those that hold tasks)
 * through one flag word each, as the reference's wavefront threads do.  d_tasks / d_ctus: DEVICE copies of what
 * ovhip_rec_itasks_by_ctu() returned.  d_sync: ovhip_intra_sync_words() 32-bit words of device memory, zeroed once by its
 * owner; epoch: != 0 and different from every epoch this d_sync saw before (a picture counter).  The waits are bounded: on
 * expiry d_sync[0] becomes non-zero (1 + index of the CTU that gave up), the launch ends, the picture is incomplete -- the
 * owner must look at d_sync[0] after the launch; abort_mirror (may be NULL) is a second, device-writable address that receives the
 * same code, e.g. a page-locked host word (ovhip_job_wait reads that one and returns OVHIP_ELAUNCH).  Picture width must be a
 * multiple of 8, the planes 8-byte aligned. */
size_t ovhip_intra_sync_words(int32_t width, int32_t height, int32_t log2_ctu_s);
int  ovhip_intra_ctu_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_pic *res, const ovhip_itask *d_tasks, const ovhip_ictu *d_ctus,
                            uint32_t n_ctus, const ovhip_lmcs_region *d_regions, const ovhip_lmcs_luts *luts, int16_t *d_scales,
                            int32_t log2_ctu_s, uint32_t *d_sync, uint32_t epoch, uint32_t *abort_mirror);
/* The ordered pass in one launch, dependencies per 4x4 unit: every (task, strip, plane) item is a workgroup that polls the state
 * words of the units its reference arms cover, reads them with agent-scope loads, predicts, stores write-through and marks its
 * own units.  d_tasks: the LEVEL-SORTED tasks (ovhip_rec_itasks_sorted); d_items: ovhip_intra_flow_items() of that list (host
 * helper; 0 = the picture cannot take this path).  d_state: ovhip_intra_flow_words() words of device memory zeroed once;
 * epoch, abort_mirror and the bounded waits as for ovhip_intra_ctu_launch (d_state[0] = abort word).  The items may be launched
 * in several calls (consecutive ranges that end on level boundaries, same epoch): prepare != 0 only on the first, which marks the
 * units of ALL n_tasks tasks.  n_workers: the launch has that many workgroups and workgroup b takes the items b, b + n_workers, ...
 * in turn -- the bound on the pollers of this launch (wave slots the kernels of the other pictures in flight do not get, and what
 * has to fit the device beside the other flow launches for the forward-progress argument to hold); 0 or >= n_items: one workgroup
 * per item.  prepare | OVHIP_FLOW_IBC: the list holds OVHIP_IT_IBC_* tasks (ovhip_rec_ibc_tasks) -- the launch then takes the
 * kernel built with the block-copy path; without the bit such a task is an error of the caller. */
#define OVHIP_FLOW_IBC 2
size_t ovhip_intra_flow_words(int32_t width, int32_t height);
size_t ovhip_intra_flow_items(const ovhip_itask *sorted, size_t n, uint32_t *items, size_t cap);
int  ovhip_intra_flow_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_pic *res, const ovhip_itask *d_tasks, uint32_t n_tasks,
                             const uint32_t *d_items, uint32_t n_items, const ovhip_lmcs_region *d_regions, const ovhip_lmcs_luts *luts,
                             int16_t *d_scales, int32_t log2_ctu_s, uint32_t *d_state, uint32_t epoch, uint32_t *abort_mirror, int32_t prepare,
                             int32_t n_workers);
/* The flow launch hands samples from task to task with bit 15 set (kernels_intra.hip, FLOW_TAG).  This clears it in the blocks the
 * ordered tasks wrote: after the picture's flow launches, before anything else reads the picture.  with_luma == 0: chroma blocks
 * only -- ovhip_lmcs_inverse_launch drops the bit of every luma sample as a side effect of its table lookup.
 * On ENTRY to the flow launch no sample of `pic` may carry bit 15: true for every picture ovhip_pic_alloc returned (zero-filled)
 * that was only written by this library or by ovhip_pic_upload of real (<= 15-bit) samples since. */
int  ovhip_intra_flow_untag_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_itask *d_tasks, uint32_t n_tasks, int32_t with_luma);
/* ovhip_lmcs_scale_launch + the state words of the picture's flow launch (ovhip_intra_flow_launch's prepare step) in ONE launch:
 * d_tasks[n_tasks] = the level-sorted ordered tasks (DEVICE), d_state / epoch as for ovhip_intra_flow_launch, whose launches of
 * this picture are then called with prepare = 0. */
int  ovhip_lmcs_scale_prepare_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_lmcs_region *d_regions, uint32_t n_regions,
                                     const ovhip_lmcs_luts *luts, int16_t *d_scales, const ovhip_itask *d_tasks, uint32_t n_tasks,
                                     uint32_t *d_state, uint32_t epoch);
/* ovhip_lmcs_inverse_launch + ovhip_intra_flow_untag_launch(with_luma = 0) in ONE launch (a picture with LMCS whose ordered pass
 * ran as flow launches). */
int  ovhip_lmcs_inverse_untag_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const uint16_t *d_bwd_lut, const ovhip_itask *d_tasks, uint32_t n_tasks);
/* planes->* are DEVICE pointers.  Filters `pic` in place: all vertical edges, then all horizontal. */
int  ovhip_dbf_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_dbf_planes *planes);
/* Same filter driven by the compact lists of ovhip_dbf_compact (DEVICE pointers). */
int  ovhip_dbf_launch_edges(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_dbf_edge *d_edges_v, uint32_t n_v,
                            const ovhip_dbf_edge *d_edges_h, uint32_t n_h, int32_t beta_offset, int32_t tc_offset);
/* Same with the per-slice offset table of ovhip_rec_dbf_edges (edge.pad selects the pair). */
int  ovhip_dbf_launch_edges_ex(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_dbf_edge *d_edges_v, uint32_t n_v,
                               const ovhip_dbf_edge *d_edges_h, uint32_t n_h, const ovhip_dbf_offsets *offsets);
/* d_params: DEVICE array of ceil(w/ctu)*ceil(h/ctu) entries.  dst and src must not alias. */
int  ovhip_sao_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *src,
                      const ovhip_sao_ctu *d_params, int32_t log2_ctu_s);
/* Classification + luma / chroma ALF + CC-ALF.  dst and src must not alias. */
int  ovhip_alf_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *src, const ovhip_alf_pic *alf);

/* ------------------------------------------------------------------------------------
 * Picture job: the per-picture "flush" in C.  One job = one picture in flight on one context (= one HIP stream, one
 * decoder frame thread): a recorder whose arrays are page-locked, the device copies of its buffers, and the launch
 * chain of the whole rcn path.  This is what the reference-side shim (shim/rcn_hip.c) calls from the LAST
 * alf.rcn_alf_filter_line of a picture (slicedec.c:940-955), before ovdpb_report_decoded_ctu_line publishes it:
 *
 *   ovhip_job_begin      rcn_attach_frame_buff (rcn_ctu.c:570): new picture, recorder reset
 *   ovhip_job_recorder   the recorder the slots append to while the picture is parsed
 *   ovhip_job_dmvr_rows  eager decoder-side MV refinement of the DMVR units recorded so far: search only, refined
 *                        vectors back on the host when it returns -- called from EVERY alf.rcn_alf_filter_line so that
 *                        the TMVP motion field of a CTU row is final before that row is published (the reference
 *                        stores the vectors right after each rcn_dmvr_mv_refine call, vcl_coding_unit.c:2621-2645)
 *   ovhip_job_flush      async H2D of commands / coefficients / edge lists / parameters, every stage launch, async D2H
 *                        of the refined vectors; returns without waiting
 *   ovhip_job_wait       blocks until the flush has completed on the device
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_job ovhip_job;

enum {                                   /* ovhip_job_params.stages (0 = all) */
    OVHIP_STAGE_MC = 1, OVHIP_STAGE_ITX = 2, OVHIP_STAGE_DBF = 4, OVHIP_STAGE_SAO = 8, OVHIP_STAGE_ALF = 16,
    OVHIP_STAGE_INTRA = 32,
    OVHIP_STAGE_INTRA_CTU = 0x20000000,  /* with OVHIP_STAGE_INTRA: the ordered pass as the one-launch CTU wavefront
                                          * (ovhip_intra_ctu_launch): measured slower than both others, DESIGN.md 4.1 */
    OVHIP_STAGE_INTRA_LEVELS = 0x10000000, /* with OVHIP_STAGE_INTRA: the ordered pass as one launch per level (ovhip_intra_level_launch)
                                            * instead of the default, one launch with per-unit dependency flags
                                            * (ovhip_intra_flow_launch; pictures it cannot take fall back to the levels) */
    OVHIP_STAGE_RESIDENT = 0x40000000    /* measurement only: no H2D / D2H, the device copies of the previous flush are replayed */
};

typedef struct ovhip_job_params {        /* picture-level side information; HOST pointers, copied by ovhip_job_flush */
    const ovhip_lmcs_luts *lmcs;         /* NULL: LMCS off                                                         */
    const ovhip_sao_ctu   *sao;          /* [n_ctu] raster, NULL: SAO off (stage skipped, dst stays deblocked)      */
    const ovhip_alf_ctu   *alf_ctus;     /* [n_ctu] raster, NULL: ALF off                                           */
    const int16_t *alf_luma_coeff, *alf_luma_clip;      /* [24][OVHIP_ALF_LUMA_SET_SIZE]                           */
    const int16_t *alf_chroma_coeff, *alf_chroma_clip;  /* [8][7]                                                  */
    const int16_t *alf_cc_coeff;                         /* [2][4][8]                                               */
    int32_t  log2_ctu_s;
    uint32_t stages;                     /* OVHIP_STAGE_* mask, 0 = all                                              */
    /* HIP events (hipEvent_t handles) the LAUNCH chain waits for on the job's stream, after the uploads have been enqueued:
     * the reference pictures (and the previous readers of dst) finishing on other streams.  The uploads do not depend on
     * them and so overlap the pictures this one waits for.  NULL / 0: none. */
    void *const *wait_events;
    uint32_t n_wait_events;
    /* Called by ovhip_job_flush on the flushing thread after the uploads have been enqueued and before the first launch: the
     * place to wait ON THE HOST for the reference pictures (what the reference's frame threads do, ovdpb_frame_synchro,
     * rcn_inter.c:131) while the uploads already run.  Unlike wait_events this leaves no barrier in the stream: a blocked
     * stream blocks the hardware queue it shares with other streams.  Non-zero return aborts the flush with OVHIP_EINVAL. */
    int (*before_launch)(void *user);
    void *before_launch_user;
    /* != 0: the flush also derives the TMVP plane cells of the refined units (ovhip_tmvp_cells_launch) and brings them back
     * with the refined vectors: ovhip_job_tmvp_cells().  nb_ctb_w of the plane = ceil(picture width / CTU size). */
    uint32_t tmvp_cells;
    /* != 0: wait_events are waited for ON THE HOST (hipEventSynchronize on the flushing thread, after the uploads have been
     * enqueued) instead of being put into the stream: before_launch without a callback into the caller's language. */
    uint32_t wait_on_host;
    /* Workers of a flow launch (ovhip_intra_flow_launch: n_workers); 0: the default -- 6 per compute unit, and never more than twice the
     * picture's widest level (an I picture: ~256).  The flow launches that run at once (one per hardware queue: 4 for a HIP process)
     * should fit the device, 16 per compute unit of that kernel; a launch that had to be abandoned halves the default for the
     * launches that follow.  A process that raises GPU_MAX_HW_QUEUES lowers this in proportion. */
    uint32_t flow_workers;
} ovhip_job_params;

typedef struct ovhip_job_stats {         /* what the last flush moved and launched */
    uint64_t h2d_bytes, d2h_bytes;
    uint32_t n_launches, n_h2d;
    uint32_t n_tb, n_mc, n_mcx, n_aff, n_edges_v, n_edges_h, n_regions, n_itasks, n_ilevels;
    uint32_t n_ordered_retries;          /* 1: ovhip_job_wait decoded the picture a second time, one launch per level (see there) */
    uint32_t flow_shift;                 /* the device's default worker count is 6 x CUs >> this: + 1 per abandoned flow launch (max 4), - 1 per 512 clean ones */
    /* host wall time of the flush call by phase, microseconds: class split + parameter block; enqueueing the copies; the
     * before_launch callback + wait events (the frame thread waiting for its reference pictures); enqueueing the launches */
    uint32_t host_us_prepare, host_us_upload, host_us_wait, host_us_launch;
} ovhip_job_stats;

int  ovhip_job_create(ovhip_ctx *ctx, int32_t pic_w, int32_t pic_h, ovhip_job **out);
void ovhip_job_destroy(ovhip_job *job);
ovhip_recorder *ovhip_job_recorder(ovhip_job *job);
/* Sizes every buffer of the job -- the recorder's page-locked arrays, the device copies, the staging blocks -- for a picture of the
 * job's size up front, so that no picture of a running decoder meets a growth (a growth of a device buffer is a device-wide
 * synchronisation, of a page-locked array an allocation + copy + free of 0.1-1.4 ms).  ovhip_frame_job() calls it for a frame thread's
 * job; ~30 MB page-locked + ~30 MB device memory at 4K. */
int  ovhip_job_reserve_for_picture(ovhip_job *job);
int  ovhip_rec_reserve_for_picture(ovhip_recorder *rec);
/* Waits until the previous flush no longer reads the recorder's arrays, then resets the recorder. */
int  ovhip_job_begin(ovhip_job *job);
/* Issues the job's next flushes on another context (= HIP stream) of the same device: a frame thread that became free takes
 * over a picture.  Waits for the job's previous flush first.  ctx == NULL: back to the context the job was created on -- a job must
 * not stay bound to a context that may be destroyed before it (ovhip_frame_submit returns a borrowed job this way). */
int  ovhip_job_bind(ovhip_job *job, ovhip_ctx *ctx);
/* dst: the picture being decoded; refs[n_refs]: the table ovhip_pu_desc.ref0/ref1 index; intra: picture with the
 * caller's planar prediction for fused CIIP blends, or NULL.  All DEVICE pictures of the job's size. */
int  ovhip_job_flush(ovhip_job *job, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs,
                     const ovhip_pic *intra, const ovhip_job_params *params);
/* Waits for the flush.  If the ordered pass's flow launch gave up (bounded wait of a workgroup for its inputs: the launches of
 * several pictures can starve each other of compute-unit slots), the picture is decoded a second time right here with one
 * launch per level, from the recorder's arrays: ovhip_job_params' tables and the pictures passed to ovhip_job_flush must
 * stay valid until this call returns.  OVHIP_ELAUNCH only if that fails too. */
int  ovhip_job_wait(ovhip_job *job);
/* int32 [n][4] (mv0x, mv0y, mv1x, mv1y per refined unit, recorder order): valid after ovhip_job_wait, or, for the
 * units covered, after ovhip_job_dmvr_rows. */
const int32_t *ovhip_job_refined_mvs(ovhip_job *job, size_t *n_units);
/* Search-only pass over the refined units [first, current count) that carry OVHIP_MC_DMVR; synchronous: when it
 * returns the vectors are in ovhip_job_refined_mvs()[first..].  Returns the new `first` (= unit count) or <0. */
int64_t ovhip_job_dmvr_rows(ovhip_job *job, const ovhip_pic *refs, uint32_t n_refs);
/* The same pass in two halves, so that the search of one CTU row runs while the next row is parsed (slicedec.c:934-956 reports
 * row y - 1 after row y has been parsed: a pass begun at the end of row y - 1 is collected right before that report).
 *   _begin    enqueues: units [first, count) up, search, vectors down -- and, with log2_ctu_s != 0, the entries of the picture's
 *             collocated motion plane they belong to (ovhip_tmvp_cells_launch; 4 per unit, recorder order) -- then an event.
 *             Does not block.  Collects a pass still in flight first.  Returns the unit count it covers, or <0.
 *   _collect  waits for that event (one D2H of vectors + one of plane entries per row, both asynchronous until here); returns the
 *             number of units whose results are valid: ovhip_job_refined_mvs()[.. 4 n], ovhip_job_tmvp_cells()[.. 4 n].  0 passes
 *             pending: returns at once.  ovhip_job_flush collects by itself. */
int64_t ovhip_job_dmvr_rows_begin(ovhip_job *job, const ovhip_pic *refs, uint32_t n_refs, int32_t log2_ctu_s);
int64_t ovhip_job_dmvr_rows_begin_upto(ovhip_job *job, const ovhip_pic *refs, uint32_t n_refs, int32_t log2_ctu_s, size_t upto_units);   /* units [.., upto) only */
int64_t ovhip_job_dmvr_rows_collect(ovhip_job *job);
int  ovhip_job_last_stats(const ovhip_job *job, ovhip_job_stats *out);
/* ---- Band-wise submission: the picture enters the device while it is still being parsed (slicedec.c:815-975 reconstructs a CTU row
 * right after parsing it; dpb.c:1309-1323 reports it; a dependent picture runs a few rows behind, rcn_inter.c:131-146).
 *
 * ovhip_job_band() takes everything recorded since the previous call as one band of CTU rows ending at luma row `row_end` (a CTU-row
 * boundary; the recorder's arrays are in decoding order, so a band is a slice of every array) and enqueues, without waiting:
 *   the band's slices in ONE upload; its prediction, residuals and ordered pass; and the band's own filters: inverse luma mapping and
 *   deblocking of its rows (the horizontal edge on the boundary to the band ABOVE is in this band's lists: after the call the rows
 *   < row_end - 8 are final for the deblocking), then the SAO and ALF rows that made final -- all but the band's last 24 rows.  Intra
 *   prediction of the band BELOW reads this band's bottom row unfiltered (the reference's saved lines, rcn_ctu.c:246-510): the row is
 *   set aside before the filters and put back while the band below is reconstructed.  With `last` != 0 the call completes the picture
 *   (row_end = the picture's height).
 * upto: counts of the recorder's arrays that end the band (NULL: everything recorded so far -- the live decoder; a replay of a
 * recorded picture passes the counts at each CTU-row boundary).  refs: every picture the band's units read must be final in the rows
 * they reach -- the caller's business (ovhip_frame_band: the device DPB's row progress).  params: lmcs / log2_ctu_s / stages as for
 * ovhip_job_flush (the same in every call of a picture); sao / alf_* must be valid for the CTU rows the call's filters cover: rows
 * < row_end - 16 (SAO), < row_end - 24 (ALF), i.e. the CTU rows of the band itself -- parsed with the band (the shim takes them in
 * band_step: the reference's own ALF hook of a row runs a row later, slicedec.c:934-956).  Pictures with stand-alone CIIP units are
 * refused (OVHIP_EUNSUP): the shim never records them.
 * ovhip_job_wait() waits for everything enqueued; a picture whose ordered pass gave up FAILS (no second pass: its bands may have been
 * read).  ovhip_job_begin() starts the next picture as before.
 * ovhip_job_band_progress(): the picture rows [0, rows_final) are final once `event` (a hipEvent_t behind the last filter launch
 * enqueued so far; NULL: nothing yet) has completed and *abort_word (page-locked; the job's, for its lifetime) is still 0. */
typedef struct ovhip_band_counts { uint32_t n_tb, n_coef, n_mc, n_mcx, n_aff, n_side, n_reg, n_itask, n_edge_v, n_edge_h; } ovhip_band_counts;
void ovhip_rec_counts(const ovhip_recorder *rec, ovhip_band_counts *out);
int  ovhip_job_band(ovhip_job *job, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs, const ovhip_job_params *params,
                    const ovhip_band_counts *upto, int32_t row_end, int32_t last);
int  ovhip_job_band_active(const ovhip_job *job);
int  ovhip_job_band_reserve(ovhip_job *job);        /* the band path's staging arena + side buffers now instead of in the first band */
int  ovhip_job_band_busy(ovhip_job *job);          /* 1: the last band's reconstruction is still running (never blocks) */
int  ovhip_job_band_progress(ovhip_job *job, int32_t *rows_final, void **event, const volatile uint32_t **abort_word);
/* row windows of the two frame-wide filters (rows: multiples of 64, or the picture's height) */
int  ovhip_sao_launch_rows(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *src, const ovhip_sao_ctu *d_params, int32_t log2_ctu_s,
                           int32_t row0, int32_t row1);
int  ovhip_alf_launch_rows(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *src, const ovhip_alf_pic *alf, int32_t row0, int32_t row1);

/* Measurement: bracket ONE launch group of every following flush with a HIP-event pair on the launch stream (stage -1:
 * off) and read back the accumulated duration.  A pair costs a few microseconds of stream time, hence one at a time. */
enum { OVHIP_TIME_MC = 0, OVHIP_TIME_MCXA, OVHIP_TIME_ITX_LUMA, OVHIP_TIME_LMCS_SCALE, OVHIP_TIME_ITX_CHROMA, OVHIP_TIME_DBF,
       OVHIP_TIME_SAO, OVHIP_TIME_ALF, OVHIP_TIME_INTRA, OVHIP_TIME_H2D, OVHIP_TIME_COUNT };
int  ovhip_job_time_stage(ovhip_job *job, int stage);
int  ovhip_job_stage_time(ovhip_job *job, double *sum_ms, uint64_t *count);

/* ------------------------------------------------------------------------------------
 * Output path.  Replaces the per-frame copy-out of examples/dectest.c:372-409
 * (write_decoded_frame_to_file): the conformance window is cropped and the three planes are packed, on the device,
 * into the byte layout that function writes -- 16-bit little-endian samples, the cropped Y rows, then Cb, then Cr, no
 * padding -- so that ONE contiguous D2H (or none, when only a digest is wanted) replaces three pitched plane copies.
 * `ovhip_window` = OVFrame.output_window (libovvc/ovframe.h): offsets in CHROMA sample units, as dectest.c:383-388
 * applies them (luma offsets are twice that).
 *
 * Digest: the reference's CI hashes the output FILE (CI/checkMD5.sh, md5sum); MD5 is a serial chain, so a whole frame
 * cannot be hashed by more than one lane, and a frame per lane of the host is ~40 ms at 4K.  Two things are offered instead:
 *   ovhip_pic_digest()           a per-picture FINGERPRINT, computed on the device, 16 bytes leaving it: a three-level hash tree over
 *                                the cropped frame -- leaf = mix128 of each 512-byte piece of a cropped row (the last piece of a row
 *                                shorter), row = mix128 of the row's leaf digests, band = mix128 of the digests of 8 consecutive
 *                                rows of one plane (the last band of a plane shorter), picture = MD5 of the band digests in the
 *                                order Y, Cb, Cr (that last step on the host).  mix128(words, tag): four 32-bit lanes seeded with
 *                                MD5's initial state (lane 0 xor tag), word i into lane i & 3 as h = (h ^ w) * 0x01000193 (FNV-1a),
 *                                murmur3's 32-bit finaliser per lane, then h0 += h1, h2 += h3, h0 += h2, h1 += h0, h2 += h0,
 *                                h3 += h0; words = two samples each, little endian; tag = samples / digests hashed.  (Until
 *                                round 4 every level was MD5: 6.5 M vector instructions per 4K picture.)  Any host can recompute
 *                                it from the written file (oracle/ovvc_oracle_output.py: picture_digest); it is NOT the md5sum of
 *                                the frame and not a cryptographic hash -- a change of any one sample changes it.
 *   ovhip_md5_* over ovhip_pic_output() frames    the plain host MD5 for callers that want the FILE's md5sum from the packed frames
 *                                (ovhip_stream_run with OVHIP_OUT_PACKED + OVHIP_STREAM_FILE_MD5 does exactly that).
 * ovhip_output_row_md5_launch (one plain MD5 per cropped row, one lane each) is the building block the first version of the
 * fingerprint used; it stays for callers that want per-row digests (~200 us per 4K picture: 120 chained blocks per lane).
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_window { uint16_t offset_lft, offset_rgt, offset_abv, offset_blw; } ovhip_window;
/* Bytes of the cropped frame / number of cropped rows (luma + 2 x chroma); 0 if the window leaves nothing. */
size_t ovhip_output_bytes(int32_t w, int32_t h, const ovhip_window *win);
size_t ovhip_output_rows(int32_t w, int32_t h, const ovhip_window *win);
/* d_out: DEVICE, ovhip_output_bytes() bytes.  Asynchronous on the ctx stream. */
int  ovhip_output_pack_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, uint16_t *d_out);
/* d_digests: DEVICE, 16 bytes per cropped row in the order Y rows, Cb rows, Cr rows.  Asynchronous. */
int  ovhip_output_row_md5_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, uint8_t *d_digests);
/* d_digests: DEVICE, 16 bytes per band (ovhip_output_bands()): the band level of the digest tree above.  Asynchronous. */
size_t ovhip_output_bands(int32_t w, int32_t h, const ovhip_window *win);
int  ovhip_output_tree_md5_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, uint8_t *d_digests);
/* Synchronous conveniences: pack + one D2H into host_dst (ovhip_output_bytes() bytes, pinned or pageable); the digest tree
 * + D2H of the band digests + MD5 over them into out[16]. */
int  ovhip_pic_output(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, void *host_dst);
int  ovhip_pic_digest(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, uint8_t out[16]);
/* Host MD5 (RFC 1321). */
typedef struct ovhip_md5_state { uint32_t h[4]; uint64_t n_bytes; uint8_t buf[64]; } ovhip_md5_state;
void ovhip_md5_init(ovhip_md5_state *st);
void ovhip_md5_update(ovhip_md5_state *st, const void *data, size_t n);
void ovhip_md5_final(ovhip_md5_state *st, uint8_t out[16]);

/* ------------------------------------------------------------------------------------
 * Decoded picture hash (SEI payload type 132, H.274 / H.266 Annex D): the one check a VVC stream carries about itself.  The reference
 * knows the payload's number (nvcl_nal_sei.c) and never reads it.  The hash covers the WHOLE decoded picture at its coded size --
 * ovhip_pic.w x h, chroma at half of each; no conformance window, before any post-processing (film grain, output resampling) -- each
 * plane on its own in the order Y, Cb, Cr (only Y with dph_sei_single_component_flag).  A plane's byte string is its samples in
 * raster order, low byte then high byte of the stored 16-bit word (bit depth 10: two bytes per sample).
 *   MD5       RFC 1321 over that byte string; 16 bytes.
 *   CRC       16-bit register, start 0xFFFF, polynomial 0x1021, every bit of the byte string most significant bit of a byte first:
 *             crc = (((crc << 1) | bit) & 0xFFFF) ^ ((old crc >> 15) ? 0x1021 : 0), then 16 more steps with bit 0; 2 bytes, high first.
 *             As polynomials over GF(2), P = x^16 + x^12 + x^5 + 1 and M the n-bit string: crc = (0xFFFF x^(n+16) + M x^16) mod P, so
 *             with R(A) = A x^16 mod P pieces combine as R(A | B) = R(A) x^|B| + R(B) and the start value enters once at the end.
 *   checksum  sum over the samples s at (x, y) of the plane of ((s & 0xFF) ^ m) + ((s >> 8) ^ m) modulo 2^32,
 *             m = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8); 4 bytes, big endian.
 * CRC and checksum are computed where the picture is, 12 bytes leaving the device: one launch over the three planes (k_pic_hash: one
 * workgroup per row, a lane owns runs of 8 samples) and a second small one (k_pic_hash_rows) that combines the rows' sums or
 * remainders -- lanes within a wave, waves within a row, rows within the plane, always in that order and without atomics: the result
 * does not depend on scheduling.  MD5 is one serial chain per plane (~0.2 s per 4K luma plane on one lane, by ovhip_output_row_md5_launch's 12 KB per
 * 200 us): it is not a device method.  ovhip_pic_hash with OVHIP_HASH_MD5 is the CONFORMANCE route: the planes are copied into the
 * context's page-locked scratch and hashed on the calling thread, ~40 ms per 4K picture at the 0.6 GB/s quoted below for
 * OVHIP_STREAM_FILE_MD5.  No 8-bit pictures.
 * ---------------------------------------------------------------------------------- */
enum { OVHIP_HASH_MD5 = 0, OVHIP_HASH_CRC = 1, OVHIP_HASH_CHECKSUM = 2 };         /* = dph_sei_hash_type */
/* value[c]: the bytes of plane c as they stand in the SEI payload (16, 2 or 4 of them); the rest of each row, and the rows of absent
 * planes, are zero. */
typedef struct ovhip_pic_hash_value { uint8_t method, n_planes, rsv[2]; uint8_t value[3][16]; } ovhip_pic_hash_value;
/* Host only, no device: tests, and callers that hold the picture in host memory (an OVFrame).  Strides in samples; n_planes 1 (cb, cr
 * are not read) or 3.  OVHIP_EINVAL for an unknown method, a missing plane, odd or non-positive sizes, a stride below the width. */
int  ovhip_pic_hash_host(int method, int n_planes, const uint16_t *y, const uint16_t *cb, const uint16_t *cr, int32_t w, int32_t h,
                         int32_t stride_y, int32_t stride_c, ovhip_pic_hash_value *out);
/* The payload of SEI message 132: dph_sei_hash_type u(8), dph_sei_single_component_flag u(1), 7 reserved bits, then per plane (1 with
 * the flag, else 3) 16 bytes of MD5, u(16) of CRC or u(32) of checksum.  OVHIP_EINVAL for a payload that is too short or a hash type
 * above 2; bytes behind the last value are ignored.  Host only. */
int  ovhip_pic_hash_parse_sei(const uint8_t *payload, size_t n, ovhip_pic_hash_value *out);
/* 1: same method, same plane count, same significant bytes of every plane's value; else 0.  Host only. */
int  ovhip_pic_hash_equal(const ovhip_pic_hash_value *a, const ovhip_pic_hash_value *b);
/* CRC and checksum only.  Asynchronous on the ctx stream.  d_out: DEVICE, one 32-bit word per plane (the CRC in its low 16 bits),
 * each written whole: nothing accumulates in it, it needs no reset.  One word per row is kept in a grow-only buffer of the context,
 * allocated at the first launch of a height (ovhip_ctx_scratch_bytes counts it).  OVHIP_EINVAL for OVHIP_HASH_MD5 (not a device method), n_planes other than
 * 1 or 3, a missing plane, odd sizes or sizes above 16384, a stride below the width. */
int  ovhip_pic_hash_launch(ovhip_ctx *ctx, const ovhip_pic *pic, int method, int n_planes, uint32_t *d_out);
/* Synchronous.  CRC / checksum: the launch, then a D2H of at most 12 bytes through the context's grow-only scratch (no allocation
 * once a size has been seen).  MD5: see above. */
int  ovhip_pic_hash(ovhip_ctx *ctx, const ovhip_pic *pic, int method, int n_planes, ovhip_pic_hash_value *out);

/* ------------------------------------------------------------------------------------
 * RGB output on the device: a finished 10-bit 4:2:0 picture as an RGB tensor (layout and dtype of the consumer) in DEVICE memory, for
 * compute that sits next to the decoder; nothing is downloaded.  Nothing in the reference does this (dectest writes planes).  The
 * definition is integer only, so every implementation of it (tests/spec_rgb.py, ovhip_rgb_host, k_rgb) is compared for equality.
 *
 *   Input    an ovhip_pic of w x h (multiples of 4) and a window in chroma units, read as the packed output reads it: the output
 *            has W = w - 2 (lft + rgt) columns and H = h - 2 (abv + blw) rows and starts at luma (2 lft, 2 abv).
 *   Chroma   at luma position (x, y) of the PICTURE (before the crop), with a = chroma_loc & 1 and b = 1 for chroma_loc 0, 1,
 *            b = 0 for 2, 3, b = 2 for 4, 5 (H.273 Chroma420SampleLocType: horizontally co-sited / centred; vertically centred,
 *            top, bottom):  U = 2x - a, V = 2y - b; i0 = U >> 2, fx = U & 3, j0 = V >> 2, fy = V & 3 (arithmetic shifts),
 *            i1 = i0 + 1, j1 = j0 + 1, all four clamped to the chroma plane of the whole picture (not of the window);
 *              c16 = (4-fx)(4-fy) c[j0][i0] + fx (4-fy) c[j0][i1] + (4-fx) fy c[j1][i0] + fx fy c[j1][i1]
 *            -- 16 times the bilinear value, not rounded.
 *   Matrix   N = 8 for U8, else 10; peak = 2^N - 1.  Limited range: sy = peak / 876, sc = peak / 896, yoff = 64; full range:
 *            sy = sc = peak / 1023, yoff = 0.  With (Kr, Kb) of `matrix` and Kg = 1 - Kr - Kb the real factors are
 *            cy = sy, rv = 2 sc (1 - Kr), bu = 2 sc (1 - Kb), gu = bu Kb / Kg, gv = rv Kr / Kg; each times 2^14, rounded to nearest on
 *            the exact rational (no case is a tie), is the integer coefficient.  L = 16 cy (Y - yoff), u = c16(Cb) - 8192,
 *            v = c16(Cr) - 8192:
 *              R = clip((L + rv v + 2^17) >> 18), G = clip((L - gu u - gv v + 2^17) >> 18), B = clip((L + bu u + 2^17) >> 18)
 *            clipped to 0..peak; every accumulator fits int32 for 10-bit input.
 *   dtype    U8, U16: that integer.  F32: (float)value * (float)(1.0 / 1023), one multiplication, round to nearest.  F16: that
 *            float converted round-to-nearest-even.
 *   layout   PLANAR: the R plane, the G plane, the B plane, each H x W (CHW); PACKED: H x W x 3 (HWC).  Both tight.
 * matrix = H.273 MatrixCoefficients: 1 (Kr 0.2126, Kb 0.0722), 5 and 6 (0.299, 0.114), 9 (0.2627, 0.0593); 2 (unspecified) is
 * OVHIP_EINVAL -- the caller must decide --, every other value OVHIP_EUNSUP.  Not done: constant-luminance and ICtCp matrices,
 * normalisation; transfer functions and tone mapping are the caller's, as a table: "RGB output through a colour table" below; a
 * smaller tensor comes from "Reduced-size output on the device" below.
 * ---------------------------------------------------------------------------------- */
enum { OVHIP_RGB_U8 = 0, OVHIP_RGB_U16 = 1, OVHIP_RGB_F16 = 2, OVHIP_RGB_F32 = 3 };      /* ovhip_rgb_format.dtype */
enum { OVHIP_RGB_PLANAR = 0, OVHIP_RGB_PACKED = 1 };                                       /* ovhip_rgb_format.layout */
typedef struct ovhip_rgb_format { uint8_t matrix, full_range, chroma_loc, dtype, layout, rsv[3]; } ovhip_rgb_format;
/* Bytes of the RGB picture of a w x h picture under win (NULL: no crop); 0 for sizes that are not positive multiples of 4, a window
 * that leaves nothing or a bad dtype / layout.  Host only. */
size_t ovhip_rgb_bytes(int32_t w, int32_t h, const ovhip_window *win, const ovhip_rgb_format *fmt);
/* The integer coefficients (cy, rv, gu, gv, bu) and yoff of a format.  OVHIP_EINVAL / OVHIP_EUNSUP as above.  Host only. */
int  ovhip_rgb_coefs(const ovhip_rgb_format *fmt, int32_t coef[5], int32_t *yoff);
/* The definition on host planes into host memory (strides in samples): tests, and callers that hold the picture on the host.
 * Refusals as the launch's; nothing is written when it refuses. */
int  ovhip_rgb_host(const uint16_t *y, const uint16_t *cb, const uint16_t *cr, int32_t w, int32_t h, int32_t stride_y, int32_t stride_c,
                    const ovhip_window *win, const ovhip_rgb_format *fmt, void *dst, size_t dst_bytes);
/* d_dst: DEVICE, at least ovhip_rgb_bytes bytes, aligned to its element (a slice of a batch tensor is no more than that; k_rgb stores
 * 16 bytes at a time where a run of 8 pixels lies so, narrower where it does not).  Asynchronous on the ctx stream; allocates nothing.
 * Refused before anything is launched, the reason in the context's error text: a null destination, dst_bytes too small, a destination
 * that is not element-aligned or overlaps the picture, a window that leaves nothing, a missing plane, a stride below the width,
 * sizes that are not multiples of 4, bad enum values (OVHIP_EINVAL; a matrix that is not built: OVHIP_EUNSUP). */
int  ovhip_rgb_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, void *d_dst, size_t dst_bytes);
/* Synchronous convenience beside ovhip_pic_output: the launch into the context's grow-only scratch, then one D2H into host_dst
 * (dst_bytes >= ovhip_rgb_bytes, pinned or pageable). */
int  ovhip_pic_output_rgb(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, void *host_dst, size_t dst_bytes);

/* ------------------------------------------------------------------------------------
 * RGB output through a colour table: the RGB output above with one table-driven step between its clip and its store -- a 3D colour
 * lookup table with tetrahedral interpolation, what a .cube file or a baked colour transform is.  The caller owns the colour science
 * (transfer function, tone mapping, gamut: all in the table's entries), the library one exact step: integer only, so every
 * implementation of it (tests/spec_rgb_lut.py, ovhip_rgb_lut_host, k_rgb_lut) is compared for equality.
 *
 *   Input    everything up to and including the clip as "RGB output on the device", with one difference: the coefficients and the
 *            clip are those of N = 10 (peak 1023) WHATEVER the dtype -- a U8 destination does not select the 8-bit coefficients.  The
 *            step works on (R, G, B) in 0..1023.
 *   Table    uint16_t table[S][S][S][3], S one of 17, 33, 65, n = S - 1; index order [b][g][r][c]: r is fastest, c = 0, 1, 2 the
 *            OUTPUT's R, G, B.  A peak P in 1..65535; every entry <= P.
 *   Cell     per input channel value v: t = v n, i = t / 1023, f = t - 1023 i; if i == n (only at v = 1023) then i = n - 1 and
 *            f = 1023.  So f is in 0..1023 and the cell is (i_r, i_g, i_b).
 *   Tetra    order the three channels by f descending, f1 >= f2 >= f3.  V0 = the cell's vertex (i_r, i_g, i_b); V1 = V0 with the
 *            index of f1's channel raised by 1; V2 = V1 with f2's channel raised by 1; V3 = V2 with f3's channel raised by 1: the
 *            opposite corner.  w0 = 1023 - f1, w1 = f1 - f2, w2 = f2 - f3, w3 = f3 (their sum is 1023); per output channel c
 *              o_c = (w0 T[V0][c] + w1 T[V1][c] + w2 T[V2][c] + w3 T[V3][c] + 511) / 1023
 *            -- an integer division of a non-negative value of at most 1023 * 65535 + 511 < 2^26: int32 holds it.  When two f are
 *            equal the order between them does not change o, because the vertex in question has the weight 0: an implementation may
 *            break ties any way it likes.
 *   dtype    U8 (requires P <= 255), U16: o.  F32: (float)o * (float)(1.0 / P), one multiplication, round to nearest.  F16: that
 *            float converted round-to-nearest-even, subnormal halves included (they occur when P > 16384).
 *   layout   PLANAR, PACKED as above; the size is that of the RGB output above.
 * With the lattice table T[b][g][r] = (1023 r, 1023 g, 1023 b) and P = 65535 the output is exactly n (R, G, B).
 * Not done: 1D shaper tables in front of the cube, other sizes, trilinear interpolation, float tables, a table per picture from dynamic
 * metadata.  A table on the surface output: "Surface output through a colour table" below.
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_rgb_lut ovhip_rgb_lut;          /* opaque: the table in device memory of ctx's device, S, P */
/* OVHIP_OK for a size of 17, 33 or 65 and a peak in 1..65535 that fmt's dtype can store (U8: peak <= 255; fmt NULL: any dtype), else
 * OVHIP_EINVAL.  Host only. */
int  ovhip_rgb_lut_check(int size, int peak, const ovhip_rgb_format *fmt);
/* The table on ctx's device: size and peak validated as above, every entry checked against the peak on the host (OVHIP_EINVAL, the
 * first offending index in the context's error text), repacked to 8-byte texels (R, G, B, 0), uploaded once and waited for.  The table
 * is immutable afterwards; host_table is not kept.  Any context of the same device may use it, from any thread. */
int  ovhip_rgb_lut_create(ovhip_ctx *ctx, int size, int peak, const uint16_t *host_table, ovhip_rgb_lut **out);
/* After the last launch that reads it is complete.  NULL: nothing. */
void ovhip_rgb_lut_destroy(ovhip_rgb_lut *lut);
/* The definition on host planes and a host table into host memory: tests, and callers that hold the picture on the host.  Refusals as
 * the launch's, and a table entry above the peak (OVHIP_EINVAL); nothing is written when it refuses. */
int  ovhip_rgb_lut_host(const uint16_t *y, const uint16_t *cb, const uint16_t *cr, int32_t w, int32_t h, int32_t stride_y, int32_t stride_c,
                        const ovhip_window *win, const ovhip_rgb_format *fmt, int size, int peak, const uint16_t *host_table, void *dst, size_t dst_bytes);
/* As the RGB launch above: d_dst in DEVICE memory, at least ovhip_rgb_bytes bytes, aligned to its element; asynchronous on the ctx
 * stream; allocates nothing.  Refused before anything is launched, the reason in the context's error text: everything the RGB launch
 * refuses, a null table, a table of another device, U8 with a table peak above 255 (OVHIP_EINVAL). */
int  ovhip_rgb_lut_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, const ovhip_rgb_lut *lut,
                          void *d_dst, size_t dst_bytes);
/* Synchronous convenience: the launch into the context's grow-only scratch, then one D2H into host_dst. */
int  ovhip_pic_output_rgb_lut(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, const ovhip_rgb_lut *lut,
                              void *host_dst, size_t dst_bytes);

/* ------------------------------------------------------------------------------------
 * Surface output on the device: a finished 10-bit 4:2:0 picture as a 4:2:0 SURFACE in DEVICE memory -- the picture's own samples in the
 * pixel format and with the row pitch a hardware encoder, a display pipeline or a video library dictates; nothing is downloaded.
 * Nothing in the reference does this (dectest writes 16-bit planes).  The definition is integer only, so every implementation of it
 * (tests/spec_surface.py, ovhip_surface_host, k_surface) is compared for equality.
 *
 *   Input    an ovhip_pic of w x h (positive, even, at most 16384) and a window in chroma units, read exactly as the packed output
 *            reads it: W = w - 2 (lft + rgt), H = h - 2 (abv + blw), the first luma sample is (2 lft, 2 abv), chroma is
 *            W/2 x H/2 from (lft, abv); a NULL window means no crop.
 *   Formats  NV12 (1-byte elements) and P010 (2 bytes, little endian): the Y plane, H rows of W elements, then ONE chroma plane of
 *            H/2 rows of W elements, Cb and Cr interleaved, Cb first.  I420 (1 byte) and I010 (2 bytes, little endian): the Y plane,
 *            the Cb plane, the Cr plane, the chroma planes H/2 rows of W/2 elements.
 *   Values   s is the stored 10-bit sample.  I010: s.  P010: s << 6 (the low six bits zero).  NV12 and I420:
 *              rounding OVHIP_SURF_ROUND    min(255, (s + 2) >> 2)
 *              rounding OVHIP_SURF_DITHER   min(255, (s + D[y & 1][x & 1]) >> 2),  D = {{0, 2}, {3, 1}}
 *            where (x, y) is the sample's column and row in its own OUTPUT plane, after the crop (the window's first sample is
 *            (0, 0)), and the Cb and the Cr of an interleaved pair share the pair's column.  Property: on a flat area of value
 *            s <= 1020 the four outputs of any 2 x 2 cell aligned to even output coordinates sum to exactly s (the thresholds are
 *            0, 1, 2, 3: the cell keeps the two bits the shift drops).  The 16-bit formats take rounding 0 only.
 *   Layout   linear.  pitch_y, pitch_c: bytes from one row to the next, 0 = tight (the row's own bytes); one pitch_c for both chroma
 *            planes of a planar format.  offset_c[k]: byte offset of chroma plane k from the base, 0 = right behind the plane
 *            before, that is pitch * rows of that plane behind its start -- so a tight surface is contiguous.  Semi-planar formats
 *            use offset_c[0] only.  The size of the surface is the largest end of a plane's LAST ROW'S OWN BYTES (with planes in
 *            their order: of the last plane's), not pitch * rows.  Bytes between a row's end and the next row's start and bytes
 *            between planes are NEVER written.  Tiled or swizzled surfaces are not built.
 * OVHIP_SURF_I010, tight, with offsets 0, is byte for byte the frame ovhip_output_pack_launch / ovhip_pic_output write.
 * Refused (OVHIP_EINVAL) before anything is launched or written, the reason in the context's error text: a null picture, plane or
 * destination; odd or non-positive sizes, or sizes above 16384; a picture stride below its width; a window that leaves nothing; an
 * unknown format or rounding; a rounding other than 0 on a 16-bit format; non-zero rsv; a non-zero offset_c[1] on a semi-planar
 * format; a pitch below the row's bytes; a pitch or offset that is not a multiple of the element size; a destination that is not
 * element-aligned; planes that overlap one another; dst_bytes below the surface's size ("too small", with both numbers); a
 * destination that overlaps the picture.  Not done: 4:2:2 and 4:4:4, NV21 / YV12 / P016, error diffusion.  A colour conversion on the
 * way: "Surface output through a colour table" below.
 * ---------------------------------------------------------------------------------- */
enum { OVHIP_SURF_NV12 = 0, OVHIP_SURF_P010 = 1, OVHIP_SURF_I420 = 2, OVHIP_SURF_I010 = 3 };      /* ovhip_surface_format.format */
enum { OVHIP_SURF_ROUND = 0, OVHIP_SURF_DITHER = 1 };                                             /* ovhip_surface_format.rounding */
typedef struct ovhip_surface_format {
    uint8_t  format, rounding, rsv[2];   /* rsv must be 0 */
    uint32_t pitch_y, pitch_c;           /* bytes from one row to the next; 0 = tight (the row's own bytes) */
    uint64_t offset_c[2];                /* byte offset of the chroma plane(s) from the base; 0 = right behind the plane before */
} ovhip_surface_format;                  /* 32 bytes */
/* Bytes of the surface of a w x h picture under win (NULL: no crop): the end of the last plane's last row's own bytes; 0 for anything
 * the launch would refuse on these arguments.  Host only. */
size_t ovhip_surface_bytes(int32_t w, int32_t h, const ovhip_window *win, const ovhip_surface_format *fmt);
/* The definition on host planes into host memory (strides in samples): tests, and callers that hold the picture on the host.
 * Refusals as the launch's; nothing is written when it refuses. */
int  ovhip_surface_host(const uint16_t *y, const uint16_t *cb, const uint16_t *cr, int32_t w, int32_t h, int32_t stride_y, int32_t stride_c,
                        const ovhip_window *win, const ovhip_surface_format *fmt, void *dst, size_t dst_bytes);
/* d_dst: DEVICE, at least ovhip_surface_bytes() bytes, aligned to its element (k_surface: one launch for all planes, a lane owns 16
 * elements of a row; 16-byte loads and stores where a run's address allows, narrower where it does not -- a row tail, an odd pitch, a
 * window offset).  Asynchronous on the ctx stream; allocates nothing. */
int  ovhip_surface_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_format *fmt, void *d_dst, size_t dst_bytes);
/* Synchronous convenience beside ovhip_pic_output: the launch into the context's grow-only scratch, then one D2H into host_dst
 * (dst_bytes >= ovhip_surface_bytes(), pinned or pageable; a layout with gaps: one strided D2H per plane, so the gaps stay unwritten
 * in host memory too). */
int  ovhip_pic_output_surface(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_format *fmt, void *host_dst, size_t dst_bytes);

/* ------------------------------------------------------------------------------------
 * Surface output through a colour table: a finished 10-bit 4:2:0 picture leaves as an NV12 / P010 / I420 / I010 surface whose samples
 * are those of the CONVERTED picture -- the decoded picture taken to R'G'B', through the caller's 3D colour table (the ovhip_rgb_lut of
 * "RGB output through a colour table": the same object, the same sizes, any peak), back to Y'CbCr with a destination matrix and range,
 * and sub-sampled to 4:2:0 at a destination chroma location.  A BT.2020 PQ or HLG picture as the BT.709 SDR NV12 an encoder or a
 * display next to the decoder takes: one launch, no intermediate picture.  Integer only, so every implementation of it
 * (tests/spec_surface_lut.py, ovhip_surface_lut_host, k_surface_lut) is compared for equality.  By definition
 *                output = surface(converted picture, window NULL, fmt)
 * with surface of "Surface output on the device", byte for byte; the converted picture has the window's size W x H:
 *
 *   Conv     ovhip_surface_conv: src_matrix, src_full_range, src_chroma_loc as the three fields of ovhip_rgb_format: same values,
 *            same refusals; dst_matrix 1, 5, 6 or 9 (2: OVHIP_EINVAL, others OVHIP_EUNSUP); dst_full_range 0 or 1; dst_chroma_loc
 *            0..3 (4 and 5: OVHIP_EUNSUP, nobody produces them); rsv 0.
 *   RGB      for every luma position of the window (R, G, B) in 0..1023 is `Input` of "RGB output through a colour table": N = 10
 *            whatever the destination, chroma taps clamped to the whole picture.  (o_r, o_g, o_b) in 0..P is its `Cell` and `Tetra`.
 *   Norm     q_c = (16368 o_c + P / 2) / P, integer divisions: 0..16368 (P = 1023: 16 o_c).
 *   Matrix   (Kr, Kb) of dst_matrix, Kg = 1 - Kr - Kb.  Limited range: sy = 876 / 1023, sc = 896 / 1023, yoff = 64; full range:
 *            sy = sc = 1, yoff = 0.  rnd = times 2^14, rounded to nearest on the exact rational (no case is a tie):
 *              T = rnd(sy), y_r = rnd(sy Kr), y_b = rnd(sy Kb), y_g = T - y_r - y_b
 *              b_r = rnd(-sc Kr / (2 (1 - Kb))), b_g = rnd(-sc Kg / (2 (1 - Kb))), b_b = -b_r - b_g
 *              r_g = rnd(-sc Kg / (2 (1 - Kr))), r_b = rnd(-sc Kb / (2 (1 - Kr))), r_r = -r_g - r_b
 *            and with arithmetic shifts, everything in int32:
 *              Y14 = 16 yoff + ((y_r q_r + y_g q_g + y_b q_b + 2^13) >> 14)
 *              Cb14 = 8192 + ((b_r q_r + b_g q_g + b_b q_b + 2^13) >> 14),  Cr14 likewise with r_r, r_g, r_b
 *            Both chroma rows sum to zero: every grey (q_r = q_g = q_b) gives exactly 8192.  BT.709 limited is (2983, 10034, 1013),
 *            (-1644, -5531, 7175), (7175, -6517, -658).
 *   Luma     of the converted picture: clip((Y14 + 8) >> 4, 0, 1023).  (The clip never acts: the row's coefficients are positive and sum
 *            to rnd(sy), and q <= 16368, so the value lies in 0..1023 for every table.  The chroma clip below acts at its upper end
 *            only: the value before it spans 1..1024.)
 *   Chroma   W/2 x H/2 samples, separable filters in WINDOW coordinates, tap positions clamped to the window's luma rectangle
 *            0..W-1, 0..H-1 (what lies outside the window is not shown: luma outside it is never read).  Horizontally
 *            dst_chroma_loc 0, 2 (co-sited): columns 2i-1, 2i, 2i+1 with weights 1, 2, 1; 1, 3 (centred): 2i, 2i+1 with 2, 2.
 *            Vertically 0, 1 (centred): rows 2j, 2j+1 with 2, 2; 2, 3 (top): rows 2j-1, 2j, 2j+1 with 1, 2, 1.
 *              C = clip((sum of w_x w_y C14 + 128) >> 8, 0, 1023)        -- the weights sum to 16.
 *            (W and H are even, so only column -1 and row -1 are ever clamped.)
 *   Surface  `Formats`, `Values` and `Layout` of "Surface output on the device" on that picture: s is its 10-bit sample, rounding and
 *            dither go by output coordinates, gaps are never written, ovhip_surface_bytes gives the size.
 * Refused before anything is launched or written, the reason in the context's error text: the conversion's refusals above; everything
 * the surface output refuses; everything the RGB output through a table refuses of the picture and the table -- a null table, a table
 * of another device, sizes that are not multiples of 4 (stricter than the surface's "even").  No restriction on P.
 * Several reduced sizes of one picture through the table: "Output ladder through a colour table" below.
 * Not done: a conversion without a table (the lattice table is the identity); destination locations 4 and 5; constant-luminance /
 * ICtCp; 4:2:2 / 4:4:4; error diffusion; a table per picture.
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_surface_conv {
    uint8_t src_matrix, src_full_range, src_chroma_loc;      /* the decoded picture: as ovhip_rgb_format's matrix, full_range, chroma_loc */
    uint8_t dst_matrix, dst_full_range, dst_chroma_loc;      /* the converted picture */
    uint8_t rsv[2];                                          /* must be 0 */
} ovhip_surface_conv;                    /* 8 bytes */
/* OVHIP_OK when the conversion, the format's picture-independent part (enums, rsv, rounding, pitch and offset multiples) and the
 * table's size and peak are all accepted, else the code the launch would give.  Host only. */
int  ovhip_surface_lut_check(const ovhip_surface_conv *conv, const ovhip_surface_format *fmt, int size, int peak);
/* The forward matrix of conv's destination: coef = y_r y_g y_b, b_r b_g b_b, r_r r_g r_b; *yoff = 64 or 0.  Host only. */
int  ovhip_surface_lut_coefs(const ovhip_surface_conv *conv, int32_t coef[9], int32_t *yoff);
/* The definition on host planes and a host table into a host surface: tests, and callers that hold the picture on the host.  Refusals
 * as the launch's, and a table entry above the peak (OVHIP_EINVAL); nothing is written when it refuses.  It allocates the converted
 * picture (OVHIP_ENOMEM). */
int  ovhip_surface_lut_host(const uint16_t *y, const uint16_t *cb, const uint16_t *cr, int32_t w, int32_t h, int32_t stride_y, int32_t stride_c,
                            const ovhip_window *win, const ovhip_surface_conv *conv, const ovhip_surface_format *fmt, int size, int peak,
                            const uint16_t *host_table, void *dst, size_t dst_bytes);
/* As the surface launch: d_dst in DEVICE memory, at least ovhip_surface_bytes() bytes, aligned to its element; asynchronous on the ctx
 * stream; allocates nothing.  ONE launch (k_surface_lut: a lane owns 8 luma columns of an output row pair and the 4 chroma pairs under
 * them, with one more column or row where the destination's chroma filter reaches across). */
int  ovhip_surface_lut_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_conv *conv, const ovhip_surface_format *fmt,
                              const ovhip_rgb_lut *lut, void *d_dst, size_t dst_bytes);
/* Synchronous convenience, as ovhip_pic_output_surface: the launch into the context's grow-only scratch, then a D2H of the rows' own
 * bytes into host_dst (the gaps stay unwritten in host memory too). */
int  ovhip_pic_output_surface_lut(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_conv *conv, const ovhip_surface_format *fmt,
                                  const ovhip_rgb_lut *lut, void *host_dst, size_t dst_bytes);

/* ------------------------------------------------------------------------------------
 * Motion field output on the device: the motion of a decoded picture -- vectors, reference slots and prediction kinds of every inter
 * block -- as a dense field on the 4x4 luma grid in DEVICE memory, in the consumer's dtype and layout; nothing is downloaded.  What
 * ffmpeg's export_mvs side data is for: compressed-domain analytics, re-encoder motion hints, temporal denoisers.  Nothing in the
 * reference does this.  The definition is exact, so every implementation of it (tests/spec_mvfield.py, ovhip_mvfield_host,
 * k_mvfield) is compared for equality.
 *
 *   Grid     W4 = (w + 3) >> 2, H4 = (h + 3) >> 2; cell (cx, cy) is luma [4cx, 4cx + 4) x [4cy, 4cy + 4).  The field is of the DECODED
 *            picture at its coded size: no conformance window, no output scale, no film grain applies to it.
 *   Sources  five unit lists, read in the recorder's order:
 *              mc    ovhip_mc_unit        without the units that carry OVHIP_MC_NO_LUMA
 *              mcx   ovhip_mc_unit        all
 *              aff   ovhip_aff_unit       all, with the side arena
 *              rpr   ovhip_rpr_unit       without the units that carry OVHIP_RPR_NO_LUMA
 *              affr  ovhip_aff_rpr_unit   all, with the same side arena
 *            A unit covers the cells x/4 .. (x + w)/4 - 1 by y/4 .. (y + h)/4 - 1, clipped to the grid.  Units that carry luma never
 *            overlap: the recorder's property, which the kernel does not check (the host twin does).  A cell no unit covers is EMPTY:
 *            intra, IBC, the intra part of CIIP, or nothing.
 *   Info     one little-endian uint32 per cell, info[cy][cx] = ref0 | ref1 << 8 | kind << 16 | scaled << 24.
 *            ref0, ref1: the unit's slot in the picture's reference table (the k of ovhip_frame_ref / ovhip_frame_ref_at; mc, mcx, aff:
 *            the unit's ref0 / ref1; rpr and affr: s[l].ref), 0xFF where the unit's dir does not use the list and in empty cells (a uni
 *            unit's unused ref field holds 0, not a marker: the rule comes from dir).
 *            kind: 1 INTER; 2 AFFINE (aff, affr); 4 GPM (OVHIP_MC_GPM of mc and mcx, OVHIP_RPR_GPM); 8 DMVR and 16 BDOF (the flags of
 *            an mcx unit); 32 BCW (dir == 3, not GPM, w0 != 4 || w1 != 4; every list); 64 PROF (OVHIP_AFF_PROF, OVHIP_AFFR_PROF); bit 7
 *            is zero.
 *            scaled: bit l is set when list l is used and reads a reference of another size (OVHIP_RPR_S0 / S1, OVHIP_AFFR_S0 / S1).
 *            Such a list carries anchors, not vectors: its vector is exported as 0.
 *            An empty cell is 0x0000FFFF.
 *   Vectors  four channels per cell, mv0x, mv0y, mv1x, mv1y, in 1/16 luma sample: the vectors the prediction read with.
 *              mc    mv0x, mv0y, mv1x, mv1y as stored (after clip_mv)
 *              mcx   the same; with vectors == OVHIP_MVF_REFINED and OVHIP_MC_DMVR set, the unit's four words of the refined array
 *                    (mv_out of ovhip_mcx_launch, 4 int32 per mcx unit) instead; units without the DMVR flag never read that array
 *              aff, affr   the cell is one sub-block: k = (cy - y/4) * (w/4) + (cx - x/4), the words side[side_off + 4k .. + 3]; for
 *                    affr only the words of an unscaled list.  ident_l, ident_c and PROF's per-sample refinement change nothing here
 *              rpr   an unscaled list gives s[l].pos_x, s[l].pos_y
 *            An unused list gives 0 (whatever the unit's fields or side words hold).  A vector v leaves as
 *              OVHIP_MVF_I32   v
 *              OVHIP_MVF_F32   (float)v * 0.0625f, in luma samples (exact: |v| < 2^24)
 *              OVHIP_MVF_F16   that float rounded to nearest even (the conversion of the RGB output's F16)
 *   Layout   both tight: OVHIP_MVF_PLANAR [4][H4][W4], OVHIP_MVF_CELLS [H4][W4][4].
 *   Sizes    ovhip_mvfield_bytes: 4 * W4 * H4 * elem for the vectors and 4 * W4 * H4 for the info.  Either destination may be NULL (not
 *            wanted); both NULL is an error.
 * Refused (OVHIP_EINVAL) before anything is launched or written, the reason in the context's error text: a null context or format;
 * both destinations NULL; non-positive sizes or sizes above 16384; an unknown dtype, layout or vectors value; non-zero rsv; a
 * destination that is not element-aligned; a byte count below the size ("too small", with both numbers); destinations that overlap
 * each other; a non-zero count with a NULL array; OVHIP_MVF_REFINED with mcx units and no refined array; and, from the host twin
 * only: a unit that is not 4-aligned, or a cell that is covered twice.  Not done: intra modes and IBC block vectors; grids coarser
 * than 4x4 (a consumer strides the tensor); vectors of scaled lists; POC distances (the caller owns the slot table); a window; an
 * event hand-off instead of completion at return; a shim entry point.
 * ---------------------------------------------------------------------------------- */
enum { OVHIP_MVF_I32 = 0, OVHIP_MVF_F32 = 1, OVHIP_MVF_F16 = 2 };                                 /* ovhip_mvfield_format.dtype */
enum { OVHIP_MVF_PLANAR = 0, OVHIP_MVF_CELLS = 1 };                                               /* ovhip_mvfield_format.layout */
enum { OVHIP_MVF_UNIT = 0, OVHIP_MVF_REFINED = 1 };                                               /* ovhip_mvfield_format.vectors */
enum { OVHIP_MVF_INTER = 1, OVHIP_MVF_AFFINE = 2, OVHIP_MVF_GPM = 4, OVHIP_MVF_DMVR = 8, OVHIP_MVF_BDOF = 16, OVHIP_MVF_BCW = 32, OVHIP_MVF_PROF = 64 };   /* kind */
#define OVHIP_MVF_EMPTY 0x0000FFFFu
typedef struct ovhip_mvfield_format {
    uint8_t dtype, layout, vectors, rsv;  /* rsv must be 0 */
} ovhip_mvfield_format;
/* The five lists with their counts, the side arena of aff and affr, and the refined array of mcx (NULL unless vectors ==
 * OVHIP_MVF_REFINED and n_mcx != 0).  HOST pointers for ovhip_mvfield_host, DEVICE pointers for ovhip_mvfield_launch. */
typedef struct ovhip_mvfield_src {
    const ovhip_mc_unit *mc, *mcx;
    const ovhip_aff_unit *aff;
    const ovhip_rpr_unit *rpr;
    const ovhip_aff_rpr_unit *affr;
    const int32_t *side;                  /* ovhip_rec_aff_side() */
    const int32_t *refined;               /* 4 int32 per mcx unit */
    uint32_t n_mc, n_mcx, n_aff, n_rpr, n_affr;
} ovhip_mvfield_src;
/* Bytes of the vectors of a w x h picture; *info_bytes (may be NULL): of the info.  0 (and *info_bytes = 0) for a size or a format
 * the launch would refuse.  Host only. */
size_t ovhip_mvfield_bytes(int32_t w, int32_t h, const ovhip_mvfield_format *fmt, size_t *info_bytes);
/* The definition over lists in host memory into host memory.  Refusals as the launch's and the two of its own; nothing is written
 * when it refuses. */
int  ovhip_mvfield_host(int32_t w, int32_t h, const ovhip_mvfield_src *src, const ovhip_mvfield_format *fmt,
                        void *vec, size_t vec_bytes, uint32_t *info, size_t info_bytes);
/* d_vec, d_info: DEVICE.  Two steps in order on the ctx stream: a clear that writes the empty cell into every byte of the wanted
 * destinations (16-byte stores where the address allows), then k_mvfield, one launch over all five lists (a lane owns one row of a
 * unit's cells; 16-byte stores where the address allows, narrower ones otherwise).  Asynchronous; allocates nothing. */
int  ovhip_mvfield_launch(ovhip_ctx *ctx, int32_t w, int32_t h, const ovhip_mvfield_src *d_src, const ovhip_mvfield_format *fmt,
                          void *d_vec, size_t vec_bytes, void *d_info, size_t info_bytes);
/* The motion field of the picture the job decoded last: valid after ovhip_job_wait of a whole-picture flush (ovhip_job_flush, a
 * resident replay included), on the job's context.  Reads the device copies that flush placed -- the refined vectors where its
 * k_mcxa left them -- and uploads nothing; asynchronous on the context's stream.  OVHIP_EUNSUP after a band-wise submission (the
 * arrays live in band arenas), OVHIP_EINVAL before any flush or after ovhip_job_begin; OVHIP_MVF_REFINED needs a flush that ran
 * the prediction stage. */
int  ovhip_job_mvfield(ovhip_job *job, const ovhip_mvfield_format *fmt, void *d_vec, size_t vec_bytes, void *d_info, size_t info_bytes);

/* ------------------------------------------------------------------------------------
 * Output resampling: a stream that changes its coded size (RPR) can leave the device at ONE size.  Replaces pp_sample_rate_conv
 * (pp_pic_scale.c:250-377), called once per plane by pp_process_frame (post_proc.c:116-126) when the decoder's `upscale` option is
 * on (ovdec.c:562; ovdec.c:479 / :523 are the call sites), for up-sampling and equal size, bit-exactly -- including its phase, which
 * is the LOW 4 (luma) / 5 (chroma) bits of the 13- / 14-bit fixed-point position.  The decoded picture is only read:
 * references keep predicting from it at its coded size.  Film grain, the first branch of pp_process_frame, is the section after this
 * one; SL-HDR, the third, is not built.
 *
 * `ovhip_scale_info` = struct ScalingInfo (ovdpb.h:85-93): the scaling window in chroma sample units and the SPS chroma collocation
 * flags; what the reference passes is the picture's own (pic->scale_info).
 *
 * Refused: OVHIP_EUNSUP (reason in ovhip_last_error) when a scale factor of luma or chroma exceeds 1 << bits on either axis --
 * down-sampling, where the reference switches to 12-tap tables and, for chroma phases >= 16, indexes past them; OVHIP_EINVAL when
 * the scaling window leaves nothing, a size is not a multiple of 4 (or above 16384), a plane is missing or dst aliases src.
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_scale_info { uint16_t win_left, win_right, win_top, win_bottom; uint8_t chroma_hor_col, chroma_ver_col; } ovhip_scale_info;
/* Host only (no device needed): the argument check the launch uses.  scale[4] = luma horizontal / vertical, chroma horizontal /
 * vertical factors, ((src - window) << bits) / dst with bits = 13 (luma) / 14 (chroma); written whenever they could be derived. */
int  ovhip_output_scale_check(int32_t src_w, int32_t src_h, const ovhip_scale_info *info, int32_t dst_w, int32_t dst_h, int32_t scale[4]);
/* Every sample of dst (its own w x h) from src.  One launch (k_output_scale), asynchronous on the ctx stream. */
int  ovhip_output_scale_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_scale_info *info, const ovhip_pic *dst);
/* Synchronous conveniences: resample into a grow-only scratch picture of the context (no allocation once a size has been seen), then
 * exactly ovhip_pic_output / ovhip_pic_digest on it; `win` applies to the resampled picture.  out_w x out_h equal to the picture's
 * size with an empty scaling window still runs the resampler (an identity copy by its arithmetic). */
int  ovhip_pic_output_scaled(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_scale_info *info, int32_t out_w, int32_t out_h,
                             const ovhip_window *win, void *host_dst);
int  ovhip_pic_digest_scaled(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_scale_info *info, int32_t out_w, int32_t out_h,
                             const ovhip_window *win, uint8_t out16[16]);
/* Device + page-locked bytes the context's grow-only scratch buffers hold (the synchronous conveniences above and of the output path):
 * constant from call to call once the sizes have been seen. */
size_t ovhip_ctx_scratch_bytes(const ovhip_ctx *ctx);

/* ------------------------------------------------------------------------------------
 * Reduced-size output on the device: a finished 10-bit 4:2:0 picture leaves SMALLER than it was coded -- 2160p as 1080p for a
 * transcoder's ladder, half- or quarter-size for a model -- by the exact area average.  Nothing in the reference does this (the
 * down-sampling branch of pp_sample_rate_conv is dead code under `upscale` and reads past its chroma tables), and the resampler above
 * keeps refusing down-sampling.  The definition is integer only, so every implementation of it (tests/spec_reduce.py,
 * ovhip_output_reduce_host, k_output_reduce) is compared for equality.
 *
 *   Input    an ovhip_pic of w x h (multiples of 4, at most 16384) and a window in chroma units, read as the packed output reads it:
 *            the region reduced starts at luma (2 lft, 2 abv) and is Ws = w - 2 (lft + rgt) by Hs = h - 2 (abv + blw), both positive
 *            multiples of 4; the chroma region starts at (lft, abv) and is Ws/2 x Hs/2.
 *   Output   Wd x Hd (positive multiples of 4), chroma Wd/2 x Hd/2, with the SAME Chroma420SampleLocType as the source.
 *   Axis     S = Ws or Hs, D = Wd or Hd, g = gcd(S, D), p = S/g, q = D/g; the chroma planes have the same p and q.  Required:
 *            D <= S, S <= 8 D, p <= 256.
 *   Weights  along one axis of a plane with S' samples (S for luma, S/2 for chroma), in units where a sample is 4q long: sample j
 *            occupies [4q j, 4q (j+1)) for every integer j, output k's footprint is [4p k - sigma, 4p (k+1) - sigma), and w(k, j)
 *            is the length of their intersection.  A j outside 0 .. S'-1 is read as the nearest sample OF THE REGION: nothing
 *            outside the window is ever read.  Every output's weights sum to 4p.  sigma = 0 for luma; for chroma
 *            sigma = (p - q)(1 - a) horizontally and (p - q)(1 - b) vertically, a and b those of the RGB output: a = chroma_loc & 1,
 *            b = 1 for chroma_loc 0, 1, b = 0 for 2, 3, b = 2 for 4, 5.
 *   Value    V = sum_jy w_y(ky, jy) sum_jx w_x(kx, jx) s(jx, jy);  out = (V + n/2) div n,  n = 16 p_x p_y.  A mean of samples stays in
 *            0..1023: no clip.  V + n/2 <= 16 * 256 * 256 * 1023 + 2^19 < 2^31: everything fits int32.
 * The luma footprints tile the region: sum V = 16 q_x q_y sum s.  For integer ratios the weights' centroid is exactly the output's
 * sample site; for other ratios the average is centred per footprint (a property of the method).  A ratio of 1 on an axis is a copy
 * along it.  Example: 2:1 with horizontally co-sited chroma weighs samples 2k-1, 2k, 2k+1 with 1, 4, 3 over 8.
 * Refused, the reason in the context's error text where there is a context: OVHIP_EUNSUP for D > S on an axis (up-sampling: that is
 * ovhip_output_scale_*), for S > 8 D (the ratio) and for p > 256 (p/q, and the advice to pick sizes with a larger common divisor);
 * OVHIP_EINVAL for sizes that are not multiples of 4 or above 16384, a window that leaves nothing or a region that is not a multiple
 * of 4, chroma_loc > 5, non-zero rsv, a missing plane, a stride below the width, dst aliasing src.  Not done: up-sampling, ratios
 * above 8, other filters, reduce together with film grain or the output scale, 4:2:2 / 4:4:4 and 8-bit pictures, a reduced motion
 * field, a shim entry point.
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_reduce_info { ovhip_window win; uint8_t chroma_loc, rsv[3]; } ovhip_reduce_info;      /* rsv must be 0 */
/* Host only (no device needed): the argument check the launch uses.  ratio[4] = p_x, q_x, p_y, q_y, written whenever they can be
 * derived (0 otherwise). */
int  ovhip_output_reduce_check(int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, int32_t dst_w, int32_t dst_h, int32_t ratio[4]);
/* The definition over pictures in HOST memory (both hold host pointers; strides in samples): tests, and callers that hold the picture
 * on the host.  Refusals as the launch's; nothing is written when it refuses. */
int  ovhip_output_reduce_host(const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_pic *dst);
/* num / n as k_output_reduce divides (a reciprocal estimate and one correction step), on the host: num < 2^31, 0 < n <= 2^20, a
 * quotient below 2048.  The twin divides with `/`; the two agree on every such pair.  Host only. */
uint32_t ovhip_output_reduce_divide(uint32_t num, uint32_t n);
/* Every sample of dst (its own w x h and strides) from the window of src.  One launch (k_output_reduce: luma and both chroma planes),
 * asynchronous on the ctx stream; allocates nothing.  16-byte loads and stores where a row's address allows, narrower otherwise. */
int  ovhip_output_reduce_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_pic *dst);
/* Synchronous conveniences: reduce into the context's grow-only scratch picture (no allocation once a size has been seen; a refused
 * request allocates nothing), then exactly ovhip_pic_output / ovhip_pic_digest on it; `win` applies to the REDUCED picture. */
int  ovhip_pic_output_reduced(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_reduce_info *info, int32_t out_w, int32_t out_h,
                              const ovhip_window *win, void *host_dst);
int  ovhip_pic_digest_reduced(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_reduce_info *info, int32_t out_w, int32_t out_h,
                              const ovhip_window *win, uint8_t out16[16]);

/* ------------------------------------------------------------------------------------
 * Output ladder on the device: ONE finished 10-bit 4:2:0 picture leaves as SEVERAL reduced surfaces -- 2160p as the 1080p, 720p, 540p
 * and 360p rungs of a transcoder's ladder --, each at its own size, format and address, from ONE launch that reads the picture once
 * per rung and writes no intermediate picture.  There is no new arithmetic, no new rounding and no new table: the ladder is the
 * composition of the two definitions above, so every implementation of it (tests/spec_ladder.py, ovhip_ladder_host, k_output_ladder)
 * is compared for equality.
 *
 *   Ladder   one ovhip_reduce_info -- the window in chroma units and chroma_loc -- for the picture shown, and n rungs,
 *            1 <= n <= OVHIP_LADDER_MAX_RUNGS = 8 (k_output_ladder's arguments for 8 rungs are about 1 KB: inside the 4 KB a
 *            launch's kernel arguments may take).
 *   Rung r   out_w x out_h, a surface format, a destination of dst_bytes.  By definition
 *                rung r = surface(reduce(src, info, out_w_r, out_h_r), window NULL, fmt_r)
 *            with reduce of "Reduced-size output on the device" and surface of "Surface output on the device", byte for byte: the
 *            dither thresholds are keyed by the coordinates in the rung's own output planes, bytes between rows and planes are
 *            never written.  Rungs are independent of one another.  A rung of the region's own size is 1:1 on both axes: allowed,
 *            the ladder's top rung.  Two rungs may have one size and different formats.
 * A ladder is ALL OR NOTHING.  Refused before anything is launched or written, the reason and the rung's index in the context's error
 * text where there is a context: whatever ovhip_output_reduce_check refuses for a rung (OVHIP_EUNSUP or OVHIP_EINVAL as there);
 * whatever the surface output refuses for a rung's size, format, destination and dst_bytes (OVHIP_EINVAL); n out of range; null
 * rungs, info or picture; a missing plane or a stride below the width; two rungs' destinations that overlap one another, or one that
 * overlaps the picture.  Rungs through a colour table: "Output ladder through a colour table" below.  RGB tensors at several sizes: "RGB pyramid on the
 * device" below.  Not done: rungs of different windows, up-sampling rungs, ratios above 8, an event hand-off to the consumer, a shim entry point.
 * ---------------------------------------------------------------------------------- */
#define OVHIP_LADDER_MAX_RUNGS 8
typedef struct ovhip_ladder_rung {
    int32_t out_w, out_h;
    ovhip_surface_format fmt;            /* its rsv must be 0, as everywhere */
    void *dst; size_t dst_bytes;         /* at least ovhip_surface_bytes(out_w, out_h, NULL, &fmt) */
} ovhip_ladder_rung;
/* Host only (no device needed): the checks the launch makes that need no picture and no destination -- n, every rung's reduce check
 * and format, against a src_w x src_h picture.  ratio[r] = p_x, q_x, p_y, q_y of rung r (ratio may be NULL), written for every rung
 * whose values can be derived (0 otherwise).  The first refusal's code. */
int  ovhip_ladder_check(int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n, int32_t ratio[][4]);
/* The definition over a picture and destinations in HOST memory: ovhip_output_reduce_host, then ovhip_surface_host, per rung (it
 * allocates one reduced picture per rung on the host heap; OVHIP_ENOMEM when that fails, before anything is written).  Refusals as the
 * launch's; nothing is written when it refuses. */
int  ovhip_ladder_host(const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n);
/* Every rung's surface at its dst (DEVICE memory, aligned to its element) from the window of src.  ONE launch (k_output_ladder: all
 * rungs, all planes; a workgroup finds its rung, plane and tile from a prefix table in the arguments, reduces the tile as
 * k_output_reduce does and stores it as the surface's elements: 16-byte stores where the address allows, narrower at row tails, odd
 * pitches and offsets; the Cb and the Cr of an interleaved row leave together).  Asynchronous on the ctx stream; allocates nothing,
 * uploads nothing. */
int  ovhip_ladder_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n);
/* Synchronous convenience, as ovhip_pic_output_surface: the rungs' dst are HOST memory; the launch into the context's grow-only
 * scratch, then one D2H per rung (a layout with gaps: one strided D2H per plane, so the gaps stay unwritten in host memory too). */
int  ovhip_pic_output_ladder(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n);

/* ------------------------------------------------------------------------------------
 * Output ladder through a colour table: ONE finished 10-bit 4:2:0 picture leaves as SEVERAL reduced surfaces whose samples are those of
 * the CONVERTED reduced pictures -- a BT.2020 PQ or HLG 2160p picture as the BT.709 SDR 1080p, 720p, 540p and 360p NV12 rungs of a
 * transcoder's ladder --, from ONE launch that writes no intermediate picture.  Nothing new is computed: with one ovhip_reduce_info, n
 * rungs (the ovhip_ladder_rung above, 1 <= n <= OVHIP_LADDER_MAX_RUNGS), one ovhip_surface_conv and one ovhip_rgb_lut table of 17, 33 or
 * 65 points per axis and any peak, by definition
 *                rung r = surface_lut(reduce(src, info, out_w_r, out_h_r), window NULL, conv, fmt_r, lut)
 * with reduce of "Reduced-size output on the device" and surface_lut of "Surface output through a colour table", byte for byte; every
 * implementation of it (tests/spec_ladder_lut.py, ovhip_ladder_lut_host, k_ladder_lut) is compared for equality.  So the source's chroma
 * taps clamp to the REDUCED picture's chroma plane, the destination chroma filter's taps to the reduced picture's luma rectangle, the
 * dither thresholds go by the rung's own output coordinates, bytes between rows and planes are never written, rungs are independent
 * of one another, and a rung of the region's own size is surface_lut of the region.  One table and one conversion serve all rungs.
 * Reduce first, then convert, on purpose: a rung equals what a frame writes with ovhip_frame_set_output_reduce in front of
 * ovhip_frame_set_surface_lut, and the conversion runs on the rungs' pixels only.  (Averaging in linear light -- convert first -- is
 * not this.)
 * A ladder is ALL OR NOTHING.  Refused before anything is launched or written, the reason and the rung's index in the context's error
 * text: everything ovhip_ladder_launch refuses; the conversion's own refusals with their codes; conv->src_chroma_loc other than
 * info->chroma_loc (OVHIP_EINVAL: the reduced picture keeps the source's sample location, so two values are a mistake that would shift
 * the chroma silently); everything ovhip_surface_lut_launch refuses of a rung's picture, format and destination -- rung sizes that
 * are not multiples of 4 among them --; a null table, a table of another device.
 * RGB tensors at several sizes, with or without a table: "RGB pyramid on the device" below.
 * Not done: a table or a conversion per rung, convert-then-reduce, rungs of different windows, up-sampling rungs, ratios
 * above 8, destination locations 4 and 5, a conversion without a table, a shim entry point.
 * ---------------------------------------------------------------------------------- */
/* Host only: the checks the launch makes that need no picture and no destination, against a src_w x src_h picture and a table of
 * `size` points and peak `peak`.  ratio as ovhip_ladder_check's.  The first refusal's code. */
int  ovhip_ladder_lut_check(int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n,
                            const ovhip_surface_conv *conv, int size, int peak, int32_t ratio[][4]);
/* The definition over a picture, a table and destinations in HOST memory: ovhip_output_reduce_host, then ovhip_surface_lut_host, per
 * rung (one reduced picture per rung on the host heap; OVHIP_ENOMEM when that fails).  Refusals as the launch's, and a table entry above
 * the peak (OVHIP_EINVAL); nothing is written when it refuses. */
int  ovhip_ladder_lut_host(const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n, const ovhip_surface_conv *conv,
                           int size, int peak, const uint16_t *host_table);
/* Every rung's surface at its dst (DEVICE memory, aligned to its element) from the window of src.  ONE launch (k_ladder_lut: all rungs,
 * all planes; a workgroup finds its rung and tile from a prefix table in the arguments, reduces the tile's Y, Cb and Cr with their halo
 * into LDS, converts from there and stores the surface's elements).  Asynchronous on the ctx stream; allocates nothing, uploads
 * nothing; no intermediate picture in device memory. */
int  ovhip_ladder_lut_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n,
                             const ovhip_surface_conv *conv, const ovhip_rgb_lut *lut);
/* Synchronous convenience, as ovhip_pic_output_ladder: the rungs' dst are HOST memory; the launch into the context's grow-only scratch,
 * then the rows' own bytes of every plane to the host (the gaps stay unwritten in host memory too). */
int  ovhip_pic_output_ladder_lut(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n,
                                 const ovhip_surface_conv *conv, const ovhip_rgb_lut *lut);

/* ------------------------------------------------------------------------------------
 * RGB pyramid on the device: ONE finished 10-bit 4:2:0 picture leaves as SEVERAL reduced RGB tensors -- 2160p as a 1080p and a 540p
 * F16 CHW tensor for two models and a 640x360 U8 HWC thumbnail --, each at its own size, dtype, layout and address, from ONE launch
 * that writes no intermediate picture.  It is an OUTPUT beside RGB, surface and ladder, not a post-process setting: film grain, the
 * output scale or a first reduce compose in front of it, and the other outputs of the picture see what they saw without it.  There is
 * no new arithmetic, no new rounding and no new table; with one ovhip_reduce_info, n levels and, optionally, one ovhip_rgb_lut table,
 * by definition
 *     without a table    level r = rgb(reduce(src, info, out_w_r, out_h_r), window NULL, fmt_r)
 *     with a table       level r = rgb_lut(reduce(src, info, out_w_r, out_h_r), window NULL, fmt_r, lut)
 * with reduce of "Reduced-size output on the device", rgb of "RGB output on the device" and rgb_lut of "RGB output through a colour
 * table", byte for byte; every implementation of it (tests/spec_rgb_pyramid.py, ovhip_rgb_pyramid_host, k_rgb_pyramid) is compared
 * for equality.  So the chroma taps clamp to the REDUCED picture's chroma plane; without a table a U8 level takes the 8-bit
 * coefficients and every other level the 10-bit ones -- two levels of one pyramid may carry different coefficient sets --; with a
 * table the matrix is at 10 bits for every dtype and a U8 level needs a peak of at most 255.
 *
 *   Pyramid  one ovhip_reduce_info -- the window in chroma units and chroma_loc -- for the picture shown, and n levels,
 *            1 <= n <= OVHIP_PYRAMID_MAX_LEVELS = 8 (k_rgb_pyramid's arguments for 8 levels are about 1 KB: inside the 4 KB a launch's
 *            kernel arguments may take).
 *   Level r  out_w x out_h (multiples of 4, as the RGB output's), an ovhip_rgb_format, a destination of dst_bytes.  dtype and layout
 *            are the level's own.  matrix, full_range and chroma_loc describe the one SOURCE and must be equal in all levels, and
 *            chroma_loc must be info->chroma_loc: the reduced picture keeps the source's sample location, so two values are a mistake
 *            that would shift the chroma silently.  A level of the region's own size is 1:1 on both axes: allowed.  Two levels may
 *            have one size and different formats.  One table serves all levels.
 * A pyramid is ALL OR NOTHING.  Refused before anything is launched or written, the reason and the level's index in the context's
 * error text where there is a context: whatever ovhip_output_reduce_check refuses for a level (OVHIP_EUNSUP or OVHIP_EINVAL as there);
 * whatever ovhip_rgb_launch -- with a table: ovhip_rgb_lut_launch -- refuses for a level's size, format, destination and dst_bytes,
 * with its code; n out of range; null levels, info or picture; a missing plane or a stride below the width; formats that disagree in
 * matrix, range or location; two levels' destinations that overlap one another, or one that overlaps the picture; a table of another
 * device.
 * Not done: a window per level, up-sampling levels, ratios above 8, normalisation (mean / std), a table per level,
 * convert-then-reduce (averaging in linear light), a shim entry point.
 * ---------------------------------------------------------------------------------- */
#define OVHIP_PYRAMID_MAX_LEVELS 8
typedef struct ovhip_rgb_level {
    int32_t out_w, out_h;
    ovhip_rgb_format fmt;
    void *dst; size_t dst_bytes;         /* at least ovhip_rgb_bytes(out_w, out_h, NULL, &fmt) */
} ovhip_rgb_level;
/* Host only (no device needed): the checks the launch makes that need no picture and no destination -- n, every level's reduce check,
 * size and format, the formats' agreement -- against a src_w x src_h picture and a table of lut_size points and peak lut_peak;
 * lut_size 0: no table.  ratio[r] = p_x, q_x, p_y, q_y of level r (ratio may be NULL), written for every level whose values can be
 * derived (0 otherwise).  The first refusal's code. */
int  ovhip_rgb_pyramid_check(int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n, int lut_size, int lut_peak,
                             int32_t ratio[][4]);
/* The definition over a picture, an optional table (lut_size 0: none) and destinations in HOST memory: ovhip_output_reduce_host, then
 * ovhip_rgb_host or ovhip_rgb_lut_host, per level (one reduced picture per level on the host heap; OVHIP_ENOMEM when that fails, before
 * anything is written).  Refusals as the launch's, and a table entry above the peak (OVHIP_EINVAL); nothing is written when it refuses. */
int  ovhip_rgb_pyramid_host(const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n, int lut_size, int lut_peak,
                            const uint16_t *host_table);
/* Every level's tensor at its dst (DEVICE memory, aligned to its element) from the window of src; lut NULL: without a table.  ONE
 * launch (k_rgb_pyramid: all levels; a workgroup finds its level and tile from a prefix table in the arguments, reduces the tile's Y,
 * Cb and Cr with the chroma halo into LDS, converts from there and stores the level's elements: 16-byte stores where the address
 * allows, narrower at row tails and unaligned bases).  Asynchronous on the ctx stream; allocates nothing, uploads nothing; no
 * intermediate picture in device memory. */
int  ovhip_rgb_pyramid_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n,
                              const ovhip_rgb_lut *lut);
/* Synchronous convenience, as ovhip_pic_output_rgb: the levels' dst are HOST memory; the launch into the context's grow-only scratch
 * (no allocation once the sizes have been seen; a refused request allocates nothing), then one D2H per level. */
int  ovhip_pic_output_rgb_pyramid(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n,
                                  const ovhip_rgb_lut *lut);

/* ------------------------------------------------------------------------------------
 * Film grain synthesis (film grain characteristics SEI, frequency-filtering model): replaces fg_grain_apply_pic
 * (pp_film_grain.c:814-978) as pp_process_frame calls it (post_proc.c:106-108: no IDR offset, edge smoothing on, 10 bit, 4:2:0),
 * bit-exactly wherever the reference is defined.  Per 8x8 block of a plane: the average of the block's samples inside the plane
 * (/ n, >> 2, clipped to 8 bits) selects an intensity interval; the interval's model values select a scale and one of 13 x 13
 * cells (horizontal x vertical cut-off frequency 2..14) of a fixed database of 64 x 64 grain patterns; a 31-bit shift register,
 * seeded per picture and component from the POC and stepped once per 16x16 block in raster order, picks the pattern's offset and
 * sign; sample = (+-scale * pattern) >> (log2_scale + 6); the grain columns either side of every vertical 8x8 edge are smoothed
 * inside a 16-row stripe; dst = clip(src + (grain << 2), 0..1023).  A component without a model is copied.  The decoded picture
 * is only read: references keep predicting from it.
 *
 * Three steps, the first two on the host without a device:
 *   ovhip_fg_params    the SEI's fields as the reference's function reads them
 *   ovhip_fg_derive    ONE call's model derivation (fg_compute_model_values, :768-807) -> ovhip_fg_model.  The reference derives
 *                      IN PLACE on every call: for chroma it halves value[..][0] and doubles value[..][1..2] (clamped to 2..14),
 *                      so a caller that hands the same struct to consecutive pictures gets 100 / 4 / 6, then 50 / 8 / 12, then
 *                      25 / 14 / 14.  `after` receives the fields as that one call leaves them: a caller that wants the
 *                      reference's sequence for a persistent SEI feeds `after` back in (the shim does); ovhip_stream_set_film_grain
 *                      and ovhip_frame_set_film_grain derive afresh from the params they were given, for every picture.
 *                      All 8 intervals are walked whatever num_intervals says, later ones overwriting earlier ones: unused
 *                      intervals with bounds 0..0 claim average 0, and the last one wins.
 *   ovhip_film_grain_launch   one launch (k_film_grain) over the luma and both chroma planes, behind a small one that steps the shift
 *                      register to every workgroup's first block (k_film_grain_seeds).
 *
 * Where the reference is undefined this back-end does not follow it:
 *   - an interval that some block average selects, whose scale is not 0 and whose cut-off (after the derivation) lies outside
 *     2..14, indexes far past the database there: OVHIP_EINVAL here.  With scale 0 the product is 0 whatever the cut-offs: such an
 *     entry gives grain 0 (and is stored with cut-offs 2, 2).
 *   - fg_model_id != 0 and fg_blending_mode_id != 0 are ignored there (H.274 gives them other semantics): OVHIP_EUNSUP here.
 *   - fg_characteristics_cancel_flag = 1 leaves the destination unwritten there: here the model has no component, the picture is
 *     copied.
 *   - a plane whose width is 1..7 mod 16 makes the reference average and write an 8x8 block that lies outside the plane (its
 *     samples are the next row's, its grain lands on the next row's columns 4..11 and, for luma, past the stripe buffer), a plane
 *     width below 8 sends its smoothing loop over the whole address space, and a plane height of 1..7 mod 16 averages rows below
 *     the plane.  Here only blocks inside the plane exist; parity is claimed for plane widths and heights of 0 or 8..15 mod 16.
 *   - grain together with output resampling: the reference resamples the UNgrained frame over the grained one (post_proc.c:107-126).
 * Sizes are multiples of 4 (at most 16384), as for the resampler: with that the smoothing never reads past a row's end.
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_fg_comp {
    uint8_t  present;              /* fg_comp_model_present_flag                                    */
    uint8_t  num_intervals;        /* fg_num_intensity_intervals_minus1 + 1 (not read: see above)   */
    uint8_t  num_model_values;     /* fg_num_model_values_minus1 + 1                                */
    uint8_t  pad_;
    uint8_t  lower[8], upper[8];   /* fg_intensity_interval_lower_bound / _upper_bound              */
    int16_t  value[8][3];          /* fg_comp_model_value: scale, horizontal, vertical cut-off      */
} ovhip_fg_comp;
typedef struct ovhip_fg_params {
    uint8_t  cancel;               /* fg_characteristics_cancel_flag */
    uint8_t  model_id;             /* fg_model_id                    */
    uint8_t  blending_mode;        /* fg_blending_mode_id            */
    uint8_t  log2_scale;           /* fg_log2_scale_factor           */
    ovhip_fg_comp comp[3];         /* Y, Cb, Cr                      */
} ovhip_fg_params;
/* entry[c][block average]: 0 = no interval (grain 0); else OVHIP_FG_VALID | scale (int16, low half) | h << 16 | v << 20 with
 * h, v = cut-off - 2 = the database cell.  The sign of the shift register's bit 0 is applied to the scale on the device. */
#define OVHIP_FG_VALID      (1u << 24)
#define OVHIP_FG_ENTRY(scale, h, v) (OVHIP_FG_VALID | (uint32_t)(uint16_t)(int16_t)(scale) | ((uint32_t)(h) << 16) | ((uint32_t)(v) << 20))
#define OVHIP_FG_DB_BYTES   (13 * 13 * 64 * 64)
typedef struct ovhip_fg_model {
    uint8_t  log2_scale;
    uint8_t  present[3];
    uint32_t entry[3][256];
} ovhip_fg_model;
/* Host only.  OVHIP_OK, or a refusal as listed above, on which neither `model` nor `after` is written.  `after` may be NULL and may
 * be `in`. */
int  ovhip_fg_derive(const ovhip_fg_params *in, ovhip_fg_model *model, ovhip_fg_params *after);
/* Host only: the grain database [h][v][row][column], OVHIP_FG_DB_BYTES of int8, as fg_data_base_generation (:666-765) builds it with
 * smoothing of the horizontal 8x8 edges on.  Built on the first call (some tens of ms), from any number of threads at once. */
const int8_t *ovhip_fg_database(void);
/* The start value of a component's shift register (c = 0 Y, 1 Cb, 2 Cr) and one step of it; host only. */
uint32_t ovhip_fg_seed(int32_t poc, int32_t idr_offset, int c);
uint32_t ovhip_fg_prng(uint32_t x);
/* out[k] = the register at the start of stripe k = `start` stepped k * blocks_per_stripe times (the register is never reset inside a
 * picture), k < n_stripes; host only.  Jumps instead of stepping: the n-step map is affine over GF(2) and kept per thread. */
void ovhip_fg_stripe_seeds(uint32_t start, int32_t blocks_per_stripe, int32_t n_stripes, uint32_t *out);
/* dst = src with grain; src and dst of one size, planes apart.  Asynchronous on the ctx stream; the database is uploaded at a
 * context's first launch (contexts that never use grain hold nothing), the model and the per-stripe seeds travel through a small
 * page-locked ring of the context.  idr_offset: 0 for the reference's caller.  OVHIP_EINVAL for a size mismatch, sizes that are not
 * multiples of 4 (or above 16384), a missing plane, dst aliasing src, or a model entry that points outside the database. */
int  ovhip_film_grain_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_fg_model *model, int32_t poc, int32_t idr_offset,
                             const ovhip_pic *dst);
/* Synchronous conveniences: grain into the context's grow-only scratch picture (the one the scaled outputs use), then exactly
 * ovhip_pic_output / ovhip_pic_digest on it. */
int  ovhip_pic_output_grain(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_fg_model *model, int32_t poc, const ovhip_window *win, void *host_dst);
int  ovhip_pic_digest_grain(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_fg_model *model, int32_t poc, const ovhip_window *win, uint8_t out16[16]);

/* ------------------------------------------------------------------------------------
 * TMVP motion plane.  The reference's caller stores what rcn_dmvr_mv_refine returned into the CTU-local
 * 16x16 array of 8x8 cells tmvp_mv[l].mvs (vcl_coding_unit.c:2629-2645: cell ((x0 + 7) >> 3, (y0 + 7) >> 3) of the <= 16x16
 * block, its right neighbour for 16-wide and lower neighbour(s) for 16-high blocks), and tmvp_store_mv copies rows
 * 0 .. nb_tmvp_unit-1 of that array into the picture's plane (drv_lines.c:270-330: plane->mvs + ctb_offset + i * pln_stride,
 * pln_stride = nb_tmvp_unit * nb_ctb_w, nb_tmvp_unit = ctu >> 3).  ovhip_tmvp_cells_launch does that address arithmetic
 * on the device: for every refined unit with OVHIP_MC_DMVR it emits the plane cells the refined vectors belong in, in
 * PICTURE-LEVEL plane coordinates, so that the host applies a per-picture (or per-CTU-row) delta to the plane without
 * keeping per-CU bookkeeping -- the compressed-plane hand-over of the decoded picture's motion field.
 * out: 4 entries per unit (entry 4 * u + k; cell == OVHIP_TMVP_NONE: unused).
 * ---------------------------------------------------------------------------------- */
#define OVHIP_TMVP_NONE 0xffffffffu
typedef struct ovhip_tmvp_cell { uint32_t cell; int32_t mv0x, mv0y, mv1x, mv1y; } ovhip_tmvp_cell;
/* d_units / d_refined (4 int32 per unit: ovhip_mcx_launch's mv_out) / d_out: DEVICE.  Asynchronous on the ctx stream. */
int  ovhip_tmvp_cells_launch(ovhip_ctx *ctx, const ovhip_mc_unit *d_units, uint32_t n_units, const int32_t *d_refined,
                             int32_t log2_ctu_s, int32_t nb_ctb_w, ovhip_tmvp_cell *d_out);
/* After ovhip_job_wait of a flush with ovhip_job_params.tmvp_cells != 0: the cells of the picture's refined units (4 per
 * unit, recorder order), valid until the job's next begin. */
const ovhip_tmvp_cell *ovhip_job_tmvp_cells(ovhip_job *job, size_t *n_entries);


/* ====================================================================================
 * Frame threads and the device DPB (reference-independent; what shim/rcn_hip.c and the stream driver below are thin
 * callers of).
 *
 * The reference decodes pictures on frame threads (ovdec_select_subdec, ovdec.c:188-248); a picture's frame lives in the DPB
 * from ovdpb_init_picture until the last picture referencing it and the output process have dropped it (dpb.c), and a frame
 * thread that needs rows of a reference picture waits on that picture's progress (ovdpb_synchro_ref_decoded_ctus,
 * dpb.c:1242-1270; rcn_inter.c:131-146), which the producer reports per CTU row (ovdpb_report_decoded_ctu_line,
 * dpb.c:1309-1323; slicedec.c:934-956).  On the device a picture is decoded by ONE flush at the end of its parse, so the
 * progress mask collapses to one transition per picture:
 *
 *   ovhip_dpb_begin    (rcn_attach_frame_buff)        DECODING: a device picture for `key` on device `dev`
 *   ovhip_dpb_publish  (after ovhip_job_wait)         DONE / FAILED: every waiter is released.  ONLY ovhip_job_wait marks a
 *                                                     picture complete: it may decode the picture a second time (ordered pass),
 *                                                     so nothing recorded after ovhip_job_flush is a "picture done" signal
 *   ovhip_dpb_acquire  (ovdpb_frame_synchro)          blocks until `key` is DONE (OVHIP_EREF if it FAILED), pins it, returns
 *                                                     the picture as device `dev` sees it
 *   ovhip_dpb_unpin                                   the reader's own decode has completed
 *   ovhip_dpb_release  (frame unreferenced)           the slot and its device memory return to the pool once nobody has it pinned
 *
 * `key` is opaque (the shim passes the OVFrame pointer).  A key handed to ovhip_dpb_begin while an older picture still owns it
 * releases that picture first: the reference's frame pool re-uses an OVFrame only after every reference to it was dropped.
 *
 * Several devices in ONE process (north_star: frames shard one per GPU, mirroring --framethr): a picture is decoded on its
 * `home` device; a device whose queued pictures list it (ovhip_dpb_want, called when such a picture BEGINS, i.e. as soon as its
 * reference lists are known -- slicedec.c:1250-1256) receives a copy over xGMI as soon as it is DONE: hipMemcpyPeerAsync on the
 * destination device's copy stream, one event per copy; ovhip_dpb_acquire hands the event to the reader, which waits for it
 * after its own uploads are under way.  Devices that never list the picture never receive it.
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_dpb ovhip_dpb;

/* Memory / copy back-end of a DPB.  ovhip_dpb_create installs the HIP one; ovhip_dpb_create_ex lets a test supply its own
 * (the state machine is plain C + pthreads and is exercised without a GPU that way; it never computes samples). */
typedef struct ovhip_dpb_ops {
    void *user;
    int  (*pic_alloc)(void *user, int dev, int32_t w, int32_t h, ovhip_pic *pic);        /* zero-filled, complete on return    */
    void (*pic_free)(void *user, int dev, ovhip_pic *pic);
    /* src (home device src_dev, complete) -> dst (dst_dev).  *event: handle for copy_wait / copy_done, or NULL = done already */
    int  (*copy_start)(void *user, int dst_dev, const ovhip_pic *dst, int src_dev, const ovhip_pic *src, void **event);
    int  (*copy_wait)(void *user, int dst_dev, void *event);                               /* blocks the calling thread          */
    void (*copy_done)(void *user, int dst_dev, void *event);                               /* the handle is no longer needed     */
    /* a picture whose last decode FAILED goes back to the pool: make it safe to decode into (no sample may carry bit 15) */
    int  (*pic_clear)(void *user, int dev, const ovhip_pic *pic);
    /* row progress (ovhip_dpb_post_rows): the handles are the producer's (hipEvent_t behind a band's last filter launch); query: 1 =
     * completed, 0 = not yet, < 0 error; wait blocks the calling thread.  NULL (test back-ends): a posted record counts as completed. */
    int  (*event_query)(void *user, int dev, void *event);
    int  (*event_wait)(void *user, int dev, void *event);
} ovhip_dpb_ops;

#define OVHIP_MAX_DEVICES 16
typedef struct ovhip_dpb_stats {
    uint32_t n_live, n_pool;             /* pictures owned by a key (home + copies) / waiting in the free pools            */
    uint64_t n_begin, n_alloc, n_recycled, n_copies, copy_bytes, n_failed;
    uint64_t n_waits;                    /* acquire calls that had to block                                                */
} ovhip_dpb_stats;

/* devices[i] = HIP device ordinal of logical device i (the same ordinal may appear twice: two logical devices on one GPU,
 * the peer copy is then a device-to-device copy -- how the multi-device path is tested on a one-GPU box). */
int  ovhip_dpb_create(ovhip_dpb **out, const int *devices, int n_devices);
int  ovhip_dpb_create_ex(ovhip_dpb **out, int n_devices, const ovhip_dpb_ops *ops);
void ovhip_dpb_destroy(ovhip_dpb *d);            /* frees every device picture; no thread may be inside a DPB call */
int  ovhip_dpb_n_devices(const ovhip_dpb *d);
int  ovhip_dpb_device(const ovhip_dpb *d, int dev);                 /* HIP ordinal of logical device dev, <0 if none     */
int  ovhip_dpb_begin(ovhip_dpb *d, const void *key, int dev, int32_t w, int32_t h, ovhip_pic *pic);
int  ovhip_dpb_want(ovhip_dpb *d, const void *key, int dev);
/* The same with the caller's picture identity (`tag`, 0 = none; the shim: coded video sequence + POC of the OVPicture).  The frame
 * pool recycles OVFrame pointers and frame threads run on their own: a reader can ask for key F while F's slot still holds the
 * PREVIOUS picture that lived in F (DONE), because the thread decoding the new one has not reached rcn_attach_frame_buff yet.  With
 * tags, a slot whose tag differs from the reader's is "not begun yet": ovhip_dpb_acquire_tag waits for the right picture (bounded
 * like an unknown key), ovhip_dpb_want_tag is remembered until ovhip_dpb_begin_tag(key, tag) picks it up. */
int  ovhip_dpb_begin_tag(ovhip_dpb *d, const void *key, uint64_t tag, int dev, int32_t w, int32_t h, ovhip_pic *pic);
int  ovhip_dpb_want_tag(ovhip_dpb *d, const void *key, uint64_t tag, int dev);
int  ovhip_dpb_acquire_tag(ovhip_dpb *d, const void *key, uint64_t tag, int dev, ovhip_pic *pic, void **event);
/* status 0: DONE, else FAILED (latched error of the producer): every exit path of a producer publishes */
int  ovhip_dpb_publish(ovhip_dpb *d, const void *key, int status);
/* *event (may be NULL when dev is the home device): a copy_wait handle the caller waits for before it reads pic, or NULL.
 * A key nobody has begun YET is waited for as well (frame threads start in decoding order but run on their own), for at most
 * ovhip_dpb_set_unknown_key_timeout milliseconds (default 10000; 0: do not wait) -- then OVHIP_EINVAL. */
void ovhip_dpb_set_unknown_key_timeout(ovhip_dpb *d, int ms);
int  ovhip_dpb_acquire(ovhip_dpb *d, const void *key, int dev, ovhip_pic *pic, void **event);
/* 1: the picture is DONE (an acquire would not wait for its decode), 0: not yet (unknown key, another picture under it, DECODING),
 * OVHIP_EREF: it failed.  Never blocks. */
int  ovhip_dpb_poll_tag(ovhip_dpb *d, const void *key, uint64_t tag);
/* ---- row progress: the device analogue of ovdpb_report_decoded_ctu_line / ovdpb_synchro_ref_decoded_ctus (dpb.c:1309-1323, :1242-1270)
 * for the pictures a band-wise job decodes (ovhip_job_band).
 * ovhip_dpb_post_rows (producer, picture DECODING): the picture's rows [0, rows) are final once `event` has completed and
 *   *abort_word (NULL: none) still reads 0.  Records are kept in order; rows must not decrease.
 * ovhip_dpb_rows_tag (reader): are the rows [0, need_rows) of the picture there for device dev?  1: yes -- *pic is the picture on dev
 *   (pin != 0: pinned, as by ovhip_dpb_acquire_tag; unpin with ovhip_dpb_unpin), *event (may be NULL) a transfer the caller still has
 *   to wait for (ovhip_dpb_wait_copy) when the picture was decoded on another device; 0: not yet (never with block != 0); OVHIP_EREF:
 *   the picture FAILED or the DPB was shut down.  A picture decoded on ANOTHER device is there only when it is complete (its transfer
 *   is picture-granular); need_rows >= the picture's height means the whole picture.  block != 0 waits -- for the producer's records
 *   on the DPB's condition variable, for a record's event through event_wait. */
int  ovhip_dpb_post_rows(ovhip_dpb *d, const void *key, int32_t rows, void *event, const volatile uint32_t *abort_word);
int  ovhip_dpb_rows_tag(ovhip_dpb *d, const void *key, uint64_t tag, int dev, int32_t need_rows, int block, int pin, ovhip_pic *pic, void **event);
int  ovhip_dpb_wait_copy(ovhip_dpb *d, int dev, void *event);
int  ovhip_dpb_unpin(ovhip_dpb *d, const void *key);
int  ovhip_dpb_release(ovhip_dpb *d, const void *key);
/* The home picture of a DONE key, without blocking (output path): OVHIP_EINVAL unknown, OVHIP_EREF not (yet) decoded. */
int  ovhip_dpb_lookup(ovhip_dpb *d, const void *key, int *home_dev, ovhip_pic *pic);
/* Wakes every waiter with OVHIP_EREF and makes every later wait fail at once (decoder teardown after an error). */
void ovhip_dpb_shutdown(ovhip_dpb *d);
int  ovhip_dpb_get_stats(ovhip_dpb *d, ovhip_dpb_stats *out);

/* ------------------------------------------------------------------------------------
 * Frame thread: one context (HIP stream) + one picture job on one logical device of a DPB -- what the shim keeps per
 * OVCTUDec.  Call order per picture:
 *
 *   ovhip_frame_begin(key)          rcn_attach_frame_buff: DPB slot + ovhip_job_begin, empty reference table
 *   ovhip_frame_ref(ref_key)        first use of a reference picture: its index in the table the recorded units carry
 *                                   (ovhip_pu_desc.ref0 / ref1); tells the DPB this device wants it
 *   ... the slots record into ovhip_frame_recorder() ...
 *   ovhip_frame_dmvr_rows_collect() every alf.rcn_alf_filter_line: the refined vectors / plane entries of the rows parsed before
 *   ovhip_frame_dmvr_rows_begin()   the last one; then the pass over the row just parsed is enqueued (waits for the references
 *                                   first) and runs while the next row is parsed (ovhip_frame_dmvr_rows: both at once)
 *   ovhip_frame_submit(params)      last row: uploads; waits for the references (host) while they run; launches;
 *                                   ovhip_job_wait (incl. its second pass); THEN publishes -- on every exit path, with the
 *                                   error if there was one -- and unpins the references; then the optional output (the
 *                                   picture's readers do not wait for it)
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_frame ovhip_frame;

enum { OVHIP_OUT_NONE = 0,     /* the picture stays on the device (readers: ovhip_dpb_lookup + ovhip_pic_output / _digest) */
       OVHIP_OUT_DIGEST = 1,   /* + ovhip_pic_digest into ovhip_frame_output.digest (16 bytes leave the device)           */
       OVHIP_OUT_PLANES = 2,   /* + the three planes into caller memory (the OVFrame: dectest.c:372-409 reads it there)   */
       OVHIP_OUT_PACKED = 3 }; /* + crop + pack on the device, ONE D2H into caller memory (ovhip_output_bytes() bytes)    */
typedef struct ovhip_frame_output {
    int32_t  mode;                       /* OVHIP_OUT_*                                                                    */
    ovhip_window window;                 /* DIGEST / PACKED                                                                */
    uint16_t *y, *cb, *cr; int32_t stride_y, stride_c;    /* PLANES: host pointers, strides in samples                     */
    void    *packed;                     /* PACKED: host pointer                                                           */
    uint8_t  digest[16];                 /* DIGEST: result                                                                 */
} ovhip_frame_output;

/* Event trace of the frame layer: one record per ovhip_frame_* call that changes a picture's state, for every frame of the process
 * -- WHEN a caller (the shim's hooks under the decoder's events, slicedec.c:934-956) begins a picture, names its references, runs
 * the eager DMVR rows, submits.  a / b: BEGIN: logical device; REF: table index; DMVR_*: refined units recorded so far (b of
 * DMVR_BEGIN: the pass covers a DMVR unit = the references were waited for); SUBMIT: refined units recorded, reference count;
 * FAIL: status.  result = what the call returned.  On a DPB made with ovhip_dpb_create_ex (no device) ovhip_frame_create makes DRY
 * frames: the same state machine, DPB calls, waits and trace, nothing launched -- how the shim's device half runs in a container
 * without a GPU (oracle/ref_harness/gen_pipe.c "device" mode -> tests/golden/shim_pipe_dev.ovg, replayed on a GPU by
 * tests/test_gpu_pipe.py). */
enum { OVHIP_FE_BEGIN = 1, OVHIP_FE_REF, OVHIP_FE_DMVR_ROWS, OVHIP_FE_DMVR_BEGIN, OVHIP_FE_DMVR_COLLECT, OVHIP_FE_SUBMIT, OVHIP_FE_FAIL,
       OVHIP_FE_BAND /* a = row_end, b = last, result: 1 the band went to the device, 0 left to the next call, < 0 error */ };
typedef struct ovhip_frame_event {
    uint32_t op; int32_t frame;          /* OVHIP_FE_*; the frame object, numbered in creation order                      */
    uint64_t key, tag;
    int64_t  a, b, result;
} ovhip_frame_event;
void ovhip_frame_set_trace(void (*sink)(void *user, const ovhip_frame_event *ev), void *user);    /* NULL: off */

int  ovhip_frame_create(ovhip_dpb *dpb, int dev, int32_t w, int32_t h, ovhip_frame **out);
void ovhip_frame_destroy(ovhip_frame *f);
ovhip_ctx      *ovhip_frame_ctx(ovhip_frame *f);
ovhip_job      *ovhip_frame_job(ovhip_frame *f);
ovhip_recorder *ovhip_frame_recorder(ovhip_frame *f);
int  ovhip_frame_begin(ovhip_frame *f, const void *key);
int  ovhip_frame_ref(ovhip_frame *f, const void *ref_key);          /* index (0..15) or <0 */
int  ovhip_frame_begin_tag(ovhip_frame *f, const void *key, uint64_t tag);       /* with the picture identity: ovhip_dpb_begin_tag */
int  ovhip_frame_ref_tag(ovhip_frame *f, const void *ref_key, uint64_t tag);
/* Same without the search for an existing entry: the table entry `slot` (= the number of entries so far) is ref_key, which may
 * already sit in another entry (a recorded picture whose units index a fixed table). */
int  ovhip_frame_ref_at(ovhip_frame *f, int slot, const void *ref_key);
int64_t ovhip_frame_dmvr_rows(ovhip_frame *f);
/* The two halves (ovhip_job_dmvr_rows_begin / _collect): _begin waits for the picture's reference pictures on the host (as
 * ovhip_frame_dmvr_rows does: only a published picture is complete, its ordered pass may run a second time), then enqueues the pass
 * over the units recorded so far and returns; _collect before the row those units belong to is reported decoded. */
/* 1: every reference picture named so far is complete (and now pinned: _begin / _submit will not wait for a decode), 0: not yet, < 0: one
 * failed.  Never waits for a decode: a caller that can go on parsing asks this before it starts a row pass. */
int  ovhip_frame_refs_ready(ovhip_frame *f);
int64_t ovhip_frame_dmvr_rows_begin(ovhip_frame *f, int32_t log2_ctu_s);
int64_t ovhip_frame_dmvr_rows_begin_upto(ovhip_frame *f, int32_t log2_ctu_s, size_t upto_units);
int64_t ovhip_frame_dmvr_rows_collect(ovhip_frame *f);
/* job: NULL = the frame's own job (the shim); else a job holding an already recorded picture of the same size, which is bound to
 * this frame's context for the flush (the stream driver's pre-recorded pictures).  intra: as ovhip_job_flush.  out: NULL =
 * OVHIP_OUT_NONE.  Returns the picture's status (what was published). */
int  ovhip_frame_submit(ovhip_frame *f, ovhip_job *job, const ovhip_pic *intra, const ovhip_job_params *params, ovhip_frame_output *out);
/* A picture that cannot be submitted (latched recorder error, unsupported tool): publishes it as FAILED so that no reader
 * waits for it for ever. */
/* ---- band-wise submission (the picture enters the device while it is parsed; see ovhip_job_band) ----
 * ovhip_frame_set_band_mode(f, 1): ovhip_frame_refs_ready / ovhip_frame_dmvr_rows_begin then ask the device DPB for the ROWS the units
 *   in question read (ovhip_dpb_rows_tag) instead of whole reference pictures.
 * ovhip_frame_band(f, params, row_end, last, out): everything recorded since the last band that went, as a band ending at the CTU-row
 *   boundary row_end.  Returns 1: enqueued (and the rows it made final posted to the DPB), 0: a reference picture does not have the rows
 *   yet -- nothing was enqueued, the next call takes this band's units too (never with last != 0, which waits), < 0: error.  With last
 *   != 0 the call completes the picture exactly as ovhip_frame_submit does: wait, publish, output. */
int  ovhip_frame_set_band_mode(ovhip_frame *f, int on);
int  ovhip_frame_band(ovhip_frame *f, const ovhip_job_params *params, int32_t row_end, int32_t last, ovhip_frame_output *out);
/* The same for a picture whose parse is AHEAD of its reference pictures (it has been recorded further than row_end): the band ends at the
 * recorder's array lengths `upto` (ovhip_rec_counts taken when row_end had just been parsed), and with block != 0 the call waits for the
 * reference rows instead of returning 0 -- how the picture's last hook works through the rows its references had not reached while it was
 * parsed, row by row as they arrive, so that ITS rows reach ITS readers as early (never the picture's last band: use ovhip_frame_band). */
int  ovhip_frame_band_upto(ovhip_frame *f, const ovhip_job_params *params, int32_t row_end, const ovhip_band_counts *upto, int32_t block);
int  ovhip_frame_band_stats(const ovhip_frame *f, int32_t *n_bands, int32_t *n_deferred);
/* Output at one size (what pp_process_frame does for the application when `upscale` is on, ovdec.c:479 / :523): while set, the DIGEST,
 * PACKED and PLANES outputs of ovhip_frame_submit and of the last ovhip_frame_band deliver the picture resampled to out_w x out_h
 * (the output's window applies to the resampled picture; for PLANES the caller's pointers describe planes of the output size).  What is
 * published to the DPB is the decoded picture, unchanged.  (0, 0) switches it off, which is the default; info is copied (NULL: no
 * scaling window, flags 0).  Refusals as ovhip_output_scale_check against the frame's size; a dry frame accepts the call and does nothing. */
int  ovhip_frame_set_output_scale(ovhip_frame *f, int32_t out_w, int32_t out_h, const ovhip_scale_info *info);
/* From now on the outputs OVHIP_OUT_DIGEST / _PLANES / _PACKED of this frame deliver the picture with film grain ("Film grain synthesis"
 * above) for the picture order count `poc`; params NULL switches it off.  What is published to the DPB stays the decoded picture:
 * references predict from it.  The model is derived afresh from a copy of *params for every picture (a non-persistent SEI); a caller
 * that holds ONE SEI struct across pictures and wants the reference's drift derives with ovhip_fg_derive and hands `after` to the next
 * call of this setter.  The refusals of ovhip_fg_derive come back from here.  OVHIP_EUNSUP while an output scale is set, and
 * ovhip_frame_set_output_scale answers OVHIP_EUNSUP while grain is set: the reference resamples the ungrained frame over the grained one
 * (post_proc.c:107-126).  A dry frame accepts the call and delivers nothing. */
int  ovhip_frame_set_film_grain(ovhip_frame *f, const ovhip_fg_params *params, int32_t poc);
/* Output at a REDUCED size ("Reduced-size output on the device" above): while set, every output of ovhip_frame_submit and of the last
 * ovhip_frame_band that shows the picture -- RGB, surface, ladder, DIGEST, PACKED, PLANES -- reads ONE reduced picture of out_w x out_h; their
 * windows, sizes and the caller's planes are those of the reduced size.  The picture hash and the motion field stay at the coded
 * picture, and what is published to the DPB is the decoded picture, unchanged.  (0, 0) switches it off, which is the default; info is
 * copied (NULL: no window, chroma_loc 0).  Refusals as ovhip_output_reduce_check against the frame's size.  A frame holds ONE post
 * setting: OVHIP_EUNSUP while film grain or an output scale is set, and those two setters answer OVHIP_EUNSUP while this is set.  A dry
 * frame accepts the call and does nothing. */
int  ovhip_frame_set_output_reduce(ovhip_frame *f, int32_t out_w, int32_t out_h, const ovhip_reduce_info *info);
/* Decoded picture hash ("Decoded picture hash" above) of every following picture: taken in ovhip_frame_submit and in the last
 * ovhip_frame_band AFTER ovhip_job_wait (a second pass of the ordered pass rewrites the picture), on the decoded picture as it is
 * published -- whatever the output mode, the output scale or the film grain setting are (those post-process a copy).  expected: what
 * the picture's SEI says (copied; NULL: compute only); it applies to the NEXT picture completed, so a caller sets it per picture.
 * method < 0 switches it off, which is the default.  A mismatch does NOT fail the picture: it is published as decoded and the caller
 * reads the verdict.  OVHIP_EINVAL for a method above 2, n_planes other than 1 or 3, an expectation of another method or plane count.
 * A dry frame accepts the call and computes nothing.  The frame trace has no event for it. */
int  ovhip_frame_set_picture_hash(ovhip_frame *f, int method, int n_planes, const ovhip_pic_hash_value *expected);
/* The last completed picture's hash into *computed (may be NULL).  1: computed, and equal to the expectation or none was given;
 * 0: it differs; OVHIP_EINVAL: nothing computed (yet). */
int  ovhip_frame_picture_hash(const ovhip_frame *f, ovhip_pic_hash_value *computed);
/* RGB output ("RGB output on the device" above) of the NEXT picture completed -- the destination is per picture, so a caller sets it
 * per picture; fmt NULL switches it off, which is the default.  The conversion runs in ovhip_frame_submit and in the last
 * ovhip_frame_band after ovhip_job_wait, on the picture the output shows -- after the frame's post-process step, so film grain and
 * the output scale compose with it (win is in chroma units of THAT picture) --, whatever out->mode is, OVHIP_OUT_NONE and a NULL out
 * included, and is complete on the device when the call returns.  What is published to the DPB is unchanged.  fmt and win are copied.
 * The format's refusals come back here, the launch's from the picture's last call: a failed conversion fails that call's return
 * value, never the picture's publication.  A dry frame accepts the call and does nothing. */
int  ovhip_frame_set_rgb_output(ovhip_frame *f, const ovhip_rgb_format *fmt, const ovhip_window *win, void *d_dst, size_t dst_bytes);
/* A colour table ("RGB output through a colour table" above) for the frame's RGB output.  Unlike the destination the setting is
 * STICKY: while a table is set, every RGB output of this frame goes through it (ovhip_rgb_lut_launch in the place of ovhip_rgb_launch,
 * after the post-process step: the window, film grain, the output scale and the reduced size compose with it); lut NULL switches it
 * off, which is the default, and the frame's calls are then what they were.  The table is borrowed: the caller keeps it alive while it
 * is set.  OVHIP_EINVAL for a table on another device than the frame's context; the launch's refusals (U8 with a peak above 255) come
 * from the picture's last call.  A dry frame accepts the call and does nothing. */
int  ovhip_frame_set_rgb_lut(ovhip_frame *f, const ovhip_rgb_lut *lut);
/* Surface output ("Surface output on the device" above) of the NEXT picture completed, exactly as the RGB output beside it: per
 * picture, fmt NULL switches it off (the default); the conversion runs in ovhip_frame_submit and in the last ovhip_frame_band after
 * ovhip_job_wait, on the picture the output shows (after the frame's post-process step; win is in chroma units of THAT picture),
 * whatever out->mode is, a NULL out included, and is complete on the device when the call returns.  What is published to the DPB is
 * unchanged; fmt and win are copied.  The format's refusals that need no picture (enum values, rsv, rounding, offset_c[1], pitch and
 * offset multiples, a null destination) come back here, the others from the picture's last call: a failed conversion fails that
 * call's return value, never the picture's publication.  A dry frame accepts the call and does nothing.  RGB and surface output are
 * independent: a frame with both set writes both.  Each of RGB output, surface output and delivery makes its own post-process step
 * (into the same scratch picture): with two of them the step runs twice, with all three three times. */
int  ovhip_frame_set_surface_output(ovhip_frame *f, const ovhip_surface_format *fmt, const ovhip_window *win, void *d_dst, size_t dst_bytes);
/* A colour table and a conversion ("Surface output through a colour table" above) for the frame's surface output.  STICKY, as
 * ovhip_frame_set_rgb_lut: while set, every surface output of this frame runs ovhip_surface_lut_launch in the place of
 * ovhip_surface_launch, after the post-process step (the window, film grain, the output scale and the reduced size compose with it);
 * lut NULL switches it off, which is the default, and the frame's calls are then what they were.  The table is borrowed, conv is
 * copied; the setting is independent of the RGB output's table (the same table may serve both).  OVHIP_EINVAL for a null conv beside a
 * table or a table on another device than the frame's context, the conversion's own refusals with their codes; the launch's refusals
 * (sizes that are not multiples of 4) come from the picture's last call.  A dry frame accepts the call and does nothing. */
int  ovhip_frame_set_surface_lut(ovhip_frame *f, const ovhip_rgb_lut *lut, const ovhip_surface_conv *conv);
/* Ladder output ("Output ladder on the device" above) of the NEXT picture completed, an output beside RGB and surface and independent
 * of them: per picture, rungs NULL switches it off (the default).  ovhip_ladder_launch runs in ovhip_frame_submit and in the last
 * ovhip_frame_band after the surface step and before the motion field, on the picture the outputs show -- after the frame's
 * post-process step, which still runs once per picture: film grain, the output scale or a first reduce compose in front of the
 * ladder, and info's window and the rungs' sizes are read against THAT picture --, whatever out->mode is, a NULL out included, and is
 * complete on the device when the call returns.  info (NULL: no window, chroma_loc 0) and the n rungs are copied; the rungs' dst are
 * DEVICE memory.  What needs no picture comes back here: n out of range, a null destination, a format's own refusals, and
 * ovhip_ladder_check against the size the post-process setting of the moment leaves (set that one first).  The others come from the picture's last call: a
 * failed ladder fails that call's return value, never the picture's publication, and writes nothing.  A dry frame accepts the call and
 * does nothing. */
int  ovhip_frame_set_ladder_output(ovhip_frame *f, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n);
/* A colour table and a conversion ("Output ladder through a colour table" above) for the frame's ladder output.  STICKY, exactly as
 * ovhip_frame_set_surface_lut: while set, the frame's ladder step runs ovhip_ladder_lut_launch in the place of ovhip_ladder_launch,
 * after the post-process step (film grain, the output scale or a first reduce compose in front of it); lut NULL switches it off, which
 * is the default, and the frame's calls and launches are then what they were.  The table is borrowed, conv is copied; the setting is
 * independent of the RGB output's table and of the surface output's (the same object may serve all three).  OVHIP_EINVAL for a null
 * conv beside a table or a table on another device than the frame's context, the conversion's own refusals with their codes.
 * conv->src_chroma_loc must be the ladder's info->chroma_loc: OVHIP_EINVAL from whichever of this setter and
 * ovhip_frame_set_ladder_output is called second (that one then asks ovhip_ladder_lut_check in the place of ovhip_ladder_check, so
 * rung sizes that are not multiples of 4 come back there too), and the launch makes the refusal again.  A dry frame accepts the call
 * and does nothing. */
int  ovhip_frame_set_ladder_lut(ovhip_frame *f, const ovhip_rgb_lut *lut, const ovhip_surface_conv *conv);
/* RGB pyramid output ("RGB pyramid on the device" above) of the NEXT picture completed, an output beside RGB, surface and ladder and
 * independent of them: per picture, levels NULL switches it off (the default).  ovhip_rgb_pyramid_launch runs in ovhip_frame_submit and
 * in the last ovhip_frame_band after the ladder step and before the motion field, on the picture the outputs show -- after the frame's
 * post-process step, which still runs once per picture: film grain, the output scale or a first reduce compose in front of the
 * pyramid, and info's window and the levels' sizes are read against THAT picture --, whatever out->mode is, a NULL out included, and
 * is complete on the device when the call returns.  info (NULL: no window, chroma_loc 0) and the n levels are copied; the levels' dst
 * are DEVICE memory.  What needs no picture comes back here: n out of range, a null destination, and ovhip_rgb_pyramid_check -- with
 * the table of ovhip_frame_set_rgb_pyramid_lut where one is set -- against the size the post-process setting of the moment leaves (set
 * that one first).  The others come from the picture's last call: a failed pyramid fails that call's return value, never the
 * picture's publication, and writes nothing.  A dry frame makes the same checks (it has a size, and never a table), accepts the call
 * and does nothing. */
int  ovhip_frame_set_rgb_pyramid_output(ovhip_frame *f, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n);
/* A colour table for the frame's RGB pyramid output.  STICKY, as ovhip_frame_set_rgb_lut: while set, the frame's pyramid step hands the
 * table to ovhip_rgb_pyramid_launch; lut NULL switches it off, which is the default.  The table is borrowed; the setting is independent
 * of the other outputs' tables (the same object may serve all).  OVHIP_EINVAL for a table on another device than the frame's context.
 * With a pyramid already set for the next picture this setter, being the second, asks ovhip_rgb_pyramid_check for those levels through
 * this table (a U8 level needs a peak of at most 255) and on a refusal leaves the setting as it was; ovhip_frame_set_rgb_pyramid_output
 * called second does the same.  A dry frame accepts the call and does nothing. */
int  ovhip_frame_set_rgb_pyramid_lut(ovhip_frame *f, const ovhip_rgb_lut *lut);
/* Motion field output ("Motion field output on the device" above) of the NEXT picture completed: per picture, fmt NULL switches it
 * off (the default); either destination may be NULL.  ovhip_job_mvfield runs in ovhip_frame_submit after a successful
 * ovhip_job_wait and after the picture's publication, on the job that decoded it -- a borrowed job goes back to its home context
 * only after it -- and is complete on the device when the call returns.  ref0 / ref1 of a cell are the k of ovhip_frame_ref /
 * ovhip_frame_ref_at.  The refusals that need no picture (format, both destinations NULL, alignment, overlap) come back here, the
 * sizes' from the picture's submit: a failed field fails that call's return value, never the picture's publication.  The setting
 * ends with the picture whatever happens, and a failed picture leaves the destinations untouched.  A dry frame accepts the call and
 * does nothing; a frame in band mode returns OVHIP_EUNSUP (and a setting made before band mode was switched on ends, unwritten, with
 * the band-wise picture). */
int  ovhip_frame_set_mvfield_output(ovhip_frame *f, const ovhip_mvfield_format *fmt, void *d_vec, size_t vec_bytes, void *d_info, size_t info_bytes);
int  ovhip_frame_fail(ovhip_frame *f, int status);
const char *ovhip_frame_last_error(const ovhip_frame *f);

/* ------------------------------------------------------------------------------------
 * Call log: the arguments of the recorder entry points of one picture (descriptors + the coefficient blocks they point to,
 * in the reference's layout), serialised in call order -- the compact pre-parsed form of a picture.  ovhip_calllog_replay
 * issues the same calls again: what a parse thread does per picture minus CABAC, used by the stream driver to put the
 * recorder into the timed region and by tools/micro/rec_throughput.c.
 * ---------------------------------------------------------------------------------- */
typedef struct ovhip_calllog ovhip_calllog;
ovhip_calllog *ovhip_calllog_create(void);
void   ovhip_calllog_destroy(ovhip_calllog *log);
void   ovhip_calllog_reset(ovhip_calllog *log);
const void *ovhip_calllog_data(const ovhip_calllog *log, size_t *bytes);
/* While a log is attached every ovhip_rec_tu / _tu_intra / _isp_cu / _pu / _affine_cu / _lmcs_region / _dbf_ctu /
 * _set_ctu_size call on `rec` is appended to it (NULL detaches).  The recorder's ovhip_rec_set_rpr_tools mask is written once per
 * log, right before the first call that takes a path it opens (an affine CU / a lone 4x4 luma PU on a scaled slot): a replay
 * opts its recorder in there, and the log of a stream without such calls holds no such record. */
void   ovhip_rec_set_calllog(ovhip_recorder *rec, ovhip_calllog *log);
/* Re-issues the calls of a serialised log on rec.  Returns the number of calls or <0 (first failing call's code). */
int64_t ovhip_calllog_replay(const void *data, size_t bytes, ovhip_recorder *rec);

/* ------------------------------------------------------------------------------------
 * Stream driver: decodes a whole stream of recorded pictures with N frame threads per device, in C (pthreads) -- the frame
 * thread pool of the reference (ovdec.c:188-248, --framethr) for the device path, and the timed region of bench.py.
 * Pictures are listed in DECODING order; a free thread of a picture's device takes the next picture of that device, records
 * it (OVHIP_STREAM_RECORD: replay of its call log into the thread's own job, as a parse thread would) or takes its
 * pre-recorded job, waits for its reference pictures (DPB), submits, publishes.  A picture is released from the DPB when the
 * last picture that lists it and the output thread are done with it.
 * ---------------------------------------------------------------------------------- */
#define OVHIP_STREAM_MAX_REFS 8
typedef struct ovhip_stream_content {      /* one recorded picture, shared by every stream picture that shows it */
    const void *calllog; size_t calllog_bytes;        /* OVHIP_STREAM_RECORD                                         */
    ovhip_job_params params;                          /* picture-level tables (host pointers, stay valid)            */
    uint32_t n_ref_slots;                             /* size of the reference table its units index (ref0 / ref1)    */
} ovhip_stream_content;

typedef struct ovhip_stream_pic {
    uint32_t content;                      /* index into contents[]                                                 */
    uint32_t job;                          /* pre-recorded mode: index into jobs[] (a job is in flight once at a time) */
    int32_t  poc;                          /* output order                                                          */
    uint16_t device;                       /* logical device it is decoded on                                       */
    uint16_t n_refs;
    uint32_t refs[OVHIP_STREAM_MAX_REFS];  /* indices (decoding order, < own) of its reference pictures: table slot k = refs[k % n_refs] */
    int32_t  owner;                        /* rank that decodes it (multi-process); != rank: arrives through xfer.recv   */
    uint32_t send_mask;                    /* ranks (bit r) it is sent to after decoding                            */
} ovhip_stream_pic;

typedef struct ovhip_stream_xfer {         /* multi-process exchange (one process per GPU): callbacks of the host harness */
    void *user;
    int (*send)(void *user, uint32_t idx, const ovhip_pic *pic, int dst_rank);     /* returns when the buffer may be reused */
    int (*recv)(void *user, uint32_t idx, const ovhip_pic *pic, int src_rank);     /* returns when the data is in place     */
} ovhip_stream_xfer;

/* RCCL transport (ovvc_rccl.hip): a ready-made ovhip_stream_xfer for one process per GPU -- the three planes of a picture as ncclSend /
 * ncclRecv in ONE ncclGroup per picture on a stream of its own, issued by the stream driver's communication thread; no collective.
 * librccl.so is opened at run time.  The launcher hands every rank the 128-byte ncclUniqueId rank 0 made (ovhip_rccl_unique_id),
 * e.g. through torch.distributed's broadcast (bench.py) or MPI.  ovhip_rccl_self_exchange: a one-rank check of the same path. */
typedef struct ovhip_rccl ovhip_rccl;
int  ovhip_rccl_unique_id(uint8_t out[128]);
int  ovhip_rccl_create(ovhip_rccl **out, const uint8_t unique_id[128], int rank, int world, int hip_device);
void ovhip_rccl_destroy(ovhip_rccl *r);
const ovhip_stream_xfer *ovhip_rccl_xfer(ovhip_rccl *r);
const char *ovhip_rccl_last_error(const ovhip_rccl *r);
int  ovhip_rccl_stats(const ovhip_rccl *r, uint64_t out[4]);      /* pictures sent, bytes sent, pictures received, bytes received */
int  ovhip_rccl_self_exchange(ovhip_rccl *r, const ovhip_pic *src, const ovhip_pic *dst);

enum { OVHIP_STREAM_RECORD = 1,            /* record every picture from its call log inside the run (else: pre-recorded jobs) */
       OVHIP_STREAM_DIGESTS = 2,           /* per-picture ovhip_pic_digest into result digests (16 bytes per picture)        */
       OVHIP_STREAM_RESIDENT = 4,          /* measurement: flushes replay the device copies (OVHIP_STAGE_RESIDENT)           */
       OVHIP_STREAM_KEEP = 8,              /* do not release pictures at the end of the run (the next run continues the stream) */
       OVHIP_STREAM_HOLD_ALL = 32,         /* (with OVHIP_STREAM_KEEP, given to the run that starts the stream) no picture is released before the
                                            * stream ends: every picture stays readable through ovhip_stream_key (tests)           */
       OVHIP_STREAM_FILE_MD5 = 16 };       /* OVHIP_OUT_PACKED: also hash the frames on the host (MD5 runs at ~0.6 GB/s per core: 40 ms per 4K
                                            * frame -- for conformance checks, not for throughput runs)                          */

typedef struct ovhip_stream_cfg {
    int32_t w, h;
    uint32_t flags;                        /* OVHIP_STREAM_*                                                         */
    int32_t threads_per_device;            /* frame threads (= pictures in flight) per logical device               */
    int32_t output;                        /* OVHIP_OUT_NONE / _DIGEST / _PACKED: an output thread takes the pictures in POC order */
    ovhip_window window;
    uint32_t extra_stages;                 /* OR-ed into every flush's stage mask (OVHIP_STAGE_INTRA_LEVELS ...)     */
    int32_t rank;                          /* this process's rank (pictures with owner != rank are received)         */
    const ovhip_stream_xfer *xfer;         /* NULL: single process                                                   */
    /* > 0: one more frame thread per device that takes pictures WITHOUT reference pictures (intra pictures) up to this many
     * pictures before their turn in decoding order -- such a picture is a dependency chain of milliseconds (ordered pass) that
     * everything after it waits for; started early it runs beside the pictures before it.  One extra picture buffer, no latency. */
    int32_t intra_lookahead;
    int32_t ahead_own_queue;               /* != 0: at creation, streams of in-order threads that share that thread's hardware queue are replaced
                                            * until none does (ovhip_ctx_shares_queue; ~2 ms per probe)                                     */
} ovhip_stream_cfg;

typedef struct ovhip_stream_result {
    double   seconds;                      /* first picture taken .. last picture published and devices idle        */
    uint64_t n_decoded, n_second_passes, n_received, n_sent;
    uint64_t out_frames, out_bytes;
    uint8_t  out_md5[16];                  /* OVHIP_OUT_PACKED + OVHIP_STREAM_FILE_MD5: MD5 of the concatenated frames in output order
                                            * = md5sum of the file dectest would write (CI/checkMD5.sh); OVHIP_OUT_DIGEST: MD5
                                            * over the pictures' digests (a private fingerprint)                            */
    double   record_seconds;               /* OVHIP_STREAM_RECORD: time spent replaying call logs, summed over threads */
    /* host seconds summed over the frame threads: the four phases of ovhip_job_stats.host_us_*, then inside ovhip_job_wait */
    double   host_seconds[5];
    int32_t  status;                       /* 0 or the first error                                                   */
    char     error[192];
    /* in: NULL, or room for 8 doubles per picture of the run -- seconds since the run began at which the picture was taken by a
     * frame thread, entered ovhip_frame_submit, was published (left it); the thread's index; then: its reference pictures were in
     * the thread's hands (uploads enqueued, references acquired), its launches were enqueued, ovhip_frame_submit returned (after
     * the output); one spare (analysis of stalls: tools/debug/dep_latency.py) */
    double  *trace;
} ovhip_stream_result;

typedef struct ovhip_stream ovhip_stream;
/* jobs: pre-recorded pictures (n_jobs may be 0 with OVHIP_STREAM_RECORD in every run).  The DPB, contents, jobs stay the
 * caller's.  Creates threads_per_device frames per device. */
int  ovhip_stream_create(ovhip_stream **out, ovhip_dpb *dpb, const ovhip_stream_cfg *cfg, const ovhip_stream_content *contents,
                         uint32_t n_contents, ovhip_job *const *jobs, uint32_t n_jobs);
void ovhip_stream_destroy(ovhip_stream *s);
/* Decodes pics[first .. first + n) of the stream pics[0 .. n_total) (indices and refs are positions in `pics`).  A call with
 * the same pics / n_total and first != 0 CONTINUES the stream of the previous call (which must have run with OVHIP_STREAM_KEEP:
 * its pictures are still in the DPB); anything else starts a new stream.  digests: n * 16 bytes or NULL.  flags: OVHIP_STREAM_*
 * of this run, OR-ed with the configuration's. */
int  ovhip_stream_run(ovhip_stream *s, const ovhip_stream_pic *pics, uint32_t n_total, uint32_t first, uint32_t n, uint32_t flags,
                      uint8_t *digests, ovhip_stream_result *res);
ovhip_frame *ovhip_stream_frame(ovhip_stream *s, int dev, int thread);
/* ahead_own_queue: streams replaced at creation / in-order streams that still share the look-ahead thread's hardware queue */
int  ovhip_stream_queue_info(const ovhip_stream *s, int *moved, int *sharing);
/* Output at one size: call it before a run.  The output thread's PACKED frames (its page-locked buffer, out_bytes, the file MD5) and the
 * frame threads' DIGEST fingerprints are those of the pictures resampled to out_w x out_h; (0, 0) switches it off.  The driver still
 * decodes pictures of one coded size (cfg.w x cfg.h). */
int  ovhip_stream_set_output_scale(ovhip_stream *s, int32_t out_w, int32_t out_h, const ovhip_scale_info *info);
/* Film grain for every picture of the following runs, each with its own ovhip_stream_pic.poc and a model derived afresh from *params
 * (ovhip_frame_set_film_grain); NULL: off.  The frames of OVHIP_OUT_PACKED -- and with them the MD5 of OVHIP_STREAM_FILE_MD5 -- and the
 * fingerprints of OVHIP_OUT_DIGEST are those of the grained pictures.  Refusals as the frame's setter. */
int  ovhip_stream_set_film_grain(ovhip_stream *s, const ovhip_fg_params *params);
/* Output at a reduced size for the following runs (ovhip_frame_set_output_reduce): call it before a run and before the setters of the
 * RGB and surface outputs, whose slots are then sized for out_w x out_h.  The output thread's PACKED frames and the frame threads'
 * DIGEST fingerprints are those of the reduced pictures; (0, 0) switches it off.  Refusals as the frame's setter. */
int  ovhip_stream_set_output_reduce(ovhip_stream *s, int32_t out_w, int32_t out_h, const ovhip_reduce_info *info);
/* Decoded picture hashes for the following runs: every frame thread hashes its own picture (ovhip_frame_set_picture_hash; nothing
 * goes through the output thread).  expected: one entry per picture of the stream (index in pics; the caller's array, read during the
 * runs) or NULL: compute only.  method < 0: off.  A mismatch leaves ovhip_stream_result.status at 0. */
int  ovhip_stream_set_picture_hashes(ovhip_stream *s, int method, int n_planes, const ovhip_pic_hash_value *expected);
/* Of the last run: computed (NULL, or room for its n pictures, in the order of pics), the number of pictures whose hash differed from
 * the expectation and the index in pics of the first of them (-1: none).  OVHIP_EINVAL when the last run computed none. */
int  ovhip_stream_picture_hashes(const ovhip_stream *s, ovhip_pic_hash_value *computed, uint32_t *n_mismatch, int32_t *first_mismatch);
/* RGB output for the following runs: picture idx of the stream (index in pics) lands at d_base + (idx % n_slots) * bytes_per_picture
 * in DEVICE memory, written by the frame thread that completes it (ovhip_frame_set_rgb_output; nothing goes through the output
 * thread), whatever the stream's output mode is.  fmt NULL: off.  OVHIP_EINVAL for a null base, n_slots 0 or a bytes_per_picture below
 * ovhip_rgb_bytes for the size the stream outputs (its output scale's, else its pictures'); the format's refusals as
 * ovhip_rgb_coefs.  A slot is the caller's to reuse once the picture n_slots later is decoded: the driver does not wait for a reader. */
int  ovhip_stream_set_rgb_output(ovhip_stream *s, const ovhip_rgb_format *fmt, const ovhip_window *win, void *d_base, size_t bytes_per_picture, uint32_t n_slots);
/* A colour table for the RGB output of the following runs (ovhip_frame_set_rgb_lut on every frame): one upload per device the stream
 * drives, through the context of that device's first frame; the stream owns the tables until the setting is cleared (host_table NULL)
 * or replaced, or the stream is destroyed.  host_table is not kept.  The refusals of ovhip_rgb_lut_create, the reason in
 * ovhip_last_error of that context; on a refusal the previous setting stands.  The slot size is still ovhip_rgb_bytes.  Between runs
 * only. */
int  ovhip_stream_set_rgb_lut(ovhip_stream *s, int size, int peak, const uint16_t *host_table);
/* Surface output for the following runs, as the RGB output above and independent of it: picture idx lands at
 * d_base + (idx % n_slots) * bytes_per_picture in DEVICE memory, written by the frame thread that completes it
 * (ovhip_frame_set_surface_output), whatever the stream's output mode is.  fmt NULL: off.  OVHIP_EINVAL for a null base, n_slots 0, a
 * format the frame's setter refuses, or a bytes_per_picture below ovhip_surface_bytes() for the size the stream outputs (its output
 * scale's, else its pictures').  A slot is the caller's to reuse once the picture n_slots later is decoded. */
int  ovhip_stream_set_surface_output(ovhip_stream *s, const ovhip_surface_format *fmt, const ovhip_window *win, void *d_base, size_t bytes_per_picture, uint32_t n_slots);
/* A colour table and a conversion for the surface output of the following runs (ovhip_frame_set_surface_lut on every frame), as
 * ovhip_stream_set_rgb_lut and independent of it: one upload per device, owned by the stream until the setting is cleared (host_table
 * NULL) or replaced, or the stream is destroyed; conv is copied.  The refusals of ovhip_rgb_lut_create and of the conversion; on a
 * refusal the previous setting stands.  The slot size is still ovhip_surface_bytes.  Between runs only. */
int  ovhip_stream_set_surface_lut(ovhip_stream *s, const ovhip_surface_conv *conv, int size, int peak, const uint16_t *host_table);
/* Ladder output for the following runs, as the surface output above and independent of it: rung r gives its base as rungs[r].dst and
 * its bytes per picture as rungs[r].dst_bytes, and rung r of picture idx lands at dst + (idx % n_slots) * dst_bytes in DEVICE memory,
 * written by the frame thread that completes it (ovhip_frame_set_ladder_output).  rungs NULL: off.  The refusals of ovhip_ladder_check
 * against the size the stream outputs (its output scale's or reduced size, else its pictures'); OVHIP_EINVAL for a null base,
 * n_slots 0, or a rung whose bytes per picture are below its surface's size. */
int  ovhip_stream_set_ladder_output(ovhip_stream *s, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n, uint32_t n_slots);
/* A colour table and a conversion for the ladder output of the following runs (ovhip_frame_set_ladder_lut on every frame), as
 * ovhip_stream_set_surface_lut and independent of it and of ovhip_stream_set_rgb_lut: one upload per device, owned by the stream until
 * the setting is cleared (host_table NULL) or replaced, or the stream is destroyed; conv is copied.  The refusals of
 * ovhip_rgb_lut_create and of the conversion, and -- from whichever of this setter and ovhip_stream_set_ladder_output is called second --
 * those of ovhip_ladder_lut_check for the ladder set; on a refusal the previous setting stands.  The rungs' slot sizes are still
 * ovhip_surface_bytes.  Between runs only. */
int  ovhip_stream_set_ladder_lut(ovhip_stream *s, const ovhip_surface_conv *conv, int size, int peak, const uint16_t *host_table);
/* RGB pyramid output for the following runs, as the ladder output above and independent of it: level r gives its base as
 * levels[r].dst and its bytes per picture as levels[r].dst_bytes, and level r of picture idx lands at dst + (idx % n_slots) * dst_bytes
 * in DEVICE memory, written by the frame thread that completes it (ovhip_frame_set_rgb_pyramid_output).  levels NULL: off.  The refusals
 * of ovhip_rgb_pyramid_check -- through the table of ovhip_stream_set_rgb_pyramid_lut where one is set -- against the size the stream
 * outputs (its output scale's or reduced size, else its pictures'); OVHIP_EINVAL for a null base, n_slots 0, or a level whose bytes
 * per picture are below its tensor's size or no multiple of its element.  On a refusal the previous setting stands. */
int  ovhip_stream_set_rgb_pyramid_output(ovhip_stream *s, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n, uint32_t n_slots);
/* A colour table for the RGB pyramid output of the following runs (ovhip_frame_set_rgb_pyramid_lut on every frame), as
 * ovhip_stream_set_rgb_lut and independent of it: one upload per device, owned by the stream until the setting is cleared (host_table
 * NULL) or replaced, or the stream is destroyed.  The refusals of ovhip_rgb_lut_create and -- from whichever of this setter and
 * ovhip_stream_set_rgb_pyramid_output is called second -- those of ovhip_rgb_pyramid_check for the pyramid set; on a refusal the
 * previous setting stands.  Between runs only. */
int  ovhip_stream_set_rgb_pyramid_lut(ovhip_stream *s, int size, int peak, const uint16_t *host_table);
/* Motion field output for the following runs: the vectors of picture idx land at d_vec_base + (idx % n_slots) *
 * vec_bytes_per_picture, its info at d_info_base + (idx % n_slots) * info_bytes_per_picture, in DEVICE memory, written by the frame
 * thread that completes it (ovhip_frame_set_mvfield_output).  Either base may be NULL (not wanted).  fmt NULL: off.  OVHIP_EINVAL
 * for both bases NULL, n_slots 0, a format the frame's setter refuses, or a wanted destination whose bytes per picture are below
 * ovhip_mvfield_bytes() for the stream's picture size or no multiple of its element.  A slot is the caller's to reuse once the
 * picture n_slots later is decoded. */
int  ovhip_stream_set_mvfield_output(ovhip_stream *s, const ovhip_mvfield_format *fmt, void *d_vec_base, size_t vec_bytes_per_picture,
                                     void *d_info_base, size_t info_bytes_per_picture, uint32_t n_slots);
/* The DPB key of picture idx of the current stream (valid while the run that decoded it kept it: OVHIP_STREAM_KEEP). */
const void *ovhip_stream_key(const ovhip_stream *s, uint32_t idx);
/* test hook: the next flush of `job` that has a flow launch is ABORTED for real (the device's abort word is set before the
 * launch, so the first pass leaves the picture incomplete) -- ovhip_job_wait must then produce the picture with its second pass */
int  ovhip_job_test_abort_next_flow(ovhip_job *job);

#ifdef __cplusplus
}
#endif
#endif /* OVVC_HIP_H */
