/* x264hip_mbanalyse.h — the intra mode decision on the device: x264_mb_analyse_intra and
 * mb_analyse_intra_chroma (reference encoder/analyse.c:586-980) with the decisions of
 * x264_macroblock_analyse around them (:2939-2946 for I, :3181-3223 for P, :3591-3618 for B
 * pictures), followed by the encode of the macroblocks that come out intra, exactly as
 * x264hip_*_mb_encode_intra (x264hip_mbintra.h) would do it with those modes.  It takes that
 * entry's place in the chain
 *   mb_mc -> mb_encode_inter -> mb_analyse_intra -> [mb_skip_convert ->] deblock_strength -> deblock_frames
 * and works in place in the same wavefront, because the analysis of a macroblock predicts from
 * the final reconstruction of its neighbours.
 *
 * The configuration: a->i_mbrd = 0; i_subpel_refine 2..5, so mbcmp is SATD and the 8x8 metric sa8d
 * (encoder/encoder.c:1409-1418); intra_mbcmp_x9_4x4 / _8x8 NULL, the C path (what x264 runs under
 * b_cpu_independent, encoder.c:1419-1422); b_lossless = 0, i_avcintra_class = 0,
 * b_avoid_topright = 0, i_satd_pcm = COST_MAX (I_PCM is never chosen), b_early_terminate = 1,
 * constrained_intra_pred = 0; one slice per picture; chroma formats 0, 1 and 2; COST_MAX = 1 << 28;
 * all cost arithmetic int32.
 *
 * Per macroblock (mb_flags and try_intra):
 *   try_intra == 0, not X264HIP_MBENC_INTRA: not touched in any array or pixel;
 *   try_intra == 0, X264HIP_MBENC_INTRA: encoded with its given type bits and modes as
 *     x264hip_*_mb_encode_intra does; decided and given macroblocks share the wavefront, and a
 *     call with no try macroblock equals x264hip_*_mb_encode_intra;
 *   try_intra != 0: analysed.  lambda = lambda_tab[qp]; i_satd_inter = COST_MAX on an I picture,
 *     satd_inter[mb] otherwise.
 *     I picture: mb_analyse_intra( COST_MAX ); I_16x16, then I_4x4 if <, then I_8x8 if <; then the
 *       chroma analysis.
 *     P / B picture: with b_chroma_me at formats 1 and 2 the chroma analysis runs first, luma gets
 *       i_satd_inter - i_satd_chroma and the three costs get += i_satd_chroma; then against
 *       i_satd_inter I_16x16, I_8x8, I_4x4, each with <, in that order; a macroblock none of them
 *       beats stays inter: only cost[mb] and mb_flags_out[mb] (= mb_flags[mb]) are written, its
 *       inter encode stands.  Without chroma ME the chroma analysis runs for the macroblocks that
 *       come out intra.  B pictures add lambda * i_mb_b_cost_table[type] to each type's cost.
 *     Decided intra: mb_flags_out[mb] = X264HIP_MBENC_INTRA, plus X264HIP_MBENC_T8x8 for I_8x8 or
 *       X264HIP_MBINTRA_I16x16 for I_16x16; pred_mode[mb][0..15] and chroma_pred_mode[mb] are
 *       written in mb_encode_intra's convention (I_16x16: entry 0 the mode, the others
 *       I_PRED_4x4_DC; I_8x8: block i's mode in entries 4*i .. 4*i+3); every output element and
 *       pixel of the macroblock is written as x264hip_mbintra.h specifies; flags_out is the decided
 *       flags & 3.
 *   cost[mb][0..3] = i_satd_i16x16, i_satd_i8x8, i_satd_i4x4, i_satd_chroma as they stand at the
 *     decision, for every try macroblock: COST_MAX for a pass that did not run or left early
 *     (plus the chroma cost on the chroma-ME leg, as the C leaves it); i_satd_chroma is COST_MAX
 *     where the chroma analysis did not run (a macroblock that stays inter without chroma ME) and 0
 *     where it ran at format 0.
 * b_fast_intra (analyse.c:446-458) depends on the neighbours' types and on running counts in
 * raster order, state a wavefront does not hold: it is the caller's input, fast_intra[mb].
 * The predicted 4x4 / 8x8 mode across macroblocks follows x264_macroblock_cache_save
 * (common/macroblock.c:1727-1737): only an I_4x4 neighbour hands over its modes, every other
 * neighbour inside the picture I_PRED_4x4_DC, one outside the picture -1.  A neighbour's type is
 * mb_flags_out of a try macroblock, mb_flags of any other.
 *
 * The contract, footprint and alignment rules, the error convention and the 2^28 limit are
 * x264hip_*_mb_encode_intra's; a try macroblock's own prior recon content never reaches a result.
 * One launch per macroblock anti-diagonal, analysis and encode in one kernel; asynchronous on
 * `stream`, no host synchronisation and no allocation, so it can be captured into a graph.
 */
#ifndef X264HIP_MBANALYSE_H
#define X264HIP_MBANALYSE_H

#include "x264hip_mbintra.h"

#ifdef __cplusplus
extern "C" {
#endif

#define X264HIP_COST_MAX (1 << 28)

typedef struct x264hip_mbanalyse_t
{
    /* as x264hip_mbintra_t */
    int32_t chroma_format;            /* 0 (luma only), 1 (4:2:0), 2 (4:2:2) */
    int32_t b_dct_decimate;
    const uint8_t *chroma_qp_table;   /* HOST */
    const void *quant4_mf, *quant4_bias;
    const void *quant8_mf, *quant8_bias;   /* all three of quant8_mf, quant8_bias, dequant8_mf may be NULL */
    const int32_t *dequant4_mf;
    const int32_t *dequant8_mf;
    const void *fenc;         intptr_t fenc_stride, fenc_frame_stride;
    const void *fenc_chroma;  intptr_t fenc_chroma_stride, fenc_chroma_frame_stride;
    void *recon;              intptr_t recon_stride, recon_frame_stride;               /* in and out */
    void *recon_chroma;       intptr_t recon_chroma_stride, recon_chroma_frame_stride; /* in and out */
    const int8_t  *qp;
    const uint8_t *mb_flags;
    int8_t  *pred_mode;               /* [mb][16]: read for given-mode intra macroblocks, written for decided ones */
    int8_t  *chroma_pred_mode;        /* [mb]; not used when chroma_format == 0 */
    void    *level;
    void    *chroma_dc;
    uint8_t *nnz;
    int32_t *cbp;
    int32_t *nz;
    uint8_t *flags_out;
    void    *luma_dc;
    /* the decision */
    int32_t slice_type;               /* 0 I, 1 P, 2 B */
    int32_t i_subpel_refine;          /* h->mb.i_subpel_refine, 2..5 */
    int32_t b_i4x4;                   /* X264_ANALYSE_I4x4 of the slice type's flag set */
    int32_t b_i8x8;                   /* X264_ANALYSE_I8x8; needs the 8x8 tables */
    int32_t b_chroma_me;              /* h->mb.b_chroma_me; read for P / B pictures at formats 1 and 2 */
    const uint16_t *lambda_tab;       /* HOST: x264_lambda_tab[0 .. QP_MAX_SPEC], read during the call */
    const uint8_t *try_intra;         /* [mb], nonzero: analyse this macroblock */
    const int32_t *satd_inter;        /* [mb], 0 .. COST_MAX; read for try macroblocks of P / B pictures; may be NULL at slice_type 0 */
    const uint8_t *fast_intra;        /* [mb], nonzero: a->b_fast_intra; NULL: 0 everywhere */
    uint8_t *mb_flags_out;            /* [mb], written for try macroblocks; may be mb_flags itself */
    int32_t *cost;                    /* [mb][4], written for try macroblocks */
} x264hip_mbanalyse_t;

/* a: host struct, read during the call (chroma_qp_table and lambda_tab included).  X264HIP_OK and
 * no launch for zero macroblocks.  X264HIP_EINVAL before any HIP call: what x264hip_*_mb_encode_intra
 * refuses, and a NULL lambda_tab, try_intra, cost or mb_flags_out; slice_type outside 0..2;
 * i_subpel_refine outside 2..5; a NULL satd_inter at slice_type 1 or 2; cost off a 4-byte boundary;
 * b_i8x8 without the 8x8 tables.  X264HIP_ENODEV without a device. */
int x264hip_8_mb_analyse_intra ( const x264hip_mbanalyse_t *a, int mb_width, int mb_height, int n_frames, void *stream );
int x264hip_10_mb_analyse_intra( const x264hip_mbanalyse_t *a, int mb_width, int mb_height, int n_frames, void *stream );

#ifdef __cplusplus
}
#endif

#endif /* X264HIP_MBANALYSE_H */
