/* x264hip_mbskip.h — P_SKIP / B_SKIP on the device: the one decision the chain
 *   mb_mc -> mb_encode_inter -> mb_encode_intra -> deblock_strength -> deblock_frames -> hpel_filter
 * (x264hip_mc.h, x264hip_mbenc.h, x264hip_mbintra.h, x264hip_deblock.h) left to the host.  Three
 * entries, each for every macroblock of n_frames frames in one launch, from the motion field as
 * macroblock_cache_save leaves it (the h->mb.mv / h->mb.ref layout of x264hip_deblock_strength_t):
 *
 *   x264hip_mb_predict_mv_pskip   x264_mb_predict_mv_pskip (reference common/mvpred.c:166-181,
 *                                 through x264_mb_predict_mv_16x16, :129-163): the skip vector;
 *   x264hip_*_mb_probe_skip       x264_macroblock_probe_skip (encoder/macroblock.c:985-1139): "does
 *                                 this macroblock code nothing at its skip vector (P) / at its direct
 *                                 prediction (B)", with the probe's own thresholds;
 *   x264hip_mb_skip_convert       the P_SKIP / B_SKIP conversion of macroblock.c:953-971, after
 *                                 mb_encode_inter.
 *
 * The caller's loops: for every P picture mb_predict_mv_pskip -> mb_probe_skip;
 * then mb_mc (a skip macroblock is its 16x16 list-0 block at the skip vector) -> mb_encode_inter
 * -> mb_skip_convert.
 *
 * All three: progressive frames, one slice per picture (a neighbour is available by its position
 * in the picture, as in mb_encode_intra); device arrays dense (stride = mb_width) and frame-major;
 * n_frames * mb_width * mb_height <= 2^28; X264HIP_OK and no launch for zero macroblocks;
 * asynchronous on `stream` (a hipStream_t, NULL = the null stream), no host synchronisation and no
 * allocation, so they can be captured into a graph; 0 or a negative X264HIP_E*.
 *
 * 1. mb_predict_mv_pskip (bit-depth independent).  mv0 int16 [frame][4*mbh][4*mbw][2], ref0 int8
 *    [frame][2*mbh][2*mbw]: list 0; an intra macroblock holds ref -1 and mv 0, a P_SKIP macroblock
 *    ref 0 and its skip vector.  For macroblock (x, y):
 *      a (left)       x > 0                 ref0[2y][2x-1]    mv0[4y][4x-1]
 *      b (top)        y > 0                 ref0[2y-1][2x]    mv0[4y-1][4x]
 *      c (top right)  y > 0 && x < mbw-1    ref0[2y-1][2x+2]  mv0[4y-1][4x+4]
 *      c fallback     y > 0 && x > 0        ref0[2y-1][2x-1]  mv0[4y-1][4x-1]   (top left)
 *    An unavailable neighbour has ref -2 and mv 0; nothing is read across a frame boundary of the
 *    batch.  pskip_mv[mb] = 0 when a or b is unavailable, or ref_a == 0 && mv_a == 0, or
 *    ref_b == 0 && mv_b == 0; otherwise the 16x16 predictor for i_ref 0: more than one of the three
 *    refs equal to 0: the component-wise median; exactly one: that neighbour's mv; none: mv_a when
 *    ref_b == -2 && ref_c == -2 && ref_a != -2, else the median.
 *
 * 2. mb_probe_skip, b_noise_reduction = 0, chroma formats 0, 1 (4:2:0), 2 (4:2:2), 3 (4:4:4).  It
 *    writes skip[mb] (1 = can be coded as a skip) and nothing else: no pixel.
 *    b_bidir = 0 (x264_macroblock_probe_pskip): pskip_mv[mb] is clipped to h->mb.mv_min / mv_max
 *      of the macroblock's position (analyse.c:336-337, 391-392: 24 pixels past the frame, in
 *      quarter pixels), so every read stays inside the 32-pixel luma / 16-pixel chroma padding
 *      under x264hip_mc.h's contract.  Prediction: luma mc_luma 16x16 of `ref` with weight[0]; at
 *      4:4:4 mc_luma of the U and V plane sets with weight[1] / weight[2]; at 4:2:0 / 4:2:2
 *      mc_chroma( mvx, mvy << c422 ), then weight[1] on U and weight[2] on V where `weighted` (the
 *      reference's mv-0 branch, load_deinterleave_chroma_fdec, equals mc_chroma at mv 0).
 *    b_bidir = 1 (x264_macroblock_probe_bskip): the prediction is read from pred / pred_chroma,
 *      the planes x264hip_*_mb_mc wrote for the direct prediction; ref, weight and pskip_mv are
 *      ignored.  Every macroblock is probed: the value for a macroblock whose pred is not its
 *      direct prediction means nothing to the caller, but it is defined.
 *    The test, with qpc = chroma_qp_table[qp].  The reference returns early from inside its loops;
 *    every one of those returns compares a running sum of non-negative scores with a bound, or
 *    tests an any-nonzero flag, so the result does not depend on the order in which they fire.
 *    That is what lets every block of a macroblock be scored at once:
 *      luma_ok(p)    = sum over the plane's 16 4x4 blocks of decimate_score16( scan_4x4(
 *                      quant_4x4( sub4x4_dct ) ) ) < 6; p = 0 with CQM_4PY at qp; at 4:4:4 also
 *                      p = 1, 2 with CQM_4PC at qpc, each plane with its own sum;
 *      thresh        = (x264_lambda2_tab[qpc] + 32) >> 6 at 4:2:0, (.. + 16) >> 5 at 4:2:2;
 *      chroma_ok(ch) = ssd(ch) < thresh
 *                      || ( every quant_2x2_dc( sub8x8_dct_dc or the halves of sub8x16_dct_dc,
 *                           mf[CQM_4PC][qpc + 3*c422][0] >> 1, bias[..][0] << 1 ) == 0
 *                           && ( ssd(ch) < 4 * thresh
 *                                || sum over the channel's 4 (4:2:2: 8) blocks of decimate_score15(
 *                                   scan_4x4( quant_4x4( sub4x4_dct, DC zeroed, CQM_4PC at qpc ) ) ) < 7 ) );
 *      skip          = every luma_ok && ( format 0 or 3 || ( chroma_ok(U) && chroma_ok(V) ) ).
 *
 * 3. mb_skip_convert (bit-depth independent).  flags[mb] = mb_flags[mb], with X264HIP_MBENC_SKIP
 *    also set for a converted macroblock; flags may be mb_flags itself.
 *    b_bframe = 0: converted when not intra, not already skip, X264HIP_MBENC_D16x16 set,
 *      (cbp & 0x3f) == 0, ref0[2y][2x] == 0 and mv0[4y][4x] == pskip_mv[mb];
 *    b_bframe = 1: converted when direct[mb] != 0 (B_DIRECT), not intra and (cbp & 0x3f) == 0.
 *
 * Not included: the wavefront that interleaves probe and search (analyse.c:1294-1307, 3002-3013);
 * direct vectors; noise reduction; several slices; MBAFF; the frame-thread limit on mv_max[1];
 * b_skip_mc's hand-over of the prediction (the probe writes no pixel: a skip macroblock is
 * mb_mc's 16x16 list-0 block at the skip vector, as before).
 */
#ifndef X264HIP_MBSKIP_H
#define X264HIP_MBSKIP_H

#include "x264hip_mbenc.h"
#include "x264hip_mc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct x264hip_mbskip_t
{
    int32_t chroma_format;            /* 0 (luma only), 1 (4:2:0), 2 (4:2:2), 3 (4:4:4) */
    int32_t b_bidir;                  /* 0: the P leg, 1: the B leg */
    const uint8_t *chroma_qp_table;   /* HOST: h->chroma_qp_table[0 .. QP_MAX_SPEC], read during the call;
                                         every entry <= QP_MAX_SPEC (- 3 at 4:2:2) */
    /* device tables as x264hip_*_cqm_init writes them (udctcoef [4][QP_MAX_SPEC+1][16]); only the
       CQM_4PY and CQM_4PC rows are read */
    const void *quant4_mf, *quant4_bias;
    /* pixel (0,0) of frame 0, strides in pixels */
    const void *fenc;             intptr_t fenc_stride, fenc_frame_stride;
    const void *fenc_chroma[2];   intptr_t fenc_chroma_stride, fenc_chroma_frame_stride;
                                      /* 4:2:0 / 4:2:2: [0] = the interleaved NV12 / NV16 plane; 4:4:4: U, V */
    /* b_bidir = 0: reference 0 of list 0 as x264hip_mc_t takes it, h->sh.weight[0][0..2], the skip vectors */
    x264hip_mc_ref_t ref;
    intptr_t ref_stride, ref_frame_stride, ref_chroma_stride, ref_chroma_frame_stride;
    x264hip_weight_t weight[3];
    const int16_t *pskip_mv;          /* device [mb][2] */
    /* b_bidir = 1: x264hip_mc_t's pred / pred_chroma */
    const void *pred;             intptr_t pred_stride, pred_frame_stride;
    const void *pred_chroma[2];   intptr_t pred_chroma_stride, pred_chroma_frame_stride;
    const int8_t *qp;                 /* device [mb]: h->mb.i_qp, 0..QP_MAX_SPEC */
    uint8_t *skip;                    /* device [mb], the output */
} x264hip_mbskip_t;

/* mv0, ref0, pskip_mv: device arrays.  X264HIP_EINVAL: a NULL array, a negative size, more than
 * 2^28 macroblocks, mv0 or pskip_mv off a 4-byte boundary (an mv is loaded and stored as one
 * dword).  X264HIP_ENODEV without a device. */
int x264hip_mb_predict_mv_pskip( const int16_t *mv0, const int8_t *ref0, int mb_width, int mb_height, int n_frames,
                                 int16_t *pskip_mv, void *stream );

/* s: host struct, read during the call (chroma_qp_table included: QP_MAX_SPEC + 1 = 52 entries at
 * 8 bit, 64 at 10 bit).  X264HIP_EINVAL: a NULL s, chroma_qp_table, quant4_mf, quant4_bias, fenc, qp
 * or skip; chroma_format outside 0..3; a NULL fenc_chroma the format needs; with b_bidir = 0 a NULL
 * ref.luma[k], ref.chroma[k] the format needs or pskip_mv, pskip_mv off a 4-byte boundary, an
 * interleaved reference chroma plane off a (U, V) pair or with an odd stride, a weight with denom
 * outside 0..7; with b_bidir = 1 a NULL pred or pred_chroma the format needs; a chroma_qp_table
 * entry above QP_MAX_SPEC (QP_MAX_SPEC - 3 at 4:2:2); a negative size; more than 2^28
 * macroblocks.  X264HIP_ENODEV without a device. */
int x264hip_8_mb_probe_skip ( const x264hip_mbskip_t *s, int mb_width, int mb_height, int n_frames, void *stream );
int x264hip_10_mb_probe_skip( const x264hip_mbskip_t *s, int mb_width, int mb_height, int n_frames, void *stream );

/* mb_flags, cbp (x264hip_mbenc_t's), mv0, ref0, pskip_mv, direct (uint8 per macroblock, nonzero =
 * B_DIRECT; may be NULL when b_bframe == 0), flags: device arrays.  X264HIP_EINVAL: a NULL
 * mb_flags, cbp or flags; with b_bframe == 0 a NULL mv0, ref0 or pskip_mv; b_bframe with a NULL
 * direct; cbp, or with b_bframe == 0 mv0 or pskip_mv, off a 4-byte boundary; a negative size; more
 * than 2^28 macroblocks.  X264HIP_ENODEV without a device. */
int x264hip_mb_skip_convert( const uint8_t *mb_flags, const int32_t *cbp, const int16_t *mv0, const int8_t *ref0,
                             const int16_t *pskip_mv, int b_bframe, const uint8_t *direct, int mb_width,
                             int mb_height, int n_frames, uint8_t *flags, void *stream );

#ifdef __cplusplus
}
#endif

#endif /* X264HIP_MBSKIP_H */
