/* x264hip_mc.h — batched motion compensation on the device: x264_mb_mc (reference
 * common/macroblock.c:31-246) for a list of equally sized partitions, built from mc_luma, get_ref,
 * mc_chroma, mc_weight and the avg table (common/mc.c:49-283).  Progressive frames, 8 and 10 bit.
 *
 * The inputs are what the batched searches of x264hip.h leave in device memory (one motion vector
 * per partition) and the reference's half-pel planes; the output is the prediction the residual
 * entries read (x264hip_*_mb_dct_quant's `pred`, x264hip_*_mb_dequant_idct_add's `pred`), so
 * search -> prediction -> residual -> reconstruction stays on the device.
 *
 * Per block (i_pixel = PIXEL_16x16 .. PIXEL_4x4, one size per call):
 *   pos[3*i]  = { frame, x, y }: the block's top-left luma pixel (the searches' layout), x and y
 *               multiples of 4;
 *   par[8*i]  = { mv0 x, y, mv1 x, y, mv_min x, y, mv_max x, y } in quarter pixels: each used mv is
 *               clipped to h->mb.mv_min / mv_max first (macroblock.c:41-42); the mv of an unused
 *               list is ignored;
 *   mode[i]   = lists | (i_weight << 8): lists 1 = list 0, 2 = list 1, 3 = both; i_weight =
 *               h->mb.bipred_weight (signed, read when lists == 3).  mode == NULL: list 0 everywhere
 *               (a P slice).
 *   lists 1:  luma = mc_luma with weight[0] (the qpel average first, then the weight); chroma at
 *             4:2:0 / 4:2:2 = mc_chroma( mvx, 2*mvy >> v_shift ) of the interleaved plane, then
 *             weight[1] on U and weight[2] on V where `weighted`; at 4:4:4 mc_luma of the U and V
 *             plane sets with weight[1] / weight[2].
 *   lists 2:  the same from list 1, unweighted (x264_weight_none).
 *   lists 3:  unweighted get_ref of both lists joined by mc.avg: i_weight 32 = the rounding
 *             average, else pixel_avg_weight_wxh with its clip; chroma = mc_chroma (get_ref at
 *             4:4:4) of both lists joined the same way.
 *   mc_weight: offset scaled by 1 << (BIT_DEPTH-8); denom >= 1 rounds, denom 0 does not
 *             (mc.c:117-137).  The chroma block of a 4x4 luma block is 2x2 at 4:2:0 (8x4: 4x2,
 *             4x8: 2x4).
 * Not included: the MB_INTERLACED chroma offset, and deriving skip / direct vectors (the caller
 * passes the mv; P_SKIP is a 16x16 list-0 block at the vector x264hip_mb_predict_mv_pskip of
 * x264hip_mbskip.h derives; direct vectors are the caller's).
 *
 * Contract: blocks of one call must not overlap in `pred`; pixels no block covers are not written
 * and `pred` is never read.  The contents of the device arrays are the caller's contract.  With
 * the mv limits of analyse.c:330-349 (mv_min / mv_max reach 24 pixels past the frame) every read
 * stays inside planes padded by PAD = 32 luma pixels and 16 chroma pixels on every side,
 * mc_chroma's extra row and column and the dword a misaligned row load rounds up to included.
 * Strides are in pixels (interleaved chroma: in samples of the interleaved plane).  pred,
 * pred_chroma[] and their strides are multiples of 4 pixels (blocks are stored as whole dwords),
 * reference strides and the reference chroma pointers multiples of 2.
 *
 * Asynchronous on `stream` (a hipStream_t, NULL = the null stream), no host synchronisation;
 * 0 or a negative X264HIP_E*.
 */
#ifndef X264HIP_MC_H
#define X264HIP_MC_H

#include "x264hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct x264hip_mc_ref_t            /* one reference picture, pointers at pixel (0,0) of frame 0 */
{
    const void *luma[4];                    /* F, H, V, C (hpel_filter's planes), common stride */
    const void *chroma[8];                  /* 4:2:0 / 4:2:2: [0] = the interleaved NV12 / NV16 plane;
                                               4:4:4: U's F,H,V,C in [0..3], V's in [4..7] (as x264hip_refine_ext_t) */
} x264hip_mc_ref_t;

typedef struct x264hip_mc_t
{
    int32_t chroma_format;                  /* 0 = luma only, 1 = 4:2:0, 2 = 4:2:2, 3 = 4:4:4 */
    x264hip_mc_ref_t ref[2];                /* list 0, list 1 (a list no block uses may be all NULL) */
    intptr_t ref_stride, ref_frame_stride, ref_chroma_stride, ref_chroma_frame_stride;
    x264hip_weight_t weight[3];             /* h->sh.weight[i_ref][0..2]; applied to list-0-only blocks, as MC_LUMA does */
    void *pred;           intptr_t pred_stride, pred_frame_stride;
    void *pred_chroma[2]; intptr_t pred_chroma_stride, pred_chroma_frame_stride;
                                            /* 4:2:0 / 4:2:2: [0] interleaved UV like the frame's plane[1];
                                               4:4:4: [0] = U, [1] = V */
} x264hip_mc_t;

/* mc: host struct, read during the call; pos, par, mode: device arrays of n blocks.
 * X264HIP_OK and no launch when n == 0.  X264HIP_EINVAL: n < 0, a NULL mc / pos / par, i_pixel
 * outside 0..6, chroma_format outside 0..3, a NULL pred, a NULL chroma output the format needs, a
 * NULL ref[0].luma[k] (or a chroma plane of list 0 the format needs) when mode == NULL, a weight
 * with denom outside 0..7, or a misaligned output (above).  X264HIP_ENODEV without a device. */
int x264hip_8_mb_mc ( const x264hip_mc_t *mc, int i_pixel, const int32_t *pos, const int16_t *par,
                      const int32_t *mode, int n, void *stream );
int x264hip_10_mb_mc( const x264hip_mc_t *mc, int i_pixel, const int32_t *pos, const int16_t *par,
                      const int32_t *mode, int n, void *stream );

#ifdef __cplusplus
}
#endif

#endif /* X264HIP_MC_H */
