/* x264hip_mb444.h — the inter and intra macroblock encodes on the device at 4:4:4 (CHROMA_444):
 * what x264hip_mbenc.h and x264hip_mbintra.h do for chroma formats 0..2, for three separate planes.
 * At 4:4:4 x264_macroblock_encode is macroblock_encode_internal( h, 3, 0 ) (reference
 * encoder/macroblock.c:974-982): plane_count = 3, chroma = 0.  There is no mb_encode_chroma: U and
 * V go through the luma paths with the chroma quant categories and the chroma qp, and
 * i_cbp_chroma is 0.  b_lossless = 0, b_trellis = 0, b_noise_reduction = 0, i_skip_intra = 0,
 * progressive, 8 and 10 bit, as the two other headers.
 *
 * The entries are the two middle links of
 *   mb_mc -> mb_encode_inter_444 -> mb_encode_intra_444 -> deblock_strength -> deblock_frames
 * (x264hip_mc.h and x264hip_deblock.h with chroma_format 3): fenc[], pred[] and recon[] are Y, U, V
 * as separate planes; plane 0 has its own stride and frame stride, planes 1 and 2 share the chroma
 * ones, exactly as x264hip_mc_t.pred_chroma[2] and x264hip_deblock_t.chroma[2] do, so the outputs
 * of x264hip_*_mb_mc and the inputs of x264hip_*_deblock_frames plug in unchanged.
 *
 * One struct serves both entries (they share every table, plane and output array, and the intra
 * entry runs on what the inter entry left): `pred` is read by the inter entry only, `pred_mode`
 * and `luma_dc` by the intra entry only, and the other entry does not look at them (they may be NULL).
 *
 * mb_flags, qp and the chroma qp are x264hip_mbenc.h's and x264hip_mbintra.h's: bit 0
 * X264HIP_MBENC_INTRA, bit 1 _T8x8, bit 2 _D16x16, bit 3 _SKIP, bit 4 X264HIP_MBINTRA_I16x16;
 * qp = h->mb.i_qp.  Per plane p: i_qp is qp for p = 0 and chroma_qp_table[qp] for p = 1, 2
 * (the `i_qp = h->mb.i_chroma_qp` of every plane loop).
 *
 * The tables (x264hip_*_cqm_init444 / x264hip_cqm_dequant444 below): x264_cqm_init with
 * num_8x8_lists = 4 (common/set.c:87,154-159,186-205): quant8_mf / quant8_bias [4][QP_MAX_SPEC+1][64]
 * with all of CQM_8IY, CQM_8PY, CQM_8IC, CQM_8PC written, from scaling_list[4..7] with the deadzones
 * { 32 - intra, 32 - inter, 32 - 11, 32 - 21 }, and dequant8_mf [4][6][64]; the 4x4 tables are
 * x264hip_*_cqm_init's and x264hip_cqm_dequant's.
 *
 * x264hip_*_mb_encode_inter_444 (macroblock.c:769-921 with plane_count = 3), every macroblock
 * that is not intra:
 *   intra: left alone except flags_out[mb] = mb_flags[mb];
 *   skip (macroblock_encode_skip, :500-520): recon[p] = pred[p] for all three planes, every output zero;
 *   transform 4 (:845-921), per plane p with quant_cat = p ? CQM_4PC : CQM_4PY (:850): sub16x16_dct,
 *     per 8x8 quant_4x4x4, for each nonzero 4x4 scan_4x4, dequant_4x4 and decimate_score16
 *     accumulated while i_decimate_8x8 < 6; i_decimate_8x8 restarts per 8x8 (0, or 6 without
 *     b_dct_decimate, :864) and an 8x8 below 4 is cleared (:900-901).  i_decimate_mb is declared
 *     outside the plane loop (:771) and never reset: each nonzero 8x8 adds its i_decimate_8x8
 *     (:899), so the test after plane p (:907) sees the scores of planes 0..p.  A plane whose own
 *     scores stay below 6 is kept when the earlier planes' scores carry it; an earlier plane that
 *     was cleared stays cleared; an 8x8 below 4 is still dropped inside a kept plane.  Kept:
 *     add8x8_idct for the 8x8s of plane_cbp (:914-918);
 *   transform 8 (:801-843), per plane with quant_cat = p ? CQM_8PC : CQM_8PY (:808): sub16x16_dct8,
 *     quant_8x8, scan_8x8, decimate_score64 per nonzero 8x8 added to the same i_decimate_mb
 *     (:823-824); an 8x8 joins plane_cbp when its score is >= 4 (always without decimation); the
 *     plane is reconstructed (dequant_8x8 with dequant8_mf[quant_cat] :838, add8x8_idct8,
 *     STORE_8x8_NNZ 1) when i_decimate_mb >= 6 || !b_decimate (:833), the same carry.
 * x264hip_*_mb_encode_intra_444 (:706-768, mb_encode_i16x16 :126-239, x264_mb_encode_i4x4 / _i8x8
 * encoder/macroblock.h:132-213), every intra macroblock, after the inter entry on the same recon
 * planes and arrays; every other macroblock is not touched in any array or pixel.  For each plane
 * the luma path of x264hip_mbintra.h runs with the same luma mode(s), pred_mode[mb][16] (there is
 * no chroma_pred_mode), the categories p ? CQM_4IC : CQM_4IY (:136, macroblock.h:163) and
 * p ? CQM_8IC : CQM_8IY (macroblock.h:103,207) and the plane's qp.  The prediction comes from
 * that plane's own reconstructed neighbours, the top-right emulation of :761-763 included.
 * I_16x16's decimate score is local to mb_encode_i16x16 (:135) and is not carried across planes.
 *
 * Outputs, device arrays, dense and frame-major, in x264hip_mbenc.h's layouts:
 *   recon[3]   every pixel of a macroblock the entry owns is written; recon[p] may be pred[p];
 *   level      dctcoef [mb][48][16]: plane p, block i (h->dct.luma4x4[16p + i]) at index 16p + i,
 *              zigzag (frame) order; a transform-8 block luma8x8[4p + idx] at block index
 *              16p + 4*idx, 64 coefficients in scan_8x8 order; I_16x16: the AC blocks, entry 0 = 0.
 *              Every block whose final non_zero_count is 0 is zeros;
 *   nnz        uint8 [mb][48], the same index, after decimation; all four entries of a kept
 *              transform-8 block are 1;
 *   luma_dc    (intra) dctcoef [mb][3][16]: luma_dc[mb][p] = h->dct.luma16x16_dc[p] in scan_4x4
 *              order; zeros when its non_zero_count is 0 or the macroblock is not I_16x16;
 *   cbp        int32 [mb] = i_cbp_luma, the OR over the three planes (:835,914, macroblock.h:161,205),
 *              | nnz(LUMA_DC + p) << (8 + p) for an I_16x16 macroblock: LUMA_DC+1 and +2 are the
 *              slots x264 calls CHROMA_DC+0 and +1, so this is macroblock.c:946-950 unchanged.
 *              Bits 4-5 are zero (i_cbp_chroma = 0, :943), and bits 8-10 of an inter macroblock;
 *   nz         int32 [mb]: x264hip_deblock_strength_t.nz's mask from plane 0's nnz only (16 bits for
 *              transform 4, 4 bits for transform 8): x264's deblock_strength reads the luma
 *              entries of non_zero_count (common/macroblock.c:1617);
 *   flags_out  uint8 [mb] as x264hip_mbenc.h / x264hip_mbintra.h, with the cbp of all planes:
 *              inter (mb_flags & 3) | (bit 2 && cbp == 0 ? bit 2 : 0), intra mb_flags & 3.
 * x264hip_deblock_strength needs no change at 4:4:4: it reads nz and flags_out only, never cbp.
 * The early exit of common/macroblock.c:1451 (a transform-8 macroblock whose i_cbp_luma is 0xf:
 * every bS 2) is skipped at 4:4:4, where i_cbp_luma mixes the planes, but the general path gives
 * the same values when all four luma 8x8s are coded, since STORE_8x8_NNZ sets all four entries of
 * an 8x8 alike; x264hip_*_deblock_frames takes chroma_format 3 already.
 *
 * Not included: I_PCM; several slices and constrained_intra_pred; lossless, trellis, noise
 * reduction; the i_skip_intra reuse; the CAVLC non_zero_count munging for 8x8dct
 * (common/macroblock.c:1568-1615; x264hip_*_zigzag_interleave_batch does the coefficients); the
 * P_SKIP / B_SKIP conversion of macroblock.c:953-971; the mode decision.
 *
 * Contract: only pixels of [0, 16*mb_width) x [0, 16*mb_height) of each plane are read or written;
 * the intra entry writes only pixels of intra macroblocks, and an intra macroblock's own prior
 * recon content never reaches a result.  A mode outside its range, or one that needs a neighbour
 * outside the picture, is the caller's error as in x264hip_mbintra.h (taken as DC_128; a missing
 * neighbour is never read).  Strides are in pixels.  recon[0..2] start on a 4-pixel boundary and
 * the four recon strides are multiples of 4 pixels (blocks are stored as whole dwords); fenc and
 * pred need only pixel alignment.  level and luma_dc need only dctcoef alignment (16-byte aligned
 * arrays are stored with 16-byte stores).  n_frames * mb_width * mb_height <= 2^28.
 *
 * Execution: plane p runs on lanes 16p .. 16p+15 of one wave, one macroblock per wave, so the
 * three planes advance side by side; the inter entry's carry is a 3-way prefix over the planes'
 * scores read across the wave, after which every lane takes the reference's decision itself.
 * Inter: one launch.  Intra: one launch per macroblock anti-diagonal d = x + 2y, as
 * x264hip_*_mb_encode_intra, three tiles of shared memory per macroblock.  Asynchronous on
 * `stream` (a hipStream_t, NULL = the null stream), no host synchronisation and no allocation, so
 * the entries can be captured into a graph; 0 or a negative X264HIP_E*.
 */
#ifndef X264HIP_MB444_H
#define X264HIP_MB444_H

#include "x264hip_mbintra.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct x264hip_mb444_t
{
    int32_t b_dct_decimate;           /* h->mb.b_dct_decimate */
    const uint8_t *chroma_qp_table;   /* HOST: h->chroma_qp_table[0 .. QP_MAX_SPEC], read during the call;
                                         every entry <= QP_MAX_SPEC */
    /* device tables as x264hip_*_cqm_init444 writes them: udctcoef [4][QP_MAX_SPEC+1][16] and [4][..][64] */
    const void *quant4_mf, *quant4_bias;
    const void *quant8_mf, *quant8_bias;   /* all three of quant8_mf, quant8_bias, dequant8_mf may be NULL: */
    /* device tables as x264hip_cqm_dequant444 writes them */
    const int32_t *dequant4_mf;            /* [4][6][16] */
    const int32_t *dequant8_mf;            /* [4][6][64]; NULL with quant8_*: a transform-8 / I_8x8 macroblock is then
                                              the caller's error and is encoded with the 4x4 transform (I_8x8: as
                                              I_4x4 with pred_mode[4*(i>>2)]) */
    /* Y, U, V: pixel (0,0) of frame 0, strides in pixels; [1] and [2] share the chroma strides */
    const void *fenc[3];  intptr_t fenc_stride, fenc_frame_stride, fenc_chroma_stride, fenc_chroma_frame_stride;
    const void *pred[3];  intptr_t pred_stride, pred_frame_stride, pred_chroma_stride, pred_chroma_frame_stride;
                                      /* inter: x264hip_mc_t's pred, pred_chroma[0], pred_chroma[1] */
    void *recon[3];       intptr_t recon_stride, recon_frame_stride, recon_chroma_stride, recon_chroma_frame_stride;
                                      /* inter: may be pred; intra: in and out */
    /* device arrays, one element (row) per MB, dense (stride = mb_width), frame-major */
    const int8_t  *qp;                /* h->mb.i_qp, 0..QP_MAX_SPEC */
    const uint8_t *mb_flags;          /* X264HIP_MBENC_*, X264HIP_MBINTRA_I16x16 */
    const int8_t  *pred_mode;         /* intra: [mb][16], see x264hip_mbintra.h */
    /* outputs, see above */
    void    *level;                   /* dctcoef [mb][48][16] */
    uint8_t *nnz;                     /* [mb][48] */
    int32_t *cbp;                     /* [mb] */
    int32_t *nz;                      /* [mb] */
    uint8_t *flags_out;               /* [mb] */
    void    *luma_dc;                 /* intra: dctcoef [mb][3][16] */
} x264hip_mb444_t;

/* Host-side table set-up, no device needed.  scaling_list[8] as sps->scaling_list (4 lists of 16,
 * 4 of 64 entries).  cqm_init444: x264hip_*_cqm_init with the 8x8 categories 2 (CQM_8IC) and 3
 * (CQM_8PC) written too; q8m / q8b are udctcoef [4][QP_MAX_SPEC+1][64]; the 4x4 tables and the
 * 8x8 categories 0 and 1 equal x264hip_*_cqm_init's.  Returns QP_MAX_SPEC.  cqm_dequant444:
 * x264hip_cqm_dequant with dq8 int32 [4][6][64]. */
int x264hip_8_cqm_init444 ( const uint8_t *const scaling_list[8], int deadzone_inter, int deadzone_intra,
                            uint16_t *q4m, uint16_t *q4b, uint16_t *q8m, uint16_t *q8b );
int x264hip_10_cqm_init444( const uint8_t *const scaling_list[8], int deadzone_inter, int deadzone_intra,
                            uint32_t *q4m, uint32_t *q4b, uint32_t *q8m, uint32_t *q8b );
void x264hip_cqm_dequant444( const uint8_t *const scaling_list[8], int32_t *dq4, int32_t *dq8 );

/* e: host struct, read during the call (chroma_qp_table included: QP_MAX_SPEC + 1 = 52 entries at
 * 8 bit, 64 at 10 bit).  X264HIP_OK and no launch when n_frames * mb_width * mb_height == 0.
 * X264HIP_EINVAL, before any HIP call: a NULL e, chroma_qp_table, quant4_mf, quant4_bias,
 * dequant4_mf, fenc[p], recon[p], qp, mb_flags, level, nnz, cbp, nz or flags_out; inter: a NULL
 * pred[p]; intra: a NULL pred_mode or luma_dc; quant8_mf, quant8_bias and dequant8_mf not all NULL
 * or all set; a chroma_qp_table entry above QP_MAX_SPEC; a negative size; more than 2^28
 * macroblocks; a recon[p] off a 4-pixel boundary or a recon stride or frame stride that is no
 * multiple of 4 pixels; level, luma_dc (intra), cbp or nz off their element's alignment.
 * X264HIP_ENODEV without a device. */
int x264hip_8_mb_encode_inter_444 ( const x264hip_mb444_t *e, int mb_width, int mb_height, int n_frames, void *stream );
int x264hip_10_mb_encode_inter_444( const x264hip_mb444_t *e, int mb_width, int mb_height, int n_frames, void *stream );
int x264hip_8_mb_encode_intra_444 ( const x264hip_mb444_t *e, int mb_width, int mb_height, int n_frames, void *stream );
int x264hip_10_mb_encode_intra_444( const x264hip_mb444_t *e, int mb_width, int mb_height, int n_frames, void *stream );

#ifdef __cplusplus
}
#endif

#endif /* X264HIP_MB444_H */
