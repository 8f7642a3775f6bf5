/* x264hip_mbintra.h — the intra macroblock encode on the device: what macroblock_encode_internal
 * does for I_16x16, I_4x4 and I_8x8 macroblocks whose modes are already decided (reference
 * encoder/macroblock.c:706-768 and :924-951, mb_encode_i16x16 :126-239, x264_mb_encode_i4x4 /
 * _i8x8 encoder/macroblock.h:132-213, mb_encode_chroma_internal macroblock.c:259-490 with
 * b_inter = 0), for every intra macroblock of n_frames frames, with b_lossless = 0, b_trellis = 0,
 * b_noise_reduction = 0, i_skip_intra = 0, progressive, 8 and 10 bit, chroma formats 0 (luma
 * only), 4:2:0 and 4:2:2 (one interleaved NV12 / NV16 plane).
 *
 * It closes the chain
 *   mb_mc -> mb_encode_inter -> mb_encode_intra -> deblock_strength -> deblock_frames
 * (x264hip_mc.h, x264hip_mbenc.h, x264hip_deblock.h): it runs after x264hip_*_mb_encode_inter on
 * the same recon planes and output arrays and fills the macroblocks that entry left alone.  An
 * intra macroblock predicts from whatever stands in recon around it, inter neighbours included
 * (constrained_intra_pred = 0), unfiltered: so before deblocking.  An I picture needs no inter call.
 *
 * Per macroblock (mb_flags, x264hip_mbenc_t's array: bit 0 X264HIP_MBENC_INTRA marks the
 * macroblocks of this entry, every other macroblock is not touched in any array or pixel; among
 * them bit 1 X264HIP_MBENC_T8x8 = I_8x8, otherwise bit 4 X264HIP_MBINTRA_I16x16 = I_16x16,
 * neither = I_4x4; qp = h->mb.i_qp, the chroma qp is chroma_qp_table[qp]).  The modes are x264's
 * own numbers, given, never derived or substituted: the _DC_LEFT / _DC_TOP / _DC_128 variants come
 * from the caller as x264's analysis stores them.
 *   I_16x16 (pred_mode[mb][0], 0..6, common/predict.h:53-60): predict_16x16[mode], sub16x16_dct,
 *     the 16 DCs to dct_dc4x4[block_idx_xy_1d], quant_4x4x4 with quant4_mf/bias[CQM_4IY][qp]; for
 *     each nonzero 4x4 scan_4x4, dequant_4x4 and decimate_score15 accumulated while the score is
 *     < 6 (it starts at 0, or at 9 without b_dct_decimate); a score < 6 clears the AC
 *     non_zero_count (CLEAR_16x16_NNZ), else i_cbp_luma = 0xf when any AC block is nonzero;
 *     dct4x4dc, quant_4x4_dc with mf[0] >> 1 and bias[0] << 1, and when nonzero scan_4x4 into
 *     luma_dc, idct4x4dc, dequant_4x4_dc; reconstruction by one of the four arms of :222-238:
 *     add16x16_idct with or without the DCs, add16x16_idct_dc, or the prediction alone;
 *   I_4x4 (pred_mode[mb][i] of block i in h->dct.luma4x4 order, 0..11, predict.h:70-82): per block
 *     in index order predict_4x4[mode] -- where (i_neighbour4[i] & (TOPRIGHT|TOP)) == TOP the
 *     top-right samples are the sample left of them repeated (macroblock.c:761-763), emulated
 *     without writing the neighbour's pixels -- sub4x4_dct, quant_4x4, and when nonzero scan_4x4,
 *     dequant_4x4, add4x4_idct, i_cbp_luma |= 1 << (i >> 2);
 *   I_8x8 (pred_mode[mb][4*i], 0..11): per 8x8 predict_8x8_filter with i_neighbour8[i] and
 *     x264_pred_i4x4_neighbors[mode], predict_8x8[mode], sub8x8_dct8, quant_8x8 with
 *     quant8_mf/bias[CQM_8IY][qp], and when nonzero scan_8x8, dequant_8x8, add8x8_idct8,
 *     STORE_8x8_NNZ, i_cbp_luma |= 1 << i;
 *   chroma (chroma_pred_mode[mb], 0..6, predict.h:36-43): predict_chroma[mode] (8x8c / 8x16c) on
 *     both channels, then mb_encode_chroma_internal with b_inter = 0, CQM_4IC, qpc =
 *     chroma_qp_table[qp]: no decimation (b_decimate = b_inter && ..., :262: i_decimate_score
 *     starts at 7) and no early termination, so one of the tails empty, DC only through
 *     mb_optimize_chroma_dc (when no AC block is nonzero), or DC + AC.
 * Neighbour availability is the position inside the picture only (one slice per picture):
 * i_neighbour_intra has LEFT when x > 0, TOP when y > 0, TOPLEFT when both, TOPRIGHT when y > 0 &&
 * x + 1 < mb_width; i_neighbour4[] / i_neighbour8[] follow common/macroblock.c:489-498,1340-1351.
 *
 * Outputs, in x264hip_mbenc_t's arrays and layouts (x264hip_mbenc.h), every element of an intra
 * macroblock written, a block whose final non_zero_count is 0 zeros:
 *   recon      luma and chroma, in and out; every pixel of an intra macroblock is written;
 *   level      dctcoef [mb][48][16]: I_4x4 blocks 0..15; I_16x16 the AC blocks with entry 0 = 0
 *              (zeros when the decimation cleared them); I_8x8 luma8x8[i], 64 coefficients in
 *              scan_8x8 order, at block index 4 * i; chroma AC as the inter entry;
 *   chroma_dc  dctcoef [mb][2][8] as the inter entry;
 *   luma_dc    dctcoef [mb][16]: h->dct.luma16x16_dc[0] in scan_4x4 order; zeros when its
 *              non_zero_count is 0 or the macroblock is not I_16x16;
 *   nnz        uint8 [mb][48]; I_16x16: 1 per nonzero AC block unless cleared;
 *   cbp        int32 [mb] = i_cbp_chroma << 4 | i_cbp_luma | nnz(LUMA_DC) << 8 |
 *              nnz(CHROMA_DC+0) << 9 | nnz(CHROMA_DC+1) << 10 (macroblock.c:946-950, CABAC form);
 *   nz         int32 [mb] from nnz as the inter entry (4 bits for I_8x8, else 16);
 *   flags_out  uint8 [mb] = mb_flags[mb] & 3.
 *
 * Not included: I_PCM; 4:4:4 (x264hip_*_mb_encode_intra_444 of x264hip_mb444.h has it); multiple
 * slices and constrained_intra_pred; lossless, trellis,
 * noise reduction; the i_skip_intra reuse of the analysis' reconstruction.  The mode decision is
 * x264hip_*_mb_analyse_intra's (x264hip_mbanalyse.h), which ends in this encode.
 *
 * Contract: only pixels of [0, 16*mb_width) x [0, 16*mb_height) of recon and fenc and the matching
 * chroma area are read; only pixels of intra macroblocks are written; an intra macroblock's own
 * prior recon content never reaches a result.  A mode outside its range, or one that needs a
 * neighbour outside the picture, is the caller's error: that macroblock's outputs are then
 * unspecified, the call still stays inside this footprint (an out-of-range mode is taken as
 * DC_128, a missing neighbour is never read).  Strides are in pixels (interleaved chroma: in
 * samples of the interleaved plane).  recon and recon_chroma start on a 4-pixel boundary and
 * their strides and frame strides are multiples of 4 pixels; fenc needs only pixel alignment.
 * level, chroma_dc and luma_dc need only dctcoef alignment (16-byte aligned arrays are stored
 * with 16-byte stores).  n_frames * mb_width * mb_height <= 2^28.
 *
 * Execution: one launch per macroblock anti-diagonal d = x + 2y, d = 0 .. mb_width +
 * 2*(mb_height-1) - 1 (a macroblock's left, top-left, top and top-right neighbours lie on earlier
 * diagonals), each over that diagonal's macroblocks of all n_frames frames; every diagonal is
 * launched, the lanes of a macroblock that is not intra return at once.  16 lanes per macroblock,
 * four macroblocks per wave; no workgroup waits for another.  Asynchronous on `stream` (a
 * hipStream_t, NULL = the null stream), no host synchronisation and no allocation, so it can be
 * captured into a graph; 0 or a negative X264HIP_E*.
 */
#ifndef X264HIP_MBINTRA_H
#define X264HIP_MBINTRA_H

#include "x264hip_mbenc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define X264HIP_MBINTRA_I16x16 16   /* mb_flags bit 4: I_16x16 (with X264HIP_MBENC_INTRA, without _T8x8) */

typedef struct x264hip_mbintra_t
{
    int32_t chroma_format;            /* 0 (luma only), 1 (4:2:0), 2 (4:2:2) */
    int32_t b_dct_decimate;           /* h->mb.b_dct_decimate; I_16x16 only */
    const uint8_t *chroma_qp_table;   /* HOST: h->chroma_qp_table[0 .. QP_MAX_SPEC], read during the call;
                                         every entry <= QP_MAX_SPEC (- 3 at 4:2:2) */
    /* device tables as x264hip_*_cqm_init writes them: udctcoef [4][QP_MAX_SPEC+1][16] and [4][..][64] */
    const void *quant4_mf, *quant4_bias;
    const void *quant8_mf, *quant8_bias;   /* all three of quant8_mf, quant8_bias, dequant8_mf may be NULL: */
    /* device tables as x264hip_cqm_dequant writes them */
    const int32_t *dequant4_mf;            /* [4][6][16] */
    const int32_t *dequant8_mf;            /* [2][6][64]; NULL with quant8_*: an I_8x8 macroblock is then the
                                              caller's error and is encoded as I_4x4 with pred_mode[4*(i>>2)] */
    /* pixel (0,0) of frame 0, strides in pixels */
    const void *fenc;         intptr_t fenc_stride, fenc_frame_stride;
    const void *fenc_chroma;  intptr_t fenc_chroma_stride, fenc_chroma_frame_stride;   /* NV12 / NV16 */
    void *recon;              intptr_t recon_stride, recon_frame_stride;               /* in and out */
    void *recon_chroma;       intptr_t recon_chroma_stride, recon_chroma_frame_stride; /* in and out */
    /* device arrays, one element (row) per MB, dense (stride = mb_width), frame-major */
    const int8_t  *qp;                /* h->mb.i_qp, 0..QP_MAX_SPEC */
    const uint8_t *mb_flags;          /* X264HIP_MBENC_INTRA, X264HIP_MBENC_T8x8, X264HIP_MBINTRA_I16x16 */
    const int8_t  *pred_mode;         /* [mb][16], see above */
    const int8_t  *chroma_pred_mode;  /* [mb]; not read when chroma_format == 0 */
    /* outputs, see above */
    void    *level;                   /* dctcoef [mb][48][16] */
    void    *chroma_dc;               /* dctcoef [mb][2][8] */
    uint8_t *nnz;                     /* [mb][48] */
    int32_t *cbp;                     /* [mb] */
    int32_t *nz;                      /* [mb] */
    uint8_t *flags_out;               /* [mb] */
    void    *luma_dc;                 /* dctcoef [mb][16] */
} x264hip_mbintra_t;

/* e: host struct, read during the call (chroma_qp_table included: QP_MAX_SPEC + 1 = 52 entries at
 * 8 bit, 64 at 10 bit).  X264HIP_OK and no launch when n_frames * mb_width * mb_height == 0.
 * X264HIP_EINVAL, before any HIP call: a NULL e, chroma_qp_table, quant4_mf, quant4_bias,
 * dequant4_mf, fenc, recon, qp, mb_flags, pred_mode or output array (luma_dc included);
 * quant8_mf, quant8_bias and dequant8_mf not all NULL or all set; chroma_format outside 0..2; a
 * NULL fenc_chroma, recon_chroma or chroma_pred_mode the format needs; a chroma_qp_table entry
 * above QP_MAX_SPEC (QP_MAX_SPEC - 3 at 4:2:2); a negative size; more than 2^28 macroblocks; recon
 * or recon_chroma off a 4-pixel boundary or with a stride or frame stride that is no multiple of
 * 4 pixels; level, chroma_dc, luma_dc, cbp or nz off their element's alignment.  X264HIP_ENODEV
 * without a device. */
int x264hip_8_mb_encode_intra ( const x264hip_mbintra_t *e, int mb_width, int mb_height, int n_frames, void *stream );
int x264hip_10_mb_encode_intra( const x264hip_mbintra_t *e, int mb_width, int mb_height, int n_frames, void *stream );

#ifdef __cplusplus
}
#endif

#endif /* X264HIP_MBINTRA_H */
