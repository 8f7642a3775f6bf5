/* x264hip_mbenc.h — the inter macroblock encode on the device: what macroblock_encode_internal
 * (reference encoder/macroblock.c:618-972) leaves for an inter macroblock after x264_mb_mc, for
 * every macroblock of n_frames frames in one launch, with b_lossless = 0, b_trellis = 0,
 * b_noise_reduction = 0, progressive, 8 and 10 bit, chroma formats 0 (luma only), 4:2:0 and 4:2:2
 * (one interleaved NV12 / NV16 plane).
 *
 * It is the middle link of
 *   mb_mc -> mb_encode_inter -> deblock_strength -> deblock_frames -> hpel_filter
 * (x264hip_mc.h, x264hip_deblock.h): it reads the prediction x264hip_*_mb_mc wrote, and its
 * `nz` and `flags_out` are what x264hip_deblock_strength and x264hip_*_deblock_frames read.
 *
 * Per macroblock (mb_flags: bit 0 intra, bit 1 transform 8x8, bit 2 partition == D_16x16, bit 3
 * P_SKIP / B_SKIP; qp = h->mb.i_qp, the chroma qp is chroma_qp_table[qp]):
 *   intra: left entirely alone; no pixel and no output element of it is written except
 *     flags_out[mb] = mb_flags[mb];
 *   skip (macroblock_encode_skip, macroblock.c:500-520): recon = pred, every output zero;
 *   luma, transform 4 (macroblock.c:845-919): sub16x16_dct; per 8x8 quant_4x4x4 with
 *     quant4_mf/bias[CQM_4PY][qp]; for each nonzero 4x4 scan_4x4, dequant_4x4 and decimate_score16
 *     accumulated while i_decimate_8x8 < 6 (it starts at 6 without b_dct_decimate);
 *     i_decimate_8x8 < 4 clears the 8x8's non_zero_count and keeps it out of the cbp;
 *     i_decimate_mb < 6 clears the macroblock; else add8x8_idct for the 8x8s of the cbp only;
 *   luma, transform 8 (macroblock.c:801-843): sub16x16_dct8, quant_8x8 with
 *     quant8_mf/bias[CQM_8PY][qp], scan_8x8, decimate_score64 per nonzero 8x8; an 8x8 joins the
 *     cbp when its score is >= 4 (always without decimation); the macroblock is reconstructed
 *     (dequant_8x8, add8x8_idct8, STORE_8x8_NNZ 1) only when i_decimate_mb >= 6 or !b_dct_decimate;
 *   chroma (mb_encode_chroma_internal, macroblock.c:259-490, b_inter = 1, CQM_4PC = CQM_4IC + 1,
 *     qpc = chroma_qp_table[qp]): when b_dct_decimate && qpc >= 18 the early termination on
 *     var2 < 4 * thresh, thresh = (x264_lambda2_tab[qpc] + 32) >> 6 ((.. + 16) >> 5 at 4:2:2): per
 *     channel with ssd[ch] > thresh sub8x8_dct_dc / sub8x16_dct_dc, quant_2x2_dc with
 *     mf[qpc + 3 * c422][0] >> 1 and bias << 1, mb_optimize_chroma_dc (1 at once when
 *     dmf > 32 * 64), the DC zigzag, idct_dequant_2x2_dconly / _2x4_dconly, add8x8_idct_dc;
 *     otherwise sub8x8_dct (twice at 4:2:2), dct2x2dc / dct2x4dc, quant_4x4x4, scan_4x4 +
 *     dequant_4x4 + decimate_score15 while the score is < 7, the DC quant, and one of the three
 *     tails: decimated (score < 7 || !nz_ac: the AC non_zero_count cleared, DC-only through
 *     mb_optimize_chroma_dc), empty, or DC + AC (idct_dequant_2x2_dc / _2x4_dc, add8x8_idct);
 *     i_cbp_chroma is 0, 1 or 2 as macroblock.c:487-489 leaves it (0 or 1 after the early
 *     termination).
 *
 * Outputs, device arrays, dense and frame-major, written for every macroblock that is not intra:
 *   recon      luma and chroma, in the layout of pred; recon may be pred itself (in place, as
 *              x264's fdec) or a separate plane; every pixel of a non-intra macroblock is written;
 *   level      dctcoef [mb][48][16] by x264's h->dct.luma4x4 block index: luma 0..15; chroma AC at
 *              16 + ch*16 + i8x8*8 + i4x4 (16..19, 32..35 at 4:2:0 and also 24..27, 40..43 at
 *              4:2:2); zigzag (frame) order as zigzagf.scan_4x4 writes it (entry 0 of a chroma AC
 *              block is 0); a transform-8 macroblock stores luma8x8[idx], 64 coefficients in
 *              scan_8x8 order, at block index 4 * idx.  Every block whose final non_zero_count is
 *              0 -- decimated blocks, unused indices, a chroma the early termination skipped -- is
 *              zeros (x264 leaves stale data there);
 *   chroma_dc  dctcoef [mb][2][8]: zigzag_scan_2x2_dc fills the first 4 (the rest 0),
 *              zigzag_scan_2x4_dc all 8; zeros where the DC non_zero_count is 0;
 *   nnz        uint8 [mb][48]: h->mb.cache.non_zero_count by the same block index, after
 *              decimation; all four entries of a kept transform-8 block are 1 (STORE_8x8_NNZ);
 *   cbp        int32 [mb] = i_cbp_chroma << 4 | i_cbp_luma | nnz(CHROMA_DC+0) << 9 |
 *              nnz(CHROMA_DC+1) << 10 (macroblock.c:946-950, the CABAC form; CAVLC masks 0xff);
 *   nz         int32 [mb]: the mask x264hip_deblock_strength_t.nz documents (16 bits, bit
 *              4*i8+i4, for a transform-4 macroblock, 4 bits for transform 8), taken from nnz;
 *   flags_out  uint8 [mb] in x264hip_deblock_t.mb_flags' format: bits 0 and 1 copied, bit 2 =
 *              input bit 2 && cbp == 0 (a skip macroblock keeps it); an intra macroblock's flags
 *              are copied unchanged.  The one array written for intra macroblocks too.
 *
 * Not included: 4:4:4 (it needs the chroma categories of dequant8_mf, which x264hip_cqm_dequant
 * does not produce, and the plane loop whose i_decimate_mb carries across planes:
 * x264hip_*_mb_encode_inter_444 of x264hip_mb444.h has both); intra
 * macroblocks; lossless, trellis, noise reduction; the P_SKIP / B_SKIP conversion of
 * macroblock.c:953-971 (it needs pskip_mv: x264hip_mb_skip_convert of x264hip_mbskip.h runs it on
 * this entry's cbp); zigzag_interleave_8x8_cavlc (x264hip_*_zigzag_interleave_batch does it).
 *
 * Contract: only pixels of [0, 16*mb_width) x [0, 16*mb_height) and the matching chroma area are
 * read or written.  Strides are in pixels (interleaved chroma: in samples of the interleaved
 * plane).  recon and recon_chroma start on a 4-pixel boundary and their strides and frame strides
 * are multiples of 4 pixels (the mb_mc rule: blocks are stored as whole dwords); fenc and pred
 * need only pixel alignment.  level and chroma_dc need only dctcoef alignment (16-byte aligned
 * arrays are stored with 16-byte stores).  n_frames * mb_width * mb_height <= 2^28.
 *
 * Execution: one launch, four macroblocks per wave (a lane per 4x4 luma block, the 8x8 transform
 * on a lane per 8x8, a lane per 4x4 position of both chroma channels); no workgroup waits for
 * another.  Asynchronous on `stream` (a hipStream_t, NULL = the null stream), no host
 * synchronisation and no allocation, so it can be captured into a graph; 0 or a negative X264HIP_E*.
 */
#ifndef X264HIP_MBENC_H
#define X264HIP_MBENC_H

#include "x264hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define X264HIP_MBENC_INTRA  1   /* mb_flags bits */
#define X264HIP_MBENC_T8x8   2
#define X264HIP_MBENC_D16x16 4
#define X264HIP_MBENC_SKIP   8

typedef struct x264hip_mbenc_t
{
    int32_t chroma_format;            /* 0 (luma only), 1 (4:2:0), 2 (4:2:2) */
    int32_t b_dct_decimate;           /* h->mb.b_dct_decimate */
    const uint8_t *chroma_qp_table;   /* HOST: h->chroma_qp_table[0 .. QP_MAX_SPEC], read during the call;
                                         every entry <= QP_MAX_SPEC (- 3 at 4:2:2) */
    /* device tables as x264hip_*_cqm_init writes them: udctcoef [4][QP_MAX_SPEC+1][16] and [4][..][64] */
    const void *quant4_mf, *quant4_bias;
    const void *quant8_mf, *quant8_bias;   /* all three of quant8_mf, quant8_bias, dequant8_mf may be NULL: */
    /* device tables as x264hip_cqm_dequant writes them */
    const int32_t *dequant4_mf;            /* [4][6][16] */
    const int32_t *dequant8_mf;            /* [2][6][64]; NULL with quant8_*: a transform-8 macroblock is then
                                              the caller's error and is encoded with the 4x4 transform */
    /* pixel (0,0) of frame 0, strides in pixels */
    const void *fenc;         intptr_t fenc_stride, fenc_frame_stride;
    const void *fenc_chroma;  intptr_t fenc_chroma_stride, fenc_chroma_frame_stride;   /* NV12 / NV16 */
    const void *pred;         intptr_t pred_stride, pred_frame_stride;                 /* x264hip_mc_t's pred */
    const void *pred_chroma;  intptr_t pred_chroma_stride, pred_chroma_frame_stride;   /* its pred_chroma[0] */
    void *recon;              intptr_t recon_stride, recon_frame_stride;               /* may be pred */
    void *recon_chroma;       intptr_t recon_chroma_stride, recon_chroma_frame_stride; /* may be pred_chroma */
    /* device arrays, one element per MB, dense (stride = mb_width), frame-major */
    const int8_t  *qp;                /* h->mb.i_qp, 0..QP_MAX_SPEC */
    const uint8_t *mb_flags;          /* X264HIP_MBENC_* */
    /* outputs, see above */
    void    *level;                   /* dctcoef [mb][48][16] */
    void    *chroma_dc;               /* dctcoef [mb][2][8] */
    uint8_t *nnz;                     /* [mb][48] */
    int32_t *cbp;                     /* [mb] */
    int32_t *nz;                      /* [mb] */
    uint8_t *flags_out;               /* [mb] */
} x264hip_mbenc_t;

/* e: host struct, read during the call (chroma_qp_table included: QP_MAX_SPEC + 1 = 52 entries at
 * 8 bit, 64 at 10 bit).  X264HIP_OK and no launch when n_frames * mb_width * mb_height == 0.
 * X264HIP_EINVAL: a NULL e, chroma_qp_table, quant4_mf, quant4_bias, dequant4_mf, fenc, pred,
 * recon, qp, mb_flags or output array; quant8_mf, quant8_bias and dequant8_mf not all NULL or all
 * set; chroma_format outside 0..2; a NULL fenc_chroma, pred_chroma or recon_chroma the format
 * needs; a chroma_qp_table entry above QP_MAX_SPEC (QP_MAX_SPEC - 3 at 4:2:2); a negative size;
 * more than 2^28 macroblocks; recon or recon_chroma off a 4-pixel boundary or with a stride or
 * frame stride that is no multiple of 4 pixels.  X264HIP_ENODEV without a device. */
int x264hip_8_mb_encode_inter ( const x264hip_mbenc_t *e, int mb_width, int mb_height, int n_frames, void *stream );
int x264hip_10_mb_encode_inter( const x264hip_mbenc_t *e, int mb_width, int mb_height, int n_frames, void *stream );

#ifdef __cplusplus
}
#endif

#endif /* X264HIP_MBENC_H */
