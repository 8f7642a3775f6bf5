/* x264hip_deblock.h — the in-loop deblocking filter on the device: x264_frame_deblock_row
 * (reference common/deblock.c:378-606) over whole frames, in place, and the derivation of the
 * boundary strengths it reads (deblock_strength_c, common/deblock.c:277-304, with the intra
 * values of x264_macroblock_deblock_strength, common/macroblock.c:1441-1447).  Progressive
 * frames, 8 and 10 bit, chroma formats 0 (luma only), 4:2:0 and 4:2:2 (one interleaved NV12 /
 * NV16 plane) and 4:4:4 (separate U and V planes).
 *
 * The filter stands between the reconstruction (x264hip_*_mb_dequant_idct_add) and everything
 * that reads a finished picture (x264hip_*_hpel_filter, x264hip_*_ssim_bands,
 * x264hip_*_ssd_plane_batch, x264hip_forward_ref), so
 *   mb_mc -> mb_dct_quant -> mb_dequant_idct_add -> deblock_strength -> deblock_frames -> hpel_filter
 * stays in device memory.
 *
 * deblock_frames.  The result is exactly what the C loop of deblock.c:378-606 leaves for
 * SLICE_MBAFF == 0, the macroblocks in raster order and, within one, vertical edges 0..3 and
 * then horizontal edges 0..3:
 *   a = alpha_c0_offset - QP_BD_OFFSET, b = beta_offset - QP_BD_OFFSET (QP_BD_OFFSET = 6 * (depth - 8));
 *   qp_thresh = 15 - min( a, b ) - max( 0, chroma_qp_index_offset ) (deblock.c:383);
 *   first_edge_only = ((mb_flags & 4) && !intra) || qp <= qp_thresh (deblock.c:415): bit 2 of
 *     mb_flags is the caller's `partition == D_16x16 && !cbp`;
 *   the left and top macroblock edges use qp = (qp + qpn + 1) >> 1 and the chroma qp
 *     (qpc + chroma_qp_table[qpn] + 1) >> 1 (deblock.c:514-516, 571-573), and the _intra filters
 *     whenever either macroblock across the edge is intra: bs is not read there;
 *   the FILTER macro literally: odd edges are skipped under transform 8x8, 4:2:0 chroma is
 *     filtered on edges 0 and 2, 4:2:2 chroma on vertical edges 0 and 2 (deblock_h_chroma_422)
 *     and on all four horizontal edges whatever the transform size; at 4:4:4 the luma filters
 *     run on U and V with the chroma qp and b_chroma = 0;
 *   deblock_edge's early return on !M32( bS ) || !alpha || !beta, the << (BIT_DEPTH-8) of alpha
 *     and beta and the * (1 << (BIT_DEPTH-8)) + b_chroma on tc; the line filters of
 *     deblock.c:79-275.
 * bs values are 0..3 wherever they are read (4 only where an intra edge ignores them).
 * Not included: MBAFF and interlaced frames; the mb_info / effective_qp reset
 * (deblock.c:523-528, 578-582); x264_macroblock_deblock, the RD-time variant; a per-call
 * x264_deblock_function_t table.
 *
 * Contract: only pixels of [0, 16*mb_width) x [0, 16*mb_height) and the matching chroma area are
 * read or written; no padding is needed.  Borders are not re-expanded: x264hip_*_hpel_filter and
 * the border expansion run afterwards, as in x264.  Strides are in pixels (interleaved chroma: in
 * samples of the interleaved plane).  bs is 4-byte aligned (an edge's four strengths are read as
 * one word).  n_frames * mb_width * mb_height <= 2^28.
 *
 * Execution: one kernel launch per anti-diagonal x + 2y of macroblocks (a macroblock needs its
 * left, top and top-right neighbours finished), each over that diagonal's macroblocks of every
 * frame: mb_width + 2 * (mb_height - 1) dependent launches per call, so batching frames is the
 * throughput lever.  No kernel waits for another workgroup.
 *
 * Asynchronous on `stream` (a hipStream_t, NULL = the null stream), no host synchronisation;
 * 0 or a negative X264HIP_E*.
 */
#ifndef X264HIP_DEBLOCK_H
#define X264HIP_DEBLOCK_H

#include "x264hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct x264hip_deblock_t
{
    int32_t chroma_format;            /* 0..3 as x264hip_mc_t */
    int32_t alpha_c0_offset;          /* h->sh.i_alpha_c0_offset (already doubled), -12..12 */
    int32_t beta_offset;              /* h->sh.i_beta_offset, -12..12 */
    int32_t chroma_qp_index_offset;   /* h->pps->i_chroma_qp_index_offset (qp_thresh only) */
    const uint8_t *chroma_qp_table;   /* HOST: h->chroma_qp_table[0 .. QP_MAX_SPEC], read during the call */
    void *luma;      intptr_t luma_stride, luma_frame_stride;         /* pixel (0,0) of frame 0, strides in pixels */
    void *chroma[2]; intptr_t chroma_stride, chroma_frame_stride;     /* as x264hip_mc_t's pred_chroma */
    /* device arrays, one element per MB, dense (stride = mb_width), frame-major */
    const int8_t  *qp;                /* h->mb.qp, 0..QP_MAX_SPEC */
    const uint8_t *mb_flags;          /* bit 0 IS_INTRA, bit 1 mb_transform_size, bit 2 (partition == D_16x16 && !cbp) */
    const uint8_t *bs;                /* [mb][2][4][4]: bs[dir][edge][i] of deblock_strength, 4-byte aligned */
    const int32_t *slice_table;       /* NULL: every MB edge inside the picture is filtered
                                         (disable_deblocking_filter_idc != 2); else h->mb.slice_table,
                                         and an MB edge between different slices is not filtered (idc 2) */
} x264hip_deblock_t;

/* d: host struct, read during the call (chroma_qp_table included: QP_MAX_SPEC + 1 = 52 entries
 * at 8 bit, 64 at 10 bit).  X264HIP_OK and no launch when n_frames * mb_width * mb_height == 0.
 * X264HIP_EINVAL: a NULL d, luma, qp, mb_flags, bs or chroma_qp_table; a NULL chroma plane the
 * format needs (chroma[0] at 4:2:0 / 4:2:2, both at 4:4:4); an offset outside -12..12; a negative
 * size; chroma_format outside 0..3; more than 2^28 macroblocks.  X264HIP_ENODEV without a device. */
int x264hip_8_deblock_frames ( const x264hip_deblock_t *d, int mb_width, int mb_height, int n_frames, void *stream );
int x264hip_10_deblock_frames( const x264hip_deblock_t *d, int mb_width, int mb_height, int n_frames, void *stream );

typedef struct x264hip_deblock_strength_t
{
    const int32_t *nz;        /* per MB: the mask x264hip_*_mb_dct_quant writes (16 bits, bit 4*i8+i4, for a
                                 transform-4 MB; 4 bits, bit i8, for a transform-8 MB: all four 4x4 blocks of
                                 an 8x8 share its bit, as x264's STORE_8x8_NNZ leaves non_zero_count) */
    const uint8_t *mb_flags;  /* as above: bit 0 intra, bit 1 transform 8x8 */
    const int16_t *mv[2];     /* h->mb.mv[l] layout: [frame][4*mbh][4*mbw][2]; mv[1] NULL unless bframe */
    const int8_t  *ref[2];    /* h->mb.ref[l] layout: [frame][2*mbh][2*mbw] (the caller has applied
                                 deblock_ref_table where weightp duplicates references) */
    int32_t bframe, mvy_limit;/* mvy_limit = 4 for progressive */
} x264hip_deblock_strength_t;

/* bs[mb][dir][edge][i] for every macroblock of n_frames frames, bit-depth independent, one launch.
 * For every edge segment between two 4x4 blocks the value is deblock_strength_c's
 * (deblock.c:277-304): 2 if either block has a coefficient, else 1 if the references differ or a
 * vector component differs by >= 4 (x) / >= mvy_limit (y) quarter pixels (both lists when bframe,
 * list l against list l), else 0.  For edge 0 the neighbouring block is column 3 of the left MB
 * or row 3 of the top MB.  An intra MB gets 3 on its inner edges (macroblock.c:1441-1447); an
 * edge-0 segment with an intra MB on either side gets 4 (x264hip_*_deblock_frames ignores it
 * there); an edge 0 on the picture border gets 0.
 * s: host struct; all its arrays and bs: device arrays.  X264HIP_OK and no launch when
 * n_frames * mb_width * mb_height == 0.  X264HIP_EINVAL: a NULL s, nz, mb_flags, mv[0], ref[0] or
 * bs; bframe with a NULL mv[1] or ref[1]; mvy_limit < 1; a negative size; more than 2^28
 * macroblocks.  bs is 4-byte aligned.  X264HIP_ENODEV without a device. */
int x264hip_deblock_strength( const x264hip_deblock_strength_t *s, int mb_width, int mb_height, int n_frames,
                              uint8_t *bs /* [mb][2][4][4] */, void *stream );

#ifdef __cplusplus
}
#endif

#endif /* X264HIP_DEBLOCK_H */
