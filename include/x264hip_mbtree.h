/* x264hip_mbtree.h — MB-tree on the device: the step x264 runs on the lookahead's per-MB
 * arrays after slicetype_frame_cost (reference encoder/slicetype.c:1026-1184 macroblock_tree /
 * macroblock_tree_propagate / macroblock_tree_finish, common/mc.c:509-598 mbtree_propagate_cost /
 * mbtree_propagate_list).
 *
 * The inputs are exactly what the lookahead entries of x264hip.h leave in device memory
 * (i_intra_cost, lowres_costs[b-p0][p1-b] as (lists_used << 14) + cost, lowres_mvs[0/1]), so the
 * lookahead stays resident up to f_qp_offset.  All arrays are per MB and dense:
 * mb_count = mb_width * mb_height elements, row stride mb_width (the reference's i_mb_stride
 * equals i_mb_width, slicetype.c:525).  Nothing depends on the pixel bit depth.
 *
 * Float contract: every float operation is one IEEE single-precision round-to-nearest operation
 * in the reference source's order (no fused multiply-add, correctly rounded division), which is
 * what the reference's C build computes.  Results are bit-exact and reproducible run to run.
 *
 * Input domain (outside it the reference itself overflows an int or divides 0 by 0):
 *   intra_cost in [1, 0x7fff], inv_qscale in [1, 0x7fff], fps_factor in (0, 1], the integer
 *   fps_factor of finish in [1, 51200], every i_propagate_cost value <= 32767 on entry.
 *   The one deliberate addition: intra_cost == 0 propagates amount 0.
 *
 * Both entries are asynchronous on `stream` (a hipStream_t, NULL = the null stream) without a
 * host synchronisation; they return 0 or a negative X264HIP_E* (X264HIP_ENODEV without a device).
 */
#ifndef X264HIP_MBTREE_H
#define X264HIP_MBTREE_H

#include "x264hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One macroblock_tree_propagate( p0, p1, b, referenced ) step; every pointer is a device pointer. */
typedef struct x264hip_mbtree_step_t
{
    const uint16_t *intra_cost;     /* frames[b]->i_intra_cost */
    const uint16_t *lowres_costs;   /* frames[b]->lowres_costs[b-p0][p1-b] */
    const uint16_t *inv_qscale;     /* i_inv_qscale_factor; NULL = 256 everywhere (AQ off, ratecontrol.c:333) */
    const uint16_t *propagate_in;   /* frames[b]->i_propagate_cost; NULL = not referenced (zeros) */
    const int16_t  *mvs[2];         /* lowres_mvs[0][b-p0-1], lowres_mvs[1][p1-b-1]; mvs[1] NULL when b == p1 */
    uint16_t       *ref_costs[2];   /* i_propagate_cost of p0 / p1, read-modify-write; [1] ignored when mvs[1] is NULL */
    float           fps_factor;     /* slicetype.c:1063 */
    int32_t         bipred_weight;  /* slicetype.c:1055; list 1 uses 64 - bipred_weight */
} x264hip_mbtree_step_t;

/* steps: host array of n >= 1 steps holding device pointers.
 *
 * Every MC_CLIP_ADD adds a non-negative amount and clips at 32767, so the adds into one element
 * commute: the call sums them per destination in 32-bit accumulators (integer atomics) and
 * applies min( dst + sum, 32767 ) once.  Steps that write the same i_propagate_cost planes but do
 * not read each other's output may therefore share one call — all B frames between two non-B
 * frames do (they are unreferenced).  A call of any size is accepted; large batches are split
 * internally so the accumulators cannot wrap.
 *
 * X264HIP_EINVAL: n < 1, a non-positive dimension, a NULL intra_cost / lowres_costs / mvs[0] /
 * ref_costs[0] (or ref_costs[1] with mvs[1] set), bipred_weight outside [0, 64], a ref_costs
 * plane of any step overlapping the propagate_in of any step of the same call (an ordering the
 * batch cannot honour), or two ref_costs planes that overlap without being identical. */
int x264hip_mbtree_propagate( const x264hip_mbtree_step_t *steps, int n, int mb_width, int mb_height, void *stream );

/* macroblock_tree_finish (slicetype.c:1039-1048) of one frame:
 *   ic = (intra_cost[i] * inv_qscale[i] + 128) >> 8; elements with ic == 0 are not written;
 *   pc = (propagate_cost[i] * fps_factor + 128) >> 8;
 *   qp_offset[i] = qp_offset_aq[i] - strength * ((x264_log2( ic + pc ) - x264_log2( ic )) + weightdelta).
 * inv_qscale NULL = 256 everywhere; qp_offset may equal qp_offset_aq.  fps_factor and weightdelta
 * are the caller's slicetype.c:1031-1034, strength its 5.0f * (1.0f - f_qcompress).
 * X264HIP_EINVAL: mb_count < 1, fps_factor < 1 or a NULL pointer other than inv_qscale. */
int x264hip_mbtree_finish( const uint16_t *intra_cost, const uint16_t *inv_qscale, const uint16_t *propagate_cost,
                           const float *qp_offset_aq, float *qp_offset, int mb_count,
                           int fps_factor, float weightdelta, float strength, void *stream );

#ifdef __cplusplus
}
#endif

#endif /* X264HIP_MBTREE_H */
