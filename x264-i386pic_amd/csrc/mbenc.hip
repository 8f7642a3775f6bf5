// The inter macroblock encode on gfx950 (include/x264hip_mbenc.h): the control flow of
// macroblock_encode_internal (reference encoder/macroblock.c:618-972) and
// mb_encode_chroma_internal (:259-490) for inter macroblocks over the transform cores of txdev.h.
//
// Mapping: 16 lanes per macroblock, four macroblocks per wave.  Luma (mbencdev.h's plane, shared
// with mb444.hip), transform 4: lane l owns the
// 4x4 block l of h->dct.luma4x4's order; transform 8: lanes 0..3 own the 8x8 blocks.  Chroma: lane
// c < 4 (4:2:0) or < 8 (4:2:2) owns the 4x4 position c of BOTH channels, the 8 interleaved samples
// of each of its rows, so that pixels move as whole dwords.  What the reference decides per 8x8,
// per macroblock and per chroma channel (the decimate sums, the 2x2 / 2x4 DC blocks) is gathered
// with ds_bpermute inside the macroblock's 16 lanes, and every lane then takes the decision
// itself: all branches that hold a cross-lane read are uniform over a macroblock's lanes, so
// macroblocks of different kinds (transform size, skip, intra) may share a wave.  The chroma
// channel and the cross-lane helpers are mbencdev.h's, shared with mbintra.hip.
#include "mbencdev.h"
#include "x264hip_mbenc.h"

#include <string.h>

namespace x264hip {

// x264_lambda2_tab, reference common/tables.c:114-127 (pinned by tests/test_cpu_mbenc.py)
__constant__ int c_lambda2_tab[82] = {
    14, 18, 22, 28, 36, 45, 57, 72,
    91, 115, 145, 182, 230, 290, 365, 460,
    580, 731, 921, 1161, 1462, 1843, 2322, 2925,
    3686, 4644, 5851, 7372, 9289, 11703, 14745, 18578,
    23407, 29491, 37156, 46814, 58982, 74313, 93628, 117964,
    148626, 187257, 235929, 297252, 374514, 471859, 594505, 749029,
    943718, 1189010, 1498059, 1887436, 2378021, 2996119, 3774873, 4756042,
    5992238, 7549747, 9512085, 11984476, 15099494, 19024170, 23968953, 30198988,
    38048341, 47937906, 60397977, 76096683, 95875813, 120795955,
    134217727, 134217727, 134217727, 134217727, 134217727, 134217727,
    134217727, 134217727, 134217727, 134217727, 134217727, 134217727,
};

constexpr int CQM_4PY = 1, CQM_4PC = 3, CQM_8PY = 1;   // reference common/set.h

// the launch's inputs, by value in the kernel arguments
template <int BD> struct MbEncParams
{
    using pixel = typename PT<BD>::pixel;
    using dctcoef = typename PT<BD>::dctcoef;
    using udctcoef = typename PT<BD>::udctcoef;
    const pixel *fenc, *fenc_c, *pred, *pred_c;
    pixel *recon, *recon_c;
    intptr_t fs, ffs, fcs, fcfs, ps, pfs, pcs, pcfs, rs, rfs, rcs, rcfs;
    const udctcoef *q4mf, *q4b, *q8mf, *q8b;
    const int32_t *dq4, *dq8;
    const int8_t *qp;
    const uint8_t *flags;
    dctcoef *level, *chroma_dc;
    uint8_t *nnz;
    int32_t *cbp, *nz;
    uint8_t *flags_out;
    int mbw, mbh, nmb, dec, al;               // al: level and chroma_dc are 16-byte aligned
    uint32_t cqp[16];                         // chroma_qp_table[0..63], four entries a word
};

template <int BD, int CF>
__global__ __launch_bounds__( 256 ) void mb_encode_inter_kernel( const MbEncParams<BD> a )
{
    using pixel = typename PT<BD>::pixel;
    using dctcoef = typename PT<BD>::dctcoef;
    constexpr int QP1 = 52 + 6 * (BD - 8);
    // the chroma qp table, indexed per lane below
    __shared__ uint32_t s_cqp[16];
#pragma unroll
    for( int k = 0; k < 16; k++ )
        if( threadIdx.x == k )
            s_cqp[k] = a.cqp[k];
    __syncthreads();
    const int l = threadIdx.x & 15;
    const int slot = (threadIdx.x & 63) >> 4;                  // the macroblock's place in its wave
    const int mb = blockIdx.x * 16 + (threadIdx.x >> 4);
    if( mb >= a.nmb )
        return;
    const int fl = a.flags[mb];
    if( fl & X264HIP_MBENC_INTRA )
    {
        if( l == 0 )
            a.flags_out[mb] = (uint8_t)fl;
        return;
    }
    const int per = a.mbw * a.mbh;
    const int f = mb / per, rem = mb - f * per;
    const int mby = rem / a.mbw, mbx = rem - mby * a.mbw;
    const int qp = min( max( (int)a.qp[mb], 0 ), QP1 - 1 );
    const bool skip = fl & X264HIP_MBENC_SKIP;
    const bool t8 = (fl & X264HIP_MBENC_T8x8) && a.q8mf;
    const bool al = a.al;
    dctcoef *lvl = a.level + (int64_t)mb * (48 * 16);

    // ---------------------------------------------------------------- luma
    // one plane (mbencdev.h): i_decimate_mb at the test after it is the plane's own sum
    PlaneCtx<BD> k;
    k.fenc = a.fenc + (intptr_t)f * a.ffs + (intptr_t)(16 * mby) * a.fs + 16 * mbx;
    k.pred = a.pred + (intptr_t)f * a.pfs + (intptr_t)(16 * mby) * a.ps + 16 * mbx;
    k.recon = a.recon + (intptr_t)f * a.rfs + (intptr_t)(16 * mby) * a.rs + 16 * mbx;
    k.fs = a.fs; k.ps = a.ps; k.rs = a.rs;
    k.mf4 = a.q4mf + (CQM_4PY * QP1 + qp) * 16; k.bias4 = a.q4b + (CQM_4PY * QP1 + qp) * 16;
    k.mf8 = a.q8mf + (CQM_8PY * QP1 + qp) * 64; k.bias8 = a.q8b + (CQM_8PY * QP1 + qp) * 64;
    k.dq4 = a.dq4 + CQM_4PY * 6 * 16; k.dq8 = a.dq8 + CQM_8PY * 6 * 64;
    k.qp = qp; k.lvl = lvl; k.al = al;
    int lmask = 0;                             // non_zero_count of the 16 luma blocks, bit = block index
    int k4 = 0;                                // transform 8: the kept 8x8 blocks
    if( !t8 )
    {
        Inter4 s;
        inter_luma4_scores<BD>( k, l, a.dec, skip, s );
        const bool nn = inter_luma4_finish<BD>( k, l, s, s.plane_score );
        lmask = (int)((__ballot( nn ) >> (16 * slot)) & 0xffff);
    }
    else
    {
        Inter8 s;
        inter_luma8_scores<BD>( k, l, a.dec, skip, s );
        const bool keep = inter_luma8_finish<BD>( k, l, a.dec, s, s.plane_score );
        k4 = (int)((__ballot( keep ) >> (16 * slot)) & 0xf);
#pragma unroll
        for( int j = 0; j < 4; j++ )
            lmask |= ((k4 >> j) & 1) * (0xf << (4 * j));
    }
    int cbp_luma = k4;
    if( !t8 )
#pragma unroll
        for( int k = 0; k < 4; k++ )
            cbp_luma |= (((lmask >> (4 * k)) & 0xf) != 0) << k;

    // ---------------------------------------------------------------- chroma
    int cbp_chroma = 0, nnz_dc0 = 0, nnz_dc1 = 0, acm0 = 0, acm1 = 0;
    int dco[2][8];
    zero( dco[0] );
    zero( dco[1] );
    if constexpr( CF != 0 )
    {
        constexpr int NCB = CF == 1 ? 4 : 8, CH = CF == 1 ? 8 : 16;
        const bool mine = l < NCB;
        const int bx = l & 1, by = (l >> 1) & 3;
        const pixel *fp = a.fenc_c + (intptr_t)f * a.fcfs + (intptr_t)(CH * mby + 4 * by) * a.fcs + 16 * mbx + 8 * bx;
        const pixel *pp = a.pred_c + (intptr_t)f * a.pcfs + (intptr_t)(CH * mby + 4 * by) * a.pcs + 16 * mbx + 8 * bx;
        pixel *rp = a.recon_c + (intptr_t)f * a.rcfs + (intptr_t)(CH * mby + 4 * by) * a.rcs + 16 * mbx + 8 * bx;
        ChromaOut u, v;
        int du[4][4], dv[4][4];
#pragma unroll
        for( int y = 0; y < 4; y++ )
#pragma unroll
            for( int x = 0; x < 4; x++ )
                du[y][x] = dv[y][x] = 0;
        if( mine && !skip )
        {
#pragma unroll
            for( int y = 0; y < 4; y++ )
            {
                int e[8], p[8];
                read_row<BD, 8>( fp + y * a.fcs, e );
                read_row<BD, 8>( pp + y * a.pcs, p );
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    du[y][x] = e[2 * x] - p[2 * x];
                    dv[y][x] = e[2 * x + 1] - p[2 * x + 1];
                }
            }
        }
        if( !skip )
        {
            const int qpc = min( (int)((s_cqp[qp >> 2] >> (8 * (qp & 3))) & 255), QP1 - 1 - (CF == 2 ? 3 : 0) );
            // the early termination (macroblock.c:283-341): pixel_var2_8x8 / 8x16, pixel.c:206-231
            bool early = false, coded_u = false, coded_v = false;
            if( a.dec && qpc >= 18 )
            {
                int su = 0, sv = 0, qu = 0, qv = 0;
#pragma unroll
                for( int y = 0; y < 4; y++ )
#pragma unroll
                    for( int x = 0; x < 4; x++ )
                    {
                        su += du[y][x]; qu += du[y][x] * du[y][x];
                        sv += dv[y][x]; qv += dv[y][x] * dv[y][x];
                    }
                su = mb_sum( su ); sv = mb_sum( sv ); qu = mb_sum( qu ); qv = mb_sum( qv );
                constexpr int SHIFT = CF == 1 ? 6 : 7;
                const int thresh = CF == 2 ? (c_lambda2_tab[qpc] + 16) >> 5 : (c_lambda2_tab[qpc] + 32) >> 6;
                const int var2 = (int)( qu - ((int64_t)su * su >> SHIFT) + qv - ((int64_t)sv * sv >> SHIFT) );
                early = var2 < thresh * 4;
                coded_u = qu > thresh;
                coded_v = qv > thresh;
            }
            const ChromaTabs<BD> ct = { a.q4mf, a.q4b, a.dq4 };
            chroma_channel<BD, CF, CQM_4PC, true>( ct, a.dec, du, l, qpc, early, coded_u, u );
            chroma_channel<BD, CF, CQM_4PC, true>( ct, a.dec, dv, l, qpc, early, coded_v, v );
            nnz_dc0 = u.nnz_dc; nnz_dc1 = v.nnz_dc;
            if( early )
                cbp_chroma = nnz_dc0 | nnz_dc1;
            else
            {
                const int t = u.ac | v.ac;                          // macroblock.c:487-489
                cbp_chroma = t + (nnz_dc0 | nnz_dc1 | t);
            }
#pragma unroll
            for( int k = 0; k < 8; k++ )
            {
                dco[0][k] = u.dc[k];
                dco[1][k] = v.dc[k];
            }
        }
        else
        {
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    u.res[y][x] = v.res[y][x] = 0;
            zero( u.lev );
            zero( v.lev );
            u.nnz_ac = v.nnz_ac = 0;
        }
        if( mine )
        {
#pragma unroll
            for( int y = 0; y < 4; y++ )
            {
                int p[8];
                read_row<BD, 8>( pp + y * a.pcs, p );
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    p[2 * x] = clip_pix<BD>( p[2 * x] + u.res[y][x] );
                    p[2 * x + 1] = clip_pix<BD>( p[2 * x + 1] + v.res[y][x] );
                }
                write_row<BD, 8>( rp + y * a.rcs, p );
            }
            const int blk = 16 + (l >> 2) * 8 + (l & 3);
            put_coefs<BD, 16>( lvl + blk * 16, u.lev, al );
            put_coefs<BD, 16>( lvl + (blk + 16) * 16, v.lev, al );
        }
        acm0 = (int)((__ballot( mine && u.nnz_ac ) >> (16 * slot)) & 0xff);
        acm1 = (int)((__ballot( mine && v.nnz_ac ) >> (16 * slot)) & 0xff);
    }

    // ---------------------------------------------------------------- the per-macroblock outputs
    // block 16 + l (and 32 + l): a chroma AC block of this format, owned by chroma lane `owner`?
    const bool cblk = CF == 1 ? l < 4 : CF == 2 ? !(l & 4) : false;
    const int owner = (l >> 3) * 4 + (l & 3);
    if( !cblk )
    {
        int z[16];
        zero( z );
        put_coefs<BD, 16>( lvl + (16 + l) * 16, z, al );
        put_coefs<BD, 16>( lvl + (32 + l) * 16, z, al );
    }
    uint8_t *nn = a.nnz + (int64_t)mb * 48;
    nn[l] = (uint8_t)((lmask >> l) & 1);
    nn[16 + l] = (uint8_t)(cblk ? (acm0 >> owner) & 1 : 0);
    nn[32 + l] = (uint8_t)(cblk ? (acm1 >> owner) & 1 : 0);
    if( l < 2 )
    {
        int o[8];
#pragma unroll
        for( int k = 0; k < 8; k++ )
            o[k] = l ? dco[1][k] : dco[0][k];
        put_coefs<BD, 8>( a.chroma_dc + (int64_t)mb * 16 + l * 8, o, al );
    }
    if( l == 0 )
    {
        const int cbp = cbp_chroma << 4 | cbp_luma | nnz_dc0 << 9 | nnz_dc1 << 10;
        a.cbp[mb] = cbp;
        a.nz[mb] = t8 ? k4 : lmask;
        a.flags_out[mb] = (uint8_t)((fl & 3) | ((fl & X264HIP_MBENC_D16x16) && !cbp ? X264HIP_MBENC_D16x16 : 0));
    }
}

// the arguments were checked by the C entry (capi.cpp x264hip_*_mb_encode_inter)
template <int BD>
hipError_t launch_mb_encode_inter( const x264hip_mbenc_t *e, int mbw, int mbh, int n_frames, hipStream_t stream )
{
    using pixel = typename PT<BD>::pixel;
    const int64_t nmb = (int64_t)n_frames * mbw * mbh;
    if( !e || nmb <= 0 )
        return hipSuccess;
    MbEncParams<BD> a;
    fill_mb_params<BD>( e, mbw, mbh, a );
    a.fenc = (const pixel *)e->fenc; a.fenc_c = (const pixel *)e->fenc_chroma;
    a.pred = (const pixel *)e->pred; a.pred_c = (const pixel *)e->pred_chroma;
    a.recon = (pixel *)e->recon; a.recon_c = (pixel *)e->recon_chroma;
    a.fs = e->fenc_stride; a.ffs = e->fenc_frame_stride;
    a.fcs = e->fenc_chroma_stride; a.fcfs = e->fenc_chroma_frame_stride;
    a.ps = e->pred_stride; a.pfs = e->pred_frame_stride;
    a.pcs = e->pred_chroma_stride; a.pcfs = e->pred_chroma_frame_stride;
    a.rs = e->recon_stride; a.rfs = e->recon_frame_stride;
    a.rcs = e->recon_chroma_stride; a.rcfs = e->recon_chroma_frame_stride;
    a.chroma_dc = (typename PT<BD>::dctcoef *)e->chroma_dc;
    a.nmb = (int)nmb;
    a.al = !(((uintptr_t)e->level | (uintptr_t)e->chroma_dc) & 15);
    const dim3 grid( (unsigned)((nmb + 15) / 16) ), blk( 256 );
    switch( e->chroma_format )
    {
        case 0: hipLaunchKernelGGL( ( mb_encode_inter_kernel<BD, 0> ), grid, blk, 0, stream, a ); break;
        case 1: hipLaunchKernelGGL( ( mb_encode_inter_kernel<BD, 1> ), grid, blk, 0, stream, a ); break;
        default: hipLaunchKernelGGL( ( mb_encode_inter_kernel<BD, 2> ), grid, blk, 0, stream, a ); break;
    }
    return hipGetLastError();
}
X264HIP_INSTANTIATE( launch_mb_encode_inter );

} // namespace x264hip
