// The intra macroblock encode on gfx950 (include/x264hip_mbintra.h): the control flow of
// macroblock_encode_internal for I_16x16 / I_4x4 / I_8x8 (reference encoder/macroblock.c:706-768,
// :126-239, :924-951, encoder/macroblock.h:132-213) and mb_encode_chroma_internal with b_inter = 0
// over the transform cores of txdev.h, the chroma channel of mbencdev.h and the predictors of
// common/predict.c.  The tile, the luma predictors and the three luma paths are mbintradev.h's,
// shared with mb444.hip.
//
// One launch per macroblock anti-diagonal d = x + 2y (deblock.hip's shape): the left, top-left,
// top and top-right neighbours of a macroblock lie on earlier diagonals, so no workgroup waits for
// another.  Mapping: 16 lanes per macroblock, four macroblocks per wave, one wave per workgroup.
// Each macroblock keeps an FDEC-style tile in shared memory: its 16x16 luma with the row above
// (17 + 8 top-right samples) and the column left, the same for both chroma channels, filled from
// recon once.  I_16x16 and chroma: lane l owns the 4x4 block l (chroma: position l of both
// channels) and predicts it from the tile's borders.  I_4x4: the blocks of one anti-diagonal
// bx + 2*by are independent, so the 16 blocks take ten steps, each lane writing its
// reconstruction into the tile for the later ones.  I_8x8: four steps; the 16 lanes build the
// filtered edge and the prediction in the tile, lane i transforms block i.  All branches that hold
// a cross-lane read or a tile exchange are uniform over a macroblock's 16 lanes.
#include "mbintradev.h"
#include "x264hip_mbintra.h"

#include <string.h>

namespace x264hip {
namespace {

constexpr int CQM_4IY = 0, CQM_4IC = 2, CQM_8IY = 0;                  // reference common/set.h
constexpr int CW = 10;                        // chroma tile row: left, 8, padding

// the launch's inputs, by value in the kernel arguments
template <int BD> struct MbIntraParams
{
    using pixel = typename PT<BD>::pixel;
    using dctcoef = typename PT<BD>::dctcoef;
    using udctcoef = typename PT<BD>::udctcoef;
    const pixel *fenc, *fenc_c;
    pixel *recon, *recon_c;
    intptr_t fs, ffs, fcs, fcfs, rs, rfs, rcs, rcfs;
    const udctcoef *q4mf, *q4b, *q8mf, *q8b;
    const int32_t *dq4, *dq8;
    const int8_t *qp;
    const uint8_t *flags;
    const int8_t *pmode, *cmode;
    dctcoef *level, *chroma_dc, *luma_dc;
    uint8_t *nnz;
    int32_t *cbp, *nz;
    uint8_t *flags_out;
    int mbw, mbh, dec, al;                    // al: level, chroma_dc and luma_dc are 16-byte aligned
    int d, ymin, count, nitems;               // the diagonal, its first row, its macroblocks per frame, in all
    uint32_t cqp[16];                         // chroma_qp_table[0..63], four entries a word
};

// predict_8x8c[mode] / predict_8x16c[mode] (common/predict.c:167-469) of the 4x4 block (bx, by) of
// one channel's tile
template <int BD, int CF>
__device__ __forceinline__ void pred_chroma( int mode, const tpx *b, int bx, int by, int (&p)[4][4] )
{
    auto T = [&]( int x ) { return (int)b[1 + x]; };
    auto L = [&]( int y ) { return (int)b[(1 + y) * CW]; };
    const int s0 = T( 0 ) + T( 1 ) + T( 2 ) + T( 3 ), s1 = T( 4 ) + T( 5 ) + T( 6 ) + T( 7 );
    const int st = bx ? s1 : s0;
    const int sl = L( 4 * by ) + L( 4 * by + 1 ) + L( 4 * by + 2 ) + L( 4 * by + 3 );
    switch( mode )
    {
        case 0:
            if( bx == 0 )
                fill( p, by == 0 ? (s0 + sl + 4) >> 3 : (sl + 2) >> 2 );
            else
                fill( p, by == 0 ? (s1 + 2) >> 2 : (s1 + sl + 4) >> 3 );
            break;
        case 1:
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    p[y][x] = L( 4 * by + y );
            break;
        case 2:
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    p[y][x] = T( 4 * bx + x );
            break;
        case 3:
        {
            int H = 0, V = 0;
#pragma unroll
            for( int i = 0; i < 4; i++ )
                H += (i + 1) * (T( 4 + i ) - T( 2 - i ));
            constexpr int NV = CF == 1 ? 4 : 8;
#pragma unroll
            for( int i = 0; i < NV; i++ )
                V += (i + 1) * (L( NV + i ) - L( NV - 2 - i ));
            const int a = 16 * (L( 2 * NV - 1 ) + T( 7 )), bb = (17 * H + 16) >> 5;
            const int c = CF == 1 ? (17 * V + 16) >> 5 : (5 * V + 32) >> 6;
            const int i00 = a - 3 * bb - (NV - 1) * c + 16;
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    p[y][x] = clip_pix<BD>( (i00 + bb * (4 * bx + x) + c * (4 * by + y)) >> 5 );
            break;
        }
        case 4: fill( p, (sl + 2) >> 2 ); break;
        case 5: fill( p, (st + 2) >> 2 ); break;
        default: fill( p, 1 << (BD - 1) ); break;
    }
}

template <int BD, int CF>
__global__ __launch_bounds__( 64 ) void mb_encode_intra_kernel( const MbIntraParams<BD> a )
{
    using pixel = typename PT<BD>::pixel;
    using dctcoef = typename PT<BD>::dctcoef;
    constexpr int QP1 = 52 + 6 * (BD - 8);
    __shared__ uint32_t s_cqp[16];
    __shared__ tpx s_y[4][TILE];              // [1 + y][1 + x]
    __shared__ tpx s_c[4][2][17 * CW];
    __shared__ tpx s_e[4][36];                // the filtered edge of an I_8x8 block
    if( threadIdx.x < 16 )
        s_cqp[threadIdx.x] = a.cqp[threadIdx.x];
    __syncthreads();
    const int l = threadIdx.x & 15, slot = threadIdx.x >> 4;
    const int item = blockIdx.x * 4 + slot;
    if( item >= a.nitems )
        return;
    const int f = item / a.count;
    const int my = a.ymin + (item - f * a.count), mx = a.d - 2 * my;
    const int mb = (f * a.mbh + my) * a.mbw + mx;
    const int fl = a.flags[mb];
    if( !(fl & X264HIP_MBENC_INTRA) )
        return;
    const int qp = min( max( (int)a.qp[mb], 0 ), QP1 - 1 );
    const bool left = mx > 0, top = my > 0, topright = top && mx + 1 < a.mbw;
    const int nb = (left ? NB_LEFT : 0) | (top ? NB_TOP : 0) | (left && top ? NB_TOPLEFT : 0) | (topright ? NB_TOPRIGHT : 0);
    const bool al = a.al;
    const bool i8 = (fl & X264HIP_MBENC_T8x8) && a.q8mf;
    const bool i16 = !(fl & X264HIP_MBENC_T8x8) && (fl & X264HIP_MBINTRA_I16x16);
    const int8_t *pm = a.pmode + (int64_t)mb * 16;
    dctcoef *lvl = a.level + (int64_t)mb * (48 * 16);
    tpx *ty = s_y[slot];

    // ---------------------------------------------------------------- the tiles' borders
    pixel *ry = a.recon + (intptr_t)f * a.rfs + (intptr_t)(16 * my) * a.rs + 16 * mx;
    int tpx_l, lpx_l;
    tile_borders<BD>( ty, ry, a.rs, l, nb, tpx_l, lpx_l );
    if constexpr( CF != 0 )
    {
        constexpr int CH = CF == 1 ? 8 : 16;
        const pixel *rc = a.recon_c + (intptr_t)f * a.rcfs + (intptr_t)(CH * my) * a.rcs + 16 * mx;
        s_c[slot][l & 1][1 + (l >> 1)] = (tpx)( top ? rc[-a.rcs + l] : 0 );
        if( l < CH )
        {
            s_c[slot][0][(1 + l) * CW] = (tpx)( left ? rc[l * a.rcs - 2] : 0 );
            s_c[slot][1][(1 + l) * CW] = (tpx)( left ? rc[l * a.rcs - 1] : 0 );
        }
        if( l < 2 )
            s_c[slot][l][0] = (tpx)( left && top ? rc[-a.rcs - 2 + l] : 0 );
    }
    tile_sync();

    // ---------------------------------------------------------------- luma
    // one plane (mbintradev.h, shared with mb444.hip)
    PlaneCtx<BD> k;
    k.fenc = a.fenc + (intptr_t)f * a.ffs + (intptr_t)(16 * my) * a.fs + 16 * mx;
    k.pred = nullptr;
    k.recon = ry;
    k.fs = a.fs; k.ps = 0; k.rs = a.rs;
    k.mf4 = a.q4mf + (CQM_4IY * QP1 + qp) * 16; k.bias4 = a.q4b + (CQM_4IY * QP1 + qp) * 16;
    k.mf8 = a.q8mf + (CQM_8IY * QP1 + qp) * 64; k.bias8 = a.q8b + (CQM_8IY * QP1 + qp) * 64;
    k.dq4 = a.dq4 + CQM_4IY * 6 * 16; k.dq8 = a.dq8 + CQM_8IY * 6 * 64;
    k.qp = qp; k.lvl = lvl; k.al = al;
    int lmask = 0, k4 = 0, cbp_luma = 0, nz_ldc = 0;
    int ldc[16];
    zero( ldc );
    if( i16 )
    {
        const bool nn = intra_i16_plane<BD>( k, ty, l, pm[0], a.dec, tpx_l, lpx_l, ldc, nz_ldc, cbp_luma );
        lmask = (int)((__ballot( nn ) >> (16 * slot)) & 0xffff);
    }
    else if( !i8 )
    {
        const int nzb = intra_i4_plane<BD>( k, ty, l, (fl & X264HIP_MBENC_T8x8) ? pm[l & 12] : pm[l], nb );
        lmask = (int)((__ballot( nzb ) >> (16 * slot)) & 0xffff);
#pragma unroll
        for( int j = 0; j < 4; j++ )
            cbp_luma |= (((lmask >> (4 * j)) & 0xf) != 0) << j;
    }
    else
    {
        const int nz8 = intra_i8_plane<BD>( k, ty, s_e[slot], l, pm, nb );
        k4 = (int)((__ballot( nz8 && l < 4 ) >> (16 * slot)) & 0xf);
        cbp_luma = k4;
#pragma unroll
        for( int j = 0; j < 4; j++ )
            lmask |= ((k4 >> j) & 1) * (0xf << (4 * j));
    }

    // ---------------------------------------------------------------- chroma
    int cbp_chroma = 0, nnz_dc0 = 0, nnz_dc1 = 0, acm0 = 0, acm1 = 0;
    int dco[2][8];
    zero( dco[0] );
    zero( dco[1] );
    if constexpr( CF != 0 )
    {
        constexpr int NCB = CF == 1 ? 4 : 8, CH = CF == 1 ? 8 : 16;
        const bool mine = l < NCB;
        const int cx = l & 1, cy = (l >> 1) & 3;
        const pixel *fp = a.fenc_c + (intptr_t)f * a.fcfs + (intptr_t)(CH * my + 4 * cy) * a.fcs + 16 * mx + 8 * cx;
        pixel *rp = a.recon_c + (intptr_t)f * a.rcfs + (intptr_t)(CH * my + 4 * cy) * a.rcs + 16 * mx + 8 * cx;
        int cmode = a.cmode[mb];
        cmode = (unsigned)cmode > 6 ? 6 : cmode;
        ChromaOut u, v;
        int pu[4][4], pv[4][4], du[4][4], dv[4][4];
        fill( pu, 0 );
        fill( pv, 0 );
        fill( du, 0 );
        fill( dv, 0 );
        if( mine )
        {
            pred_chroma<BD, CF>( cmode, s_c[slot][0], cx, cy, pu );
            pred_chroma<BD, CF>( cmode, s_c[slot][1], cx, cy, pv );
#pragma unroll
            for( int y = 0; y < 4; y++ )
            {
                int e[8];
                read_row<BD, 8>( fp + y * a.fcs, e );
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    du[y][x] = e[2 * x] - pu[y][x];
                    dv[y][x] = e[2 * x + 1] - pv[y][x];
                }
            }
        }
        const int qpc = min( (int)((s_cqp[qp >> 2] >> (8 * (qp & 3))) & 255), QP1 - 1 - (CF == 2 ? 3 : 0) );
        const ChromaTabs<BD> ct = { a.q4mf, a.q4b, a.dq4 };
        chroma_channel<BD, CF, CQM_4IC, false>( ct, false, du, l, qpc, false, false, u );
        chroma_channel<BD, CF, CQM_4IC, false>( ct, false, dv, l, qpc, false, false, v );
        nnz_dc0 = u.nnz_dc; nnz_dc1 = v.nnz_dc;
        const int t = u.ac | v.ac;                              // macroblock.c:487-489
        cbp_chroma = t + (nnz_dc0 | nnz_dc1 | t);
#pragma unroll
        for( int k = 0; k < 8; k++ )
        {
            dco[0][k] = u.dc[k];
            dco[1][k] = v.dc[k];
        }
        if( mine )
        {
#pragma unroll
            for( int y = 0; y < 4; y++ )
            {
                int p[8];
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    p[2 * x] = clip_pix<BD>( pu[y][x] + u.res[y][x] );
                    p[2 * x + 1] = clip_pix<BD>( pv[y][x] + v.res[y][x] );
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
    if( l == 2 )
        put_coefs<BD, 16>( a.luma_dc + (int64_t)mb * 16, ldc, al );
    if( l == 0 )
    {
        a.cbp[mb] = cbp_chroma << 4 | cbp_luma | nz_ldc << 8 | nnz_dc0 << 9 | nnz_dc1 << 10;
        a.nz[mb] = i8 ? k4 : lmask;
        a.flags_out[mb] = (uint8_t)(fl & 3);
    }
}

template <int BD, int CF>
void mb_encode_intra_go( const MbIntraParams<BD> &a, hipStream_t stream )
{
    hipLaunchKernelGGL( ( mb_encode_intra_kernel<BD, CF> ), dim3( (unsigned)((a.nitems + 3) / 4) ), dim3( 64 ), 0, stream, a );
}

} // namespace

// the arguments were checked by the C entry (capi.cpp x264hip_*_mb_encode_intra)
template <int BD>
hipError_t launch_mb_encode_intra( const x264hip_mbintra_t *e, int mbw, int mbh, int n_frames, hipStream_t stream )
{
    using pixel = typename PT<BD>::pixel;
    using dctcoef = typename PT<BD>::dctcoef;
    if( !e || mbw <= 0 || mbh <= 0 || n_frames <= 0 )
        return hipSuccess;
    MbIntraParams<BD> a;
    fill_mb_params<BD>( e, mbw, mbh, a );
    a.fenc = (const pixel *)e->fenc; a.fenc_c = (const pixel *)e->fenc_chroma;
    a.recon = (pixel *)e->recon; a.recon_c = (pixel *)e->recon_chroma;
    a.fs = e->fenc_stride; a.ffs = e->fenc_frame_stride;
    a.fcs = e->fenc_chroma_stride; a.fcfs = e->fenc_chroma_frame_stride;
    a.rs = e->recon_stride; a.rfs = e->recon_frame_stride;
    a.rcs = e->recon_chroma_stride; a.rcfs = e->recon_chroma_frame_stride;
    a.pmode = e->pred_mode; a.cmode = e->chroma_pred_mode;
    a.chroma_dc = (dctcoef *)e->chroma_dc; a.luma_dc = (dctcoef *)e->luma_dc;
    a.al = !(((uintptr_t)e->level | (uintptr_t)e->chroma_dc | (uintptr_t)e->luma_dc) & 15);
    // one launch per anti-diagonal, in dependency order
    for_each_diagonal( mbw, mbh, [&]( int d, int ymin, int count )
    {
        a.d = d; a.ymin = ymin; a.count = count; a.nitems = count * n_frames;
        switch( e->chroma_format )
        {
            case 0: mb_encode_intra_go<BD, 0>( a, stream ); break;
            case 1: mb_encode_intra_go<BD, 1>( a, stream ); break;
            default: mb_encode_intra_go<BD, 2>( a, stream ); break;
        }
    } );
    return hipGetLastError();
}
X264HIP_INSTANTIATE( launch_mb_encode_intra );

} // namespace x264hip
