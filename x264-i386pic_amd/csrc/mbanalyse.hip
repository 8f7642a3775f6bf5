// The intra mode decision on gfx950 (include/x264hip_mbanalyse.h): x264_mb_analyse_intra and
// mb_analyse_intra_chroma (reference encoder/analyse.c:586-980) with the decisions of
// x264_macroblock_analyse (:2939-2946, :3181-3223, :3591-3618), then the encode of the macroblocks
// that come out intra, in one kernel.
//
// The execution shape is mbintra.hip's: one launch per macroblock anti-diagonal d = x + 2y, 16
// lanes per macroblock, four macroblocks per wave, one wave per workgroup, the FDEC-style tiles in
// shared memory filled once from recon; the lanes of a macroblock meet through the tile with
// tile_sync().  A try macroblock is analysed first: I_16x16 and the chroma candidates one 4x4 block
// per lane (a 16x16 or chroma SATD is the sum of its 4x4 SATDs: the 16 coefficients of a 4x4
// Hadamard share a parity, so every block sum is even and the halving commutes with the sum),
// I_8x8 block by block, I_4x4 on the ten block anti-diagonals (mbanalysedev.h).  Trial
// reconstruction lives only in the tile; the borders stay, so the final encode of the decided
// type starts from the same neighbours.  The decided modes go to shared memory, from where the
// encode reads them for decided and given macroblocks alike.
//
// The macroblock's encode below (pred_chroma, chroma_borders, intra_mb_encode) is
// mb_encode_intra_kernel's body, kept as a copy: moving that body into a function shared by the
// two kernels changed mb_encode_intra_kernel's instruction stream.  All branches that
// hold a cross-lane read or a tile exchange are uniform over a macroblock's 16 lanes.
#include "mbanalysedev.h"
#include "x264hip_mbanalyse.h"

#include <string.h>

namespace x264hip {
namespace {

constexpr int CQM_4IY = 0, CQM_4IC = 2, CQM_8IY = 0;                  // reference common/set.h
constexpr int CW = 10;                        // chroma tile row: left, 8, padding

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

// the chroma tiles' borders from recon_c (a tile_sync() follows in the caller); c: [2][17 * CW]
template <int BD, int CF, typename P>
__device__ __forceinline__ void chroma_borders( const P &a, tpx (*c)[17 * CW], int l, int f, int mx, int my, bool left, bool top )
{
    using pixel = typename PT<BD>::pixel;
    constexpr int CH = CF == 1 ? 8 : 16;
    const pixel *rc = a.recon_c + (intptr_t)f * a.rcfs + (intptr_t)(CH * my) * a.rcs + 16 * mx;
    c[l & 1][1 + (l >> 1)] = (tpx)( top ? rc[-a.rcs + l] : 0 );
    if( l < CH )
    {
        c[0][(1 + l) * CW] = (tpx)( left ? rc[l * a.rcs - 2] : 0 );
        c[1][(1 + l) * CW] = (tpx)( left ? rc[l * a.rcs - 1] : 0 );
    }
    if( l < 2 )
        c[l][0] = (tpx)( left && top ? rc[-a.rcs - 2 + l] : 0 );
}

// One intra macroblock after its tiles' borders stand, as mb_encode_intra_kernel (mbintra.hip) runs
// it: macroblock_encode_internal's luma by type through intra_i16_plane / intra_i4_plane /
// intra_i8_plane, the chroma through chroma_channel, and every per-macroblock output.  a: the
// kernel's argument block; fl: the type bits; pm: the 16 modes; cm: the chroma mode (not read at
// CF == 0); s_cqp: the packed chroma qp table; ty, sc, se: the macroblock's tiles and edge buffer.
template <int BD, int CF, typename P>
__device__ __forceinline__ void intra_mb_encode( const P &a, const uint32_t *s_cqp, tpx *ty, tpx (*sc)[17 * CW], tpx *se,
                                                 int slot, int l, int f, int mx, int my, int mb, int fl, int qp, int nb,
                                                 const int8_t *pm, const int8_t *cm, int tpx_l, int lpx_l )
{
    using pixel = typename PT<BD>::pixel;
    using dctcoef = typename PT<BD>::dctcoef;
    constexpr int QP1 = 52 + 6 * (BD - 8);
    const bool al = a.al;
    const bool i8 = (fl & X264HIP_MBENC_T8x8) && a.q8mf;
    const bool i16 = !(fl & X264HIP_MBENC_T8x8) && (fl & X264HIP_MBINTRA_I16x16);
    dctcoef *lvl = a.level + (int64_t)mb * (48 * 16);
    pixel *ry = a.recon + (intptr_t)f * a.rfs + (intptr_t)(16 * my) * a.rs + 16 * mx;
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
        const int nz8 = intra_i8_plane<BD>( k, ty, se, l, pm, nb );
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
        int cmode = *cm;
        cmode = (unsigned)cmode > 6 ? 6 : cmode;
        ChromaOut u, v;
        int pu[4][4], pv[4][4], du[4][4], dv[4][4];
        fill( pu, 0 );
        fill( pv, 0 );
        fill( du, 0 );
        fill( dv, 0 );
        if( mine )
        {
            pred_chroma<BD, CF>( cmode, sc[0], cx, cy, pu );
            pred_chroma<BD, CF>( cmode, sc[1], cx, cy, pv );
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

// the launch's inputs, by value in the kernel arguments
template <int BD> struct MbAnalyseParams
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
    int8_t *pmode, *cmode;
    dctcoef *level, *chroma_dc, *luma_dc;
    uint8_t *nnz;
    int32_t *cbp, *nz;
    uint8_t *flags_out;
    const uint8_t *try_intra, *fast;
    const int32_t *satd_inter;
    uint8_t *flags_o;
    int32_t *cost;
    int mbw, mbh, dec, al;                    // al: level, chroma_dc and luma_dc are 16-byte aligned
    int d, ymin, count, nitems;               // the diagonal, its first row, its macroblocks per frame, in all
    int slice, subme, b_i4, b_i8, b_cme;
    uint32_t cqp[16];                         // chroma_qp_table[0..63], four entries a word
    uint32_t lam[32];                         // x264_lambda_tab[0..63], two entries a word
};

// mb_analyse_intra_chroma, analyse.c:615-664: chroma lane l owns position l of both channels.  The
// x3 branch and the list loop are one loop here: both score satd( U ) + satd( V ) + lambda *
// bs_size_ue( fixed mode ) in list order with COPY2_IF_LT.
template <int BD, int CF, typename P>
__device__ __forceinline__ void analyse_chroma( const P &a, tpx (*sc)[17 * CW], int l, int f, int mx, int my, int nb,
                                                int lambda, int &i_satd_chroma, int &i_predict8x8chroma )
{
    using pixel = typename PT<BD>::pixel;
    constexpr int NCB = CF == 1 ? 4 : 8, CH = CF == 1 ? 8 : 16;
    const bool mine = l < NCB;
    const int cx = l & 1, cy = (l >> 1) & 3;
    const pixel *fp = a.fenc_c + (intptr_t)f * a.fcfs + (intptr_t)(CH * my + 4 * cy) * a.fcs + 16 * mx + 8 * cx;
    int fu[4][4], fv[4][4];
    fill( fu, 0 );
    fill( fv, 0 );
    if( mine )
    {
#pragma unroll
        for( int y = 0; y < 4; y++ )
        {
            int e[8];
            read_row<BD, 8>( fp + y * a.fcs, e );
#pragma unroll
            for( int x = 0; x < 4; x++ )
            {
                fu[y][x] = e[2 * x];
                fv[y][x] = e[2 * x + 1];
            }
        }
    }
    const uint64_t list = chroma_mode_available( avail_idx( nb ) );
    i_satd_chroma = COST_MAX;
    i_predict8x8chroma = 0;
#pragma unroll 1
    for( int i = 0; mode_at( list, i ) != 15; i++ )
    {
        const int i_mode = mode_at( list, i );
        int s = 0;
        if( mine )
        {
            int p[4][4], d[4][4];
            pred_chroma<BD, CF>( i_mode, sc[0], cx, cy, p );
            sub4( fu, p, d );
            s = satd4( d );
            pred_chroma<BD, CF>( i_mode, sc[1], cx, cy, p );
            sub4( fv, p, d );
            s += satd4( d );
        }
        const int i_satd = mb_sum( s ) + lambda * ue_chroma( i_mode );
        if( i_satd < i_satd_chroma ) { i_satd_chroma = i_satd; i_predict8x8chroma = i_mode; }
    }
}

template <int BD, int CF>
__global__ __launch_bounds__( 64 ) void mb_analyse_intra_kernel( const MbAnalyseParams<BD> a )
{
    using pixel = typename PT<BD>::pixel;
    constexpr int QP1 = 52 + 6 * (BD - 8);
    __shared__ uint32_t s_cqp[16];
    __shared__ uint32_t s_lam[32];
    __shared__ tpx s_y[4][TILE];              // [1 + y][1 + x]
    __shared__ tpx s_c[4][2][17 * CW];
    __shared__ tpx s_e[4][36];                // the filtered edge of an I_8x8 block
    __shared__ int8_t s_pm[4][16];            // the macroblock's modes, given or decided
    __shared__ int8_t s_cm[4][4];             // its chroma mode (entry 0)
    __shared__ int8_t s_m4[4][16];            // the I_4x4 pass' modes
    __shared__ int8_t s_nm[4][8];             // the neighbour macroblocks' modes: left rows, top columns
    if( threadIdx.x < 16 )
        s_cqp[threadIdx.x] = a.cqp[threadIdx.x];
    if( threadIdx.x < 32 )
        s_lam[threadIdx.x] = a.lam[threadIdx.x];
    __syncthreads();
    const int l = threadIdx.x & 15, slot = threadIdx.x >> 4;
    const int item = blockIdx.x * 4 + slot;
    if( item >= a.nitems )
        return;
    const int f = item / a.count;
    const int my = a.ymin + (item - f * a.count), mx = a.d - 2 * my;
    const int mb = (f * a.mbh + my) * a.mbw + mx;
    int fl = a.flags[mb];
    const bool tr = a.try_intra[mb] != 0;
    if( !tr && !(fl & X264HIP_MBENC_INTRA) )
        return;
    const int qp = min( max( (int)a.qp[mb], 0 ), QP1 - 1 );
    const bool left = mx > 0, top = my > 0, topright = top && mx + 1 < a.mbw;
    const int nb = (left ? NB_LEFT : 0) | (top ? NB_TOP : 0) | (left && top ? NB_TOPLEFT : 0) | (topright ? NB_TOPRIGHT : 0);
    tpx *ty = s_y[slot];

    // ---------------------------------------------------------------- the tiles' borders
    pixel *ry = a.recon + (intptr_t)f * a.rfs + (intptr_t)(16 * my) * a.rs + 16 * mx;
    int tpx_l, lpx_l;
    tile_borders<BD>( ty, ry, a.rs, l, nb, tpx_l, lpx_l );
    if constexpr( CF != 0 )
        chroma_borders<BD, CF>( a, s_c[slot], l, f, mx, my, left, top );
    if( !tr )
    {
        s_pm[slot][l] = a.pmode[(int64_t)mb * 16 + l];
        if( CF != 0 && l == 0 )
            s_cm[slot][0] = a.cmode[mb];
    }
    else if( l < 8 )
    {
        // intra4x4_pred_mode of the left (rows 0..3: its blocks 5, 7, 13, 15) and top (columns 0..3:
        // its blocks 10, 11, 14, 15) macroblocks, common/macroblock.c:883-967 and :1727-1737
        const bool lft = l < 4;
        int m = -1;
        if( lft ? left : top )
        {
            const int n = lft ? mb - 1 : mb - a.mbw;
            const int nfl = a.try_intra[n] ? a.flags_o[n] : a.flags[n];
            const bool i4 = (nfl & X264HIP_MBENC_INTRA) && !(nfl & (X264HIP_MBENC_T8x8 | X264HIP_MBINTRA_I16x16));
            const int blk = lft ? 5 + 2 * (l & 1) + 8 * (l >> 1) : 10 + (l & 1) + 4 * ((l >> 1) & 1);
            m = i4 ? (int)a.pmode[(int64_t)n * 16 + blk] : 2;
        }
        s_nm[slot][l] = (int8_t)m;
    }
    tile_sync();

    // ---------------------------------------------------------------- the decision
    if( tr )
    {
        const int lambda = (int)((s_lam[qp >> 1] >> (16 * (qp & 1))) & 0xffff);
        const int i_satd_inter = a.slice == 0 ? COST_MAX : a.satd_inter[mb];
        const bool b_fast_intra = a.fast && a.fast[mb];
        const bool chroma_first = CF != 0 && a.slice != 0 && a.b_cme;   // analyse.c:3181-3196, 3591-3606
        const int b_prefix = a.slice == 2 ? lambda * MB_B_COST_INTRA : 0;  // :736-738, 756, 874
        const int bx = blk_x( l ), by = blk_y( l );
        PlaneCtx<BD> k;
        k.fenc = a.fenc + (intptr_t)f * a.ffs + (intptr_t)(16 * my) * a.fs + 16 * mx;
        k.pred = nullptr;
        k.recon = ry;
        k.fs = a.fs; k.ps = 0; k.rs = a.rs;
        k.mf4 = a.q4mf + (CQM_4IY * QP1 + qp) * 16; k.bias4 = a.q4b + (CQM_4IY * QP1 + qp) * 16;
        k.mf8 = a.q8mf + (CQM_8IY * QP1 + qp) * 64; k.bias8 = a.q8b + (CQM_8IY * QP1 + qp) * 64;
        k.dq4 = a.dq4 + CQM_4IY * 6 * 16; k.dq8 = a.dq8 + CQM_8IY * 6 * 64;
        k.qp = qp; k.lvl = nullptr; k.al = false;
        int fe[4][4];
#pragma unroll
        for( int y = 0; y < 4; y++ )
            read_row<BD, 4>( k.fenc + (4 * by + y) * k.fs + 4 * bx, fe[y] );

        int i_satd_chroma = COST_MAX, cmode = 0;
        if constexpr( CF != 0 )
            if( chroma_first )
                analyse_chroma<BD, CF>( a, s_c[slot], l, f, mx, my, nb, lambda, i_satd_chroma, cmode );
        const int i_satd_luma = chroma_first ? i_satd_inter - i_satd_chroma : i_satd_inter;

        // I_16x16, :690-742
        const int i16x16_thresh = b_fast_intra ? (i16x16_thresh_lut( a.subme ) * i_satd_luma) >> 1 : COST_MAX;
        int i_satd_i16x16 = COST_MAX, i_satd_i8x8 = COST_MAX, i_satd_i4x4 = COST_MAX, i_predict16x16 = 0;
        {
            const int st = mb_sum( tpx_l ), sl = mb_sum( lpx_l );
            const int ai = avail_idx( nb );
            const uint64_t list = i16x16_mode_available( ai );
#pragma unroll 1
            for( int i = 0; mode_at( list, i ) != 15; i++ )
            {
                const int i_mode = mode_at( list, i );
                if( ai == 4 && i_mode == 3 && i_satd_i16x16 > i16x16_thresh )   // Plane, :709
                    break;
                int p[4][4], d[4][4];
                pred16x16<BD>( i_mode, ty, 4 * bx, 4 * by, st, sl, p );
                sub4( fe, p, d );
                const int i_satd = mb_sum( satd4( d ) ) + lambda * ue_mode16( i_mode );
                if( i_satd < i_satd_i16x16 ) { i_satd_i16x16 = i_satd; i_predict16x16 = i_mode; }
            }
        }
        i_satd_i16x16 += b_prefix;
        bool go = i_satd_i16x16 <= i16x16_thresh;                 // :740

        // I_8x8, :746-862
        I8Out o8;
        o8.mode[0] = o8.mode[1] = o8.mode[2] = o8.mode[3] = 2;
        if( go && a.b_i8 )
        {
            analyse_i8_plane<BD>( k, ty, s_e[slot], s_nm[slot], l, nb, lambda, lambda * 4 + b_prefix,
                                  min( i_satd_luma, i_satd_i16x16 ), o8 );
            i_satd_i8x8 = o8.i_satd_i8x8;
            if( min( o8.i_cost, i_satd_i16x16 ) > (i_satd_luma * i8x8_thresh( a.subme )) >> 2 )   // :860
                go = false;
        }

        // I_4x4, :865-979: every block is scored, then the loop's early termination is replayed
        // over the sixteen costs in the reference's order
        int mode4 = 2;
        if( go && a.b_i4 )
        {
            const int block_cost = analyse_i4_plane<BD>( k, ty, s_m4[slot], s_nm[slot], l, nb, lambda, fe );
            const int i_satd_thresh = min( i_satd_luma, min( i_satd_i16x16, i_satd_i8x8 ) );
            int i_cost = lambda * (24 + 16) + b_prefix, idx;
#pragma unroll 1
            for( idx = 0;; idx++ )
            {
                i_cost += mb_lane( block_cost, idx );
                if( i_cost > i_satd_thresh || idx == 15 )
                    break;
            }
            if( idx == 15 )
                i_satd_i4x4 = i_cost;
            mode4 = s_m4[slot][l];
        }

        if( chroma_first )
        {
            i_satd_i16x16 += i_satd_chroma;
            i_satd_i8x8 += i_satd_chroma;
            i_satd_i4x4 += i_satd_chroma;
        }
        int type = -1;                                            // -1 inter, 0 I_4x4, 1 I_8x8, 2 I_16x16
        if( a.slice == 0 )                                        // :2943-2946
        {
            int i_cost = i_satd_i16x16;
            type = 2;
            if( i_satd_i4x4 < i_cost ) { i_cost = i_satd_i4x4; type = 0; }
            if( i_satd_i8x8 < i_cost ) { i_cost = i_satd_i8x8; type = 1; }
        }
        else                                                      // :3221-3223, :3616-3618
        {
            int i_cost = i_satd_inter;
            if( i_satd_i16x16 < i_cost ) { i_cost = i_satd_i16x16; type = 2; }
            if( i_satd_i8x8 < i_cost ) { i_cost = i_satd_i8x8; type = 1; }
            if( i_satd_i4x4 < i_cost ) { i_cost = i_satd_i4x4; type = 0; }
        }
        if( type >= 0 && !chroma_first )                          // analyse_update_cache
        {
            i_satd_chroma = 0;
            if constexpr( CF != 0 )
                analyse_chroma<BD, CF>( a, s_c[slot], l, f, mx, my, nb, lambda, i_satd_chroma, cmode );
        }
        const int newfl = X264HIP_MBENC_INTRA | (type == 1 ? X264HIP_MBENC_T8x8 : type == 2 ? X264HIP_MBINTRA_I16x16 : 0);
        if( l < 4 )
            a.cost[(int64_t)mb * 4 + l] = l == 0 ? i_satd_i16x16 : l == 1 ? i_satd_i8x8 : l == 2 ? i_satd_i4x4 : i_satd_chroma;
        if( l == 0 )
            a.flags_o[mb] = (uint8_t)( type >= 0 ? newfl : fl );
        if( type < 0 )
            return;
        fl = newfl;
        const int mode = type == 2 ? (l == 0 ? i_predict16x16 : 2) : type == 1 ? pick( o8.mode, l >> 2 ) : mode4;
        s_pm[slot][l] = (int8_t)mode;
        a.pmode[(int64_t)mb * 16 + l] = (int8_t)mode;
        if( CF != 0 && l == 0 )
        {
            s_cm[slot][0] = (int8_t)cmode;
            a.cmode[mb] = (int8_t)cmode;
        }
        tile_sync();
    }

    // ---------------------------------------------------------------- the encode
    intra_mb_encode<BD, CF>( a, s_cqp, ty, s_c[slot], s_e[slot], slot, l, f, mx, my, mb, fl, qp, nb, s_pm[slot], s_cm[slot],
                             tpx_l, lpx_l );
}

template <int BD, int CF>
void mb_analyse_intra_go( const MbAnalyseParams<BD> &a, hipStream_t stream )
{
    hipLaunchKernelGGL( ( mb_analyse_intra_kernel<BD, CF> ), dim3( (unsigned)((a.nitems + 3) / 4) ), dim3( 64 ), 0, stream, a );
}

} // namespace

// the arguments were checked by the C entry (capi.cpp x264hip_*_mb_analyse_intra)
template <int BD>
hipError_t launch_mb_analyse_intra( const x264hip_mbanalyse_t *e, int mbw, int mbh, int n_frames, hipStream_t stream )
{
    using pixel = typename PT<BD>::pixel;
    using dctcoef = typename PT<BD>::dctcoef;
    if( !e || mbw <= 0 || mbh <= 0 || n_frames <= 0 )
        return hipSuccess;
    MbAnalyseParams<BD> a;
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
    a.try_intra = e->try_intra; a.fast = e->fast_intra; a.satd_inter = e->satd_inter;
    a.flags_o = e->mb_flags_out; a.cost = e->cost;
    a.slice = e->slice_type; a.subme = e->i_subpel_refine;
    a.b_i4 = e->b_i4x4 != 0; a.b_i8 = e->b_i8x8 != 0; a.b_cme = e->b_chroma_me != 0;
    // x264_lambda_tab[0 .. QP_MAX_SPEC] into the argument block, as pack_cqp carries the chroma qp table
    uint16_t lam[64] = { 0 };
    memcpy( lam, e->lambda_tab, (52 + 6 * (BD - 8)) * sizeof( uint16_t ) );
    memcpy( a.lam, lam, sizeof( lam ) );
    // one launch per anti-diagonal, in dependency order
    for_each_diagonal( mbw, mbh, [&]( int d, int ymin, int count )
    {
        a.d = d; a.ymin = ymin; a.count = count; a.nitems = count * n_frames;
        switch( e->chroma_format )
        {
            case 0: mb_analyse_intra_go<BD, 0>( a, stream ); break;
            case 1: mb_analyse_intra_go<BD, 1>( a, stream ); break;
            default: mb_analyse_intra_go<BD, 2>( a, stream ); break;
        }
    } );
    return hipGetLastError();
}
X264HIP_INSTANTIATE( launch_mb_analyse_intra );

} // namespace x264hip
