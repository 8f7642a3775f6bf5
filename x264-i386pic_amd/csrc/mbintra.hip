// The intra macroblock encode on gfx950 (include/x264hip_mbintra.h): the control flow of
// macroblock_encode_internal for I_16x16 / I_4x4 / I_8x8 (reference encoder/macroblock.c:706-768,
// :126-239, :924-951, encoder/macroblock.h:132-213) and mb_encode_chroma_internal with b_inter = 0
// over the transform cores of txdev.h, the chroma channel of mbencdev.h and the predictors of
// common/predict.c.
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
#include "intradev.h"
#include "mbencdev.h"
#include "x264hip_mbintra.h"

#include <string.h>

namespace x264hip {
namespace {

constexpr int CQM_4IY = 0, CQM_4IC = 2, CQM_8IY = 0;                  // reference common/set.h
constexpr int NB_LEFT = 1, NB_TOP = 2, NB_TOPRIGHT = 4, NB_TOPLEFT = 8;   // common/macroblock.h:33-36

typedef uint16_t tpx;                         // a tile sample
constexpr int TW = 28;                        // tile row: left, 16, 8 top-right (row 0), padding
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

// what one lane wrote to the tile is read by the other lanes of its macroblock (the same wave)
__device__ __forceinline__ void tile_sync()
{
    __builtin_amdgcn_fence( __ATOMIC_RELEASE, "workgroup" );
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "workgroup" );
}

template <int N> __device__ __forceinline__ void fill( int (&p)[N][N], int v )
{
#pragma unroll
    for( int y = 0; y < N; y++ )
#pragma unroll
        for( int x = 0; x < N; x++ )
            p[y][x] = v;
}

// predict_4x4[mode] (common/predict.c:481-621) from the 13 neighbours: t top and top-right, lf
// left, lt; the six directional modes in closed form over n[] = l3 l2 l1 l0 lt t0 t1 t2 t3
template <int BD>
__device__ __forceinline__ void pred4x4( int mode, const int (&t)[8], const int (&lf)[4], int lt, int (&p)[4][4] )
{
    const int n[9] = { lf[3], lf[2], lf[1], lf[0], lt, t[0], t[1], t[2], t[3] };
    const int st = t[0] + t[1] + t[2] + t[3], sl = lf[0] + lf[1] + lf[2] + lf[3];
    switch( mode )
    {
        case 0:
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    p[y][x] = t[x];
            break;
        case 1:
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    p[y][x] = lf[y];
            break;
        case 2: fill( p, (st + sl + 4) >> 3 ); break;
        case 3:   // DDL
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    const int z = x + y;
                    p[y][x] = f2( t[z], t[z + 1], t[z + 2 < 7 ? z + 2 : 7] );
                }
            break;
        case 4:   // DDR
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    const int c = 4 + x - y;
                    p[y][x] = f2( n[c - 1], n[c], n[c + 1] );
                }
            break;
        case 5:   // VR
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    const int z = 2 * x - y;
                    if( z < 0 )
                        p[y][x] = f2( n[4 + z], n[5 + z], n[6 + z] );
                    else if( !(z & 1) )
                        p[y][x] = f1( n[4 + z / 2], n[5 + z / 2] );
                    else
                        p[y][x] = f2( n[4 + z / 2], n[5 + z / 2], n[6 + z / 2] );
                }
            break;
        case 6:   // HD
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    const int z = 2 * y - x;
                    if( z < 0 )
                        p[y][x] = f2( n[2 - z], n[3 - z], n[4 - z] );
                    else if( !(z & 1) )
                        p[y][x] = f1( n[4 - z / 2], n[3 - z / 2] );
                    else
                        p[y][x] = f2( n[4 - z / 2], n[3 - z / 2], n[2 - z / 2] );
                }
            break;
        case 7:   // VL
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    const int c = x + (y >> 1);
                    p[y][x] = (y & 1) ? f2( t[c], t[c + 1], t[c + 2] ) : f1( t[c], t[c + 1] );
                }
            break;
        case 8:   // HU
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    const int z = x + 2 * y, c = z >> 1;
                    if( z > 5 )
                        p[y][x] = lf[3];
                    else if( z == 5 )
                        p[y][x] = f2( lf[2], lf[3], lf[3] );
                    else
                        p[y][x] = (z & 1) ? f2( lf[c], lf[c + 1], lf[c + 2 < 3 ? c + 2 : 3] ) : f1( lf[c], lf[c + 1] );
                }
            break;
        case 9: fill( p, (sl + 2) >> 2 ); break;
        case 10: fill( p, (st + 2) >> 2 ); break;
        default: fill( p, 1 << (BD - 1) ); break;
    }
}

// one entry of predict_8x8_filter's edge (common/predict.c:632-675) for the 8x8 block whose
// pixel (0,0) is at tile[1][1] of `b`: every entry is formed, whatever the mode's filter set
// (a mode reads only the entries its set covers); a sample the block's neighbours do not give is
// not read
__device__ __forceinline__ int edge_at( const tpx *b, int k, bool have_lt, bool have_tr )
{
    auto S = [&]( int x, int y ) { return (int)b[(1 + y) * TW + 1 + x]; };
    if( k <= 14 )
    {
        const int y = k < 7 ? 7 : 14 - k;
        if( y == 7 )
            return (S( -1, 6 ) + 3 * S( -1, 7 ) + 2) >> 2;
        if( y == 0 )
            return ((have_lt ? S( -1, -1 ) : S( -1, 0 )) + 2 * S( -1, 0 ) + S( -1, 1 ) + 2) >> 2;
        return f2( S( -1, y - 1 ), S( -1, y ), S( -1, y + 1 ) );
    }
    if( k == 15 )
        return f2( S( 0, -1 ), S( -1, -1 ), S( -1, 0 ) );
    const int x = k > 31 ? 15 : k - 16;
    if( x == 0 )
        return ((have_lt ? S( -1, -1 ) : S( 0, -1 )) + 2 * S( 0, -1 ) + S( 1, -1 ) + 2) >> 2;
    if( x < 7 )
        return f2( S( x - 1, -1 ), S( x, -1 ), S( x + 1, -1 ) );
    if( x == 7 )
        return (S( 6, -1 ) + 2 * S( 7, -1 ) + (have_tr ? S( 8, -1 ) : S( 7, -1 )) + 2) >> 2;
    if( !have_tr )
        return S( 7, -1 );
    if( x == 15 )
        return (S( 14, -1 ) + 3 * S( 15, -1 ) + 2) >> 2;
    return f2( S( x - 1, -1 ), S( x, -1 ), S( x + 1, -1 ) );
}

// predict_8x8[mode] (common/predict.c:700-884) at (x, y) from the edge; dc: the value of the
// mode's DC variant
__device__ __forceinline__ int pred8_px( int mode, const tpx *e, int x, int y, int dc )
{
    switch( mode )
    {
        case 0: return e[16 + x];
        case 1: return e[14 - y];
        case 3: return pred8_dir<3>( e, x, y );
        case 4: return pred8_dir<4>( e, x, y );
        case 5: return pred8_dir<5>( e, x, y );
        case 6: return pred8_dir<6>( e, x, y );
        case 7: return pred8_dir<7>( e, x, y );
        case 8: return pred8_dir<8>( e, x, y );
        default: return dc;
    }
}

// predict_16x16[mode] (common/predict.c:67-160) of the 4x4 block at (x0, y0); st / sl: the sums of
// the 16 top / left samples
template <int BD>
__device__ __forceinline__ void pred16x16( int mode, const tpx *b, int x0, int y0, int st, int sl, int (&p)[4][4] )
{
    auto T = [&]( int x ) { return (int)b[1 + x]; };
    auto L = [&]( int y ) { return (int)b[(1 + y) * TW]; };
    switch( mode )
    {
        case 0:
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    p[y][x] = T( x0 + x );
            break;
        case 1:
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    p[y][x] = L( y0 + y );
            break;
        case 2: fill( p, (st + sl + 16) >> 5 ); break;
        case 3:
        {
            int H = 0, V = 0;
#pragma unroll
            for( int i = 0; i < 8; i++ )
            {
                H += (i + 1) * (T( 8 + i ) - T( 6 - i ));
                V += (i + 1) * (L( 8 + i ) - L( 6 - i ));
            }
            const int a = 16 * (L( 15 ) + T( 15 )), bb = (5 * H + 32) >> 6, c = (5 * V + 32) >> 6;
            const int i00 = a - 7 * bb - 7 * c + 16;
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    p[y][x] = clip_pix<BD>( (i00 + bb * (x0 + x) + c * (y0 + y)) >> 5 );
            break;
        }
        case 4: fill( p, (sl + 8) >> 4 ); break;
        case 5: fill( p, (st + 8) >> 4 ); break;
        default: fill( p, 1 << (BD - 1) ); break;
    }
}

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
    using udctcoef = typename PT<BD>::udctcoef;
    constexpr int QP1 = 52 + 6 * (BD - 8);
    __shared__ uint32_t s_cqp[16];
    __shared__ tpx s_y[4][17 * TW];           // [1 + y][1 + x]
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
    const int tpx_l = top ? ry[-a.rs + l] : 0, lpx_l = left ? ry[l * a.rs - 1] : 0;
    ty[1 + l] = (tpx)tpx_l;
    ty[(1 + l) * TW] = (tpx)lpx_l;
    if( l < 8 )
        ty[17 + l] = (tpx)( topright ? ry[-a.rs + 16 + l] : 0 );
    if( l == 0 )
        ty[0] = (tpx)( left && top ? ry[-a.rs - 1] : 0 );
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
    // lane l's 4x4 block of h->dct.luma4x4's order
    const int bx = ((l >> 2) & 1) * 2 + (l & 1), by = (l >> 3) * 2 + ((l >> 1) & 1);
    const pixel *fy = a.fenc + (intptr_t)f * a.ffs + (intptr_t)(16 * my) * a.fs + 16 * mx;
    int lmask = 0, k4 = 0, cbp_luma = 0, nz_ldc = 0;
    int ldc[16];
    zero( ldc );
    if( i16 )
    {
        // mb_encode_i16x16, macroblock.c:126-239
        int mode = pm[0];
        mode = (unsigned)mode > 6 ? 6 : mode;
        int p[4][4], d[4][4], c[16];
        pred16x16<BD>( mode, ty, 4 * bx, 4 * by, mb_sum( tpx_l ), mb_sum( lpx_l ), p );
#pragma unroll
        for( int y = 0; y < 4; y++ )
        {
            int e[4];
            read_row<BD, 4>( fy + (4 * by + y) * a.fs + 4 * bx, e );
#pragma unroll
            for( int x = 0; x < 4; x++ )
                d[y][x] = e[x] - p[y][x];
        }
        dct4x4_core<BD>( d, c );
        const int c0 = c[0];
        c[0] = 0;
        const udctcoef *mf = a.q4mf + (CQM_4IY * QP1 + qp) * 16, *bias = a.q4b + (CQM_4IY * QP1 + qp) * 16;
        int acc = 0;
#pragma unroll
        for( int k = 0; k < 16; k++ )
        {
            c[k] = sto<BD>( quant_one( c[k], mf[k], bias[k] ) );
            acc |= c[k];
        }
        const int nzb = acc != 0;
        int score = 0;
        if( a.dec && nzb )
            score = decimate_score<16, 1>( [&]( int i ) { return c[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )]; } );
        int decimate = a.dec ? 0 : 9, any = 0;
#pragma unroll
        for( int k = 0; k < 16; k++ )
        {
            const int nzk = mb_lane( nzb, k ), sk = mb_lane( score, k );
            if( nzk )
            {
                any = 1;
                if( decimate < 6 )
                    decimate += sk;
            }
        }
        const bool block_cbp = any && decimate >= 6;
        cbp_luma = block_cbp ? 0xf : 0;
        // the DC block, dct_dc4x4[block_idx_xy_1d[idx]]: raster order
        int dcs[16];
#pragma unroll
        for( int r = 0; r < 16; r++ )
        {
            const int rx = r & 3, ryy = r >> 2;
            dcs[r] = mb_lane( c0, ((ryy >> 1) * 2 + (rx >> 1)) * 4 + (ryy & 1) * 2 + (rx & 1) );
        }
        had4x4dc<BD, true>( dcs );
        const uint32_t dcmf = (uint32_t)mf[0] >> 1, dcb = (uint32_t)bias[0] << 1;
        acc = 0;
#pragma unroll
        for( int k = 0; k < 16; k++ )
        {
            dcs[k] = sto<BD>( quant_one( dcs[k], dcmf, dcb ) );
            acc |= dcs[k];
        }
        nz_ldc = acc != 0;
        if( nz_ldc )
        {
#pragma unroll
            for( int i = 0; i < 16; i++ )
                ldc[i] = dcs[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )];
            had4x4dc<BD, false>( dcs );
            const int m = a.dq4[(CQM_4IY * 6 + qp % 6) * 16], qb = qp / 6 - 6;
#pragma unroll
            for( int k = 0; k < 16; k++ )
                dcs[k] = sto<BD>( dequant_dc_one( dcs[k], m, qb ) );
        }
        const bool nn = block_cbp && nzb;
        int lev[16], res[4][4];
        zero( lev );
        fill( res, 0 );
        const int mydc = pick( dcs, 4 * by + bx );
        if( block_cbp )
        {
            if( nzb )
            {
#pragma unroll
                for( int i = 0; i < 16; i++ )
                    lev[i] = c[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )];
                const int32_t *m = a.dq4 + (CQM_4IY * 6 + qp % 6) * 16;
                const int qb = qp / 6 - 4;
#pragma unroll
                for( int k = 0; k < 16; k++ )
                    c[k] = sto<BD>( dequant_one( c[k], m[k], qb ) );
            }
            if( nz_ldc )
                c[0] = mydc;
            idct4_residual<BD>( c, res );                      // add16x16_idct
        }
        else if( nz_ldc )
            fill( res, (mydc + 32) >> 6 );                     // add16x16_idct_dc, dct.c:442-471
        put_coefs<BD, 16>( lvl + l * 16, lev, al );
#pragma unroll
        for( int y = 0; y < 4; y++ )
        {
            int v[4];
#pragma unroll
            for( int x = 0; x < 4; x++ )
                v[x] = clip_pix<BD>( p[y][x] + res[y][x] );
            write_row<BD, 4>( ry + (4 * by + y) * a.rs + 4 * bx, v );
        }
        lmask = (int)((__ballot( nn ) >> (16 * slot)) & 0xffff);
    }
    else if( !i8 )
    {
        // I_4x4, macroblock.c:738-768 and x264_mb_encode_i4x4: the ten block anti-diagonals
        int mode = (fl & X264HIP_MBENC_T8x8) ? pm[l & 12] : pm[l];
        mode = (unsigned)mode > 11 ? 11 : mode;
        // i_neighbour4[l], common/macroblock.c:489-498, 1340-1351
        int n4;
        if( l == 0 )
            n4 = (nb & (NB_TOP | NB_LEFT | NB_TOPLEFT)) | (top ? NB_TOPRIGHT : 0);
        else if( l == 1 || l == 4 )
            n4 = NB_LEFT | (top ? NB_TOP | NB_TOPLEFT | NB_TOPRIGHT : 0);
        else if( l == 2 || l == 8 || l == 10 )
            n4 = NB_TOP | NB_TOPRIGHT | (left ? NB_LEFT | NB_TOPLEFT : 0);
        else if( l == 5 )
            n4 = NB_LEFT | (nb & NB_TOPRIGHT) | (top ? NB_TOP | NB_TOPLEFT : 0);
        else if( l == 6 || l == 9 || l == 12 || l == 14 )
            n4 = NB_LEFT | NB_TOP | NB_TOPLEFT | NB_TOPRIGHT;
        else
            n4 = NB_LEFT | NB_TOP | NB_TOPLEFT;
        const bool splat = (n4 & (NB_TOPRIGHT | NB_TOP)) == NB_TOP;
        const udctcoef *mf = a.q4mf + (CQM_4IY * QP1 + qp) * 16, *bias = a.q4b + (CQM_4IY * QP1 + qp) * 16;
        int nzb = 0;
        tpx *b = ty + (4 * by) * TW + 4 * bx;                  // (-1,-1) of the block
#pragma unroll 1
        for( int s = 0; s < 10; s++ )
        {
            if( bx + 2 * by == s )
            {
                int t[8], lf[4], p[4][4], d[4][4], c[16];
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    t[x] = b[1 + x];
                    lf[x] = b[(1 + x) * TW];
                }
#pragma unroll
                for( int x = 4; x < 8; x++ )
                    t[x] = splat ? t[3] : (int)b[1 + x];
                pred4x4<BD>( mode, t, lf, b[0], p );
#pragma unroll
                for( int y = 0; y < 4; y++ )
                {
                    int e[4];
                    read_row<BD, 4>( fy + (4 * by + y) * a.fs + 4 * bx, e );
#pragma unroll
                    for( int x = 0; x < 4; x++ )
                        d[y][x] = e[x] - p[y][x];
                }
                dct4x4_core<BD>( d, c );
                int acc = 0;
#pragma unroll
                for( int k = 0; k < 16; k++ )
                {
                    c[k] = sto<BD>( quant_one( c[k], mf[k], bias[k] ) );
                    acc |= c[k];
                }
                nzb = acc != 0;
                int lev[16], res[4][4];
                zero( lev );
                fill( res, 0 );
                if( nzb )
                {
#pragma unroll
                    for( int i = 0; i < 16; i++ )
                        lev[i] = c[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )];
                    const int32_t *m = a.dq4 + (CQM_4IY * 6 + qp % 6) * 16;
                    const int qb = qp / 6 - 4;
#pragma unroll
                    for( int k = 0; k < 16; k++ )
                        c[k] = sto<BD>( dequant_one( c[k], m[k], qb ) );
                    idct4_residual<BD>( c, res );
                }
                put_coefs<BD, 16>( lvl + l * 16, lev, al );
#pragma unroll
                for( int y = 0; y < 4; y++ )
                {
                    int v[4];
#pragma unroll
                    for( int x = 0; x < 4; x++ )
                    {
                        v[x] = clip_pix<BD>( p[y][x] + res[y][x] );
                        b[(1 + y) * TW + 1 + x] = (tpx)v[x];
                    }
                    write_row<BD, 4>( ry + (4 * by + y) * a.rs + 4 * bx, v );
                }
            }
            tile_sync();
        }
        lmask = (int)((__ballot( nzb ) >> (16 * slot)) & 0xffff);
#pragma unroll
        for( int k = 0; k < 4; k++ )
            cbp_luma |= (((lmask >> (4 * k)) & 0xf) != 0) << k;
    }
    else
    {
        // I_8x8, macroblock.c:713-737 and x264_mb_encode_i8x8
        tpx *e = s_e[slot];
        int nz8 = 0;
#pragma unroll 1
        for( int idx = 0; idx < 4; idx++ )
        {
            int mode = pm[4 * idx];
            mode = (unsigned)mode > 11 ? 11 : mode;
            // i_neighbour8[idx], common/macroblock.c:498, 1340-1351
            const int n8 = idx == 0 ? (nb & (NB_TOP | NB_LEFT | NB_TOPLEFT)) | (top ? NB_TOPRIGHT : 0)
                         : idx == 1 ? NB_LEFT | (nb & NB_TOPRIGHT) | (top ? NB_TOP | NB_TOPLEFT : 0)
                         : idx == 2 ? NB_TOP | NB_TOPRIGHT | (left ? NB_LEFT | NB_TOPLEFT : 0)
                                    : NB_LEFT | NB_TOP | NB_TOPLEFT;
            tpx *b = ty + (8 * (idx >> 1)) * TW + 8 * (idx & 1);
            // predict_8x8_filter: two entries a lane
#pragma unroll
            for( int j = 0; j < 2; j++ )
            {
                const int k = 6 + l + 16 * j;
                if( k <= 32 )
                    e[k] = (tpx)edge_at( b, k, n8 & NB_TOPLEFT, n8 & NB_TOPRIGHT );
            }
            tile_sync();
            int sl = 0, st = 0;
#pragma unroll
            for( int k = 0; k < 8; k++ )
            {
                sl += e[7 + k];
                st += e[16 + k];
            }
            const int dc = mode == 2 ? (sl + st + 8) >> 4 : mode == 9 ? (sl + 4) >> 3 : mode == 10 ? (st + 4) >> 3 : 1 << (BD - 1);
            // predict_8x8[mode] into the tile: four pixels a lane
            {
                const int y = l >> 1, x0 = (l & 1) * 4;
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    b[(1 + y) * TW + 1 + x0 + x] = (tpx)pred8_px( mode, e, x0 + x, y, dc );
            }
            tile_sync();
            if( l == idx )
            {
                const int ox = 8 * (idx & 1), oy = 8 * (idx >> 1);
                int d[8][8], c[64];
#pragma unroll
                for( int y = 0; y < 8; y++ )
                {
                    int fe[8];
                    read_row<BD, 8>( fy + (oy + y) * a.fs + ox, fe );
#pragma unroll
                    for( int x = 0; x < 8; x++ )
                        d[y][x] = fe[x] - (int)b[(1 + y) * TW + 1 + x];
                }
                dct8x8_core<BD>( d, c );
                const udctcoef *mf = a.q8mf + (CQM_8IY * QP1 + qp) * 64, *bias = a.q8b + (CQM_8IY * QP1 + qp) * 64;
                int acc = 0;
#pragma unroll
                for( int k = 0; k < 64; k++ )
                {
                    c[k] = sto<BD>( quant_one( c[k], mf[k], bias[k] ) );
                    acc |= c[k];
                }
                nz8 = acc != 0;
                {
                    int lev[64];
#pragma unroll
                    for( int i = 0; i < 64; i++ )
                        lev[i] = c[ZZF<8>::x( i ) * 8 + ZZF<8>::y( i )];     // (all zero without nz8)
                    put_coefs<BD, 64>( lvl + idx * 64, lev, al );
                }
                int res[8][8];
                if( nz8 )
                {
                    const int32_t *m = a.dq8 + (CQM_8IY * 6 + qp % 6) * 64;
                    const int qb = qp / 6 - 6;
#pragma unroll
                    for( int k = 0; k < 64; k++ )
                        c[k] = sto<BD>( dequant_one( c[k], m[k], qb ) );
                    idct8_residual<BD>( c, res );
                }
                else
                    fill( res, 0 );
#pragma unroll
                for( int y = 0; y < 8; y++ )
                {
                    int v[8];
#pragma unroll
                    for( int x = 0; x < 8; x++ )
                    {
                        v[x] = clip_pix<BD>( (int)b[(1 + y) * TW + 1 + x] + res[y][x] );
                        b[(1 + y) * TW + 1 + x] = (tpx)v[x];
                    }
                    write_row<BD, 8>( ry + (oy + y) * a.rs + ox, v );
                }
            }
            tile_sync();
        }
        k4 = (int)((__ballot( nz8 && l < 4 ) >> (16 * slot)) & 0xf);
        cbp_luma = k4;
#pragma unroll
        for( int k = 0; k < 4; k++ )
            lmask |= ((k4 >> k) & 1) * (0xf << (4 * k));
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
    using udctcoef = typename PT<BD>::udctcoef;
    if( !e || mbw <= 0 || mbh <= 0 || n_frames <= 0 )
        return hipSuccess;
    constexpr int QP_MAX_SPEC = 51 + 6 * (BD - 8);
    MbIntraParams<BD> a;
    a.fenc = (const pixel *)e->fenc; a.fenc_c = (const pixel *)e->fenc_chroma;
    a.recon = (pixel *)e->recon; a.recon_c = (pixel *)e->recon_chroma;
    a.fs = e->fenc_stride; a.ffs = e->fenc_frame_stride;
    a.fcs = e->fenc_chroma_stride; a.fcfs = e->fenc_chroma_frame_stride;
    a.rs = e->recon_stride; a.rfs = e->recon_frame_stride;
    a.rcs = e->recon_chroma_stride; a.rcfs = e->recon_chroma_frame_stride;
    a.q4mf = (const udctcoef *)e->quant4_mf; a.q4b = (const udctcoef *)e->quant4_bias;
    a.q8mf = (const udctcoef *)e->quant8_mf; a.q8b = (const udctcoef *)e->quant8_bias;
    a.dq4 = e->dequant4_mf; a.dq8 = e->dequant8_mf;
    a.qp = e->qp; a.flags = e->mb_flags; a.pmode = e->pred_mode; a.cmode = e->chroma_pred_mode;
    a.level = (dctcoef *)e->level; a.chroma_dc = (dctcoef *)e->chroma_dc; a.luma_dc = (dctcoef *)e->luma_dc;
    a.nnz = e->nnz; a.cbp = e->cbp; a.nz = e->nz; a.flags_out = e->flags_out;
    a.mbw = mbw; a.mbh = mbh;
    a.dec = e->b_dct_decimate != 0;
    a.al = !(((uintptr_t)e->level | (uintptr_t)e->chroma_dc | (uintptr_t)e->luma_dc) & 15);
    uint8_t cqp[64] = { 0 };
    memcpy( cqp, e->chroma_qp_table, QP_MAX_SPEC + 1 );
    memcpy( a.cqp, cqp, sizeof( cqp ) );
    // the anti-diagonals x + 2y = d in dependency order; rows ymin .. ymax of diagonal d
    const int ndiag = mbw + 2 * (mbh - 1);
    for( int d = 0; d < ndiag; d++ )
    {
        const int ymin = d >= mbw ? (d - mbw + 2) / 2 : 0, ymax = d / 2 < mbh - 1 ? d / 2 : mbh - 1;
        if( ymax < ymin )
            continue;
        a.d = d; a.ymin = ymin; a.count = ymax - ymin + 1; a.nitems = a.count * n_frames;
        switch( e->chroma_format )
        {
            case 0: mb_encode_intra_go<BD, 0>( a, stream ); break;
            case 1: mb_encode_intra_go<BD, 1>( a, stream ); break;
            default: mb_encode_intra_go<BD, 2>( a, stream ); break;
        }
    }
    return hipGetLastError();
}
X264HIP_INSTANTIATE( launch_mb_encode_intra );

} // namespace x264hip
