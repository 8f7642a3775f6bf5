// Device helpers shared by the intra macroblock encodes, mbintra.hip and mb444.hip: the FDEC-style
// tile of one plane in shared memory, the luma predictors of common/predict.c over it, and one
// luma-coded plane of an I_16x16 / I_4x4 / I_8x8 macroblock (reference encoder/macroblock.c:126-239,
// :706-768, encoder/macroblock.h:132-213) as the plane's 16 lanes run it.  At 4:4:4 U and V go
// through the same functions with their own tile, quant category and qp.
#pragma once
#include "intradev.h"
#include "mbencdev.h"

namespace x264hip {

constexpr int NB_LEFT = 1, NB_TOP = 2, NB_TOPRIGHT = 4, NB_TOPLEFT = 8;   // common/macroblock.h:33-36

typedef uint16_t tpx;                         // a tile sample
constexpr int TW = 28;                        // tile row: left, 16, 8 top-right (row 0), padding
constexpr int TILE = 17 * TW;                 // a plane's tile: [1 + y][1 + x]

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

// ---------------------------------------------------------------- one plane of an intra macroblock
// k: the plane (mbencdev.h; pred is not used: the prediction is formed in the tile); ty: its tile;
// l: the lane inside the plane's 16; nb: i_neighbour_intra of the macroblock.  All three paths are
// uniform over the plane's lanes except l, and hold tile exchanges: every lane of the plane runs them.

// lane l's 4x4 block of h->dct.luma4x4's order
__device__ __forceinline__ int blk_x( int l ) { return ((l >> 2) & 1) * 2 + (l & 1); }
__device__ __forceinline__ int blk_y( int l ) { return (l >> 3) * 2 + ((l >> 1) & 1); }

// the tile's borders from recon (ry: pixel (0,0) of the macroblock); a tile_sync() follows in the
// caller.  tpx_l / lpx_l: the top / left sample this lane read (0 without the neighbour)
template <int BD>
__device__ __forceinline__ void tile_borders( tpx *ty, const typename PT<BD>::pixel *ry, intptr_t rs, int l, int nb,
                                              int &tpx_l, int &lpx_l )
{
    const bool left = nb & NB_LEFT, top = nb & NB_TOP;
    tpx_l = top ? ry[-rs + l] : 0;
    lpx_l = left ? ry[l * rs - 1] : 0;
    ty[1 + l] = (tpx)tpx_l;
    ty[(1 + l) * TW] = (tpx)lpx_l;
    if( l < 8 )
        ty[17 + l] = (tpx)( (nb & NB_TOPRIGHT) ? ry[-rs + 16 + l] : 0 );
    if( l == 0 )
        ty[0] = (tpx)( (nb & NB_TOPLEFT) ? ry[-rs - 1] : 0 );
}

// mb_encode_i16x16, macroblock.c:126-239.  ldc: h->dct.luma16x16_dc[p] (zeros without nz_ldc);
// cbp_luma: block_cbp as :213 ORs it in.  Returns this lane's final AC non_zero_count.
template <int BD>
__device__ __forceinline__ bool intra_i16_plane( const PlaneCtx<BD> &k, const tpx *ty, int l, int mode, bool dec,
                                                 int tpx_l, int lpx_l, int (&ldc)[16], int &nz_ldc, int &cbp_luma )
{
    const int bx = blk_x( l ), by = blk_y( l );
    mode = (unsigned)mode > 6 ? 6 : mode;
    int p[4][4], d[4][4], c[16];
    pred16x16<BD>( mode, ty, 4 * bx, 4 * by, mb_sum( tpx_l ), mb_sum( lpx_l ), p );
#pragma unroll
    for( int y = 0; y < 4; y++ )
    {
        int e[4];
        read_row<BD, 4>( k.fenc + (4 * by + y) * k.fs + 4 * bx, e );
#pragma unroll
        for( int x = 0; x < 4; x++ )
            d[y][x] = e[x] - p[y][x];
    }
    dct4x4_core<BD>( d, c );
    const int c0 = c[0];
    c[0] = 0;
    int acc = 0;
#pragma unroll
    for( int j = 0; j < 16; j++ )
    {
        c[j] = sto<BD>( quant_one( c[j], k.mf4[j], k.bias4[j] ) );
        acc |= c[j];
    }
    const int nzb = acc != 0;
    int score = 0;
    if( dec && nzb )
        score = decimate_score<16, 1>( [&]( int i ) { return c[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )]; } );
    int decimate = dec ? 0 : 9, any = 0;
#pragma unroll
    for( int j = 0; j < 16; j++ )
    {
        const int nzk = mb_lane( nzb, j ), sk = mb_lane( score, j );
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
    const uint32_t dcmf = (uint32_t)k.mf4[0] >> 1, dcb = (uint32_t)k.bias4[0] << 1;
    acc = 0;
#pragma unroll
    for( int j = 0; j < 16; j++ )
    {
        dcs[j] = sto<BD>( quant_one( dcs[j], dcmf, dcb ) );
        acc |= dcs[j];
    }
    nz_ldc = acc != 0;
    zero( ldc );
    if( nz_ldc )
    {
#pragma unroll
        for( int i = 0; i < 16; i++ )
            ldc[i] = dcs[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )];
        had4x4dc<BD, false>( dcs );
        const int m = k.dq4[(k.qp % 6) * 16], qb = k.qp / 6 - 6;
#pragma unroll
        for( int j = 0; j < 16; j++ )
            dcs[j] = sto<BD>( dequant_dc_one( dcs[j], m, qb ) );
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
            const int32_t *m = k.dq4 + (k.qp % 6) * 16;
            const int qb = k.qp / 6 - 4;
#pragma unroll
            for( int j = 0; j < 16; j++ )
                c[j] = sto<BD>( dequant_one( c[j], m[j], qb ) );
        }
        if( nz_ldc )
            c[0] = mydc;
        idct4_residual<BD>( c, res );                      // add16x16_idct
    }
    else if( nz_ldc )
        fill( res, (mydc + 32) >> 6 );                     // add16x16_idct_dc, dct.c:442-471
    put_coefs<BD, 16>( k.lvl + l * 16, lev, k.al );
#pragma unroll
    for( int y = 0; y < 4; y++ )
    {
        int v[4];
#pragma unroll
        for( int x = 0; x < 4; x++ )
            v[x] = clip_pix<BD>( p[y][x] + res[y][x] );
        write_row<BD, 4>( k.recon + (4 * by + y) * k.rs + 4 * bx, v );
    }
    return nn;
}

// I_4x4, macroblock.c:738-768 and x264_mb_encode_i4x4: the ten block anti-diagonals.  mode: of
// this lane's block.  Returns this lane's non_zero_count.
template <int BD>
__device__ __forceinline__ int intra_i4_plane( const PlaneCtx<BD> &k, tpx *ty, int l, int mode, int nb )
{
    const int bx = blk_x( l ), by = blk_y( l );
    const bool left = nb & NB_LEFT, top = nb & NB_TOP;
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
                read_row<BD, 4>( k.fenc + (4 * by + y) * k.fs + 4 * bx, e );
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    d[y][x] = e[x] - p[y][x];
            }
            dct4x4_core<BD>( d, c );
            int acc = 0;
#pragma unroll
            for( int j = 0; j < 16; j++ )
            {
                c[j] = sto<BD>( quant_one( c[j], k.mf4[j], k.bias4[j] ) );
                acc |= c[j];
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
                const int32_t *m = k.dq4 + (k.qp % 6) * 16;
                const int qb = k.qp / 6 - 4;
#pragma unroll
                for( int j = 0; j < 16; j++ )
                    c[j] = sto<BD>( dequant_one( c[j], m[j], qb ) );
                idct4_residual<BD>( c, res );
            }
            put_coefs<BD, 16>( k.lvl + l * 16, lev, k.al );
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
                write_row<BD, 4>( k.recon + (4 * by + y) * k.rs + 4 * bx, v );
            }
        }
        tile_sync();
    }
    return nzb;
}

// I_8x8, macroblock.c:713-737 and x264_mb_encode_i8x8.  pm: the macroblock's 16 modes (entry 4*i
// is block i's); e: 36 samples of shared memory for the filtered edge.  Returns the
// non_zero_count of block l on lanes 0..3, 0 on the others.
template <int BD>
__device__ __forceinline__ int intra_i8_plane( const PlaneCtx<BD> &k, tpx *ty, tpx *e, int l, const int8_t *pm, int nb )
{
    const bool left = nb & NB_LEFT, top = nb & NB_TOP;
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
            const int q = 6 + l + 16 * j;
            if( q <= 32 )
                e[q] = (tpx)edge_at( b, q, n8 & NB_TOPLEFT, n8 & NB_TOPRIGHT );
        }
        tile_sync();
        int sl = 0, st = 0;
#pragma unroll
        for( int j = 0; j < 8; j++ )
        {
            sl += e[7 + j];
            st += e[16 + j];
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
                read_row<BD, 8>( k.fenc + (oy + y) * k.fs + ox, fe );
#pragma unroll
                for( int x = 0; x < 8; x++ )
                    d[y][x] = fe[x] - (int)b[(1 + y) * TW + 1 + x];
            }
            dct8x8_core<BD>( d, c );
            int acc = 0;
#pragma unroll
            for( int j = 0; j < 64; j++ )
            {
                c[j] = sto<BD>( quant_one( c[j], k.mf8[j], k.bias8[j] ) );
                acc |= c[j];
            }
            nz8 = acc != 0;
            {
                int lev[64];
#pragma unroll
                for( int i = 0; i < 64; i++ )
                    lev[i] = c[ZZF<8>::x( i ) * 8 + ZZF<8>::y( i )];     // (all zero without nz8)
                put_coefs<BD, 64>( k.lvl + idx * 64, lev, k.al );
            }
            int res[8][8];
            if( nz8 )
            {
                const int32_t *m = k.dq8 + (k.qp % 6) * 64;
                const int qb = k.qp / 6 - 6;
#pragma unroll
                for( int j = 0; j < 64; j++ )
                    c[j] = sto<BD>( dequant_one( c[j], m[j], qb ) );
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
                write_row<BD, 8>( k.recon + (oy + y) * k.rs + ox, v );
            }
        }
        tile_sync();
    }
    return nz8;
}

} // namespace x264hip
