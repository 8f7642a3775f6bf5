// Device cores of the transform path, shared by dct.hip (forward transforms and quantisation),
// idct.hip (dequantisation, inverse transforms, reconstruction), mbenc.hip and mbintra.hip (the fused
// inter and intra macroblock encodes): every block lives in one lane's registers.
//
// Semantics (reference, all integer, bit-exact):
//   sub4x4_dct                     common/dct.c:157-189 (int16 temps at 8 bit)
//   sub8x8_dct8                    common/dct.c:332-377
//   QUANT_ONE                      common/quant.c:50-57 (uint32 arithmetic)
//   add4x4_idct                    common/dct.c:272-301
//   add8x8_idct8                   common/dct.c:388-440
//   dequant_4x4 / dequant_8x8      common/quant.c:106-146
//   the 2x2 / 2x4 DC butterflies   common/dct.c:109-143, 207-270, common/quant.c:164-208
//   dct4x4dc / idct4x4dc           common/dct.c:47-107
//   dequant_4x4_dc                 common/quant.c:148-165
//   optimize_chroma_2x2_dc/2x4_dc  common/quant.c:210-293
//   decimate_score15/16/64         common/quant.c:318-352
// Every dctcoef store of the reference (int16 at 8 bit) is reproduced with sto<BD>.
#pragma once
#include "hipcommon.h"

namespace x264hip {

// ---------------------------------------------------------------- forward
template <int BD, int N>
__device__ __forceinline__ void load_diff( int (&d)[N][N], const typename PT<BD>::pixel *a, intptr_t sa,
                                           const typename PT<BD>::pixel *b, intptr_t sb )
{
    constexpr int NDW = N / PT<BD>::PPD;
#pragma unroll
    for( int y = 0; y < N; y++ )
    {
        uint32_t ra[NDW], rb[NDW];
        load_packed<NDW>( a + y * sa, ra );
        load_packed<NDW>( b + y * sb, rb );
#pragma unroll
        for( int x = 0; x < N; x++ )
            d[y][x] = upix<BD>( ra[x / PT<BD>::PPD], x % PT<BD>::PPD ) - upix<BD>( rb[x / PT<BD>::PPD], x % PT<BD>::PPD );
    }
}


// sub4x4_dct on a difference block: out[i*4+k] (reference order)
template <int BD>
__device__ __forceinline__ void dct4x4_core( int (&d)[4][4], int (&out)[16] )
{
    int tmp[4][4];   // tmp[k][i]: second index = source row
#pragma unroll
    for( int i = 0; i < 4; i++ )
    {
        int s03 = d[i][0] + d[i][3], s12 = d[i][1] + d[i][2];
        int d03 = d[i][0] - d[i][3], d12 = d[i][1] - d[i][2];
        tmp[0][i] = sto<BD>( s03 + s12 );
        tmp[1][i] = sto<BD>( 2 * d03 + d12 );
        tmp[2][i] = sto<BD>( s03 - s12 );
        tmp[3][i] = sto<BD>( d03 - 2 * d12 );
    }
#pragma unroll
    for( int i = 0; i < 4; i++ )
    {
        int s03 = tmp[i][0] + tmp[i][3], s12 = tmp[i][1] + tmp[i][2];
        int d03 = tmp[i][0] - tmp[i][3], d12 = tmp[i][1] - tmp[i][2];
        out[i * 4 + 0] = sto<BD>( s03 + s12 );
        out[i * 4 + 1] = sto<BD>( 2 * d03 + d12 );
        out[i * 4 + 2] = sto<BD>( s03 - s12 );
        out[i * 4 + 3] = sto<BD>( d03 - 2 * d12 );
    }
}

// DCT8_1D, reference common/dct.c:332-356 (src/dst via lambdas on indices)
#define DCT8_1D_ARR( S, D )                                                             \
    {                                                                                   \
        int s07 = S( 0 ) + S( 7 ), s16 = S( 1 ) + S( 6 ), s25 = S( 2 ) + S( 5 ),        \
            s34 = S( 3 ) + S( 4 );                                                      \
        int a0 = s07 + s34, a1 = s16 + s25, a2 = s07 - s34, a3 = s16 - s25;             \
        int d07 = S( 0 ) - S( 7 ), d16 = S( 1 ) - S( 6 ), d25 = S( 2 ) - S( 5 ),        \
            d34 = S( 3 ) - S( 4 );                                                      \
        int a4 = d16 + d25 + ( d07 + ( d07 >> 1 ) );                                    \
        int a5 = d07 - d34 - ( d25 + ( d25 >> 1 ) );                                    \
        int a6 = d07 + d34 - ( d16 + ( d16 >> 1 ) );                                    \
        int a7 = d16 - d25 + ( d34 + ( d34 >> 1 ) );                                    \
        D( 0, a0 + a1 );                                                                \
        D( 1, a4 + ( a7 >> 2 ) );                                                       \
        D( 2, a2 + ( a3 >> 1 ) );                                                       \
        D( 3, a5 + ( a6 >> 2 ) );                                                       \
        D( 4, a0 - a1 );                                                                \
        D( 5, a6 - ( a5 >> 2 ) );                                                       \
        D( 6, ( a2 >> 1 ) - a3 );                                                       \
        D( 7, ( a4 >> 2 ) - a7 );                                                       \
    }

// sub8x8_dct8 on a difference block (d[y][x]); out[x*8+i] reference order
template <int BD>
__device__ __forceinline__ void dct8x8_core( int (&d)[8][8], int (&out)[64] )
{
    // column pass in place: column i, SRC(x) = d[x][i]
#pragma unroll
    for( int i = 0; i < 8; i++ )
    {
#define S( x ) d[x][i]
#define D( x, v ) t[x] = sto<BD>( v )
        int t[8];
        DCT8_1D_ARR( S, D )
#pragma unroll
        for( int x = 0; x < 8; x++ )
            d[x][i] = t[x];
#undef S
#undef D
    }
    // row pass: row i, SRC(x) = d[i][x], DST(x) = dct[x*8+i]
#pragma unroll
    for( int i = 0; i < 8; i++ )
    {
#define S( x ) d[i][x]
#define D( x, v ) out[(x) * 8 + i] = sto<BD>( v )
        DCT8_1D_ARR( S, D )
#undef S
#undef D
    }
}

// QUANT_ONE, reference common/quant.c:50-57, branch-free: s = 0 for coef > 0,
// -1 otherwise (coef == 0 takes the reference's negative branch too), so
// |coef| = (coef ^ s) - s and the result is (q ^ s) - s.
__device__ __forceinline__ int quant_one( int coef, uint32_t mf, uint32_t f )
{
    const int s = (coef > 0) - 1;
    const uint32_t mag = (uint32_t)((coef ^ s) - s);
    const int q = (int)(((f + mag) * mf) >> 16);
    return (q ^ s) - s;
}

// k-th entry of a uniform mf / bias row, read as dwords so the loads are
// scalar (s_load) even for the 16-bit tables of 8-bit depth
template <typename U>
__device__ __forceinline__ uint32_t urow( const U *__restrict__ p, int k )
{
    if constexpr( sizeof( U ) == 2 )
    {
        const uint32_t w = ((const uint32_t *)p)[k >> 1];
        return (k & 1) ? w >> 16 : w & 0xffff;
    }
    else
        return p[k];
}

// ---------------------------------------------------------------- inverse
// read N pixels of a row at any alignment
template <int BD, int N>
__device__ __forceinline__ void read_row( const typename PT<BD>::pixel *p, int (&v)[N] )
{
    constexpr int PPD = PT<BD>::PPD;
    uint32_t r[N / PPD];
    load_packed<N / PPD>( p, r );
#pragma unroll
    for( int x = 0; x < N; x++ )
        v[x] = upix<BD>( r[x / PPD], x % PPD );
}

// write N pixels of a row: packed dword stores when aligned, pixel stores otherwise
template <int BD, int N>
__device__ __forceinline__ void write_row( typename PT<BD>::pixel *p, const int (&v)[N] )
{
    constexpr int PPD = PT<BD>::PPD;
    if( ((uintptr_t)p & 3) == 0 )
    {
#pragma unroll
        for( int k = 0; k < N / PPD; k++ )
        {
            uint32_t w = 0;
#pragma unroll
            for( int j = 0; j < PPD; j++ )
                w |= (uint32_t)v[k * PPD + j] << (j * (32 / PPD));
            ((uint32_t *)p)[k] = w;
        }
    }
    else
    {
#pragma unroll
        for( int x = 0; x < N; x++ )
            p[x] = (typename PT<BD>::pixel)v[x];
    }
}

// residual of add4x4_idct: r[y][x] (dct.c:272-301, tmp and d stored as dctcoef)
template <int BD>
__device__ __forceinline__ void idct4_residual( const int (&c)[16], int (&r)[4][4] )
{
    int t[16];
#pragma unroll
    for( int i = 0; i < 4; i++ )
    {
        int s02 = c[0 * 4 + i] + c[2 * 4 + i], d02 = c[0 * 4 + i] - c[2 * 4 + i];
        int s13 = c[1 * 4 + i] + (c[3 * 4 + i] >> 1), d13 = (c[1 * 4 + i] >> 1) - c[3 * 4 + i];
        t[i * 4 + 0] = sto<BD>( s02 + s13 );
        t[i * 4 + 1] = sto<BD>( d02 + d13 );
        t[i * 4 + 2] = sto<BD>( d02 - d13 );
        t[i * 4 + 3] = sto<BD>( s02 - s13 );
    }
#pragma unroll
    for( int i = 0; i < 4; i++ )
    {
        int s02 = t[0 * 4 + i] + t[2 * 4 + i], d02 = t[0 * 4 + i] - t[2 * 4 + i];
        int s13 = t[1 * 4 + i] + (t[3 * 4 + i] >> 1), d13 = (t[1 * 4 + i] >> 1) - t[3 * 4 + i];
        r[0][i] = sto<BD>( (s02 + s13 + 32) >> 6 );
        r[1][i] = sto<BD>( (d02 + d13 + 32) >> 6 );
        r[2][i] = sto<BD>( (d02 - d13 + 32) >> 6 );
        r[3][i] = sto<BD>( (s02 - s13 + 32) >> 6 );
    }
}

// add a residual block to pred and store to dst (may alias pred)
template <int BD, int N>
__device__ __forceinline__ void add_block( const typename PT<BD>::pixel *pred, intptr_t ps, typename PT<BD>::pixel *dst,
                                           intptr_t ds, const int (&r)[N][N] )
{
#pragma unroll
    for( int y = 0; y < N; y++ )
    {
        int v[N];
        read_row<BD, N>( pred + y * ps, v );
#pragma unroll
        for( int x = 0; x < N; x++ )
            v[x] = clip_pix<BD>( v[x] + r[y][x] );
        write_row<BD, N>( dst + y * ds, v );
    }
}

// IDCT8_1D, dct.c:388-418
#define IDCT8_1D( SRC, DST )                                                                   \
    {                                                                                          \
        int a0 = SRC( 0 ) + SRC( 4 ), a2 = SRC( 0 ) - SRC( 4 );                                \
        int a4 = (SRC( 2 ) >> 1) - SRC( 6 ), a6 = (SRC( 6 ) >> 1) + SRC( 2 );                  \
        int b0 = a0 + a6, b2 = a2 + a4, b4 = a2 - a4, b6 = a0 - a6;                            \
        int a1 = -SRC( 3 ) + SRC( 5 ) - SRC( 7 ) - (SRC( 7 ) >> 1);                            \
        int a3 = SRC( 1 ) + SRC( 7 ) - SRC( 3 ) - (SRC( 3 ) >> 1);                             \
        int a5 = -SRC( 1 ) + SRC( 7 ) + SRC( 5 ) + (SRC( 5 ) >> 1);                            \
        int a7 = SRC( 3 ) + SRC( 5 ) + SRC( 1 ) + (SRC( 1 ) >> 1);                             \
        int b1 = (a7 >> 2) + a1, b3 = a3 + (a5 >> 2), b5 = (a3 >> 2) - a5, b7 = a7 - (a1 >> 2); \
        DST( 0, b0 + b7 ); DST( 1, b2 + b5 ); DST( 2, b4 + b3 ); DST( 3, b6 + b1 );            \
        DST( 4, b6 - b1 ); DST( 5, b4 - b3 ); DST( 6, b2 - b5 ); DST( 7, b0 - b7 );            \
    }

// residual of add8x8_idct8 (dct.c:420-440): c is modified as the reference does
// in place (dc rounding and the column pass stored as dctcoef); r[row][col]
template <int BD>
__device__ __forceinline__ void idct8_residual( int (&c)[64], int (&r)[8][8] )
{
    c[0] = sto<BD>( c[0] + 32 );
#pragma unroll
    for( int i = 0; i < 8; i++ )
    {
#define SRC( x ) c[(x) * 8 + i]
#define DST( x, v ) o[x] = sto<BD>( v )
        int o[8];
        IDCT8_1D( SRC, DST )
#pragma unroll
        for( int x = 0; x < 8; x++ )
            c[x * 8 + i] = o[x];
#undef SRC
#undef DST
    }
#pragma unroll
    for( int i = 0; i < 8; i++ )
    {
#define SRC( x ) c[i * 8 + (x)]
#define DST( x, v ) r[x][i] = (v) >> 6
        IDCT8_1D( SRC, DST )
#undef SRC
#undef DST
    }
}

// dequant_4x4 / dequant_8x8 of one coefficient (quant.c:106-146): m = dequant_mf[qp % 6][j],
// qb = qp / 6 - 4 (4x4) or qp / 6 - 6 (8x8); the caller stores the result with sto<BD>
__device__ __forceinline__ int dequant_one( int v, int m, int qb )
{
    return qb >= 0 ? (v * m) * (1 << qb) : (v * m + (1 << (-qb - 1))) >> (-qb);
}

// ---------------------------------------------------------------- chroma DC
// the 2x2 butterfly of sub8x8_dct_dc (dct.c:218-231), dct2x2dc and IDCT_DEQUANT_2X2_START
// (encoder/macroblock.c:56-96)
__device__ __forceinline__ void had2x2( const int (&s)[4], int (&o)[4] )
{
    const int d0 = s[0] + s[1], d1 = s[2] + s[3], d2 = s[0] - s[1], d3 = s[2] - s[3];
    o[0] = d0 + d1;
    o[1] = d0 - d1;
    o[2] = d2 + d3;
    o[3] = d2 - d3;
}

// the 2x4 butterfly of sub8x16_dct_dc, dct2x4dc (dct.c:109-143, 233-270) and
// idct_dequant_2x4_dc / _dconly / optimize_chroma_2x4_dc (quant.c:164-208, 236-260)
__device__ __forceinline__ void had2x4( const int (&d)[8], int (&v)[8] )
{
    const int a0 = d[0] + d[1], a1 = d[2] + d[3], a2 = d[4] + d[5], a3 = d[6] + d[7];
    const int a4 = d[0] - d[1], a5 = d[2] - d[3], a6 = d[4] - d[5], a7 = d[6] - d[7];
    const int b0 = a0 + a1, b1 = a2 + a3, b2 = a4 + a5, b3 = a6 + a7;
    const int b4 = a0 - a1, b5 = a2 - a3, b6 = a4 - a5, b7 = a6 - a7;
    v[0] = b0 + b1; v[1] = b2 + b3; v[2] = b0 - b1; v[3] = b2 - b3;
    v[4] = b4 - b5; v[5] = b6 - b7; v[6] = b4 + b5; v[7] = b6 + b7;
}

// ---------------------------------------------------------------- luma DC (I_16x16)
// dct4x4dc (FWD: the halving second pass) and idct4x4dc, dct.c:47-107, in place; tmp and d are
// stored as dctcoef
template <int BD, bool FWD> __device__ __forceinline__ void had4x4dc( int (&d)[16] )
{
    int t[16];
#pragma unroll
    for( int i = 0; i < 4; i++ )
    {
        const int s01 = d[i * 4 + 0] + d[i * 4 + 1], d01 = d[i * 4 + 0] - d[i * 4 + 1];
        const int s23 = d[i * 4 + 2] + d[i * 4 + 3], d23 = d[i * 4 + 2] - d[i * 4 + 3];
        t[0 * 4 + i] = sto<BD>( s01 + s23 );
        t[1 * 4 + i] = sto<BD>( s01 - s23 );
        t[2 * 4 + i] = sto<BD>( d01 - d23 );
        t[3 * 4 + i] = sto<BD>( d01 + d23 );
    }
    constexpr int R = FWD ? 1 : 0;
#pragma unroll
    for( int i = 0; i < 4; i++ )
    {
        const int s01 = t[i * 4 + 0] + t[i * 4 + 1], d01 = t[i * 4 + 0] - t[i * 4 + 1];
        const int s23 = t[i * 4 + 2] + t[i * 4 + 3], d23 = t[i * 4 + 2] - t[i * 4 + 3];
        d[i * 4 + 0] = sto<BD>( (s01 + s23 + R) >> R );
        d[i * 4 + 1] = sto<BD>( (s01 - s23 + R) >> R );
        d[i * 4 + 2] = sto<BD>( (d01 - d23 + R) >> R );
        d[i * 4 + 3] = sto<BD>( (d01 + d23 + R) >> R );
    }
}

// dequant_4x4_dc of one coefficient (quant.c:148-165): m = dequant_mf[qp % 6][0], qb = qp / 6 - 6
__device__ __forceinline__ int dequant_dc_one( int v, int m, int qb )
{
    return qb >= 0 ? v * (m << qb) : (v * m + (1 << (-qb - 1))) >> (-qb);
}

// optimize_chroma_2x2_dc / 2x4_dc (quant.c:210-293): the dequantised, inverse-transformed DC
// block the greedy search compares
template <int NC>
__device__ __forceinline__ void oc_idq( const int (&d)[NC], int dmf, int (&out)[NC] )
{
    if constexpr( NC == 8 )
    {
        int v[8];
        had2x4( d, v );
#pragma unroll
        for( int k = 0; k < 8; k++ )
            out[k] = (v[k] * dmf + 2080) >> 6;
    }
    else
    {
        int d0 = d[0] + d[1], d1 = d[2] + d[3], d2 = d[0] - d[1], d3 = d[2] - d[3];
        out[0] = ((d0 + d1) * dmf >> 5) + 32;
        out[1] = ((d0 - d1) * dmf >> 5) + 32;
        out[2] = ((d2 + d3) * dmf >> 5) + 32;
        out[3] = ((d2 - d3) * dmf >> 5) + 32;
    }
}

// the reference's greedy search on d, in place: -1 when the block reconstructs to nothing and d
// is left as it was (the reference returns 0 there), else its return value 0 / 1
template <int BD, int NC>
__device__ __forceinline__ int oc_search( int (&d)[NC], int dmf )
{
    int orig[NC], out[NC];
    oc_idq<NC>( d, dmf, orig );
    int sum = 0;
#pragma unroll
    for( int k = 0; k < NC; k++ )
        sum |= sto<BD>( orig[k] );
    if( !(sum >> 6) )
        return -1;
    int nz = 0;
#pragma unroll
    for( int k = 0; k < NC; k++ )
        orig[k] = sto<BD>( orig[k] );
#pragma unroll
    for( int coeff = NC - 1; coeff >= 0; coeff-- )
    {
        int level = d[coeff];
        const int sign = (level >> 31) | 1;
        while( level )
        {
            d[coeff] = sto<BD>( level - sign );
            oc_idq<NC>( d, dmf, out );
            int diff = 0;
#pragma unroll
            for( int k = 0; k < NC; k++ )
                diff |= orig[k] ^ sto<BD>( out[k] );
            if( diff >> 6 )
            {
                nz = 1;
                d[coeff] = level;
                break;
            }
            level -= sign;
        }
    }
    return nz;
}

// ---------------------------------------------------------------- zigzag
// The progressive (frame) zigzag scans of dct.c:768-816 as compile-time (y, x) pairs, so fully
// unrolled loops index registers: level[i] = dct[x*W + y].  The frame scan is the plain zigzag --
// anti-diagonal s = y + x after anti-diagonal, y rising on the odd ones and falling on the even
// ones -- so it is generated, not restated: idct.hip holds the tables (pinned to the reference by
// tests/test_ref_tables.py) and asserts at compile time that this walk equals them.
template <int W> struct ZigzagTab
{
    uint8_t yx[W * W][2];
};
template <int W> constexpr ZigzagTab<W> zigzag_frame_walk()
{
    ZigzagTab<W> t{};
    int i = 0;
    for( int s = 0; s < 2 * W - 1; s++ )
    {
        const int lo = s < W ? 0 : s - W + 1, hi = s < W ? s : W - 1;
        for( int k = lo; k <= hi; k++ )
        {
            const int y = (s & 1) ? k : lo + hi - k;
            t.yx[i][0] = (uint8_t)y;
            t.yx[i][1] = (uint8_t)(s - y);
            i++;
        }
    }
    return t;
}
template <int W> struct ZZF
{
    static constexpr ZigzagTab<W> tab = zigzag_frame_walk<W>();
    static constexpr int y( int i ) { return tab.yx[i][0]; }
    static constexpr int x( int i ) { return tab.yx[i][1]; }
};

// ---------------------------------------------------------------- decimate scores
// decimate_score15 / 16 / 64 (quant.c:318-352) on coefficients in registers: `at( i )` is the
// i-th level in scan order, i = FIRST .. NUM - 1 (FIRST = 1: score15 on a 16-entry block).  The
// reference walks down from the last nonzero level, returns 9 at the first |level| > 1 and adds
// x264_decimate_table4/8[run of zeros below each nonzero level]; the tables are step functions
// of the run (3, 2 2, 1 1 1, 0 ... and 3 x 4, 2 x 8, 1 x 12, 0 ...)
template <int NUM, int FIRST, typename F>
__device__ __forceinline__ int decimate_score( F at )
{
    int score = 0, run = 0;
    bool seen = false, big = false;
#pragma unroll
    for( int i = NUM - 1; i >= FIRST; i-- )
    {
        const int v = at( i );
        if( v )
        {
            if( seen )
                score += NUM == 64 ? (run < 4 ? 3 : run < 12 ? 2 : run < 24 ? 1 : 0)
                                   : (run < 1 ? 3 : run < 3 ? 2 : run < 6 ? 1 : 0);
            big |= (unsigned)(v + 1) > 2;
            seen = true;
            run = 0;
        }
        else
            run++;
    }
    if( seen )
        score += NUM == 64 ? (run < 4 ? 3 : run < 12 ? 2 : run < 24 ? 1 : 0)
                           : (run < 1 ? 3 : run < 3 ? 2 : run < 6 ? 1 : 0);
    return big ? 9 : score;
}

} // namespace x264hip
