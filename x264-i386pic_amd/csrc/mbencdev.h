// Device helpers shared by the macroblock encodes, mbenc.hip (inter) and mbintra.hip (intra): the
// 16-lanes-per-macroblock cross-lane reads, the coefficient stores, the static inlines of
// encoder/macroblock.c:35-96 with their 2x4 counterparts, and one channel of
// mb_encode_chroma_internal (reference encoder/macroblock.c:259-490) over the cores of txdev.h.
#pragma once
#include "txdev.h"

namespace x264hip {

// N coefficients to memory: 16-byte stores when the array is 16-byte aligned
template <int BD, int N>
__device__ __forceinline__ void put_coefs( typename PT<BD>::dctcoef *p, const int (&v)[N], bool al )
{
    if( al )
    {
        if constexpr( BD == 8 )
        {
#pragma unroll
            for( int k = 0; k < N / 8; k++ )
            {
                uint32_t w[4];
#pragma unroll
                for( int j = 0; j < 4; j++ )
                    w[j] = ((uint32_t)v[8 * k + 2 * j] & 0xffff) | ((uint32_t)v[8 * k + 2 * j + 1] << 16);
                ((uint4 *)p)[k] = make_uint4( w[0], w[1], w[2], w[3] );
            }
        }
        else
        {
#pragma unroll
            for( int k = 0; k < N / 4; k++ )
                ((int4 *)p)[k] = make_int4( v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3] );
        }
    }
    else
    {
#pragma unroll
        for( int k = 0; k < N; k++ )
            p[k] = (typename PT<BD>::dctcoef)v[k];
    }
}

template <int N> __device__ __forceinline__ void zero( int (&v)[N] )
{
#pragma unroll
    for( int k = 0; k < N; k++ )
        v[k] = 0;
}

// v[j] of a register array for a per-lane j, without indexing registers by a lane value
template <int N> __device__ __forceinline__ int pick( const int (&v)[N], int j )
{
    int r = 0;
#pragma unroll
    for( int k = 0; k < N; k++ )
        r = j == k ? v[k] : r;
    return r;
}

// the value of lane j of this macroblock's 16 lanes (every lane of the macroblock is active)
__device__ __forceinline__ int mb_lane( int v, int j ) { return __shfl( v, j, 16 ); }

// sum over the macroblock's 16 lanes
__device__ __forceinline__ int mb_sum( int v )
{
#pragma unroll
    for( int m = 1; m < 16; m <<= 1 )
        v += __shfl_xor( v, m, 16 );
    return v;
}

// ---- the static inlines of encoder/macroblock.c:35-96 and their 2x4 counterparts
template <int NDC> __device__ __forceinline__ void zigzag_dc( const int (&dct)[NDC], int (&level)[8] )
{
    zero( level );
    if constexpr( NDC == 4 )
    {
        level[0] = dct[0]; level[1] = dct[2]; level[2] = dct[1]; level[3] = dct[3];
    }
    else
    {
        level[0] = dct[0]; level[1] = dct[2]; level[2] = dct[1]; level[3] = dct[4];
        level[4] = dct[6]; level[5] = dct[3]; level[6] = dct[5]; level[7] = dct[7];
    }
}

// idct_dequant_2x2_dc / _dconly (macroblock.c:56-79) and idct_dequant_2x4_dc / _dconly
// (quant.c:164-208): the value each 4x4 block's DC gets; dmf = dequant_mf[q % 6][0] << q / 6
template <int BD, int NDC>
__device__ __forceinline__ void idct_dequant_dc( const int (&dct)[NDC], int dmf, int (&out)[NDC] )
{
    if constexpr( NDC == 4 )
    {
        int o[4];
        had2x2( dct, o );
#pragma unroll
        for( int k = 0; k < 4; k++ )
            out[k] = sto<BD>( o[k] * dmf >> 5 );
    }
    else
    {
        int o[8];
        had2x4( dct, o );
#pragma unroll
        for( int k = 0; k < 8; k++ )
            out[k] = sto<BD>( (o[k] * dmf + 32) >> 6 );
    }
}

// what one chroma channel leaves
struct ChromaOut
{
    int res[4][4];      // this lane's residual
    int lev[16];        // this lane's AC block in zigzag order (zeros when its nnz is 0)
    int dc[8];          // h->dct.chroma_dc[ch] (zeros when its nnz is 0)
    int nnz_ac, nnz_dc; // this lane's AC non_zero_count, the channel's DC non_zero_count
    int ac;             // the channel took the DC + AC tail
};

// quant_2x2_dc (twice at 4:2:2) and, where `optimise`, mb_optimize_chroma_dc: 1 when a DC is coded
template <int BD, int NDC>
__device__ __forceinline__ int quant_chroma_dc( int (&dc)[NDC], uint32_t mf, uint32_t bias )
{
    int acc = 0;
#pragma unroll
    for( int k = 0; k < NDC; k++ )
    {
        dc[k] = sto<BD>( quant_one( dc[k], mf, bias ) );
        acc |= dc[k];
    }
    return acc != 0;
}

template <int BD, int NDC> __device__ __forceinline__ int optimize_chroma_dc( int (&dc)[NDC], int dmf )
{
    if( dmf > 32 * 64 )                       // macroblock.c:250
        return 1;
    return oc_search<BD, NDC>( dc, dmf ) > 0;
}

// DC-only reconstruction: zigzag, idct_dequant_*_dconly, add8x8_idct_dc's value for this lane
template <int BD, int NDC>
__device__ __forceinline__ void chroma_dc_only( const int (&dc)[NDC], int dmf, int l, ChromaOut &o )
{
    o.nnz_dc = 1;
    zigzag_dc<NDC>( dc, o.dc );
    int v[NDC];
    idct_dequant_dc<BD, NDC>( dc, dmf, v );
    const int r = sto<BD>( (pick( v, l ) + 32) >> 6 );      // add8x8_idct_dc, dct.c:448-466
#pragma unroll
    for( int y = 0; y < 4; y++ )
#pragma unroll
        for( int x = 0; x < 4; x++ )
            o.res[y][x] = r;
}

// the tables one chroma channel reads (x264hip_mbenc_t's)
template <int BD> struct ChromaTabs
{
    const typename PT<BD>::udctcoef *q4mf, *q4b;
    const int32_t *dq4;
};

// One channel of mb_encode_chroma_internal with the quant category CQ (CQM_4PC inter, CQM_4IC
// intra).  INTER: b_inter, which is what allows the decimation (b_decimate = b_inter &&
// h->mb.b_dct_decimate, macroblock.c:262) and the early termination; without it `dec`, `early` and
// `coded` are not looked at.  d: this lane's 4x4 difference block (zeros on the lanes past the
// channel's blocks); early / coded: the early termination was taken / this channel's ssd is above
// its threshold.  Uniform over the macroblock's lanes except d and l.
template <int BD, int CF, int CQ, bool INTER>
__device__ __forceinline__ void chroma_channel( const ChromaTabs<BD> &a, bool dec, int (&d)[4][4], int l, int qpc,
                                                bool early, bool coded, ChromaOut &o )
{
    constexpr int NDC = CF == 1 ? 4 : 8;
    constexpr int QP1 = 52 + 6 * (BD - 8);
    const bool mine = l < NDC;
    const int qdc = qpc + (CF == 2 ? 3 : 0);
    const uint32_t dcmf = (uint32_t)a.q4mf[(CQ * QP1 + qdc) * 16] >> 1;
    const uint32_t dcb = (uint32_t)a.q4b[(CQ * QP1 + qdc) * 16] << 1;
    const int dmf = a.dq4[(CQ * 6 + qdc % 6) * 16] << (qdc / 6);
    if constexpr( !INTER )
        dec = false;
#pragma unroll
    for( int y = 0; y < 4; y++ )
#pragma unroll
        for( int x = 0; x < 4; x++ )
            o.res[y][x] = 0;
    zero( o.lev );
    zero( o.dc );
    o.nnz_ac = o.nnz_dc = o.ac = 0;
    int dc[NDC];
    if constexpr( INTER )
    {
        if( early )
        {
            if( !coded )
                return;
            // sub8x8_dct_dc / sub8x16_dct_dc (dct.c:207-270): the 4x4 sums, then the butterflies
            int t = 0;
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    t += d[y][x];
            int s[NDC];
#pragma unroll
            for( int k = 0; k < NDC; k++ )
                s[k] = CF == 1 ? sto<BD>( mb_lane( t, k ) ) : mb_lane( t, k );
            if constexpr( CF == 1 )
                had2x2( s, dc );
            else
                had2x4( s, dc );
#pragma unroll
            for( int k = 0; k < NDC; k++ )
                dc[k] = sto<BD>( dc[k] );
            if( quant_chroma_dc<BD, NDC>( dc, dcmf, dcb ) && optimize_chroma_dc<BD, NDC>( dc, dmf ) )
                chroma_dc_only<BD, NDC>( dc, dmf, l, o );
            return;
        }
    }
    // sub8x8_dct, dct2x2dc / dct2x4dc
    int c[16];
    dct4x4_core<BD>( d, c );
    int g[NDC];
#pragma unroll
    for( int k = 0; k < NDC; k++ )
        g[k] = mb_lane( c[0], k );
    if constexpr( CF == 1 )
        had2x2( g, dc );
    else
        had2x4( g, dc );
#pragma unroll
    for( int k = 0; k < NDC; k++ )
        dc[k] = sto<BD>( dc[k] );
    c[0] = 0;
    // quant_4x4x4, decimate_score15 while the score is < 7
    const typename PT<BD>::udctcoef *mf = a.q4mf + (CQ * QP1 + qpc) * 16, *bias = a.q4b + (CQ * QP1 + qpc) * 16;
    int acc = 0;
#pragma unroll
    for( int k = 0; k < 16; k++ )
    {
        c[k] = sto<BD>( quant_one( c[k], mf[k], bias[k] ) );
        acc |= c[k];
    }
    const int nzb = mine && acc != 0;
    int score = 0;
    if( dec && nzb )
        score = decimate_score<16, 1>( [&]( int i ) { return c[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )]; } );
    int i_decimate_score = dec ? 0 : 7, nz_ac = 0;
#pragma unroll
    for( int k = 0; k < NDC; k++ )
    {
        const int nzk = mb_lane( nzb, k ), sk = mb_lane( score, k );
        if( nzk )
        {
            nz_ac = 1;
            if( i_decimate_score < 7 )
                i_decimate_score += sk;
        }
    }
    const int nz_dc = quant_chroma_dc<BD, NDC>( dc, dcmf, dcb );
    if( i_decimate_score < 7 || !nz_ac )
    {
        // decimated: DC-only through mb_optimize_chroma_dc, or empty
        if( nz_dc && optimize_chroma_dc<BD, NDC>( dc, dmf ) )
            chroma_dc_only<BD, NDC>( dc, dmf, l, o );
        return;
    }
    // DC + AC
    o.ac = 1;
    o.nnz_ac = nzb;
    o.nnz_dc = nz_dc;
    if( nzb )
    {
#pragma unroll
        for( int i = 0; i < 16; i++ )
            o.lev[i] = c[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )];
        const int32_t *m = a.dq4 + (CQ * 6 + qpc % 6) * 16;
        const int qb = qpc / 6 - 4;
#pragma unroll
        for( int k = 0; k < 16; k++ )
            c[k] = sto<BD>( dequant_one( c[k], m[k], qb ) );
    }
    if( nz_dc )
    {
        zigzag_dc<NDC>( dc, o.dc );
        int v[NDC];
        idct_dequant_dc<BD, NDC>( dc, dmf, v );
        c[0] = pick( v, l );
    }
    if( mine )
        idct4_residual<BD>( c, o.res );
}

} // namespace x264hip
