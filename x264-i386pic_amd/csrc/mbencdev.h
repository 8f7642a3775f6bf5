// Device helpers shared by the macroblock encodes, mbenc.hip (inter), mbintra.hip (intra) and
// mb444.hip (both at 4:4:4): the 16-lanes-per-macroblock cross-lane reads, the coefficient stores,
// the static inlines of encoder/macroblock.c:35-96 with their 2x4 counterparts, one channel of
// mb_encode_chroma_internal (reference encoder/macroblock.c:259-490) and one luma-coded plane of
// an inter macroblock (:801-921) over the cores of txdev.h.  Host side: the fill of their
// kernel-argument blocks.
#pragma once
#include "txdev.h"

namespace x264hip {

// Host: what the public structs of the macroblock encodes (x264hip_mbenc_t, x264hip_mbintra_t,
// x264hip_mb444_t) and the kernel-argument blocks of mbenc.hip, mbintra.hip and mb444.hip name
// alike, from e into a.  The launcher adds its planes and strides, pred_mode / chroma_pred_mode,
// luma_dc / chroma_dc and al (the dctcoef outputs it has are 16-byte aligned).
template <int BD, typename E, typename A> void fill_mb_params( const E *e, int mbw, int mbh, A &a )
{
    using dctcoef = typename PT<BD>::dctcoef;
    using udctcoef = typename PT<BD>::udctcoef;
    a.q4mf = (const udctcoef *)e->quant4_mf; a.q4b = (const udctcoef *)e->quant4_bias;
    a.q8mf = (const udctcoef *)e->quant8_mf; a.q8b = (const udctcoef *)e->quant8_bias;
    a.dq4 = e->dequant4_mf; a.dq8 = e->dequant8_mf;
    a.qp = e->qp; a.flags = e->mb_flags;
    a.level = (dctcoef *)e->level;
    a.nnz = e->nnz; a.cbp = e->cbp; a.nz = e->nz; a.flags_out = e->flags_out;
    a.mbw = mbw; a.mbh = mbh;
    a.dec = e->b_dct_decimate != 0;
    pack_cqp<BD>( e->chroma_qp_table, a.cqp );
}

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

// ---------------------------------------------------------------- one luma-coded plane
// One plane of one macroblock as its 16 lanes see it: the luma plane of mbenc.hip / mbintra.hip,
// or Y, U or V of a 4:4:4 macroblock (mb444.hip), each with its own quant category and qp.
template <int BD> struct PlaneCtx
{
    using pixel = typename PT<BD>::pixel;
    const pixel *fenc, *pred;                  // pixel (0,0) of the macroblock; pred: inter only
    pixel *recon;
    intptr_t fs, ps, rs;
    const typename PT<BD>::udctcoef *mf4, *bias4, *mf8, *bias8;   // the category's rows at qp
    const int32_t *dq4, *dq8;                  // the category's dequant4_mf [6][16] / dequant8_mf [6][64]
    int qp;
    typename PT<BD>::dctcoef *lvl;             // level of the plane's block 0
    bool al;                                   // lvl is 16-byte aligned
};

// Inter, transform 4 (macroblock.c:848-919).  The first half runs up to the plane's own sum of
// i_decimate_8x8 (what it adds to i_decimate_mb); the caller forms i_decimate_mb as the test
// after this plane sees it (:907), and the second half takes the decisions and reconstructs.
// Lane l owns block l of h->dct.luma4x4's order; uniform over the plane's lanes except l.
struct Inter4
{
    int c[16];
    int nzb, i_decimate_8x8, nnz8x8, plane_score;
};

template <int BD>
__device__ __forceinline__ void inter_luma4_scores( const PlaneCtx<BD> &k, int l, bool dec, bool skip, Inter4 &s )
{
    const int i8 = l >> 2, i4 = l & 3;
    const int x = (i8 & 1) * 8 + (i4 & 1) * 4, y = (i8 >> 1) * 8 + (i4 >> 1) * 4;
    zero( s.c );
    int score = 0;
    s.nzb = 0;
    if( !skip )
    {
        int d[4][4];
        load_diff<BD, 4>( d, k.fenc + y * k.fs + x, k.fs, k.pred + y * k.ps + x, k.ps );
        dct4x4_core<BD>( d, s.c );
        int acc = 0;
#pragma unroll
        for( int j = 0; j < 16; j++ )
        {
            s.c[j] = sto<BD>( quant_one( s.c[j], k.mf4[j], k.bias4[j] ) );
            acc |= s.c[j];
        }
        s.nzb = acc != 0;
        if( dec && s.nzb )
            score = decimate_score<16, 0>( [&]( int i ) { return s.c[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )]; } );
    }
    // the 8x8's decision (macroblock.c:862-905), taken by each of its four lanes
    s.i_decimate_8x8 = dec ? 0 : 6;
    s.nnz8x8 = 0;
#pragma unroll
    for( int j = 0; j < 4; j++ )
    {
        const int nzk = mb_lane( s.nzb, (l & 12) + j ), sk = mb_lane( score, (l & 12) + j );
        if( nzk )
        {
            s.nnz8x8 = 1;
            if( s.i_decimate_8x8 < 6 )
                s.i_decimate_8x8 += sk;
        }
    }
    const int contrib = s.nnz8x8 ? s.i_decimate_8x8 : 0;
    s.plane_score = 0;
#pragma unroll
    for( int j = 0; j < 4; j++ )
        s.plane_score += mb_lane( contrib, 4 * j );
}

// returns this lane's final non_zero_count
template <int BD>
__device__ __forceinline__ bool inter_luma4_finish( const PlaneCtx<BD> &k, int l, Inter4 &s, int i_decimate_mb )
{
    const int i8 = l >> 2, i4 = l & 3;
    const int x = (i8 & 1) * 8 + (i4 & 1) * 4, y = (i8 >> 1) * 8 + (i4 >> 1) * 4;
    const bool keep = s.nnz8x8 && s.i_decimate_8x8 >= 4 && i_decimate_mb >= 6;
    const bool nn = keep && s.nzb;
    int lev[16], res[4][4];
    zero( lev );
#pragma unroll
    for( int yy = 0; yy < 4; yy++ )
#pragma unroll
        for( int xx = 0; xx < 4; xx++ )
            res[yy][xx] = 0;
    if( nn )
    {
#pragma unroll
        for( int i = 0; i < 16; i++ )
            lev[i] = s.c[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )];
        const int32_t *m = k.dq4 + (k.qp % 6) * 16;
        const int qb = k.qp / 6 - 4;
#pragma unroll
        for( int j = 0; j < 16; j++ )
            s.c[j] = sto<BD>( dequant_one( s.c[j], m[j], qb ) );
        idct4_residual<BD>( s.c, res );
    }
    put_coefs<BD, 16>( k.lvl + l * 16, lev, k.al );
    add_block<BD, 4>( k.pred + y * k.ps + x, k.ps, k.recon + y * k.rs + x, k.rs, res );
    return nn;
}

// Inter, transform 8 (macroblock.c:806-843), split the same way (the test after the plane: :833).
// Lanes 0..3 of the plane own the 8x8 blocks; the other lanes take part in the cross-lane reads.
struct Inter8
{
    int c[64];
    int nzb, score, plane_score;
};

template <int BD>
__device__ __forceinline__ void inter_luma8_scores( const PlaneCtx<BD> &k, int l, bool dec, bool skip, Inter8 &s )
{
    const int x = (l & 1) * 8, y = ((l >> 1) & 1) * 8;
    zero( s.c );
    s.nzb = s.score = 0;
    if( l < 4 && !skip )
    {
        int d[8][8];
        load_diff<BD, 8>( d, k.fenc + y * k.fs + x, k.fs, k.pred + y * k.ps + x, k.ps );
        dct8x8_core<BD>( d, s.c );
        int acc = 0;
#pragma unroll
        for( int j = 0; j < 64; j++ )
        {
            s.c[j] = sto<BD>( quant_one( s.c[j], k.mf8[j], k.bias8[j] ) );
            acc |= s.c[j];
        }
        s.nzb = acc != 0;
        if( dec && s.nzb )
            s.score = decimate_score<64, 0>( [&]( int i ) { return s.c[ZZF<8>::x( i ) * 8 + ZZF<8>::y( i )]; } );
    }
    // macroblock.c:813-831
    s.plane_score = 0;
#pragma unroll
    for( int j = 0; j < 4; j++ )
    {
        const int nzk = mb_lane( s.nzb, j ), sk = mb_lane( s.score, j );
        if( dec && nzk )
            s.plane_score += sk;
    }
}

// returns whether this lane's 8x8 block is kept (false on the lanes past 3)
template <int BD>
__device__ __forceinline__ bool inter_luma8_finish( const PlaneCtx<BD> &k, int l, bool dec, Inter8 &s, int i_decimate_mb )
{
    const int x = (l & 1) * 8, y = ((l >> 1) & 1) * 8;
    const bool keep = s.nzb && (!dec || (s.score >= 4 && i_decimate_mb >= 6));
    if( l < 4 )
    {
        int lev[64];
        zero( lev );
        if( keep )
        {
#pragma unroll
            for( int i = 0; i < 64; i++ )
                lev[i] = s.c[ZZF<8>::x( i ) * 8 + ZZF<8>::y( i )];
        }
        put_coefs<BD, 64>( k.lvl + l * 64, lev, k.al );
        int res[8][8];
        if( keep )
        {
            const int32_t *m = k.dq8 + (k.qp % 6) * 64;
            const int qb = k.qp / 6 - 6;
#pragma unroll
            for( int j = 0; j < 64; j++ )
                s.c[j] = sto<BD>( dequant_one( s.c[j], m[j], qb ) );
            idct8_residual<BD>( s.c, res );
        }
        else
        {
#pragma unroll
            for( int yy = 0; yy < 8; yy++ )
#pragma unroll
                for( int xx = 0; xx < 8; xx++ )
                    res[yy][xx] = 0;
        }
        add_block<BD, 8>( k.pred + y * k.ps + x, k.ps, k.recon + y * k.rs + x, k.rs, res );
    }
    return keep && l < 4;
}

} // namespace x264hip
