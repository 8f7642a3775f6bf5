// P_SKIP / B_SKIP on gfx950 (include/x264hip_mbskip.h): x264_mb_predict_mv_pskip (reference
// common/mvpred.c:129-181), x264_macroblock_probe_skip (encoder/macroblock.c:985-1139) and the
// skip conversion of macroblock.c:953-971, each for every macroblock of a batch of frames in one
// launch, over the transform cores of txdev.h, the prediction core of mcdev.h and the cross-lane
// helpers of mbencdev.h.
//
// The probe takes mbenc.hip's mapping: 16 lanes per macroblock, four macroblocks per wave; lane l
// owns the 4x4 luma block l of h->dct.luma4x4's order (and, at 4:4:4, that block of U and V); lane
// c < 4 (4:2:0) or < 8 (4:2:2) owns the 4x4 position c of BOTH chroma channels, the 8 interleaved
// samples of each of its rows.  A lane builds its own prediction tile (the P leg: get_ref's plane
// pair and mc_chroma at the clipped skip vector, as mbmc.hip's lanes do, then the weights) or
// reads it (the B leg), transforms and quantises its blocks, and scores them.  The reference's
// early returns all compare a sum of non-negative scores with a bound or test an any-nonzero
// flag, so their order does not matter: the decimate sums, the channel SSDs and the DC block sums
// are gathered over the macroblock's 16 lanes (mb_sum / mb_lane) and every lane takes the
// decision.  The branches that hold a cross-lane read are uniform over a macroblock's lanes.
// Nothing is written but skip[mb]: the four macroblocks of a wave are consecutive, so the wave's
// lane 0 stores their four bytes as one dword when the array is aligned and the wave is full.
#include "mbencdev.h"
#include "mcdev.h"
#include "x264hip_mbskip.h"

#include <stddef.h>

namespace x264hip {
namespace {

// x264_lambda2_tab, reference common/tables.c:114-127 (pinned by tests/test_cpu_mbskip.py): host
// only, the kernel gets the thresholds of macroblock.c:1037 per chroma qp
const int k_lambda2_tab[82] = {
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

constexpr int SKIP_4PY = 1, SKIP_4PC = 3;      // CQM_4PY, CQM_4PC: reference common/set.h

// ---------------------------------------------------------------- x264_mb_predict_mv_pskip
__device__ __forceinline__ int median3( int a, int b, int c ) { return max( min( a, b ), min( max( a, b ), c ) ); }

// one lane per macroblock; an mv is one dword (x in the low half)
__global__ __launch_bounds__( 256 ) void mb_predict_mv_pskip_kernel( const uint32_t *__restrict__ mv0,
                                                                     const int8_t *__restrict__ ref0, int mbw, int mbh,
                                                                     int nmb, uint32_t *__restrict__ out )
{
    const int mb = blockIdx.x * 256 + threadIdx.x;
    if( mb >= nmb )
        return;
    const int per = mbw * mbh;
    const int f = mb / per, rem = mb - f * per;
    const int y = rem / mbw, x = rem - y * mbw;
    // the frame's own arrays: a neighbour off the picture is never read
    const uint32_t *mv = mv0 + (int64_t)f * per * 16 + (int64_t)(4 * y) * (4 * mbw) + 4 * x;
    const int8_t *rf = ref0 + (int64_t)f * per * 4 + (int64_t)(2 * y) * (2 * mbw) + 2 * x;
    int ra = -2, rb = -2, rc = -2;
    uint32_t ma = 0, mvb = 0, mc = 0;
    if( x > 0 )
    {
        ra = rf[-1];
        ma = mv[-1];
    }
    if( y > 0 )
    {
        rb = rf[-2 * mbw];
        mvb = mv[-4 * mbw];
        if( x < mbw - 1 )
        {
            rc = rf[-2 * mbw + 2];
            mc = mv[-4 * mbw + 4];
        }
        if( rc == -2 && x > 0 )               // mvpred.c:137-141
        {
            rc = rf[-2 * mbw - 1];
            mc = mv[-4 * mbw - 1];
        }
    }
    uint32_t r;
    if( ra == -2 || rb == -2 || !( (uint32_t)ra | ma ) || !( (uint32_t)rb | mvb ) )
        r = 0;
    else
    {
        const int cnt = (ra == 0) + (rb == 0) + (rc == 0);
        if( cnt == 1 )
            r = ra == 0 ? ma : rb == 0 ? mvb : mc;
        else if( cnt == 0 && rb == -2 && rc == -2 && ra != -2 )
            r = ma;
        else
        {
            const int mx = median3( (int16_t)ma, (int16_t)mvb, (int16_t)mc );
            const int my = median3( (int16_t)(ma >> 16), (int16_t)(mvb >> 16), (int16_t)(mc >> 16) );
            r = ((uint32_t)mx & 0xffff) | ((uint32_t)my << 16);
        }
    }
    out[mb] = r;
}

// ---------------------------------------------------------------- the skip conversion
__global__ __launch_bounds__( 256 ) void mb_skip_convert_kernel( const uint8_t *mb_flags, const int32_t *__restrict__ cbp,
                                                                 const uint32_t *__restrict__ mv0,
                                                                 const int8_t *__restrict__ ref0,
                                                                 const uint32_t *__restrict__ pskip, int bframe,
                                                                 const uint8_t *__restrict__ direct, int mbw, int mbh,
                                                                 int nmb, uint8_t *flags )
{
    const int mb = blockIdx.x * 256 + threadIdx.x;
    if( mb >= nmb )
        return;
    const int fl = mb_flags[mb];
    bool conv = !( fl & X264HIP_MBENC_INTRA ) && !( cbp[mb] & 0x3f );
    if( bframe )
        conv = conv && direct[mb];
    else
    {
        conv = conv && !( fl & X264HIP_MBENC_SKIP ) && ( fl & X264HIP_MBENC_D16x16 );
        if( conv )
        {
            const int per = mbw * mbh;
            const int f = mb / per, rem = mb - f * per;
            const int y = rem / mbw, x = rem - y * mbw;
            conv = ref0[(int64_t)f * per * 4 + (int64_t)(2 * y) * (2 * mbw) + 2 * x] == 0 &&
                   mv0[(int64_t)f * per * 16 + (int64_t)(4 * y) * (4 * mbw) + 4 * x] == pskip[mb];
        }
    }
    flags[mb] = (uint8_t)( fl | ( conv ? X264HIP_MBENC_SKIP : 0 ) );
}

// ---------------------------------------------------------------- x264_macroblock_probe_skip
template <int BD> struct SkipPlanes          // F, H, V, C of one plane of the reference
{
    const typename PT<BD>::pixel *p0, *p1, *p2, *p3;
};

// the launch's inputs, by value in the kernel arguments (named members for everything a lane
// selects from, mcdev.h's rule)
template <int BD> struct SkipParams
{
    using pixel = typename PT<BD>::pixel;
    using udctcoef = typename PT<BD>::udctcoef;
    const pixel *fenc, *fc0, *fc1;
    intptr_t fs, ffs, fcs, fcfs;
    SkipPlanes<BD> ry, ru, rv;                // the P leg; ru.p0: the interleaved plane at 4:2:0 / 4:2:2
    intptr_t rs, rfs, rcs, rfcs;
    RsWeight wy, wu, wv;
    const uint32_t *pskip;
    const pixel *pred, *pc0, *pc1;            // the B leg
    intptr_t ps, pfs, pcs, pfcs;
    const udctcoef *q4mf, *q4b;
    const int8_t *qp;
    uint8_t *skip;
    int mbw, mbh, nmb, al;                    // al: skip is 4-byte aligned
    uint32_t cqp[16];                         // chroma_qp_table[0..63], four entries a word
    uint32_t thr[64];                         // macroblock.c:1037's thresh of every chroma qp
};

constexpr int LEG_P = 0, LEG_PW = 1, LEG_B = 2;   // the P leg without and with a weight, the B leg

// this lane's 4x4 difference block of one plane: fenc - prediction.  e: the block in fenc; P leg:
// q the plane's F, H, V, C, at the block's offset in them; B leg: p the block in pred
template <int BD, int LEG>
__device__ __forceinline__ void plane_diff( const typename PT<BD>::pixel *e, intptr_t es, const SkipPlanes<BD> &q,
                                            intptr_t at, intptr_t rs, int mvx, int mvy, const RsWeight &wt,
                                            const typename PT<BD>::pixel *p, intptr_t ps, int ( &d )[4][4] )
{
    if constexpr( LEG == LEG_B )
        load_diff<BD, 4>( d, e, es, p, ps );
    else
    {
        constexpr int PPD = PT<BD>::PPD, LW = 4 / PPD;
        uint32_t r[4][LW];
        ref_tile<BD, LW, true>( q.p0, q.p1, q.p2, q.p3, at, rs, mvx, mvy, r );
        if constexpr( LEG == LEG_PW )
            if( wt.on )
            {
#pragma unroll
                for( int y = 0; y < 4; y++ )
#pragma unroll
                    for( int k = 0; k < LW; k++ )
                        r[y][k] = weigh_packed<BD>( r[y][k], wt );
            }
#pragma unroll
        for( int y = 0; y < 4; y++ )
        {
            uint32_t w[LW];
            load_packed<LW>( e + y * es, w );
#pragma unroll
            for( int x = 0; x < 4; x++ )
                d[y][x] = upix<BD>( w[x / PPD], x % PPD ) - upix<BD>( r[y][x / PPD], x % PPD );
        }
    }
}

// decimate_score16 of this lane's block of a luma-coded plane (macroblock.c:1015-1029); mf, bias:
// the category's rows at the plane's qp
template <int BD>
__device__ __forceinline__ int plane_score( int ( &d )[4][4], const typename PT<BD>::udctcoef *mf,
                                            const typename PT<BD>::udctcoef *bias )
{
    int c[16];
    dct4x4_core<BD>( d, c );
    int acc = 0;
#pragma unroll
    for( int j = 0; j < 16; j++ )
    {
        c[j] = sto<BD>( quant_one( c[j], mf[j], bias[j] ) );
        acc |= c[j];
    }
    if( !acc )
        return 0;
    return decimate_score<16, 0>( [&]( int i ) { return c[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )]; } );
}

// mc_chroma (mc.c:252-283) of this lane's 4 rows of 4 (U, V) pairs at s (the interleaved plane at
// the block's first U sample): five source rows of five pairs, m[y][x] = the pair as u16 lanes
template <int BD>
__device__ __forceinline__ void chroma_pairs4( const typename PT<BD>::pixel *s, intptr_t rcs, int mvx, int mvyc,
                                               rs_us2 ( &m )[4][4] )
{
    typedef const __attribute__( ( address_space( 1 ) ) ) uint32_t gword;
    constexpr int NDW = BD == 8 ? 3 : 5;
    const ChromaTapsPk t = chroma_taps_pk( mvx, mvyc );
    s += chroma_off( mvx, mvyc, rcs );
    uint32_t w[5][NDW];
#pragma unroll
    for( int y = 0; y < 5; y++ )
    {
        if constexpr( BD == 8 )
        {
            // ten bytes from a (U, V) pair boundary lie in the three dwords from the aligned-down
            // address: nothing past them is read
            const uint32_t sh = (uint32_t)( (uintptr_t)( s + y * rcs ) & 3 );
            gword *b = (gword *)( (uintptr_t)( s + y * rcs ) & ~(uintptr_t)3 );
            const uint32_t w0 = b[0], w1 = b[1], w2 = b[2];
            w[y][0] = __builtin_amdgcn_alignbyte( w1, w0, sh );
            w[y][1] = __builtin_amdgcn_alignbyte( w2, w1, sh );
            w[y][2] = __builtin_amdgcn_alignbyte( w2, w2, sh );
        }
        else
        {
            // a 10-bit pair is a dword: the row's five words as they lie
            gword *b = (gword *)(uintptr_t)( s + y * rcs );
#pragma unroll
            for( int k = 0; k < NDW; k++ )
                w[y][k] = b[k];
        }
    }
#pragma unroll
    for( int y = 0; y < 4; y++ )
#pragma unroll
        for( int x = 0; x < 4; x++ )
            m[y][x] = chroma_pair<BD>( t, w[y], w[y + 1], x );
}

// what is left of one chroma channel once its ssd is not below thresh (macroblock.c:1069-1121):
// the DC blocks must quantise to nothing, then 4 * thresh or the AC decimate sum decides.  d: this
// lane's 4x4 difference block (zeros on the lanes past the channel's blocks).  Uniform over the
// macroblock's lanes except d.
template <int BD, int CF>
__device__ __forceinline__ bool chroma_rest( const SkipParams<BD> &a, int ( &d )[4][4], int qpc, int ssd, int thresh )
{
    constexpr int NDC = CF == 1 ? 4 : 8;
    constexpr int QP1 = 52 + 6 * (BD - 8);
    // sub8x8_dct_dc / sub8x16_dct_dc (dct.c:207-270): the 4x4 sums, then the butterflies
    int t = 0;
#pragma unroll
    for( int y = 0; y < 4; y++ )
#pragma unroll
        for( int x = 0; x < 4; x++ )
            t += d[y][x];
    int s[NDC], dc[NDC];
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
    const int qdc = qpc + ( CF == 2 ? 3 : 0 );
    const uint32_t dcmf = (uint32_t)a.q4mf[( SKIP_4PC * QP1 + qdc ) * 16] >> 1;
    const uint32_t dcb = (uint32_t)a.q4b[( SKIP_4PC * QP1 + qdc ) * 16] << 1;
    if( quant_chroma_dc<BD, NDC>( dc, dcmf, dcb ) )
        return false;
    if( ssd < thresh * 4 )
        return true;
    // sub8x8_dct with the DCs zeroed, quant_4x4x4, decimate_score15
    int c[16];
    dct4x4_core<BD>( d, c );
    c[0] = 0;
    const typename PT<BD>::udctcoef *mf = a.q4mf + ( SKIP_4PC * QP1 + qpc ) * 16, *bias = a.q4b + ( SKIP_4PC * QP1 + qpc ) * 16;
    int acc = 0;
#pragma unroll
    for( int k = 0; k < 16; k++ )
    {
        c[k] = sto<BD>( quant_one( c[k], mf[k], bias[k] ) );
        acc |= c[k];
    }
    int score = 0;
    if( acc )
        score = decimate_score<16, 1>( [&]( int i ) { return c[ZZF<4>::x( i ) * 4 + ZZF<4>::y( i )]; } );
    return mb_sum( score ) < 7;
}

template <int BD, int CF, int LEG>
__global__ __launch_bounds__( 256 ) void mb_probe_skip_kernel( const SkipParams<BD> a )
{
    using pixel = typename PT<BD>::pixel;
    constexpr int QP1 = 52 + 6 * (BD - 8);
    // The chroma qp table and the thresholds, indexed per lane below: the 80 words as they lie in
    // the kernel-argument segment (the block is the kernel's one argument, at offset 0), a word per
    // lane.  mbenc.hip's fill, an unrolled `if( threadIdx.x == k )` per word, holds every word in
    // an SGPR: with 80 of them the compiler spilled SGPRs through v_writelane and the kernel grew to
    // 50 000 instructions.
    __shared__ uint32_t s_cqp[16 + 64];
    const uint32_t *s_thr = s_cqp + 16;
    static_assert( offsetof( SkipParams<BD>, thr ) == offsetof( SkipParams<BD>, cqp ) + 64, "cqp and thr lie together" );
    if( threadIdx.x < ( CF == 1 || CF == 2 ? 80 : 16 ) )
    {
        typedef const __attribute__( ( address_space( 4 ) ) ) uint32_t kword;
        kword *ka = (kword *)( (const __attribute__( ( address_space( 4 ) ) ) char *)__builtin_amdgcn_kernarg_segment_ptr() +
                               offsetof( SkipParams<BD>, cqp ) );
        s_cqp[threadIdx.x] = ka[threadIdx.x];
    }
    __syncthreads();
    const int l = threadIdx.x & 15;
    const int slot = ( threadIdx.x & 63 ) >> 4;               // the macroblock's place in its wave
    const int mb_own = blockIdx.x * 16 + ( threadIdx.x >> 4 );
    // the lanes past the batch probe its last macroblock again and store nothing: the wave's
    // result is gathered from all four slots
    const bool live = mb_own < a.nmb;
    const int mb = live ? mb_own : a.nmb - 1;
    const int per = a.mbw * a.mbh;
    const int f = mb / per, rem = mb - f * per;
    const int mby = rem / a.mbw, mbx = rem - mby * a.mbw;
    const int qp = min( max( (int)a.qp[mb], 0 ), QP1 - 1 );
    const int qpc = min( (int)( ( s_cqp[qp >> 2] >> ( 8 * ( qp & 3 ) ) ) & 255 ), QP1 - 1 - ( CF == 2 ? 3 : 0 ) );

    // the skip vector, clipped to h->mb.mv_min / mv_max (macroblock.c:1001-1002, analyse.c:336-337, 391-392)
    int mvx = 0, mvy = 0;
    if constexpr( LEG != LEG_B )
    {
        const uint32_t m = a.pskip[mb];
        mvx = min( max( (int)(int16_t)m, 4 * ( -16 * mbx - 24 ) ), 4 * ( 16 * ( a.mbw - mbx - 1 ) + 24 ) );
        mvy = min( max( (int)(int16_t)( m >> 16 ), 4 * ( -16 * mby - 24 ) ), 4 * ( 16 * ( a.mbh - mby - 1 ) + 24 ) );
    }

    // ---------------------------------------------------------------- the differences
    const int i8 = l >> 2, i4 = l & 3;
    const int bx = ( i8 & 1 ) * 8 + ( i4 & 1 ) * 4, by = ( i8 >> 1 ) * 8 + ( i4 >> 1 ) * 4;
    const int px = 16 * mbx + bx, py = 16 * mby + by;
    int dy[4][4];
    plane_diff<BD, LEG>( a.fenc + (intptr_t)f * a.ffs + (intptr_t)py * a.fs + px, a.fs, a.ry,
                         (intptr_t)f * a.rfs + (intptr_t)py * a.rs + px, a.rs, mvx, mvy, a.wy,
                         a.pred + (intptr_t)f * a.pfs + (intptr_t)py * a.ps + px, a.ps, dy );
    int du[4][4], dv[4][4];
    if constexpr( CF == 3 )
    {
        const intptr_t fo = (intptr_t)f * a.fcfs + (intptr_t)py * a.fcs + px;
        const intptr_t at = (intptr_t)f * a.rfcs + (intptr_t)py * a.rcs + px;
        const intptr_t po = (intptr_t)f * a.pfcs + (intptr_t)py * a.pcs + px;
        plane_diff<BD, LEG>( a.fc0 + fo, a.fcs, a.ru, at, a.rcs, mvx, mvy, a.wu, a.pc0 + po, a.pcs, du );
        plane_diff<BD, LEG>( a.fc1 + fo, a.fcs, a.rv, at, a.rcs, mvx, mvy, a.wv, a.pc1 + po, a.pcs, dv );
    }
    else if constexpr( CF != 0 )
    {
        constexpr int NCB = CF == 1 ? 4 : 8, CH = CF == 1 ? 8 : 16;
#pragma unroll
        for( int y = 0; y < 4; y++ )
#pragma unroll
            for( int x = 0; x < 4; x++ )
                du[y][x] = dv[y][x] = 0;
        if( l < NCB )
        {
            const int cx = 16 * mbx + 8 * ( l & 1 ), cy = CH * mby + 4 * ( l >> 1 );
            const pixel *fp = a.fc0 + (intptr_t)f * a.fcfs + (intptr_t)cy * a.fcs + cx;
            if constexpr( LEG == LEG_B )
            {
                const pixel *pp = a.pc0 + (intptr_t)f * a.pfcs + (intptr_t)cy * a.pcs + cx;
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
            else
            {
                // mc_chroma( mvx, mvy << c422 ) (macroblock.c:1045-1047), then the weights (:1058-1061)
                rs_us2 m[4][4];
                chroma_pairs4<BD>( a.ru.p0 + (intptr_t)f * a.rfcs + (intptr_t)cy * a.rcs + cx, a.rcs, mvx,
                                   CF == 2 ? 2 * mvy : mvy, m );
                if constexpr( LEG == LEG_PW )
                    if( a.wu.on | a.wv.on )
                    {
#pragma unroll
                        for( int y = 0; y < 4; y++ )
#pragma unroll
                            for( int x = 0; x < 4; x++ )
                                m[y][x] = weigh_pair<BD>( m[y][x], a.wu, a.wv );
                    }
#pragma unroll
                for( int y = 0; y < 4; y++ )
                {
                    int e[8];
                    read_row<BD, 8>( fp + y * a.fcs, e );
#pragma unroll
                    for( int x = 0; x < 4; x++ )
                    {
                        du[y][x] = e[2 * x] - (int)m[y][x].x;
                        dv[y][x] = e[2 * x + 1] - (int)m[y][x].y;
                    }
                }
            }
        }
    }

    // ---------------------------------------------------------------- luma (macroblock.c:995-1031)
    bool ok = mb_sum( plane_score<BD>( dy, a.q4mf + ( SKIP_4PY * QP1 + qp ) * 16, a.q4b + ( SKIP_4PY * QP1 + qp ) * 16 ) ) < 6;
    if constexpr( CF == 3 )
    {
        const typename PT<BD>::udctcoef *mf = a.q4mf + ( SKIP_4PC * QP1 + qpc ) * 16, *bias = a.q4b + ( SKIP_4PC * QP1 + qpc ) * 16;
        ok = ok && mb_sum( plane_score<BD>( du, mf, bias ) ) < 6;
        ok = ok && mb_sum( plane_score<BD>( dv, mf, bias ) ) < 6;
    }
    // ---------------------------------------------------------------- chroma (:1033-1123)
    // a macroblock whose luma failed is decided: its lanes leave the chroma alone
    if constexpr( CF == 1 || CF == 2 )
        if( ok )
        {
            int qu = 0, qv = 0;
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                {
                    qu += du[y][x] * du[y][x];
                    qv += dv[y][x] * dv[y][x];
                }
            qu = mb_sum( qu );
            qv = mb_sum( qv );
            const int thresh = (int)s_thr[qpc];
            if( qu >= thresh )
                ok = chroma_rest<BD, CF>( a, du, qpc, qu, thresh );
            if( ok && qv >= thresh )
                ok = chroma_rest<BD, CF>( a, dv, qpc, qv, thresh );
        }

    // ---------------------------------------------------------------- skip[mb]
    const uint64_t all = __ballot( ok );
    const int mb0 = mb_own - slot;                            // the wave's first macroblock, a multiple of 4
    if( a.al && mb0 + 3 < a.nmb )
    {
        if( ( threadIdx.x & 63 ) == 0 )
            *(uint32_t *)( a.skip + mb0 ) = (uint32_t)( all & 1 ) | (uint32_t)( ( all >> 16 ) & 1 ) << 8 |
                                            (uint32_t)( ( all >> 32 ) & 1 ) << 16 | (uint32_t)( ( all >> 48 ) & 1 ) << 24;
    }
    else if( l == 0 && live )
        a.skip[mb_own] = (uint8_t)ok;
}

// x264_weight_t as the core takes it (what mbmc.hip's own mc_weight_of states for mb_mc)
template <int BD> RsWeight skip_weight_of( const x264hip_weight_t &w )
{
    return { w.weighted ? 1 : 0, w.scale, w.weighted ? w.denom : 0, w.weighted && w.denom > 0 ? 1 << ( w.denom - 1 ) : 0,
             w.offset * ( 1 << ( BD - 8 ) ) };
}

template <int BD, int CF>
void probe_go( int leg, dim3 g, hipStream_t stream, const SkipParams<BD> &a )
{
    switch( leg )
    {
        case LEG_P: hipLaunchKernelGGL( ( mb_probe_skip_kernel<BD, CF, LEG_P> ), g, dim3( 256 ), 0, stream, a ); break;
        case LEG_PW: hipLaunchKernelGGL( ( mb_probe_skip_kernel<BD, CF, LEG_PW> ), g, dim3( 256 ), 0, stream, a ); break;
        default: hipLaunchKernelGGL( ( mb_probe_skip_kernel<BD, CF, LEG_B> ), g, dim3( 256 ), 0, stream, a ); break;
    }
}

} // namespace

// the arguments were checked by the C entries (capi.cpp)
hipError_t launch_mb_predict_mv_pskip( const int16_t *mv0, const int8_t *ref0, int mbw, int mbh, int n_frames,
                                       int16_t *pskip_mv, hipStream_t stream )
{
    const int64_t nmb = (int64_t)n_frames * mbw * mbh;
    if( nmb <= 0 )
        return hipSuccess;
    hipLaunchKernelGGL( mb_predict_mv_pskip_kernel, dim3( (unsigned)( ( nmb + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        (const uint32_t *)mv0, ref0, mbw, mbh, (int)nmb, (uint32_t *)pskip_mv );
    return hipGetLastError();
}

hipError_t launch_mb_skip_convert( const uint8_t *mb_flags, const int32_t *cbp, const int16_t *mv0, const int8_t *ref0,
                                   const int16_t *pskip_mv, int b_bframe, const uint8_t *direct, int mbw, int mbh,
                                   int n_frames, uint8_t *flags, hipStream_t stream )
{
    const int64_t nmb = (int64_t)n_frames * mbw * mbh;
    if( nmb <= 0 )
        return hipSuccess;
    hipLaunchKernelGGL( mb_skip_convert_kernel, dim3( (unsigned)( ( nmb + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        mb_flags, cbp, (const uint32_t *)mv0, ref0, (const uint32_t *)pskip_mv, b_bframe != 0, direct,
                        mbw, mbh, (int)nmb, flags );
    return hipGetLastError();
}

template <int BD>
hipError_t launch_mb_probe_skip( const x264hip_mbskip_t *s, int mbw, int mbh, int n_frames, hipStream_t stream )
{
    using cp = const typename PT<BD>::pixel *;
    const int64_t nmb = (int64_t)n_frames * mbw * mbh;
    if( !s || nmb <= 0 )
        return hipSuccess;
    const int cf = s->chroma_format;
    SkipParams<BD> a;
    memset( &a, 0, sizeof( a ) );
    a.fenc = (cp)s->fenc; a.fc0 = (cp)s->fenc_chroma[0]; a.fc1 = (cp)s->fenc_chroma[1];
    a.fs = s->fenc_stride; a.ffs = s->fenc_frame_stride;
    a.fcs = s->fenc_chroma_stride; a.fcfs = s->fenc_chroma_frame_stride;
    int leg = LEG_B;
    if( s->b_bidir )
    {
        a.pred = (cp)s->pred; a.pc0 = (cp)s->pred_chroma[0]; a.pc1 = (cp)s->pred_chroma[1];
        a.ps = s->pred_stride; a.pfs = s->pred_frame_stride;
        a.pcs = s->pred_chroma_stride; a.pfcs = s->pred_chroma_frame_stride;
    }
    else
    {
        const x264hip_mc_ref_t &r = s->ref;
        a.ry = { (cp)r.luma[0], (cp)r.luma[1], (cp)r.luma[2], (cp)r.luma[3] };
        a.ru = { (cp)r.chroma[0], (cp)r.chroma[1], (cp)r.chroma[2], (cp)r.chroma[3] };
        a.rv = { (cp)r.chroma[4], (cp)r.chroma[5], (cp)r.chroma[6], (cp)r.chroma[7] };
        a.rs = s->ref_stride; a.rfs = s->ref_frame_stride;
        a.rcs = s->ref_chroma_stride; a.rfcs = s->ref_chroma_frame_stride;
        a.wy = skip_weight_of<BD>( s->weight[0] );
        a.wu = skip_weight_of<BD>( s->weight[1] );
        a.wv = skip_weight_of<BD>( s->weight[2] );
        a.pskip = (const uint32_t *)s->pskip_mv;
        // the weighting kernel only where a weight the format reads is on
        leg = a.wy.on || ( cf && ( a.wu.on || a.wv.on ) ) ? LEG_PW : LEG_P;
    }
    a.q4mf = (const typename PT<BD>::udctcoef *)s->quant4_mf;
    a.q4b = (const typename PT<BD>::udctcoef *)s->quant4_bias;
    a.qp = s->qp;
    a.skip = s->skip;
    a.mbw = mbw; a.mbh = mbh; a.nmb = (int)nmb;
    a.al = !( (uintptr_t)s->skip & 3 );
    pack_cqp<BD>( s->chroma_qp_table, a.cqp );
    for( int q = 0; q < 64; q++ )
        a.thr[q] = (uint32_t)( cf == 2 ? ( k_lambda2_tab[q] + 16 ) >> 5 : ( k_lambda2_tab[q] + 32 ) >> 6 );
    const dim3 g( (unsigned)( ( nmb + 15 ) / 16 ) );
    switch( cf )
    {
        case 0: probe_go<BD, 0>( leg, g, stream, a ); break;
        case 1: probe_go<BD, 1>( leg, g, stream, a ); break;
        case 2: probe_go<BD, 2>( leg, g, stream, a ); break;
        default: probe_go<BD, 3>( leg, g, stream, a ); break;
    }
    return hipGetLastError();
}
X264HIP_INSTANTIATE( launch_mb_probe_skip );

} // namespace x264hip
