// The motion-compensation core every predicting kernel shares (refine.hip, mbmc.hip, mc.hip,
// weightp.hip, lookahead.hip): get_ref's plane pair and rounding average, mc_chroma's taps,
// mc_weight and the bipred averages of reference common/mc.c:49-283.
//
// Rules of this header (each learned at one site, DESIGN.md §5 "Motion compensation core"):
//  * a plane is selected over four separate pointers (ref_ptr0 / ref_ptr1), never over an array or a struct
//    member indexed per lane: such selects became indexed loads through scratch memory;
//  * tables are read as bit fields of compile-time words (pack_fields / field), never as memory;
//  * pointers never round-trip through integers on their way to a load (a global load turns flat);
//  * clip( v >> S ) is written shr_clip<BD, S>( v );
//  * load_al_pad reads up to 4 bytes past the pixels asked for: padded planes only;
//  * every function is __device__ __forceinline__, and whether the second plane's loads sit
//    behind a branch is a template parameter the call site decides, not a run-time choice here.
#pragma once
#include "hipcommon.h"

namespace x264hip {

// ---- get_ref (mc.c:221-249) ----
// the plane pair per qpel phase (mc.c:203-209, common/tables.c:183-184): the only copies
constexpr uint8_t c_ref0[16] = { 0, 1, 1, 1, 0, 1, 1, 1, 2, 3, 3, 3, 0, 1, 1, 1 };   // x264_hpel_ref0
constexpr uint8_t c_ref1[16] = { 0, 0, 1, 0, 2, 2, 3, 2, 2, 2, 3, 2, 2, 2, 3, 2 };   // x264_hpel_ref1
constexpr uint32_t k_ref0 = pack_fields( c_ref0, 2 ), k_ref1 = pack_fields( c_ref1, 2 );

// a quarter-pel mv decoded: its phase (idx = 4 fy + fx), planes i0 / i1 of F, H, V, C and the
// pixel offset of the full-pel part (from `at`).  The first plane steps a row down at fy == 3,
// the second a column right at fx == 3; idx & 5 says whether the phase averages two planes (at
// a full- or half-pel phase both name one plane at one offset, and avg( a, a ) = a)
struct RefPhase
{
    int idx, fx, fy, i0, i1;
    intptr_t off;
    __device__ __forceinline__ bool two() const { return idx & 5; }
};
__device__ __forceinline__ RefPhase ref_phase( int mvx, int mvy, intptr_t rs, intptr_t at = 0 )
{
    const int idx = ((mvy & 3) << 2) + (mvx & 3);
    const intptr_t off = at + (intptr_t)(mvy >> 2) * rs + (mvx >> 2);
    return { idx, mvx & 3, mvy & 3, field( k_ref0, 2, idx ), field( k_ref1, 2, idx ), off };
}
// the first / second source pointer: a select over four plane pointers ...
template <typename P>
__device__ __forceinline__ const P *ref_ptr0( const RefPhase &ph, const P *q0, const P *q1, const P *q2, const P *q3,
                                              intptr_t rs )
{
    return (ph.i0 == 0 ? q0 : ph.i0 == 1 ? q1 : ph.i0 == 2 ? q2 : q3) + ph.off + (ph.fy == 3) * rs;
}
template <typename P>
__device__ __forceinline__ const P *ref_ptr1( const RefPhase &ph, const P *q0, const P *q1, const P *q2, const P *q3 )
{
    return (ph.i1 == 0 ? q0 : ph.i1 == 1 ? q1 : ph.i1 == 2 ? q2 : q3) + ph.off + (ph.fx == 3);
}
// ... or four planes equally spaced by pd (the lookahead's lowres buffer): one multiply-add
template <typename P> __device__ __forceinline__ const P *ref_ptr0( const RefPhase &ph, const P *p0, intptr_t pd, intptr_t rs )
{
    return p0 + ph.i0 * pd + ph.off + (ph.fy == 3) * rs;
}
template <typename P> __device__ __forceinline__ const P *ref_ptr1( const RefPhase &ph, const P *p0, intptr_t pd )
{
    return p0 + ph.i1 * pd + ph.off + (ph.fx == 3);
}

// four rows of LW words of get_ref( mvx, mvy ) (unweighted) at q + at + the mv's offset.
// BOTH: both planes always, with no branch between the loads (the second load of a one-plane
// phase hits the line the first brought); else the second plane only at a two-plane phase
template <int BD, int LW, bool BOTH>
__device__ __forceinline__ void ref_tile( const typename PT<BD>::pixel *q0, const typename PT<BD>::pixel *q1,
                                          const typename PT<BD>::pixel *q2, const typename PT<BD>::pixel *q3,
                                          intptr_t at, intptr_t rs, int mvx, int mvy, uint32_t ( &r )[4][LW] )
{
    const RefPhase ph = ref_phase( mvx, mvy, rs, at );
    const typename PT<BD>::pixel *s1 = ref_ptr0( ph, q0, q1, q2, q3, rs ), *s2 = ref_ptr1( ph, q0, q1, q2, q3 );
    uint32_t r2[4][LW];
#pragma unroll
    for( int y = 0; y < 4; y++ )
    {
        load_al_pad<LW>( s1 + y * rs, r[y] );
        if constexpr( BOTH )
            load_al_pad<LW>( s2 + y * rs, r2[y] );
    }
    if( BOTH || ph.two() )
    {
        if constexpr( !BOTH )
        {
#pragma unroll
            for( int y = 0; y < 4; y++ )
                load_al_pad<LW>( s2 + y * rs, r2[y] );
        }
#pragma unroll
        for( int y = 0; y < 4; y++ )
#pragma unroll
            for( int k = 0; k < LW; k++ )
                r[y][k] = avg_round<BD>( r[y][k], r2[y][k] );
    }
}

// ---- mc_weight (mc.c:117-137) ----
// explicit weight of one plane (x264_weight_t): rnd = 1 << (denom - 1) or 0, offset already
// scaled by 1 << (BIT_DEPTH - 8)
struct RsWeight
{
    int on, scale, denom, rnd, offset;
};
// one pixel: clip( ((v * scale + rnd) >> denom) + offset )
template <int BD> __device__ __forceinline__ int weigh_pixel( int v, int scale, int rnd, int denom, int offset )
{
    return clip_pix<BD>( ((v * scale + rnd) >> denom) + offset );
}
template <int BD> __device__ __forceinline__ int weigh_pixel( int v, const RsWeight &wt )
{
    return weigh_pixel<BD>( v, wt.scale, wt.rnd, wt.denom, wt.offset );
}
template <int BD> __device__ __forceinline__ uint32_t weigh_packed( uint32_t w, const RsWeight &wt )
{
    constexpr int PPD = PT<BD>::PPD, SH = 32 / PPD;
    uint32_t r = 0;
#pragma unroll
    for( int k = 0; k < PPD; k++ )
        r |= (uint32_t)weigh_pixel<BD>( upix<BD>( w, k ), wt ) << (SH * k);
    return r;
}

// ---- mc_chroma (mc.c:252-283) ----
// the (U, V) samples of pixel x of a row of interleaved (NV12 / NV16) words, as u16 lanes
typedef unsigned short rs_us2 __attribute__( ( ext_vector_type( 2 ) ) );
__device__ __forceinline__ rs_us2 as_us2( uint32_t v ) { return __builtin_bit_cast( rs_us2, v ); }
template <int BD> __device__ __forceinline__ rs_us2 nv_pair( const uint32_t *w, int x )
{
    if constexpr( BD == 8 )
        return as_us2( __builtin_amdgcn_perm( 0u, w[x >> 1], (x & 1) ? 0x0c030c02u : 0x0c010c00u ) );
    else
        return as_us2( w[x] );
}
// a (U, V) pair weighted by its planes' weights (either may be off)
template <int BD> __device__ __forceinline__ rs_us2 weigh_pair( rs_us2 m, const RsWeight &wu, const RsWeight &wv )
{
    int lo = m.x, hi = m.y;
    if( wu.on )
        lo = weigh_pixel<BD>( lo, wu );
    if( wv.on )
        hi = weigh_pixel<BD>( hi, wv );
    return (rs_us2){ (uint16_t)lo, (uint16_t)hi };
}

// the four bilinear taps of ( mvx, mvyc ) (they sum to 64) and the interleaved plane's offset
// of the mv's full-pel part
struct ChromaTaps
{
    uint32_t cA, cB, cC, cD;
};
__device__ __forceinline__ ChromaTaps chroma_taps( int mvx, int mvyc )
{
    const uint32_t dx = mvx & 7, dy = mvyc & 7;
    return { (8 - dx) * (8 - dy), dx * (8 - dy), (8 - dx) * dy, dx * dy };
}
__device__ __forceinline__ intptr_t chroma_off( int mvx, int mvyc, intptr_t rcs )
{
    return (intptr_t)(mvyc >> 3) * rcs + (mvx >> 3) * 2;
}
// both planes at once as packed u16 multiply-adds (64 * 1023 + 32 fits): output pair x from
// the words of source rows y (w0) and y + 1 (w1)
struct ChromaTapsPk
{
    rs_us2 kA, kB, kC, kD;
};
__device__ __forceinline__ ChromaTapsPk chroma_taps_pk( int mvx, int mvyc )
{
    const ChromaTaps t = chroma_taps( mvx, mvyc );
    return { (rs_us2)(uint16_t)t.cA, (rs_us2)(uint16_t)t.cB, (rs_us2)(uint16_t)t.cC, (rs_us2)(uint16_t)t.cD };
}
template <int BD>
__device__ __forceinline__ rs_us2 chroma_pair( const ChromaTapsPk &t, const uint32_t *w0, const uint32_t *w1, int x )
{
    return (t.kA * nv_pair<BD>( w0, x ) + t.kB * nv_pair<BD>( w0, x + 1 ) + t.kC * nv_pair<BD>( w1, x ) +
            t.kD * nv_pair<BD>( w1, x + 1 ) + (rs_us2)32) >> (rs_us2)6;
}

// ---- the bipred average (mc.avg, mc.c:49-87) ----
// pixel_avg_weight_wxh of one pixel / of packed words, any weight: clipped (clamp-first shift)
template <int BD> __device__ __forceinline__ int bi_weighted_px( int a, int b, int w1 )
{
    return shr_clip<BD, 6>( a * w1 + b * (64 - w1) + 32 );
}
template <int BD> __device__ __forceinline__ uint32_t bi_weighted( uint32_t a, uint32_t b, int w1, int w2 )
{
    constexpr int PPD = PT<BD>::PPD, SH = 32 / PPD;
    uint32_t r = 0;
#pragma unroll
    for( int k = 0; k < PPD; k++ )
        r |= (uint32_t)shr_clip<BD, 6>( upix<BD>( a, k ) * w1 + upix<BD>( b, k ) * w2 + 32 ) << (SH * k);
    return r;
}
// weight 32 = pixel_avg_wxh, the rounding average
template <int BD> __device__ __forceinline__ uint32_t bi_packed( uint32_t a, uint32_t b, int w1 )
{
    return w1 == 32 ? avg_round<BD>( a, b ) : bi_weighted<BD>( a, b, w1, 64 - w1 );
}
// (a caller with a weight per partition decides it once per tile, not per word: per word the
// bidir refine gained ~15 exec-mask branches per instance.  That kernel keeps its weighted loop
// local, see refine.hip.)

// the lookahead's form, a different function: ONLY for w in [0, 64] (slicetype.c's bipred
// weights), where no clip is needed and (a*w + b*(64-w) + 32) >> 6 runs in packed u16 lanes
// (1023 * 64 + 32 < 2^16).  Not folded into the clipped form: its kernel was measured with it.
template <int BD> __device__ __forceinline__ uint32_t bi_packed_noclip( uint32_t a, uint32_t b, int w )
{
    if( w == 32 )
        return avg_round<BD>( a, b );
    const rs_us2 wa = (rs_us2)(unsigned short)w, wb = (rs_us2)(unsigned short)(64 - w);
    auto f = [&]( uint32_t x, uint32_t y ) {
        const rs_us2 r = (as_us2( x ) * wa + as_us2( y ) * wb + (rs_us2)32) >> (rs_us2)6;
        return __builtin_bit_cast( uint32_t, r );
    };
    if constexpr( BD == 8 )
    {
        const uint32_t lo = f( __builtin_amdgcn_perm( 0u, a, 0x0c020c00u ), __builtin_amdgcn_perm( 0u, b, 0x0c020c00u ) );
        const uint32_t hi = f( __builtin_amdgcn_perm( 0u, a, 0x0c030c01u ), __builtin_amdgcn_perm( 0u, b, 0x0c030c01u ) );
        return __builtin_amdgcn_perm( hi, lo, 0x06020400u );
    }
    else
        return f( a, b );
}

} // namespace x264hip
