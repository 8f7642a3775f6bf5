// Batched motion compensation: x264_mb_mc (reference common/macroblock.c:31-246) of a list of
// equally sized partitions into caller-owned prediction planes (include/x264hip_mc.h), from
// mc_luma / get_ref / mc_chroma / mc_weight / the avg table of common/mc.c:49-283.
//
// A streaming kernel: a lane builds one 4x4 luma tile of a partition and the chroma under it --
// the 2x2 (4:2:0) or 2x4 (4:2:2) block of (U, V) pairs of the interleaved plane, or the 4x4 tiles
// of the U and V planes (4:4:4) -- so every row it stores is one dword (8 bit) or two (10 bit) and
// the lanes of a partition's tile row store one contiguous run.  A partition takes
// (w / 4) * (h / 4) consecutive lanes (16x16: 16, 4x4: one), a wave 4 .. 64 partitions; nothing
// crosses lanes and no LDS is used.  Rows are read as the dword-aligned words that hold them and
// realigned with v_alignbyte (load_al_pad: the planes are padded), the qpel average is get_ref's
// plane pair joined by one v_lerp_u8 per dword (packed u16 adds at 10 bit), and mc_chroma runs on
// (U, V) pairs as packed u16 multiply-adds (the taps sum to 64, so 64 * 1023 + 32 fits).
//
// A lane issues every load it needs -- both planes of get_ref's pair with no branch between them
// (at a full- or half-pel phase the pair is one address and avg( a, a ) = a), then the chroma rows
// -- before its first store, since the outputs may alias the inputs as far as the compiler knows.
// Measured (tools/mc_time.py, DESIGN.md §5 Motion compensation): the kernel's time follows its
// vector-L1 line accesses (a partition's row segments in two planes, three chroma rows for two),
// not its instruction count: an 8-pixel run per lane halved the instructions for 3 %.
//
// GEN = false is the whole-call fast path -- mode == NULL and no weight, the P slice without
// weighted prediction: one get_ref and a store.  GEN = true reads mode[] per partition: the
// list(s), the bipred weight (32: the rounding average; else pixel_avg_weight_wxh with its clip)
// and, for list-0-only partitions, mc->weight (mc_weight after the average, as mc_luma does).
// `pred` is only written.
#include "mcdev.h"
#include "x264hip_mc.h"

namespace x264hip {
namespace {

template <int BD> struct McPlanes            // F, H, V, C of one plane of one reference
{
    const typename PT<BD>::pixel *p0, *p1, *p2, *p3;
};
template <int BD> struct McList
{
    McPlanes<BD> y, u, v;                     // u, v: 4:4:4
    const typename PT<BD>::pixel *nv;         // 4:2:0 / 4:2:2: the interleaved plane
};
// the launch's inputs, by value in the kernel arguments (named members, no arrays: a lane-dependent
// select over an array's elements becomes an indexed load)
template <int BD> struct McParams
{
    McList<BD> l0, l1;
    intptr_t rs, rfs, rcs, rfcs;
    RsWeight wy, wu, wv;
    typename PT<BD>::pixel *pred, *pc0, *pc1;
    intptr_t ps, pfs, pcs, pfcs;
    const int32_t *pos;
    const int16_t *par;
    const int32_t *mode;
    int n;
};

// one plane's 4x4 tile of a partition: MC_LUMA / MC_LUMA_BI (macroblock.c:31-35, 104-110)
template <int BD, bool GEN>
__device__ __forceinline__ void mc_plane( const McPlanes<BD> &q0, const McPlanes<BD> &q1, intptr_t at, intptr_t rs,
                                          int lists, int biw, int mvx0, int mvy0, int mvx1, int mvy1,
                                          const RsWeight &wt, uint32_t ( &r )[4][4 / PT<BD>::PPD] )
{
    // ref_tile's both-planes form: a lane-dependent branch between the planes would put the
    // second plane's latency behind the first's in this streaming kernel
    constexpr int LW = 4 / PT<BD>::PPD;
    if constexpr( !GEN )
        ref_tile<BD, LW, true>( q0.p0, q0.p1, q0.p2, q0.p3, at, rs, mvx0, mvy0, r );
    else
    {
        // the first (or only) list's tile, then list 1's for a bipred partition
        const bool one = lists == 2;
        ref_tile<BD, LW, true>( one ? q1.p0 : q0.p0, one ? q1.p1 : q0.p1, one ? q1.p2 : q0.p2, one ? q1.p3 : q0.p3,
                                at, rs, one ? mvx1 : mvx0, one ? mvy1 : mvy0, r );
        if( lists == 3 )
        {
            uint32_t s[4][LW];
            ref_tile<BD, LW, true>( q1.p0, q1.p1, q1.p2, q1.p3, at, rs, mvx1, mvy1, s );
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int k = 0; k < LW; k++ )
                    r[y][k] = bi_packed<BD>( r[y][k], s[y][k], biw );
        }
        else if( lists == 1 && wt.on )
        {
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int k = 0; k < LW; k++ )
                    r[y][k] = weigh_packed<BD>( r[y][k], wt );
        }
    }
}

template <int BD, int ROWS>
__device__ __forceinline__ void store_tile( typename PT<BD>::pixel *d, intptr_t ds,
                                            const uint32_t ( &r )[ROWS][4 / PT<BD>::PPD] )
{
#pragma unroll
    for( int y = 0; y < ROWS; y++ )
    {
        if constexpr( BD == 8 )
            *(uint32_t *)(d + y * ds) = r[y][0];
        else
            *(uint2 *)(d + y * ds) = make_uint2( r[y][0], r[y][1] );
    }
}

// mc_chroma (mc.c:252-283) of the ROWS x 2 block of (U, V) pairs at s (the interleaved plane at
// the block's first U sample): m[y][x] = the pair as u16 lanes
template <int BD, int ROWS>
__device__ __forceinline__ void chroma_pairs( const typename PT<BD>::pixel *s, intptr_t rcs, int mvx, int mvyc,
                                              rs_us2 ( &m )[ROWS][2] )
{
    constexpr int NDW = BD == 8 ? 2 : 3;    // three (U, V) pairs of a source row
    const ChromaTapsPk t = chroma_taps_pk( mvx, mvyc );
    s += chroma_off( mvx, mvyc, rcs );
    uint32_t w[ROWS + 1][NDW];
#pragma unroll
    for( int y = 0; y <= ROWS; y++ )
    {
        if constexpr( BD == 8 )
            load_al_pad<NDW>( s + y * rcs, w[y] );
        else
        {
            // a 10-bit pair is a dword: the row's three words as they lie
            typedef const __attribute__( ( address_space( 1 ) ) ) uint32_t gword;
            gword *b = (gword *)(uintptr_t)(s + y * rcs);
#pragma unroll
            for( int k = 0; k < NDW; k++ )
                w[y][k] = b[k];
        }
    }
#pragma unroll
    for( int y = 0; y < ROWS; y++ )
#pragma unroll
        for( int x = 0; x < 2; x++ )
            m[y][x] = chroma_pair<BD>( t, w[y], w[y + 1], x );
}

template <int BD, int IPIX, int CF, bool GEN>
__global__ __launch_bounds__( 256 ) void mb_mc_kernel( const McParams<BD> a )
{
    constexpr int LW = 4 / PT<BD>::PPD;
    constexpr int TXN = pix_w( IPIX ) / 4, LPB = TXN * (pix_h( IPIX ) / 4);   // powers of two
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t j = t / LPB;
    if( j >= a.n )
        return;
    const int u = (int)(t & (LPB - 1));
    const int f = a.pos[3 * j];
    const int x = a.pos[3 * j + 1] + 4 * (u % TXN), y = a.pos[3 * j + 2] + 4 * (u / TXN);
    const int16_t *p = a.par + 8 * j;
    int lists = 1, biw = 32;
    if constexpr( GEN )
        if( a.mode )
        {
            const int m = a.mode[j];
            lists = m & 3;
            biw = m >> 8;
        }
    // x264_clip3 to h->mb.mv_min / mv_max (macroblock.c:41-42); an unused list's mv is never used
    const int mnx = p[4], mny = p[5], mxx = p[6], mxy = p[7];
    auto clip3 = []( int v, int lo, int hi ) { return v < lo ? lo : v > hi ? hi : v; };
    const int mvx0 = clip3( p[0], mnx, mxx ), mvy0 = clip3( p[1], mny, mxy );
    const int mvx1 = GEN ? clip3( p[2], mnx, mxx ) : 0, mvy1 = GEN ? clip3( p[3], mny, mxy ) : 0;

    // every plane's loads come before the first store: the outputs may alias the inputs as far as
    // the compiler knows, so a store between them would hold the next plane's loads back
    uint32_t r[4][LW];
    mc_plane<BD, GEN>( a.l0.y, a.l1.y, (intptr_t)f * a.rfs + (intptr_t)y * a.rs + x, a.rs, lists, biw, mvx0, mvy0, mvx1,
                       mvy1, a.wy, r );
    typename PT<BD>::pixel *const py = a.pred + (intptr_t)f * a.pfs + (intptr_t)y * a.ps + x;

    if constexpr( CF == 0 )
        store_tile<BD, 4>( py, a.ps, r );
    else if constexpr( CF == 3 )
    {
        const intptr_t at = (intptr_t)f * a.rfcs + (intptr_t)y * a.rcs + x;
        const intptr_t to = (intptr_t)f * a.pfcs + (intptr_t)y * a.pcs + x;
        uint32_t ru[4][LW], rv[4][LW];
        mc_plane<BD, GEN>( a.l0.u, a.l1.u, at, a.rcs, lists, biw, mvx0, mvy0, mvx1, mvy1, a.wu, ru );
        mc_plane<BD, GEN>( a.l0.v, a.l1.v, at, a.rcs, lists, biw, mvx0, mvy0, mvx1, mvy1, a.wv, rv );
        store_tile<BD, 4>( py, a.ps, r );
        store_tile<BD, 4>( a.pc0 + to, a.pcs, ru );
        store_tile<BD, 4>( a.pc1 + to, a.pcs, rv );
    }
    else if constexpr( CF == 1 || CF == 2 )
    {
        // the tile's chroma: 2 pairs wide, 4 >> v_shift rows, at interleaved column x of chroma
        // row y >> v_shift; mc_chroma( mvx, 2 * mvy >> v_shift ) (macroblock.c:58-64)
        constexpr int VS = CF == 1, ROWS = 4 >> VS;
        const intptr_t crow = y >> VS;
        const intptr_t at = (intptr_t)f * a.rfcs + crow * a.rcs + x;
        rs_us2 m[ROWS][2];
        if constexpr( !GEN )
            chroma_pairs<BD, ROWS>( a.l0.nv + at, a.rcs, mvx0, 2 * mvy0 >> VS, m );
        else
        {
            const bool one = lists == 2;
            chroma_pairs<BD, ROWS>( (one ? a.l1.nv : a.l0.nv) + at, a.rcs, one ? mvx1 : mvx0,
                                    2 * (one ? mvy1 : mvy0) >> VS, m );
            if( lists == 3 )
            {
                rs_us2 m1[ROWS][2];
                chroma_pairs<BD, ROWS>( a.l1.nv + at, a.rcs, mvx1, 2 * mvy1 >> VS, m1 );
#pragma unroll
                for( int cy = 0; cy < ROWS; cy++ )
#pragma unroll
                    for( int cx = 0; cx < 2; cx++ )
                    {
                        if( biw == 32 )
                            m[cy][cx] = (m[cy][cx] + m1[cy][cx] + (rs_us2)1) >> (rs_us2)1;
                        else
                            m[cy][cx] = (rs_us2){ (uint16_t)bi_weighted_px<BD>( m[cy][cx].x, m1[cy][cx].x, biw ),
                                                  (uint16_t)bi_weighted_px<BD>( m[cy][cx].y, m1[cy][cx].y, biw ) };
                    }
            }
            else if( lists == 1 && (a.wu.on | a.wv.on) )
            {
#pragma unroll
                for( int cy = 0; cy < ROWS; cy++ )
#pragma unroll
                    for( int cx = 0; cx < 2; cx++ )
                        m[cy][cx] = weigh_pair<BD>( m[cy][cx], a.wu, a.wv );
            }
        }
        uint32_t c[ROWS][LW];
#pragma unroll
        for( int cy = 0; cy < ROWS; cy++ )
        {
            const uint32_t e0 = __builtin_bit_cast( uint32_t, m[cy][0] ), e1 = __builtin_bit_cast( uint32_t, m[cy][1] );
            if constexpr( BD == 8 )         // U0 V0 U1 V1: the low bytes of the four u16 lanes
                c[cy][0] = __builtin_amdgcn_perm( e1, e0, 0x06040200u );
            else
            {
                c[cy][0] = e0;
                c[cy][LW - 1] = e1;
            }
        }
        store_tile<BD, 4>( py, a.ps, r );
        store_tile<BD, ROWS>( a.pc0 + (intptr_t)f * a.pfcs + crow * a.pcs + x, a.pcs, c );
    }
}

template <int BD> RsWeight mc_weight_of( const x264hip_weight_t &w )
{
    return { w.weighted ? 1 : 0, w.scale, w.weighted ? w.denom : 0, w.weighted && w.denom > 0 ? 1 << (w.denom - 1) : 0,
             w.offset * (1 << (BD - 8)) };
}

template <int BD> McList<BD> mc_list_of( const x264hip_mc_ref_t &r )
{
    using cp = const typename PT<BD>::pixel *;
    return { { (cp)r.luma[0], (cp)r.luma[1], (cp)r.luma[2], (cp)r.luma[3] },
             { (cp)r.chroma[0], (cp)r.chroma[1], (cp)r.chroma[2], (cp)r.chroma[3] },
             { (cp)r.chroma[4], (cp)r.chroma[5], (cp)r.chroma[6], (cp)r.chroma[7] },
             (cp)r.chroma[0] };
}

template <int BD, int IPIX, int CF>
void mc_go( bool gen, dim3 g, hipStream_t stream, const McParams<BD> &a )
{
    if( gen )
        hipLaunchKernelGGL( ( mb_mc_kernel<BD, IPIX, CF, true> ), g, dim3( 256 ), 0, stream, a );
    else
        hipLaunchKernelGGL( ( mb_mc_kernel<BD, IPIX, CF, false> ), g, dim3( 256 ), 0, stream, a );
}

template <int BD, int IPIX>
void mc_go_cf( int cf, bool gen, dim3 g, hipStream_t stream, const McParams<BD> &a )
{
    switch( cf )
    {
        case 0: mc_go<BD, IPIX, 0>( gen, g, stream, a ); break;
        case 1: mc_go<BD, IPIX, 1>( gen, g, stream, a ); break;
        case 2: mc_go<BD, IPIX, 2>( gen, g, stream, a ); break;
        default: mc_go<BD, IPIX, 3>( gen, g, stream, a ); break;
    }
}

} // namespace

// the arguments were checked by the C entry (capi.cpp x264hip_*_mb_mc)
template <int BD>
hipError_t launch_mb_mc( const x264hip_mc_t *mc, int i_pixel, const int32_t *pos, const int16_t *par,
                         const int32_t *mode, int n, hipStream_t stream )
{
    using pixel = typename PT<BD>::pixel;
    if( n <= 0 )
        return hipSuccess;
    if( !mc || i_pixel < 0 || i_pixel > 6 || mc->chroma_format < 0 || mc->chroma_format > 3 )
        return hipErrorInvalidValue;
    McParams<BD> a;
    a.l0 = mc_list_of<BD>( mc->ref[0] );
    a.l1 = mc_list_of<BD>( mc->ref[1] );
    a.rs = mc->ref_stride; a.rfs = mc->ref_frame_stride;
    a.rcs = mc->ref_chroma_stride; a.rfcs = mc->ref_chroma_frame_stride;
    a.wy = mc_weight_of<BD>( mc->weight[0] );
    a.wu = mc_weight_of<BD>( mc->weight[1] );
    a.wv = mc_weight_of<BD>( mc->weight[2] );
    a.pred = (pixel *)mc->pred; a.pc0 = (pixel *)mc->pred_chroma[0]; a.pc1 = (pixel *)mc->pred_chroma[1];
    a.ps = mc->pred_stride; a.pfs = mc->pred_frame_stride;
    a.pcs = mc->pred_chroma_stride; a.pfcs = mc->pred_chroma_frame_stride;
    a.pos = pos; a.par = par; a.mode = mode; a.n = n;
    const int cf = mc->chroma_format;
    // the general kernel only where something asks for it: a mode array, or a weight the format reads
    const bool gen = mode || a.wy.on || ( cf && ( a.wu.on || a.wv.on ) );
    const int64_t lanes = (int64_t)n * (pix_w( i_pixel ) / 4) * (pix_h( i_pixel ) / 4);
    const dim3 g( (unsigned)((lanes + 255) / 256) );
    switch( i_pixel )
    {
        case 0: mc_go_cf<BD, 0>( cf, gen, g, stream, a ); break;
        case 1: mc_go_cf<BD, 1>( cf, gen, g, stream, a ); break;
        case 2: mc_go_cf<BD, 2>( cf, gen, g, stream, a ); break;
        case 3: mc_go_cf<BD, 3>( cf, gen, g, stream, a ); break;
        case 4: mc_go_cf<BD, 4>( cf, gen, g, stream, a ); break;
        case 5: mc_go_cf<BD, 5>( cf, gen, g, stream, a ); break;
        default: mc_go_cf<BD, 6>( cf, gen, g, stream, a ); break;
    }
    return hipGetLastError();
}
X264HIP_INSTANTIATE( launch_mb_mc );

} // namespace x264hip
