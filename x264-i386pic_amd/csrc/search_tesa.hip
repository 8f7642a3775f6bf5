// TESA through x264_me_search_ref for a batch of partitions of any size (reference
// encoder/me.c:618-749, 774-797; x264hip_*_me_search_ref_tesa): the window stage between the
// predictor stage (refine.hip's me_search_ref_kernel, PRED form: fpelcmp = SATD at subme > 1,
// encoder.c:1423-1426) and refine_subpel (refine.hip), chained through stream-ordered scratch.
//
// One wave per partition.  The window is at most 2 * 32 + 1 rows of (max_x - min_x + 3) & ~3 <= 64
// columns (me.c:621-626), so a row is one lane per column and rows stay sequential, as in me.hip's
// 16x16 scan: the bsad a candidate meets is min( the row's starting bsad, the SADs of the ADS
// survivors left of it ) -- a SAD below bsad always passes bsad * sad_thresh >> 3, so
// COPY1_IF_LT (me.c:680) sees every survivor's SAD whether or not it was appended.  Per row: the
// ADS of the lane's column against bsad * 17 >> 4 (pixel.c:759-833: ads4 / ads2 / ads1 by size,
// :840-842, 1605-1608), the block SAD on the surviving lanes only (at me_range <= 16 the window
// is at most 32 columns wide, and the upper 32 lanes take the lower half of each block: the kernel's
// HALF form), an exclusive prefix minimum,
// the SAD threshold, and a ballot + prefix-count append of ( sad + ycost, mv ) to the list in LDS,
// which is sized for the whole window (no input can overrun it).  The two prunes (me.c:705-746)
// keep the reference's order: the halving loop is a stable filter sad <= sad_thresh (its index
// arithmetic copies every entry down and advances on the unsigned ( sad - ( sad_thresh + 1 ) ) >>
// 31), run as a chunked ballot compaction in place; the second loop drops the first maximum and
// moves the last entry into the hole, the maximum found by the wave.  The survivors
// ( <= me_range >> 1 <= 16 ) are then scored with fpelcmp in list order with COST_MV's strict <
// (me.c:747-748): SAD a survivor per lane, SATD a 4x4 block per lane (PIXEL_SATD_C's sums of
// satd_8x4 / satd_4x4, pixel.c:265-332, are the sum over 4x4 blocks of sum |coef| >> 1, each 4x4
// sum being even), summed through LDS.
#include "hipcommon.h"

namespace x264hip {
namespace {

constexpr int ST_INF = 0x7fffffff;

__device__ __forceinline__ int st_pack( int a, int b ) { return (int)((uint32_t)(uint16_t)a | ((uint32_t)(uint16_t)b << 16)); }

// inclusive prefix minimum over the wave's lanes
__device__ __forceinline__ int wave_scan_min( int v, int lane )
{
#pragma unroll
    for( int d = 1; d < 64; d <<= 1 )
    {
        const int o = __shfl_up( v, d );
        if( lane >= d )
            v = min( v, o );
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_max_u64( uint64_t k )
{
#pragma unroll
    for( int d = 32; d >= 1; d >>= 1 )
    {
        const uint32_t hi = (uint32_t)__shfl_xor( (int)(uint32_t)(k >> 32), d );
        const uint32_t lo = (uint32_t)__shfl_xor( (int)(uint32_t)k, d );
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}

// the SAD of the partition's rows y0 .. y0 + NR - 1 at r (NR = its height: pixf.sad[i_pixel]):
// fenc's packed rows in LDS (the lanes read the same word), the reference's rows realigned from
// dword loads
template <int BD, int IPIX, int NR = pix_h( IPIX )>
__device__ __forceinline__ int block_sad( const uint32_t *fl, const typename PT<BD>::pixel *r, intptr_t rs,
                                          int y0 = 0 )
{
    constexpr int LW = pix_w( IPIX ) / PT<BD>::PPD;
    uint32_t acc = 0;
#pragma unroll 4
    for( int y = y0; y < y0 + NR; y++ )
    {
        uint32_t t[LW];
        load_al_pad<LW>( r + y * rs, t );
#pragma unroll
        for( int k = 0; k < LW; k++ )
            acc = sadp<BD>( fl[y * LW + k], t[k], acc );
    }
    return (int)acc;
}

// sum |coef| >> 1 of the 4x4 Hadamard of fenc - ref (satd_4x4, pixel.c:265-288)
template <int BD>
__device__ __forceinline__ int satd4x4( const typename PT<BD>::pixel *f, int fstride, const typename PT<BD>::pixel *r,
                                        intptr_t rs )
{
    int t[4][4];
#pragma unroll
    for( int y = 0; y < 4; y++ )
    {
        int d[4];
#pragma unroll
        for( int x = 0; x < 4; x++ )
            d[x] = (int)f[y * fstride + x] - (int)r[y * rs + x];
        const int a0 = d[0] + d[1], a1 = d[0] - d[1], a2 = d[2] + d[3], a3 = d[2] - d[3];
        t[y][0] = a0 + a2; t[y][2] = a0 - a2; t[y][1] = a1 + a3; t[y][3] = a1 - a3;
    }
    int acc = 0;
#pragma unroll
    for( int x = 0; x < 4; x++ )
    {
        const int a0 = t[0][x] + t[1][x], a1 = t[0][x] - t[1][x], a2 = t[2][x] + t[3][x], a3 = t[2][x] - t[3][x];
        acc += abs( a0 + a2 ) + abs( a0 - a2 ) + abs( a1 + a3 ) + abs( a1 - a3 );
    }
    return acc >> 1;
}

constexpr int ST_HDR = 128 + 16;                          // LDS words before the list: fenc, the SATD sums

// HALF (me_range <= 16: width <= 32): a row's columns take the lower 32 lanes, and lane 32 + c
// scores the lower half of column c's block, so a candidate's SAD is two lanes' work
template <int BD, int IPIX, bool HALF>
__global__ __launch_bounds__( 64 ) void me_search_tesa_window_kernel(
    const typename PT<BD>::pixel *__restrict__ fenc, intptr_t fs, intptr_t ffs,
    const typename PT<BD>::pixel *__restrict__ fw, intptr_t rs, intptr_t rfs, const uint16_t *__restrict__ integral,
    intptr_t ifs, int subme, int me_range, int cap, const int32_t *__restrict__ pos,
    const int16_t *__restrict__ par, const uint16_t *__restrict__ cost_mv, const int32_t *__restrict__ stage,
    int32_t *__restrict__ out, int16_t *__restrict__ rpar, int32_t *__restrict__ rinit,
    int32_t *__restrict__ nevals, int32_t *__restrict__ scan )
{
    using pixel = typename PT<BD>::pixel;
    constexpr int BW = pix_w( IPIX ), BH = pix_h( IPIX ), LW = BW / PT<BD>::PPD;
    constexpr int S = IPIX <= 3 ? 8 : 4;                  // sad_size's edge (me.c:637-638)
    constexpr int NS = ads_nsums( IPIX );
    constexpr bool VERT = IPIX == 0 || IPIX == 2 || IPIX == 5;   // delta *= stride (me.c:648-649)
    constexpr int NB = (BW / 4) * (BH / 4);               // 4x4 blocks of the partition
    extern __shared__ uint32_t st_lds[];
    uint32_t *const fl = st_lds;                          // fenc: BH rows of LW packed words
    uint32_t *const sums = st_lds + 128;                  // SATD of up to 16 survivors
    uint32_t *const l_sad = st_lds + ST_HDR, *const l_mv = l_sad + cap;
    const int lane = (int)threadIdx.x;
    const int64_t j = blockIdx.x;
    const int f = pos[3 * j], bx = pos[3 * j + 1], by = pos[3 * j + 2];
    const int16_t *p = par + 12 * j;
    const int mvpx = p[0], mvpy = p[1];
    const int xmin = p[2], ymin = p[3], xmax = p[4], ymax = p[5];
    const uint16_t *cmx = cost_mv - mvpx, *cmy = cost_mv - mvpy;
    const int4 s0 = *(const int4 *)(stage + 8 * j), s1 = *(const int4 *)(stage + 8 * j + 4);
    int bmx = (int16_t)(s0.x & 0xffff), bmy = (int16_t)((uint32_t)s0.x >> 16);
    int bcost = s0.y;
    const int bpred_cost = s0.z;
    const uint32_t bpred_mv = (uint32_t)s0.w, pmv = (uint32_t)s1.x;
    const bool fsatd = subme > 1;                         // mbcmp_init (encoder.c:1423-1426)

    const pixel *const fe = fenc + f * ffs + (intptr_t)by * fs + bx;
    for( int w = lane; w < BH * LW; w += 64 )
    {
        uint32_t t[1];
        load_row_u<1>( fe + (intptr_t)(w / LW) * fs + (w % LW) * PT<BD>::PPD, t );
        fl[w] = t[0];
    }
    if( lane < 16 )
        sums[lane] = 0;
    __syncthreads();
    const pixel *const fp = (const pixel *)fl;            // fenc as pixels, row stride BW

    // enc_dc (me.c:643-651): the sad_size blocks the partition's ads reads -- ads4 all four of a
    // 16x16, ads2 the horizontal (16x8, 8x4) or vertical (8x16, 4x8: enc_dc[1] = enc_dc[2]) pair
    int dsum = 0;
    if( lane < NS )
    {
        const int ox = NS == 4 ? S * (lane & 1) : VERT ? 0 : S * lane;
        const int oy = NS == 4 ? S * (lane >> 1) : VERT ? S * lane : 0;
        for( int y = 0; y < S; y++ )
            for( int x = 0; x < S; x++ )
                dsum += fp[(oy + y) * BW + ox + x];
    }
    int dc[4];
    intptr_t so[4];
#pragma unroll
    for( int k = 0; k < 4; k++ )
    {
        dc[k] = k < NS ? __shfl( dsum, k ) : 0;
        // ads4: sums[0], [8], [delta], [delta + 8]; ads2: [0], [delta]; delta = S or S * stride
        so[k] = NS == 4 ? (intptr_t)(k & 1) * S + (intptr_t)(k >> 1) * S * rs : VERT ? (intptr_t)k * S * rs : k * S;
    }

    const int min_x = max( bmx - me_range, xmin ), min_y = max( bmy - me_range, ymin );
    const int max_x = min( bmx + me_range, xmax ), max_y = min( bmy + me_range, ymax );
    const int width = (max_x - min_x + 3) & ~3;
    const pixel *const rb = fw + f * rfs + (intptr_t)by * rs + bx;
    const uint16_t *const ib = integral + f * ifs + (intptr_t)by * rs + bx;
    int sad_thresh = me_range <= 16 ? 10 : me_range <= 24 ? 11 : 12;
    int bsad = block_sad<BD, IPIX>( fl, rb + (intptr_t)bmy * rs + bmx, rs ) + (int)cmx[4 * bmx] + (int)cmy[4 * bmy];
    int nmv = 0, nscan = 1;
    const uint64_t lt = lane ? ~0ull >> (64 - lane) : 0ull;   // the lanes below this one
    const int col = HALF ? lane & 31 : lane, hb = HALF ? lane >> 5 : 0;
    const bool active = col < width;
    const int mx = min_x + col;
    const int xcost = active ? (int)cmx[4 * mx] : 0;
    for( int my = min_y; my <= max_y; my++ )
    {
        const int ycost = cmy[4 * my];
        if( bsad <= ycost )
            continue;
        bsad -= ycost;
        bool live = false;
        if( active )
        {
            const uint16_t *s = ib + (intptr_t)my * rs + mx;
            int ads = xcost;
#pragma unroll
            for( int k = 0; k < NS; k++ )
                ads += abs( dc[k] - (int)s[so[k]] );
            live = ads < (bsad * 17 >> 4);
        }
        int sad = ST_INF;
        if constexpr( HALF )
        {
            // (live is the same in both lanes of a column: they read the same sums)
            int part = 0;
            if( live )
                part = block_sad<BD, IPIX, BH / 2>( fl, rb + (intptr_t)my * rs + mx, rs, hb * (BH / 2) );
            part += __shfl_xor( part, 32 );
            live &= hb == 0;
            if( live )
                sad = part + xcost;
        }
        else if( live )
            sad = block_sad<BD, IPIX>( fl, rb + (intptr_t)my * rs + mx, rs ) + xcost;
        const int inc = wave_scan_min( sad, lane );
        const int ex = __shfl_up( inc, 1 );
        const int pb = lane ? min( bsad, ex ) : bsad;     // bsad as this candidate meets it
        const bool keep = live && sad < (pb * sad_thresh >> 3);
        const uint64_t km = __ballot( keep );
        if( keep )
        {
            const int o = nmv + __popcll( km & lt );
            l_sad[o] = (uint32_t)(sad + ycost);
            l_mv[o] = (uint32_t)st_pack( mx, my );
        }
        nmv += __popcll( km );
        nscan += __popcll( __ballot( live ) );
        bsad = min( bsad, __shfl( inc, 63 ) ) + ycost;
    }
    __syncthreads();
    const int nlist = nmv;

    // me.c:705-734
    const int limit = me_range >> 1;
    sad_thresh = bsad * sad_thresh >> 3;
    while( nmv > limit * 2 && sad_thresh > bsad )
    {
        sad_thresh = (sad_thresh + bsad) >> 1;
        int w = 0;
        for( int b = 0; b < nmv; b += 64 )
        {
            const int i = b + lane;
            const bool in = i < nmv;
            const uint32_t s = in ? l_sad[i] : 0u, m = in ? l_mv[i] : 0u;
            const bool keep = in && ((s - (uint32_t)(sad_thresh + 1)) >> 31);
            const uint64_t km = __ballot( keep );
            __syncthreads();                              // the chunk is read before its slots are written
            if( keep )
            {
                const int o = w + __popcll( km & lt );
                l_sad[o] = s;
                l_mv[o] = m;
            }
            w += __popcll( km );
        }
        __syncthreads();
        nmv = w;
    }
    // me.c:735-746
    while( nmv > limit )
    {
        uint64_t key = 0;                                 // ( sad, ~index ): the first maximum
        for( int i = lane; i < nmv; i += 64 )
        {
            const uint64_t k = ((uint64_t)l_sad[i] << 32) | (uint32_t)~i;
            key = k > key ? k : key;
        }
        key = wave_max_u64( key );
        const int bi = (int)~(uint32_t)key;
        nmv--;
        __syncthreads();
        if( lane == 0 )
        {
            l_sad[bi] = l_sad[nmv];
            l_mv[bi] = l_mv[nmv];
        }
        __syncthreads();
    }

    // COST_MV over the survivors in list order (me.c:747-748)
    int cst_l = 0;
    if( !fsatd )
    {
        if( lane < nmv )
        {
            const uint32_t m = l_mv[lane];
            const int sx = (int16_t)(m & 0xffff), sy = (int16_t)(m >> 16);
            cst_l = block_sad<BD, IPIX>( fl, rb + (intptr_t)sy * rs + sx, rs );
        }
    }
    else
    {
        constexpr int PER = 64 / NB;                      // survivors per round
        for( int b = 0; b < nmv; b += PER )
        {
            const int i = b + lane / NB, blk = lane % NB;
            if( i < nmv )
            {
                const uint32_t m = l_mv[i];
                const int sx = (int16_t)(m & 0xffff), sy = (int16_t)(m >> 16);
                const int ox = 4 * (blk % (BW / 4)), oy = 4 * (blk / (BW / 4));
                const int c = satd4x4<BD>( fp + oy * BW + ox, BW, rb + (intptr_t)(sy + oy) * rs + sx + ox, rs );
                atomicAdd( &sums[i], (uint32_t)c );
            }
        }
        __syncthreads();
        if( lane < nmv )
            cst_l = (int)sums[lane];
    }
    for( int i = 0; i < nmv; i++ )
    {
        const uint32_t m = l_mv[i];
        const int sx = (int16_t)(m & 0xffff), sy = (int16_t)(m >> 16);
        const int c = __shfl( cst_l, i ) + (int)cmx[4 * sx] + (int)cmy[4 * sy];
        if( c < bcost )
        {
            bcost = c;
            bmx = sx;
            bmy = sy;
        }
    }

    // -> qpel mv (me.c:774-789)
    int qx, qy, cst, cmv;
    if( subme < 3 )
    {
        cmv = (int)cmx[4 * bmx] + (int)cmy[4 * bmy];
        cst = bcost + ((uint32_t)st_pack( bmx, bmy ) == pmv ? cmv : 0);
        qx = 4 * bmx;
        qy = 4 * bmy;
    }
    else
    {
        if( bpred_cost < bcost )
        {
            qx = (int16_t)(bpred_mv & 0xffff);
            qy = (int16_t)(bpred_mv >> 16);
        }
        else
        {
            qx = 4 * bmx;
            qy = 4 * bmy;
        }
        cst = min( bpred_cost, bcost );
        cmv = (int)cmx[qx] + (int)cmy[qy];
    }
    if( lane == 0 )
    {
        if( !rpar )                                       // (with the refine, out is the refine's)
            *(int4 *)(out + 4 * j) = make_int4( cst, qx, qy, cmv );
        else
        {
            *(int4 *)(rpar + 8 * j) = make_int4( st_pack( qx, qy ), st_pack( mvpx, mvpy ), st_pack( p[6], p[7] ),
                                                 st_pack( p[8], p[9] ) );
            rinit[j] = cst;
        }
        if( nevals )
        {
            nevals[2 * j] = s1.y + nmv;                   // (the get_ref calls stay in the upper half)
            if( subme < 2 )
                nevals[2 * j + 1] = 0;                    // no refine_subpel (me.c:792)
        }
        if( scan )
        {
            scan[2 * j] = nscan;
            scan[2 * j + 1] = nlist;
        }
    }
}

} // namespace

template <int BD>
hipError_t launch_me_search_ref_tesa( const typename PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                      const typename PT<BD>::pixel *fw, const typename PT<BD>::pixel *const planes[4],
                                      intptr_t rs, intptr_t rfs, const uint16_t *integral8, const uint16_t *integral4,
                                      intptr_t ifs, int i_pixel, int subme, int me_range, const int32_t *pos,
                                      const int16_t *par, const int16_t *mvc, const uint16_t *cost_mv, int n,
                                      int32_t *out, int32_t *nevals, int32_t *scan, int32_t *thr,
                                      const int32_t *rcost, const x264hip_refine_ext_t *xe, hipStream_t stream )
{
    if( i_pixel < 0 || i_pixel > 6 || subme < 1 || subme > 11 || me_range < 4 || me_range > 32 ||
        ((uintptr_t)out & 15) || !integral8 || (i_pixel > 3 && !integral4) )
        return hipErrorInvalidValue;
    if( n <= 0 )
        return hipSuccess;
    const uint16_t *integral = i_pixel <= 3 ? integral8 : integral4;   // me.c:635-647
    const bool refine = subme >= 2;
    // stage [n][8] int32, then the refine's par [n][8] int16 and init cost [n]
    void *buf = nullptr;
    hipError_t e = scratch_alloc( &buf, (size_t)n * (32 + 16 + 4) + 16, stream );
    if( e != hipSuccess )
        return e;
    int32_t *stage = (int32_t *)buf;
    int16_t *rpar = refine ? (int16_t *)((char *)buf + (size_t)n * 32) : nullptr;
    int32_t *rinit = refine ? (int32_t *)((char *)buf + (size_t)n * 48) : nullptr;
    e = launch_me_search_pred<BD>( fenc, fs, ffs, fw, planes, rs, rfs, i_pixel, subme, pos, par, mvc, cost_mv, n, stage,
                                   xe, stream );
    if( e == hipSuccess )
    {
        // the list holds the whole window: (2 * me_range + 1) rows of up to (2 * me_range + 3) & ~3
        const int cap = (2 * me_range + 1) * ((2 * me_range + 3) & ~3);
        const size_t lds = (size_t)(ST_HDR + 2 * cap) * sizeof( uint32_t );
#define ST_CASE( I )                                                                                              \
    case I:                                                                                                       \
        if( me_range <= 16 )                                                                                      \
            hipLaunchKernelGGL( ( me_search_tesa_window_kernel<BD, I, true> ), dim3( (unsigned)n ), dim3( 64 ), lds,  \
                                stream, fenc, fs, ffs, fw, rs, rfs, integral, ifs, subme, me_range, cap, pos, par,    \
                                cost_mv, stage, out, rpar, rinit, nevals, scan );                                     \
        else                                                                                                      \
            hipLaunchKernelGGL( ( me_search_tesa_window_kernel<BD, I, false> ), dim3( (unsigned)n ), dim3( 64 ), lds, \
                                stream, fenc, fs, ffs, fw, rs, rfs, integral, ifs, subme, me_range, cap, pos, par,    \
                                cost_mv, stage, out, rpar, rinit, nevals, scan );                                     \
        break;
        switch( i_pixel )
        {
            ST_CASE( 0 ) ST_CASE( 1 ) ST_CASE( 2 ) ST_CASE( 3 ) ST_CASE( 4 ) ST_CASE( 5 ) ST_CASE( 6 )
            default: break;
        }
#undef ST_CASE
        e = hipGetLastError();
    }
    if( e == hipSuccess && refine )
        e = launch_me_search_refine<BD>( fenc, fs, ffs, planes, rs, rfs, i_pixel, subme, 1, pos, rpar, rinit, cost_mv, n,
                                         out, nevals ? nevals + 1 : nullptr, thr, rcost, xe, stream );
    const hipError_t ef = hipFreeAsync( buf, stream );
    return e == hipSuccess ? ef : e;
}
X264HIP_INSTANTIATE( launch_me_search_ref_tesa );

} // namespace x264hip
