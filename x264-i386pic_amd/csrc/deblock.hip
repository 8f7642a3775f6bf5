// The in-loop deblocking filter: x264_frame_deblock_row (reference common/deblock.c:378-606) over
// whole frames in place, and deblock_strength_c (deblock.c:277-304) from the arrays the device
// already holds (include/x264hip_deblock.h).
//
// Order.  x264 filters the macroblocks in raster order and, within one, vertical edges 0..3 and
// then horizontal edges 0..3; that order is observable.  MB (x,y) reads pixels that (x-1,y),
// (x,y-1) and -- through that MB's left edge, which rewrites columns 13..15 of (x,y-1) --
// (x+1,y-1) have finished, and nothing else, so the MBs of one anti-diagonal d = x + 2y are
// independent: their footprints (columns 16x-4 .. 16x+15, rows 16y-4 .. 16y+15) are disjoint.
// One launch per anti-diagonal, d = 0 .. mbw + 2(mbh-1), each over that diagonal's MBs of every
// frame; the stream orders the launches.  No kernel waits for another workgroup.
//
// One wave per MB.  The 20x20 luma tile (4 columns to the left, 4 rows above) and the chroma tiles
// (U and V de-interleaved) are read once into LDS -- every load issued before the first wait -- with
// the MB's strengths and the table entries of its six qp values, so no edge waits for memory; lanes
// 0..15 take the luma rows, 16..31 U's and
// 32..47 V's and run the four vertical edges of their row in order; after a barrier the same lanes
// take columns and run the four horizontal edges; after another every pixel an edge of this MB can
// change is stored once (rows 0..15 with the 3 columns -- chroma: 1 -- left of the MB when its
// left edge is filtered, and the 3 rows -- chroma: 1 -- above it when its top edge is; never the
// corner toward (x-1,y-1)).
#include "hipcommon.h"
#include "x264hip_deblock.h"

#include <string.h>
#include <algorithm>

namespace x264hip {
namespace {

// deblock.c:32-76, indexed by qp + offset + 24
__constant__ uint8_t c_alpha_table[88] = {
      0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
      0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   4,   4,   5,   6,
      7,   8,   9,  10,  12,  13,  15,  17,  20,  22,  25,  28,  32,  36,  40,  45,  50,  56,  63,  71,  80,  90,
    101, 113, 127, 144, 162, 182, 203, 226, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
};
__constant__ uint8_t c_beta_table[88] = {
      0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
      0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   2,   2,   2,   3,
      3,   3,   3,   4,   4,   4,   6,   6,   7,   7,   8,   8,   9,   9,  10,  10,  11,  11,  12,  12,  13,  13,
     14,  14,  15,  15,  16,  16,  17,  17,  18,  18,  18,  18,  18,  18,  18,  18,  18,  18,  18,  18,  18,  18,
};
__constant__ __attribute__(( aligned( 4 ) )) int8_t c_tc0_table[88][4] = {   // (a row is read as one word)
    {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0},
    {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0},
    {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0},
    {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0},
    {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0}, {-1,0,0,0},
    {-1,0,0,0}, {-1,0,0,1}, {-1,0,0,1}, {-1,0,0,1}, {-1,0,0,1}, {-1,0,1,1}, {-1,0,1,1}, {-1,1,1,1},
    {-1,1,1,1}, {-1,1,1,1}, {-1,1,1,1}, {-1,1,1,2}, {-1,1,1,2}, {-1,1,1,2}, {-1,1,1,2}, {-1,1,2,3},
    {-1,1,2,3}, {-1,2,2,3}, {-1,2,2,4}, {-1,2,3,4}, {-1,2,3,4}, {-1,3,3,5}, {-1,3,4,6}, {-1,3,4,6},
    {-1,4,5,7}, {-1,4,5,8}, {-1,4,6,9}, {-1,5,7,10}, {-1,6,8,11}, {-1,6,8,13}, {-1,7,10,14}, {-1,8,11,16},
    {-1,9,12,18}, {-1,10,13,20}, {-1,11,15,23}, {-1,13,17,25}, {-1,13,17,25}, {-1,13,17,25}, {-1,13,17,25}, {-1,13,17,25},
    {-1,13,17,25}, {-1,13,17,25}, {-1,13,17,25}, {-1,13,17,25}, {-1,13,17,25}, {-1,13,17,25}, {-1,13,17,25}, {-1,13,17,25},
};

constexpr int TP = 20;                        // tile pitch: 4 pixels before the MB, 16 in it
using tpix = uint16_t;

// the launch's inputs, by value in the kernel arguments
template <int BD> struct DbParams
{
    typename PT<BD>::pixel *y, *c0, *c1;
    intptr_t ys, yfs, cs, cfs;
    const int8_t *qp;
    const uint8_t *flags, *bs;
    const int32_t *slice;
    int mbw, mbh, a, b, qp_thresh;
    int d, ymin, count;                       // this launch: the MBs (d - 2y, y), y = ymin .. ymin + count - 1
    uint32_t cqp[16];                         // chroma_qp_table[0..63], four entries a word
};

__device__ __forceinline__ int clip3( int v, int lo, int hi ) { return v < lo ? lo : v > hi ? hi : v; }

// deblock_edge_luma_c, deblock.c:79-109: pix at q0, xs between the samples across the edge
template <int BD>
__device__ __forceinline__ void edge_luma( tpix *pix, int xs, int alpha, int beta, int tc0 )
{
    const int p2 = pix[-3 * xs], p1 = pix[-2 * xs], p0 = pix[-1 * xs];
    const int q0 = pix[0], q1 = pix[xs], q2 = pix[2 * xs];
    if( abs( p0 - q0 ) < alpha && abs( p1 - p0 ) < beta && abs( q1 - q0 ) < beta )
    {
        int tc = tc0;
        if( abs( p2 - p0 ) < beta )
        {
            if( tc0 )
                pix[-2 * xs] = (tpix)( p1 + clip3( (( p2 + ((p0 + q0 + 1) >> 1)) >> 1) - p1, -tc0, tc0 ) );
            tc++;
        }
        if( abs( q2 - q0 ) < beta )
        {
            if( tc0 )
                pix[xs] = (tpix)( q1 + clip3( (( q2 + ((p0 + q0 + 1) >> 1)) >> 1) - q1, -tc0, tc0 ) );
            tc++;
        }
        const int delta = clip3( (((q0 - p0) * 4) + (p1 - q1) + 4) >> 3, -tc, tc );
        pix[-1 * xs] = (tpix)clip_pix<BD>( p0 + delta );
        pix[0] = (tpix)clip_pix<BD>( q0 - delta );
    }
}

// deblock_edge_chroma_c, deblock.c:137-150
template <int BD>
__device__ __forceinline__ void edge_chroma( tpix *pix, int xs, int alpha, int beta, int tc )
{
    const int p1 = pix[-2 * xs], p0 = pix[-1 * xs], q0 = pix[0], q1 = pix[xs];
    if( abs( p0 - q0 ) < alpha && abs( p1 - p0 ) < beta && abs( q1 - q0 ) < beta )
    {
        const int delta = clip3( (((q0 - p0) * 4) + (p1 - q1) + 4) >> 3, -tc, tc );
        pix[-1 * xs] = (tpix)clip_pix<BD>( p0 + delta );
        pix[0] = (tpix)clip_pix<BD>( q0 - delta );
    }
}

// deblock_edge_luma_intra_c, deblock.c:183-221
__device__ __forceinline__ void edge_luma_intra( tpix *pix, int xs, int alpha, int beta )
{
    const int p2 = pix[-3 * xs], p1 = pix[-2 * xs], p0 = pix[-1 * xs];
    const int q0 = pix[0], q1 = pix[xs], q2 = pix[2 * xs];
    if( abs( p0 - q0 ) < alpha && abs( p1 - p0 ) < beta && abs( q1 - q0 ) < beta )
    {
        if( abs( p0 - q0 ) < ((alpha >> 2) + 2) )
        {
            if( abs( p2 - p0 ) < beta )
            {
                const int p3 = pix[-4 * xs];
                pix[-1 * xs] = (tpix)( ( p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4 ) >> 3 );
                pix[-2 * xs] = (tpix)( ( p2 + p1 + p0 + q0 + 2 ) >> 2 );
                pix[-3 * xs] = (tpix)( ( 2 * p3 + 3 * p2 + p1 + p0 + q0 + 4 ) >> 3 );
            }
            else
                pix[-1 * xs] = (tpix)( ( 2 * p1 + p0 + q1 + 2 ) >> 2 );
            if( abs( q2 - q0 ) < beta )
            {
                const int q3 = pix[3 * xs];
                pix[0] = (tpix)( ( p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4 ) >> 3 );
                pix[xs] = (tpix)( ( p0 + q0 + q1 + q2 + 2 ) >> 2 );
                pix[2 * xs] = (tpix)( ( 2 * q3 + 3 * q2 + q1 + q0 + p0 + 4 ) >> 3 );
            }
            else
                pix[0] = (tpix)( ( 2 * q1 + q0 + p1 + 2 ) >> 2 );
        }
        else
        {
            pix[-1 * xs] = (tpix)( ( 2 * p1 + p0 + q1 + 2 ) >> 2 );
            pix[0] = (tpix)( ( 2 * q1 + q0 + p1 + 2 ) >> 2 );
        }
    }
}

// deblock_edge_chroma_intra_c, deblock.c:241-253
__device__ __forceinline__ void edge_chroma_intra( tpix *pix, int xs, int alpha, int beta )
{
    const int p1 = pix[-2 * xs], p0 = pix[-1 * xs], q0 = pix[0], q1 = pix[xs];
    if( abs( p0 - q0 ) < alpha && abs( p1 - p0 ) < beta && abs( q1 - q0 ) < beta )
    {
        pix[-1 * xs] = (tpix)( ( 2 * p1 + p0 + q1 + 2 ) >> 2 );
        pix[0] = (tpix)( ( 2 * q1 + q0 + p1 + 2 ) >> 2 );
    }
}

// Rows -R0 .. H-1, columns -R0 .. W-1 of a plane's MB on their way into its tile: fetch() issues
// every load of the lane with no branch between them, put() stores them to LDS.  Nothing outside
// the picture is read: where the MB has no (filtered) left or top neighbour the lane reads column
// or row 0 of the MB instead, and the tile entry it fills is never used.
template <typename pixel, int W, int H, int R0> struct TileRegs
{
    static constexpr int TW = W + R0, N = (H + R0) * TW, K = (N + 63) / 64;
    pixel v[K];
    __device__ __forceinline__ void fetch( const pixel *base, intptr_t stride, int step, bool left, bool top, int tid )
    {
#pragma unroll
        for( int k = 0; k < K; k++ )
        {
            const int i = min( tid + 64 * k, N - 1 );
            const int r = i / TW - R0, c = i % TW - R0;
            v[k] = base[( r < 0 && !top ? 0 : r ) * stride + ( c < 0 && !left ? 0 : c ) * step];
        }
    }
    __device__ __forceinline__ void put( tpix ( *t )[TP], int tid ) const
    {
#pragma unroll
        for( int k = 0; k < K; k++ )
        {
            const int i = tid + 64 * k;
            if( i < N )
                t[i / TW - R0 + 4][i % TW - R0 + 4] = v[k];
        }
    }
};

// CF: the chroma format.  Planes 1 and 2 of the tile are U and V: luma-type (16x16, the luma
// filters) at 4:4:4, chroma-type (8 wide, 8 or 16 high) at 4:2:0 / 4:2:2.
template <int BD, int CF>
__global__ __launch_bounds__( 64 ) void deblock_diag_kernel( const DbParams<BD> a )
{
    using pixel = typename PT<BD>::pixel;
    constexpr int NPL = CF ? 3 : 1;
    constexpr bool C444 = CF == 3;
    constexpr int CW = C444 ? 16 : 8, CH = CF == 1 ? 8 : 16;      // a macroblock of a chroma plane
    constexpr int CR = C444 ? 4 : 2, CS = C444 ? 3 : 1;           // pixels before the MB read / stored
    __shared__ tpix tile[NPL][TP][TP];                            // [plane][4 + row][4 + column]
    __shared__ uint32_t s_bs[8];                                  // bs[dir][edge] of this MB, a word each
    __shared__ int s_abt[6][3];                                   // alpha, beta, the tc0 row: [qp kind] below

    const int tid = threadIdx.x;
    const int f = blockIdx.x / a.count;
    const int my = a.ymin + blockIdx.x % a.count, mx = a.d - 2 * my;
    const int64_t xy = ( (int64_t)f * a.mbh + my ) * a.mbw + mx;

    // macroblock_cache_load_neighbours_deblock, deblock.c:370-375
    bool left = mx > 0, top = my > 0;
    const int64_t xyl = left ? xy - 1 : xy, xyt = top ? xy - a.mbw : xy;     // (in range at the picture's border too)
    if( a.slice )
    {
        const int s = a.slice[xy], sl = a.slice[xyl], st = a.slice[xyt];
        left = left && sl == s;
        top = top && st == s;
    }
    // every load of the kernel is issued before the first wait: the per-MB values of this MB and its
    // neighbours (of this MB itself where there is none: not used then), then the tiles
    const int fl = a.flags[xy], fll = a.flags[xyl], flt = a.flags[xyt];
    const int qp = a.qp[xy], qpl = a.qp[xyl], qpt = a.qp[xyt];
    const uint32_t bsw = ( (const uint32_t *)( a.bs + xy * 32 ) )[tid & 7];

    pixel *const py = a.y + f * a.yfs + (intptr_t)16 * my * a.ys + 16 * mx;
    pixel *pc[2] = { nullptr, nullptr };
    if constexpr( CF != 0 )
    {
        pixel *const c = a.c0 + f * a.cfs + (intptr_t)CH * my * a.cs + 16 * mx;
        pc[0] = c;
        pc[1] = C444 ? a.c1 + f * a.cfs + (intptr_t)CH * my * a.cs + 16 * mx : c + 1;
    }
    constexpr int cstep = ( CF == 1 || CF == 2 ) ? 2 : 1;
    TileRegs<pixel, 16, 16, 4> ry;
    TileRegs<pixel, CW, CH, CR> ru, rv;
    ry.fetch( py, a.ys, 1, left, top, tid );
    if constexpr( CF != 0 )
    {
        ru.fetch( pc[0], a.cs, cstep, left, top, tid );
        rv.fetch( pc[1], a.cs, cstep, left, top, tid );
    }

    const bool intra = fl & 1, t8 = fl & 2;
    const bool intra_l = ( fl | fll ) & 1, intra_t = ( fl | flt ) & 1;
    auto cq = [&]( int q ) { q = clip3( q, 0, 63 ); return (int)( a.cqp[q >> 2] >> (8 * (q & 3)) & 255 ); };
    const int qpc = cq( qp );
    const bool first_edge_only = ( (fl & 4) && !intra ) || qp <= a.qp_thresh;         // deblock.c:415
    // what the edges read besides pixels goes to LDS too: the MB's 32 strengths (lanes 0..7) and the
    // table entries of its six qp kinds (lanes 8..13: this MB's luma and chroma qp, the averages with
    // the left MB's, those with the top MB's, deblock.c:309-312), so no edge waits for memory
    if( tid < 8 )
        s_bs[tid] = bsw;
    else if( tid < 14 )
    {
        const int k = tid - 8, qn = k < 4 ? qpl : qpt;
        const int q = k < 2 ? ( k ? qpc : qp ) : ( k & 1 ) ? ( qpc + cq( qn ) + 1 ) >> 1 : ( qp + qn + 1 ) >> 1;
        const int ia = clip3( q + a.a + 24, 0, 87 ), ib = clip3( q + a.b + 24, 0, 87 );
        s_abt[k][0] = c_alpha_table[ia] << (BD - 8);
        s_abt[k][1] = c_beta_table[ib] << (BD - 8);
        s_abt[k][2] = *(const int *)c_tc0_table[ia];
    }
    ry.put( tile[0], tid );
    if constexpr( CF != 0 )
    {
        ru.put( tile[1], tid );
        rv.put( tile[2], tid );
    }
    __syncthreads();

    const int pl = tid >> 4, l = tid & 15;                 // plane and line (row, then column) of the lane
    const bool luma_type = pl == 0 || C444;
#pragma unroll
    for( int dir = 0; dir < 2; dir++ )
    {
        if( dir )
            __syncthreads();
        const int lines = pl == 0 ? 16 : dir ? CW : CH;
        if( pl < NPL && l < lines )
        {
            const bool mb_edge = dir ? top : left;
            const bool intra_0 = dir ? intra_t : intra_l;
            for( int edge = 0; edge < 4; edge++ )
            {
                if( edge ? first_edge_only : !mb_edge )
                    continue;
                // the FILTER macro, deblock.c:417-447: which edges of which plane, and where
                int at;
                if( luma_type )
                {
                    if( ( edge & 1 ) && t8 )
                        continue;
                    at = 4 * edge;
                }
                else if( CF == 1 || !dir )
                {
                    if( edge & 1 )
                        continue;
                    at = 2 * edge;
                }
                else
                    at = 4 * edge;                           // 4:2:2, horizontal edges: all four
                const int k = ( edge ? 0 : dir ? 4 : 2 ) + ( pl != 0 );
                const int alpha = s_abt[k][0], beta = s_abt[k][1];
                if( !alpha || !beta )
                    continue;
                tpix *const pix = dir ? &tile[pl][4 + at][4 + l] : &tile[pl][4 + l][4 + at];
                const int xs = dir ? TP : 1;
                if( !edge && intra_0 )
                {
                    if( luma_type )
                        edge_luma_intra( pix, xs, alpha, beta );
                    else
                        edge_chroma_intra( pix, xs, alpha, beta );
                    continue;
                }
                const uint32_t bs4 = s_bs[dir * 4 + edge];
                if( !bs4 )
                    continue;
                // the bS of this line: 4 lines each for the luma filters and deblock_h_chroma_422,
                // 2 for the other chroma filters (deblock.c:110-122, 151-181)
                const int seg = ( luma_type || ( CF == 2 && !dir ) ) ? l >> 2 : l >> 1;
                const int s = bs4 >> (8 * seg) & 3;
                const int tc = (int8_t)( s_abt[k][2] >> (8 * s) ) * (1 << (BD - 8)) + ( luma_type ? 0 : 1 );
                if( luma_type )
                {
                    if( tc >= 0 )
                        edge_luma<BD>( pix, xs, alpha, beta, tc );
                }
                else if( tc > 0 )
                    edge_chroma<BD>( pix, xs, alpha, beta, tc );
            }
        }
    }
    __syncthreads();

    // what an edge of this MB can have changed: rows 0 .. h-1 from column -s0 (where the left edge
    // is filtered) and rows -s0 .. -1 of the MB's own columns (where the top edge is)
    auto store = [&]( int p, pixel *base, intptr_t stride, int step, int w, int h, int s0 )
    {
        const int tw = w + s0;
        for( int i = tid; i < (h + s0) * tw; i += 64 )
        {
            const int r = i / tw - s0, c = i % tw - s0;
            if( r >= 0 ? ( c >= 0 || left ) : ( c >= 0 && top ) )
                base[r * stride + c * step] = (pixel)tile[p][r + 4][c + 4];
        }
    };
    store( 0, py, a.ys, 1, 16, 16, 3 );
    if constexpr( CF != 0 )
    {
        store( 1, pc[0], a.cs, cstep, CW, CH, CS );
        store( 2, pc[1], a.cs, cstep, CW, CH, CS );
    }
}

struct BsParams
{
    const int32_t *nz;
    const uint8_t *flags;
    const int16_t *mv0, *mv1;
    const int8_t *ref0, *ref1;
    uint8_t *bs;
    int mbw, mbh, bframe, mvy_limit;
    int64_t n;                                // n_frames * mbw * mbh * 8 edges
};

// a thread per (MB, dir, edge): the four segments of the edge, stored as one word
__global__ __launch_bounds__( 256 ) void deblock_strength_kernel( const BsParams a )
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if( t >= a.n )
        return;
    const int edge = t & 3, dir = t >> 2 & 1;
    const int64_t xy = t >> 3;
    const int mbs = a.mbw * a.mbh;
    const int64_t f = xy / mbs;
    const int my = (int)( xy % mbs ) / a.mbw, mx = (int)( xy % mbs ) % a.mbw;
    const int fl = a.flags[xy];
    uint32_t out = 0;
    if( edge )
    {
        if( fl & 1 )
            out = 0x03030303u;                // macroblock.c:1441-1447
    }
    else if( ( dir ? my : mx ) == 0 )
        out = 0;                              // the picture border: never filtered
    else if( ( fl | a.flags[xy - ( dir ? a.mbw : 1 )] ) & 1 )
        out = 0x04040404u;
    if( ( edge || ( dir ? my : mx ) > 0 ) && !out )
    {
        const int64_t xyn = edge ? xy : xy - ( dir ? a.mbw : 1 );
        const int fln = a.flags[xyn];
        const int nzq = a.nz[xy], nzp = a.nz[xyn];
        // (the block's bit: transform 4: 4*i8+i4; transform 8: i8)
        auto bit = [&]( int m, int t8, int bx, int by )
        {
            const int i8 = (by >> 1) * 2 + (bx >> 1);
            return m >> ( t8 ? i8 : 4 * i8 + (by & 1) * 2 + (bx & 1) ) & 1;
        };
        const intptr_t s4 = 4 * a.mbw, s8 = 2 * a.mbw;
#pragma unroll
        for( int i = 0; i < 4; i++ )
        {
            // deblock.c:283-301: q = the block of this MB, p = the one before it across the edge
            const int bx = dir ? i : edge, by = dir ? edge : i;
            const int px = edge ? ( dir ? bx : bx - 1 ) : ( dir ? bx : 3 );
            const int py = edge ? ( dir ? by - 1 : by ) : ( dir ? 3 : by );
            int v;
            if( bit( nzq, fl & 2, bx, by ) || bit( nzp, fln & 2, px, py ) )
                v = 2;
            else
            {
                // the blocks' places in the frame's 4x4 and 8x8 grids
                const int gx = 4 * mx + bx, gy = 4 * my + by;
                const int hx = gx - ( dir ? 0 : 1 ), hy = gy - ( dir ? 1 : 0 );
                const int64_t q4 = ( f * 4 * a.mbh + gy ) * s4 + gx, p4 = ( f * 4 * a.mbh + hy ) * s4 + hx;
                const int64_t q8 = ( f * 2 * a.mbh + (gy >> 1) ) * s8 + (gx >> 1);
                const int64_t p8 = ( f * 2 * a.mbh + (hy >> 1) ) * s8 + (hx >> 1);
                v = a.ref0[q8] != a.ref0[p8] || abs( a.mv0[2 * q4] - a.mv0[2 * p4] ) >= 4 ||
                    abs( a.mv0[2 * q4 + 1] - a.mv0[2 * p4 + 1] ) >= a.mvy_limit;
                if( a.bframe && !v )
                    v = a.ref1[q8] != a.ref1[p8] || abs( a.mv1[2 * q4] - a.mv1[2 * p4] ) >= 4 ||
                        abs( a.mv1[2 * q4 + 1] - a.mv1[2 * p4 + 1] ) >= a.mvy_limit;
            }
            out |= (uint32_t)v << (8 * i);
        }
    }
    *(uint32_t *)( a.bs + xy * 32 + (dir * 4 + edge) * 4 ) = out;
}

template <int BD, int CF>
void deblock_go( const DbParams<BD> &a, unsigned blocks, hipStream_t stream )
{
    hipLaunchKernelGGL( ( deblock_diag_kernel<BD, CF> ), dim3( blocks ), dim3( 64 ), 0, stream, a );
}

} // namespace

// the arguments were checked by the C entry (capi.cpp x264hip_*_deblock_frames)
template <int BD>
hipError_t launch_deblock_frames( const x264hip_deblock_t *d, int mbw, int mbh, int n_frames, hipStream_t stream )
{
    using pixel = typename PT<BD>::pixel;
    if( !d || mbw <= 0 || mbh <= 0 || n_frames <= 0 )
        return hipSuccess;
    constexpr int QP_BD_OFFSET = 6 * (BD - 8);
    DbParams<BD> a;
    a.y = (pixel *)d->luma; a.c0 = (pixel *)d->chroma[0]; a.c1 = (pixel *)d->chroma[1];
    a.ys = d->luma_stride; a.yfs = d->luma_frame_stride;
    a.cs = d->chroma_stride; a.cfs = d->chroma_frame_stride;
    a.qp = d->qp; a.flags = d->mb_flags; a.bs = d->bs; a.slice = d->slice_table;
    a.mbw = mbw; a.mbh = mbh;
    a.a = d->alpha_c0_offset - QP_BD_OFFSET;
    a.b = d->beta_offset - QP_BD_OFFSET;
    a.qp_thresh = 15 - std::min( a.a, a.b ) - std::max( 0, d->chroma_qp_index_offset );      // deblock.c:383
    pack_cqp<BD>( d->chroma_qp_table, a.cqp );
    const int cf = d->chroma_format;
    for_each_diagonal( mbw, mbh, [&]( int dg, int ymin, int count )
    {
        a.d = dg; a.ymin = ymin; a.count = count;
        const unsigned blocks = (unsigned)count * (unsigned)n_frames;
        switch( cf )
        {
            case 0: deblock_go<BD, 0>( a, blocks, stream ); break;
            case 1: deblock_go<BD, 1>( a, blocks, stream ); break;
            case 2: deblock_go<BD, 2>( a, blocks, stream ); break;
            default: deblock_go<BD, 3>( a, blocks, stream ); break;
        }
    } );
    return hipGetLastError();
}
X264HIP_INSTANTIATE( launch_deblock_frames );

hipError_t launch_deblock_strength( const x264hip_deblock_strength_t *s, int mbw, int mbh, int n_frames, uint8_t *bs,
                                    hipStream_t stream )
{
    BsParams a;
    a.nz = s->nz; a.flags = s->mb_flags;
    a.mv0 = s->mv[0]; a.mv1 = s->mv[1]; a.ref0 = s->ref[0]; a.ref1 = s->ref[1];
    a.bs = bs; a.mbw = mbw; a.mbh = mbh; a.bframe = s->bframe != 0; a.mvy_limit = s->mvy_limit;
    a.n = (int64_t)n_frames * mbw * mbh * 8;
    if( a.n <= 0 )
        return hipSuccess;
    hipLaunchKernelGGL( deblock_strength_kernel, dim3( (unsigned)( (a.n + 255) / 256 ) ), dim3( 256 ), 0, stream, a );
    return hipGetLastError();
}

} // namespace x264hip
