// Device helpers of the intra mode decision (mbanalyse.hip): the reference's mode tables as packed
// immediates, the 4x4 / 8x8 Hadamard metrics of one lane, and x264_mb_analyse_intra's I_4x4 and
// I_8x8 passes (reference encoder/analyse.c:746-979) over the tile of mbintradev.h.  The trial
// reconstruction of a block lives only in the tile.
#pragma once
#include "mbintradev.h"

#include <initializer_list>

namespace x264hip {

constexpr int COST_MAX = 1 << 28;             // encoder/analyse.c:120

// A mode list of the reference as one immediate: a mode a nibble, the first mode lowest, 15 ends it.
constexpr uint64_t modes( std::initializer_list<int> l )
{
    uint64_t v = ~0ull;
    int i = 0;
    for( int m : l )
    {
        v = (v & ~(15ull << (4 * i))) | ((uint64_t)m << (4 * i));
        i++;
    }
    return v;
}
__device__ __forceinline__ int mode_at( uint64_t list, int i ) { return (int)((list >> (4 * i)) & 15); }

// the row of a *_mode_available table: predict_*_mode_available, analyse.c:530-558
__device__ __forceinline__ int avail_idx( int n )
{
    const int idx = n & (NB_TOP | NB_LEFT | NB_TOPLEFT);
    return idx == (NB_TOP | NB_LEFT | NB_TOPLEFT) ? 4 : idx & (NB_TOP | NB_LEFT);
}

// i16x16_mode_available, analyse.c:476-483
__device__ __forceinline__ uint64_t i16x16_mode_available( int idx )
{
    switch( idx )
    {
        case 0: return modes( { 6 } );
        case 1: return modes( { 4, 1 } );
        case 2: return modes( { 5, 0 } );
        case 3: return modes( { 0, 1, 2 } );
        default: return modes( { 0, 1, 2, 3 } );
    }
}

// chroma_mode_available, analyse.c:485-492
__device__ __forceinline__ uint64_t chroma_mode_available( int idx )
{
    switch( idx )
    {
        case 0: return modes( { 6 } );
        case 1: return modes( { 4, 1 } );
        case 2: return modes( { 5, 2 } );
        case 3: return modes( { 2, 1, 0 } );
        default: return modes( { 2, 1, 0, 3 } );
    }
}

// i4x4_mode_available[0] and i8x8_mode_available[0] (b_avoid_topright = 0), analyse.c:494-528: the
// two are the same lists
__device__ __forceinline__ uint64_t i4x4_mode_available( int idx )
{
    switch( idx )
    {
        case 0: return modes( { 11 } );
        case 1: return modes( { 9, 1, 8 } );
        case 2: return modes( { 10, 0, 3, 7 } );
        case 3: return modes( { 2, 1, 0, 3, 7, 8 } );
        default: return modes( { 2, 1, 0, 3, 4, 5, 6, 7, 8 } );
    }
}
__device__ __forceinline__ uint64_t i8x8_mode_available( int idx )
{
    switch( idx )
    {
        case 0: return modes( { 11 } );
        case 1: return modes( { 9, 1, 8 } );
        case 2: return modes( { 10, 0, 3, 7 } );
        case 3: return modes( { 2, 1, 0, 3, 7, 8 } );
        default: return modes( { 2, 1, 0, 3, 4, 5, 6, 7, 8 } );
    }
}

// intra_analysis_shortcut[0][predict_mode[8] >= 0][favor_vertical], analyse.c:673-683
__device__ __forceinline__ uint64_t intra_analysis_shortcut( bool all, bool favor_vertical )
{
    switch( all * 2 + favor_vertical )
    {
        case 0: return modes( { 8 } );
        case 1: return modes( { 3, 7 } );
        case 2: return modes( { 4, 6, 8 } );
        default: return modes( { 3, 4, 5, 7 } );
    }
}

// i16x16_thresh_lut, i8x8_thresh (analyse.c:695, 859) at i_subpel_refine 2..5 and cost_div_fix8 (:854)
__device__ __forceinline__ int i16x16_thresh_lut( int subme ) { return (int)((modes( { 2, 2, 2, 3, 3, 4 } ) >> (4 * subme)) & 15); }
__device__ __forceinline__ int i8x8_thresh( int subme ) { return (int)((modes( { 4, 4, 4, 5, 5, 5 } ) >> (4 * subme)) & 15); }
__device__ __forceinline__ int cost_div_fix8( int idx ) { return idx == 0 ? 1024 : idx == 1 ? 512 : 341; }
constexpr int MB_B_COST_INTRA = 9;            // i_mb_b_cost_table[I_4x4], [I_8x8], [I_16x16], analyse.c:124-127

// bs_size_ue( x264_mb_pred_mode16x16_fix[mode] ) and bs_size_ue( x264_mb_chroma_pred_mode_fix[mode] )
// (common/predict.h:45-66, common/bitstream.h x264_ue_size_tab): the fixed mode is the mode below
// 4 and DC above; ue(0) = 1, ue(1) = ue(2) = 3, ue(3) = 5
__device__ __forceinline__ int ue_mode16( int mode ) { return mode == 0 ? 1 : mode == 3 ? 5 : 3; }
__device__ __forceinline__ int ue_chroma( int mode ) { return mode == 1 || mode == 2 ? 3 : mode == 3 ? 5 : 1; }

// x264_mb_pred_mode4x4_fix( mode ), predict.h:84-92
__device__ __forceinline__ int fix4( int mode ) { return mode < 0 ? -1 : mode > 8 ? 2 : mode; }

// x264_mb_predict_intra4x4_mode, common/macroblock.h:419-431
__device__ __forceinline__ int predict_mode4( int ma, int mb )
{
    const int m = min( fix4( ma ), fix4( mb ) );
    return m < 0 ? 2 : m;
}

// pixel_satd_4x4 (common/pixel.c:265-288) of a difference block
__device__ __forceinline__ int satd4( const int (&d)[4][4] )
{
    int t[4][4], sum = 0;
#pragma unroll
    for( int y = 0; y < 4; y++ )
    {
        const int a0 = d[y][0] + d[y][1], a1 = d[y][0] - d[y][1], a2 = d[y][2] + d[y][3], a3 = d[y][2] - d[y][3];
        t[y][0] = a0 + a2; t[y][1] = a1 + a3; t[y][2] = a0 - a2; t[y][3] = a1 - a3;
    }
#pragma unroll
    for( int x = 0; x < 4; x++ )
    {
        const int a0 = t[0][x] + t[1][x], a1 = t[0][x] - t[1][x], a2 = t[2][x] + t[3][x], a3 = t[2][x] - t[3][x];
        sum += abs( a0 + a2 ) + abs( a1 + a3 ) + abs( a0 - a2 ) + abs( a1 - a3 );
    }
    return sum >> 1;
}

// pixel_sa8d_8x8 (pixel.c:334-373) of a difference block, in place
__device__ __forceinline__ int sa8d8( int (&d)[8][8] )
{
    auto had8 = []( int &v0, int &v1, int &v2, int &v3, int &v4, int &v5, int &v6, int &v7 )
    {
        const int a0 = v0 + v1, a1 = v0 - v1, a2 = v2 + v3, a3 = v2 - v3, a4 = v4 + v5, a5 = v4 - v5, a6 = v6 + v7, a7 = v6 - v7;
        const int b0 = a0 + a2, b1 = a1 + a3, b2 = a0 - a2, b3 = a1 - a3, b4 = a4 + a6, b5 = a5 + a7, b6 = a4 - a6, b7 = a5 - a7;
        v0 = b0 + b4; v1 = b1 + b5; v2 = b2 + b6; v3 = b3 + b7; v4 = b0 - b4; v5 = b1 - b5; v6 = b2 - b6; v7 = b3 - b7;
    };
#pragma unroll
    for( int y = 0; y < 8; y++ )
        had8( d[y][0], d[y][1], d[y][2], d[y][3], d[y][4], d[y][5], d[y][6], d[y][7] );
    int sum = 0;
#pragma unroll
    for( int x = 0; x < 8; x++ )
    {
        had8( d[0][x], d[1][x], d[2][x], d[3][x], d[4][x], d[5][x], d[6][x], d[7][x] );
#pragma unroll
        for( int y = 0; y < 8; y++ )
            sum += abs( d[y][x] );
    }
    return (sum + 2) >> 2;
}

// fenc - p
__device__ __forceinline__ void sub4( const int (&f)[4][4], const int (&p)[4][4], int (&d)[4][4] )
{
#pragma unroll
    for( int y = 0; y < 4; y++ )
#pragma unroll
        for( int x = 0; x < 4; x++ )
            d[y][x] = f[y][x] - p[y][x];
}

// i_neighbour4[l], common/macroblock.c:489-498, 1340-1351 (as intra_i4_plane has it)
__device__ __forceinline__ int neighbour4( int l, int nb )
{
    const bool left = nb & NB_LEFT, top = nb & NB_TOP;
    if( l == 0 )
        return (nb & (NB_TOP | NB_LEFT | NB_TOPLEFT)) | (top ? NB_TOPRIGHT : 0);
    if( l == 1 || l == 4 )
        return NB_LEFT | (top ? NB_TOP | NB_TOPLEFT | NB_TOPRIGHT : 0);
    if( l == 2 || l == 8 || l == 10 )
        return NB_TOP | NB_TOPRIGHT | (left ? NB_LEFT | NB_TOPLEFT : 0);
    if( l == 5 )
        return NB_LEFT | (nb & NB_TOPRIGHT) | (top ? NB_TOP | NB_TOPLEFT : 0);
    if( l == 6 || l == 9 || l == 12 || l == 14 )
        return NB_LEFT | NB_TOP | NB_TOPLEFT | NB_TOPRIGHT;
    return NB_LEFT | NB_TOP | NB_TOPLEFT;
}

// the index of the 4x4 block at (bx, by) in h->dct.luma4x4's order
__device__ __forceinline__ int blk_idx( int bx, int by ) { return (by >> 1) * 8 + (bx >> 1) * 4 + (by & 1) * 2 + (bx & 1); }

// The I_4x4 pass, analyse.c:877-961, on the ten block anti-diagonals: a block's predicted mode and
// samples come from its left, top, top-left and top-right blocks only, so the serial order of the
// reference and this one score every block alike.  Each lane runs its block's candidate loop as
// the C has it, then encodes the block with the winner into the tile (x264_mb_encode_i4x4; the
// coefficients are dropped).  f: this lane's fenc block; m4: the macroblock's 16 chosen modes in
// shared memory; nm: the neighbour macroblocks' modes, [0..3] left rows, [4..7] top columns, -1
// outside the picture.  Returns i_best + 3 * lambda of this lane's block; the caller replays the
// loop's early termination over the sixteen.
template <int BD>
__device__ __forceinline__ int analyse_i4_plane( const PlaneCtx<BD> &k, tpx *ty, int8_t *m4, const int8_t *nm, int l, int nb,
                                                 int lambda, const int (&f)[4][4] )
{
    const int bx = blk_x( l ), by = blk_y( l );
    const int n4 = neighbour4( l, nb ), ai = avail_idx( n4 );
    const bool splat = (n4 & (NB_TOPRIGHT | NB_TOP)) == NB_TOP;
    tpx *b = ty + (4 * by) * TW + 4 * bx;                  // (-1,-1) of the block
    int block_cost = 0;
#pragma unroll 1
    for( int s = 0; s < 10; s++ )
    {
        if( bx + 2 * by == s )
        {
            const int i_pred_mode = predict_mode4( bx ? (int)m4[blk_idx( bx - 1, by )] : (int)nm[by],
                                                   by ? (int)m4[blk_idx( bx, by - 1 )] : (int)nm[4 + bx] );
            int t[8], lf[4], p[4][4], d[4][4];
#pragma unroll
            for( int x = 0; x < 4; x++ )
            {
                t[x] = b[1 + x];
                lf[x] = b[(1 + x) * TW];
            }
#pragma unroll
            for( int x = 4; x < 8; x++ )
                t[x] = splat ? t[3] : (int)b[1 + x];           // :886-888
            const int lt = b[0];
            int i_best = COST_MAX, best_mode = 2;
            uint64_t list = i4x4_mode_available( ai );
            if( ai >= 3 )                                      // predict_mode[5] >= 0, :903-920
            {
                int satd[3];
#pragma unroll
                for( int m = 0; m < 3; m++ )
                {
                    pred4x4<BD>( m, t, lf, lt, p );
                    sub4( f, p, d );
                    satd[m] = satd4( d );
                }
                const bool favor_vertical = satd[1] > satd[0];
#pragma unroll
                for( int m = 0; m < 3; m++ )
                    if( i_pred_mode == m )
                        satd[m] -= 3 * lambda;
                i_best = satd[2]; best_mode = 2;
                if( satd[1] < i_best ) { i_best = satd[1]; best_mode = 1; }
                if( satd[0] < i_best ) { i_best = satd[0]; best_mode = 0; }
                list = intra_analysis_shortcut( ai == 4, favor_vertical );
            }
            if( i_best > 0 )                                   // :922-948
            {
#pragma unroll 1
                for( int i = 0; mode_at( list, i ) != 15; i++ )
                {
                    const int i_mode = mode_at( list, i );
                    pred4x4<BD>( i_mode, t, lf, lt, p );
                    sub4( f, p, d );
                    int i_satd = satd4( d );
                    if( i_pred_mode == fix4( i_mode ) )
                    {
                        i_satd -= lambda * 3;
                        if( i_satd <= 0 )
                        {
                            i_best = i_satd;
                            best_mode = i_mode;
                            break;
                        }
                    }
                    if( i_satd < i_best ) { i_best = i_satd; best_mode = i_mode; }
                }
            }
            block_cost = i_best + 3 * lambda;
            m4[l] = (int8_t)best_mode;
            // x264_mb_encode_i4x4 into the tile
            int c[16], res[4][4];
            pred4x4<BD>( best_mode, t, lf, lt, p );
            sub4( f, p, d );
            dct4x4_core<BD>( d, c );
            int acc = 0;
#pragma unroll
            for( int j = 0; j < 16; j++ )
            {
                c[j] = sto<BD>( quant_one( c[j], k.mf4[j], k.bias4[j] ) );
                acc |= c[j];
            }
            fill( res, 0 );
            if( acc )
            {
                const int32_t *m = k.dq4 + (k.qp % 6) * 16;
                const int qb = k.qp / 6 - 4;
#pragma unroll
                for( int j = 0; j < 16; j++ )
                    c[j] = sto<BD>( dequant_one( c[j], m[j], qb ) );
                idct4_residual<BD>( c, res );
            }
#pragma unroll
            for( int y = 0; y < 4; y++ )
#pragma unroll
                for( int x = 0; x < 4; x++ )
                    b[(1 + y) * TW + 1 + x] = (tpx)clip_pix<BD>( p[y][x] + res[y][x] );
        }
        tile_sync();
    }
    return block_cost;
}

// predict_8x8[mode] (common/predict.c:700-884) of a whole block from the filtered edge; dc: the
// value of the mode's DC variant
__device__ __forceinline__ void pred8_block( int mode, const tpx *e, int dc, int (&p)[8][8] )
{
#define X264HIP_P8( expr )                      \
    _Pragma( "unroll" )                         \
    for( int y = 0; y < 8; y++ )                \
        _Pragma( "unroll" )                     \
        for( int x = 0; x < 8; x++ )            \
            p[y][x] = ( expr )
    switch( mode )
    {
        case 0: X264HIP_P8( (int)e[16 + x] ); break;
        case 1: X264HIP_P8( (int)e[14 - y] ); break;
        case 3: X264HIP_P8( pred8_dir<3>( e, x, y ) ); break;
        case 4: X264HIP_P8( pred8_dir<4>( e, x, y ) ); break;
        case 5: X264HIP_P8( pred8_dir<5>( e, x, y ) ); break;
        case 6: X264HIP_P8( pred8_dir<6>( e, x, y ) ); break;
        case 7: X264HIP_P8( pred8_dir<7>( e, x, y ) ); break;
        case 8: X264HIP_P8( pred8_dir<8>( e, x, y ) ); break;
        default: X264HIP_P8( dc ); break;
    }
#undef X264HIP_P8
}

// what the I_8x8 pass leaves: a->i_satd_i8x8, i_cost as :860 reads it, the four modes
struct I8Out
{
    int i_satd_i8x8, i_cost;
    int mode[4];
};

// The I_8x8 pass, analyse.c:746-857, block by block as the C runs it (uniform over the
// macroblock's lanes): the 16 lanes build the filtered edge, lane m scores mode m with sa8d, every
// lane replays the candidate loop over the twelve scores, the winner is predicted into the tile
// and lane idx encodes it there (x264_mb_encode_i8x8; the coefficients are dropped).
// i_cost: lambda * 4 plus the B prefix.
template <int BD>
__device__ __forceinline__ void analyse_i8_plane( const PlaneCtx<BD> &k, tpx *ty, tpx *e, const int8_t *nm, int l, int nb,
                                                  int lambda, int i_cost, int i_satd_thresh, I8Out &o )
{
    const bool left = nb & NB_LEFT, top = nb & NB_TOP;
    o.mode[0] = o.mode[1] = o.mode[2] = o.mode[3] = 2;
    int idx;
#pragma unroll 1
    for( idx = 0;; idx++ )
    {
        // i_neighbour8[idx], common/macroblock.c:498, 1340-1351
        const int n8 = idx == 0 ? (nb & (NB_TOP | NB_LEFT | NB_TOPLEFT)) | (top ? NB_TOPRIGHT : 0)
                     : idx == 1 ? NB_LEFT | (nb & NB_TOPRIGHT) | (top ? NB_TOP | NB_TOPLEFT : 0)
                     : idx == 2 ? NB_TOP | NB_TOPRIGHT | (left ? NB_LEFT | NB_TOPLEFT : 0)
                                : NB_LEFT | NB_TOP | NB_TOPLEFT;
        const int ai = avail_idx( n8 );
        // x264_mb_predict_intra4x4_mode( h, 4 * idx ): the cache holds this pass' earlier blocks
        const int ma = idx == 0 ? (int)nm[0] : idx == 1 ? o.mode[0] : idx == 2 ? (int)nm[2] : o.mode[2];
        const int mb = idx == 0 ? (int)nm[4] : idx == 1 ? (int)nm[6] : idx == 2 ? o.mode[0] : o.mode[1];
        const int i_pred_mode = predict_mode4( ma, mb );
        tpx *b = ty + (8 * (idx >> 1)) * TW + 8 * (idx & 1);
        const int ox = 8 * (idx & 1), oy = 8 * (idx >> 1);
        // predict_8x8_filter with ALL_NEIGHBORS: two entries a lane
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
        auto dc_of = [&]( int mode )
        {
            return mode == 2 ? (sl + st + 8) >> 4 : mode == 9 ? (sl + 4) >> 3 : mode == 10 ? (st + 4) >> 3 : 1 << (BD - 1);
        };
        const uint64_t avail = i8x8_mode_available( ai );
        bool mine = false;
#pragma unroll
        for( int i = 0; i < 9; i++ )
            mine = mine || mode_at( avail, i ) == l;
        int score = COST_MAX;
        if( mine )
        {
            int d[8][8];
            pred8_block( l, e, dc_of( l ), d );
#pragma unroll
            for( int y = 0; y < 8; y++ )
            {
                int fe[8];
                read_row<BD, 8>( k.fenc + (oy + y) * k.fs + ox, fe );
#pragma unroll
                for( int x = 0; x < 8; x++ )
                    d[y][x] -= fe[x];
            }
            score = sa8d8( d );
        }
        int i_best = COST_MAX, best_mode = 2;
        uint64_t list = avail;
        if( ai >= 3 )                                          // predict_mode[5] >= 0, :784-804
        {
            int satd[3] = { mb_lane( score, 0 ), mb_lane( score, 1 ), mb_lane( score, 2 ) };
            const bool favor_vertical = satd[1] > satd[0];
#pragma unroll
            for( int m = 0; m < 3; m++ )
                if( i_pred_mode == m )
                    satd[m] -= 3 * lambda;
#pragma unroll
            for( int i = 2; i >= 0; i-- )
                if( satd[i] < i_best ) { i_best = satd[i]; best_mode = i; }
            list = intra_analysis_shortcut( ai == 4, favor_vertical );
        }
#pragma unroll 1
        for( int i = 0; mode_at( list, i ) != 15 && i_best >= 0; i++ )   // :806-822
        {
            const int i_mode = mode_at( list, i );
            int i_satd = mb_lane( score, i_mode );
            if( i_pred_mode == fix4( i_mode ) )
                i_satd -= 3 * lambda;
            if( i_satd < i_best ) { i_best = i_satd; best_mode = i_mode; }
        }
        i_cost += i_best + 3 * lambda;
#pragma unroll
        for( int j = 0; j < 4; j++ )
            o.mode[j] = idx == j ? best_mode : o.mode[j];
        if( idx == 3 || i_cost > i_satd_thresh )
            break;
        // predict_8x8[best] into the tile, four pixels a lane, then x264_mb_encode_i8x8 by lane idx
        {
            const int y = l >> 1, x0 = (l & 1) * 4, dc = dc_of( best_mode );
#pragma unroll
            for( int x = 0; x < 4; x++ )
                b[(1 + y) * TW + 1 + x0 + x] = (tpx)pred8_px( best_mode, e, x0 + x, y, dc );
        }
        tile_sync();
        if( l == idx )
        {
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
            if( acc )
            {
                int res[8][8];
                const int32_t *m = k.dq8 + (k.qp % 6) * 64;
                const int qb = k.qp / 6 - 6;
#pragma unroll
                for( int j = 0; j < 64; j++ )
                    c[j] = sto<BD>( dequant_one( c[j], m[j], qb ) );
                idct8_residual<BD>( c, res );
#pragma unroll
                for( int y = 0; y < 8; y++ )
#pragma unroll
                    for( int x = 0; x < 8; x++ )
                        b[(1 + y) * TW + 1 + x] = (tpx)clip_pix<BD>( (int)b[(1 + y) * TW + 1 + x] + res[y][x] );
            }
        }
        tile_sync();
    }
    if( idx == 3 )
        o.i_satd_i8x8 = i_cost;
    else
    {
        o.i_satd_i8x8 = COST_MAX;
        i_cost = (i_cost * cost_div_fix8( idx )) >> 8;         // :852-857
    }
    o.i_cost = i_cost;
}

} // namespace x264hip
