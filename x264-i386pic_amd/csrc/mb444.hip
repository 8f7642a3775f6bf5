// The inter and intra macroblock encodes at 4:4:4 on gfx950 (include/x264hip_mb444.h):
// macroblock_encode_internal( h, 3, 0 ) (reference encoder/macroblock.c:618-972 with
// plane_count = 3, chroma = 0).  U and V go through the luma paths with the chroma quant
// categories and the chroma qp; the paths are the ones mbenc.hip and mbintra.hip run on their luma
// plane (mbencdev.h, mbintradev.h), here on three planes side by side.
//
// Mapping: one macroblock per wave, plane p on lanes 16p .. 16p+15 (lanes 48..63 leave at once), so
// the 16-lane cross-lane reads of the plane functions stay inside a plane and the three serial
// chains of an intra macroblock advance together.  What couples the planes is read across the
// wave: the inter entry's i_decimate_mb, which the reference never resets between planes
// (macroblock.c:771), is a prefix sum over the three planes' own scores, and the cbp is the OR of
// the planes' bits.  A macroblock's kind (transform size, skip, intra type) is the same in all
// three planes, so every branch that holds a cross-lane read or a tile exchange is uniform over
// the wave's 48 lanes.  Intra: one launch per anti-diagonal x + 2y as mbintra.hip, one tile of
// shared memory per plane.
#include "mbintradev.h"
#include "x264hip_mb444.h"

#include <string.h>

namespace x264hip {
namespace {

// reference common/set.h: CQM_4IY, 4PY, 4IC, 4PC = 0..3 and CQM_8IY, 8PY, 8IC, 8PC = 0..3, so the
// category of plane p is the luma one + 2 * !!p for both transform sizes
constexpr int CQM_IY = 0, CQM_PY = 1, CQM_CHROMA = 2;

// the launch's inputs, by value in the kernel arguments; stride pairs: [0] Y, [1] U and V
template <int BD> struct Mb444Params
{
    using pixel = typename PT<BD>::pixel;
    using dctcoef = typename PT<BD>::dctcoef;
    using udctcoef = typename PT<BD>::udctcoef;
    const pixel *fenc[3], *pred[3];
    pixel *recon[3];
    intptr_t fs[2], ffs[2], ps[2], pfs[2], rs[2], rfs[2];
    const udctcoef *q4mf, *q4b, *q8mf, *q8b;
    const int32_t *dq4, *dq8;
    const int8_t *qp;
    const uint8_t *flags;
    const int8_t *pmode;
    dctcoef *level, *luma_dc;
    uint8_t *nnz;
    int32_t *cbp, *nz;
    uint8_t *flags_out;
    int mbw, mbh, nmb, dec, al;               // al: level (and luma_dc) are 16-byte aligned
    int d, ymin, count, nitems;               // intra: the diagonal, its first row, its macroblocks per frame, in all
    uint32_t cqp[16];                         // chroma_qp_table[0..63], four entries a word
};

// the value of lane j of the wave (a plane's lane 0 is 16 * p)
__device__ __forceinline__ int wave_lane( int v, int j ) { return __shfl( v, j, 64 ); }

// v of planes 0, 1, 2 combined over the wave
__device__ __forceinline__ int planes_or( int v ) { return wave_lane( v, 0 ) | wave_lane( v, 16 ) | wave_lane( v, 32 ); }

// plane p's entry of three kernel arguments, without indexing them by a lane value
template <typename T> __device__ __forceinline__ T of_plane( int p, T const (&v)[3] )
{
    return p == 0 ? v[0] : p == 1 ? v[1] : v[2];
}

// the luma (c = 0) or chroma (c = 1) entry of a stride pair
__device__ __forceinline__ intptr_t of_kind( int c, const intptr_t (&v)[2] ) { return c ? v[1] : v[0]; }

// plane p of macroblock (mbx, mby) of frame f; qp: the luma qp, qpc: the chroma qp
template <int BD, bool INTRA>
__device__ __forceinline__ void plane_ctx( const Mb444Params<BD> &a, int p, int f, int mbx, int mby, int qp, int qpc,
                                           typename PT<BD>::dctcoef *lvl, PlaneCtx<BD> &k )
{
    constexpr int QP1 = 52 + 6 * (BD - 8);
    const int c = p != 0;
    k.fs = of_kind( c, a.fs ); k.ps = of_kind( c, a.ps ); k.rs = of_kind( c, a.rs );
    k.fenc = of_plane( p, a.fenc ) + (intptr_t)f * of_kind( c, a.ffs ) + (intptr_t)(16 * mby) * k.fs + 16 * mbx;
    k.pred = nullptr;
    if constexpr( !INTRA )
        k.pred = of_plane( p, a.pred ) + (intptr_t)f * of_kind( c, a.pfs ) + (intptr_t)(16 * mby) * k.ps + 16 * mbx;
    k.recon = of_plane( p, a.recon ) + (intptr_t)f * of_kind( c, a.rfs ) + (intptr_t)(16 * mby) * k.rs + 16 * mbx;
    const int cat = (INTRA ? CQM_IY : CQM_PY) + CQM_CHROMA * c;
    k.qp = c ? qpc : qp;
    k.mf4 = a.q4mf + (cat * QP1 + k.qp) * 16; k.bias4 = a.q4b + (cat * QP1 + k.qp) * 16;
    k.mf8 = a.q8mf + (cat * QP1 + k.qp) * 64; k.bias8 = a.q8b + (cat * QP1 + k.qp) * 64;
    k.dq4 = a.dq4 + cat * 6 * 16; k.dq8 = a.dq8 + cat * 6 * 64;
    k.lvl = lvl + p * (16 * 16);
    k.al = a.al;
}

template <int BD>
__global__ __launch_bounds__( 256 ) void mb_encode_inter_444_kernel( const Mb444Params<BD> a )
{
    constexpr int QP1 = 52 + 6 * (BD - 8);
    __shared__ uint32_t s_cqp[16];
#pragma unroll
    for( int j = 0; j < 16; j++ )
        if( threadIdx.x == j )
            s_cqp[j] = a.cqp[j];
    __syncthreads();
    const int lane = threadIdx.x & 63, p = lane >> 4, l = lane & 15;
    const int mb = blockIdx.x * 4 + (threadIdx.x >> 6);
    if( mb >= a.nmb || p == 3 )
        return;
    const int fl = a.flags[mb];
    if( fl & X264HIP_MBENC_INTRA )
    {
        if( lane == 0 )
            a.flags_out[mb] = (uint8_t)fl;
        return;
    }
    const int per = a.mbw * a.mbh;
    const int f = mb / per, rem = mb - f * per;
    const int mby = rem / a.mbw, mbx = rem - mby * a.mbw;
    const int qp = min( max( (int)a.qp[mb], 0 ), QP1 - 1 );
    const int qpc = min( (int)((s_cqp[qp >> 2] >> (8 * (qp & 3))) & 255), QP1 - 1 );
    const bool skip = fl & X264HIP_MBENC_SKIP;
    const bool t8 = (fl & X264HIP_MBENC_T8x8) && a.q8mf;
    PlaneCtx<BD> k;
    plane_ctx<BD, false>( a, p, f, mbx, mby, qp, qpc, a.level + (int64_t)mb * (48 * 16), k );

    int lmask = 0;                             // this plane's non_zero_count, bit = block index
    int k4 = 0;                                // transform 8: this plane's kept 8x8 blocks
    int plane_cbp = 0;
    if( !t8 )
    {
        Inter4 s;
        inter_luma4_scores<BD>( k, l, a.dec, skip, s );
        // i_decimate_mb at the test after plane p (macroblock.c:907): the scores of planes 0..p
        const int s0 = wave_lane( s.plane_score, 0 ), s1 = wave_lane( s.plane_score, 16 ), s2 = wave_lane( s.plane_score, 32 );
        const int i_decimate_mb = s0 + (p >= 1 ? s1 : 0) + (p >= 2 ? s2 : 0);
        const bool nn = inter_luma4_finish<BD>( k, l, s, i_decimate_mb );
        lmask = (int)((__ballot( nn ) >> (16 * p)) & 0xffff);
#pragma unroll
        for( int j = 0; j < 4; j++ )
            plane_cbp |= (((lmask >> (4 * j)) & 0xf) != 0) << j;
    }
    else
    {
        Inter8 s;
        inter_luma8_scores<BD>( k, l, a.dec, skip, s );
        // the same carry at :833
        const int s0 = wave_lane( s.plane_score, 0 ), s1 = wave_lane( s.plane_score, 16 ), s2 = wave_lane( s.plane_score, 32 );
        const int i_decimate_mb = s0 + (p >= 1 ? s1 : 0) + (p >= 2 ? s2 : 0);
        const bool keep = inter_luma8_finish<BD>( k, l, a.dec, s, i_decimate_mb );
        k4 = (int)((__ballot( keep ) >> (16 * p)) & 0xf);
        plane_cbp = k4;
#pragma unroll
        for( int j = 0; j < 4; j++ )
            lmask |= ((k4 >> j) & 1) * (0xf << (4 * j));
    }

    // ---------------------------------------------------------------- the per-macroblock outputs
    a.nnz[(int64_t)mb * 48 + lane] = (uint8_t)((lmask >> l) & 1);
    const int cbp = planes_or( plane_cbp );
    if( lane == 0 )
    {
        a.cbp[mb] = cbp;
        a.nz[mb] = t8 ? k4 : lmask;                             // plane 0's
        a.flags_out[mb] = (uint8_t)((fl & 3) | ((fl & X264HIP_MBENC_D16x16) && !cbp ? X264HIP_MBENC_D16x16 : 0));
    }
}

template <int BD>
__global__ __launch_bounds__( 64 ) void mb_encode_intra_444_kernel( const Mb444Params<BD> a )
{
    constexpr int QP1 = 52 + 6 * (BD - 8);
    __shared__ uint32_t s_cqp[16];
    __shared__ tpx s_t[3][TILE];               // a tile per plane
    __shared__ tpx s_e[3][36];                 // the filtered edge of an I_8x8 block, per plane
#pragma unroll
    for( int j = 0; j < 16; j++ )
        if( threadIdx.x == j )
            s_cqp[j] = a.cqp[j];
    __syncthreads();
    const int lane = threadIdx.x, p = lane >> 4, l = lane & 15;
    const int item = blockIdx.x;
    if( item >= a.nitems || p == 3 )
        return;
    const int f = item / a.count;
    const int my = a.ymin + (item - f * a.count), mx = a.d - 2 * my;
    const int mb = (f * a.mbh + my) * a.mbw + mx;
    const int fl = a.flags[mb];
    if( !(fl & X264HIP_MBENC_INTRA) )
        return;
    const int qp = min( max( (int)a.qp[mb], 0 ), QP1 - 1 );
    const int qpc = min( (int)((s_cqp[qp >> 2] >> (8 * (qp & 3))) & 255), QP1 - 1 );
    const bool left = mx > 0, top = my > 0, topright = top && mx + 1 < a.mbw;
    const int nb = (left ? NB_LEFT : 0) | (top ? NB_TOP : 0) | (left && top ? NB_TOPLEFT : 0) | (topright ? NB_TOPRIGHT : 0);
    const bool i8 = (fl & X264HIP_MBENC_T8x8) && a.q8mf;
    const bool i16 = !(fl & X264HIP_MBENC_T8x8) && (fl & X264HIP_MBINTRA_I16x16);
    const int8_t *pm = a.pmode + (int64_t)mb * 16;
    PlaneCtx<BD> k;
    plane_ctx<BD, true>( a, p, f, mx, my, qp, qpc, a.level + (int64_t)mb * (48 * 16), k );
    tpx *ty = s_t[p];
    int tpx_l, lpx_l;
    tile_borders<BD>( ty, k.recon, k.rs, l, nb, tpx_l, lpx_l );
    tile_sync();

    // the plane's luma path with the macroblock's luma mode(s)
    int lmask = 0, k4 = 0, cbp_luma = 0, nz_ldc = 0;
    int ldc[16];
    zero( ldc );
    if( i16 )
    {
        const bool nn = intra_i16_plane<BD>( k, ty, l, pm[0], a.dec, tpx_l, lpx_l, ldc, nz_ldc, cbp_luma );
        lmask = (int)((__ballot( nn ) >> (16 * p)) & 0xffff);
    }
    else if( !i8 )
    {
        const int nzb = intra_i4_plane<BD>( k, ty, l, (fl & X264HIP_MBENC_T8x8) ? pm[l & 12] : pm[l], nb );
        lmask = (int)((__ballot( nzb ) >> (16 * p)) & 0xffff);
#pragma unroll
        for( int j = 0; j < 4; j++ )
            cbp_luma |= (((lmask >> (4 * j)) & 0xf) != 0) << j;
    }
    else
    {
        const int nz8 = intra_i8_plane<BD>( k, ty, s_e[p], l, pm, nb );
        k4 = (int)((__ballot( nz8 && l < 4 ) >> (16 * p)) & 0xf);
        cbp_luma = k4;
#pragma unroll
        for( int j = 0; j < 4; j++ )
            lmask |= ((k4 >> j) & 1) * (0xf << (4 * j));
    }

    // ---------------------------------------------------------------- the per-macroblock outputs
    a.nnz[(int64_t)mb * 48 + lane] = (uint8_t)((lmask >> l) & 1);
    if( l == 2 )
        put_coefs<BD, 16>( a.luma_dc + ((int64_t)mb * 3 + p) * 16, ldc, a.al );
    // nnz( LUMA_DC + p ) << (8 + p), macroblock.c:946-950
    const int cbp = planes_or( cbp_luma | nz_ldc << (8 + p) );
    if( lane == 0 )
    {
        a.cbp[mb] = cbp;
        a.nz[mb] = i8 ? k4 : lmask;                             // plane 0's
        a.flags_out[mb] = (uint8_t)(fl & 3);
    }
}

template <int BD>
void fill_params( const x264hip_mb444_t *e, int mbw, int mbh, bool intra, Mb444Params<BD> &a )
{
    using pixel = typename PT<BD>::pixel;
    memset( &a, 0, sizeof( a ) );
    fill_mb_params<BD>( e, mbw, mbh, a );
    for( int p = 0; p < 3; p++ )
    {
        a.fenc[p] = (const pixel *)e->fenc[p];
        a.pred[p] = (const pixel *)e->pred[p];
        a.recon[p] = (pixel *)e->recon[p];
    }
    a.fs[0] = e->fenc_stride; a.ffs[0] = e->fenc_frame_stride;
    a.fs[1] = e->fenc_chroma_stride; a.ffs[1] = e->fenc_chroma_frame_stride;
    a.ps[0] = e->pred_stride; a.pfs[0] = e->pred_frame_stride;
    a.ps[1] = e->pred_chroma_stride; a.pfs[1] = e->pred_chroma_frame_stride;
    a.rs[0] = e->recon_stride; a.rfs[0] = e->recon_frame_stride;
    a.rs[1] = e->recon_chroma_stride; a.rfs[1] = e->recon_chroma_frame_stride;
    a.pmode = e->pred_mode;
    a.luma_dc = (typename PT<BD>::dctcoef *)e->luma_dc;
    a.al = !(((uintptr_t)e->level | (intra ? (uintptr_t)e->luma_dc : 0)) & 15);
}

} // namespace

// the arguments were checked by the C entries (capi.cpp x264hip_*_mb_encode_inter_444 / _intra_444)
template <int BD>
hipError_t launch_mb_encode_inter_444( const x264hip_mb444_t *e, int mbw, int mbh, int n_frames, hipStream_t stream )
{
    const int64_t nmb = (int64_t)n_frames * mbw * mbh;
    if( !e || nmb <= 0 )
        return hipSuccess;
    Mb444Params<BD> a;
    fill_params<BD>( e, mbw, mbh, false, a );
    a.nmb = (int)nmb;
    hipLaunchKernelGGL( ( mb_encode_inter_444_kernel<BD> ), dim3( (unsigned)((nmb + 3) / 4) ), dim3( 256 ), 0, stream, a );
    return hipGetLastError();
}
X264HIP_INSTANTIATE( launch_mb_encode_inter_444 );

template <int BD>
hipError_t launch_mb_encode_intra_444( const x264hip_mb444_t *e, int mbw, int mbh, int n_frames, hipStream_t stream )
{
    if( !e || mbw <= 0 || mbh <= 0 || n_frames <= 0 )
        return hipSuccess;
    Mb444Params<BD> a;
    fill_params<BD>( e, mbw, mbh, true, a );
    // one launch per anti-diagonal, in dependency order
    for_each_diagonal( mbw, mbh, [&]( int d, int ymin, int count )
    {
        a.d = d; a.ymin = ymin; a.count = count; a.nitems = count * n_frames;
        hipLaunchKernelGGL( ( mb_encode_intra_444_kernel<BD> ), dim3( (unsigned)a.nitems ), dim3( 64 ), 0, stream, a );
    } );
    return hipGetLastError();
}
X264HIP_INSTANTIATE( launch_mb_encode_intra_444 );

} // namespace x264hip
