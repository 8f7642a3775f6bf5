// MB-tree on the device (include/x264hip_mbtree.h): macroblock_tree_propagate and
// macroblock_tree_finish of reference encoder/slicetype.c:1026-1089 with the table entries
// mbtree_propagate_cost / mbtree_propagate_list of common/mc.c:509-598, over the per-MB arrays
// the lookahead kernels leave in device memory.
//
// Propagate.  Every MC_CLIP_ADD adds a non-negative amount and clips at 32767, so any sequence
// of them into one element equals min( initial + sum, 32767 ) in any order.  One thread per
// (step, MB) computes the MB's amount in registers and adds its up to eight bilinear shares into
// 32-bit accumulators, one per distinct destination plane, with no-return integer atomics
// (order-free, hence bit-exact and reproducible); a merge pass then applies the clip once.
// Three dispatches per batch: memset, scatter, merge.
//
// Float contract: the reference's expression order, one IEEE round-to-nearest operation each.
// hipcc contracts a + b * c into an FMA by default; the pragma below switches that off for the
// whole file, and the division is the correctly rounded one (hipcc's default for `/`).
#include "hipcommon.h"
#include "x264hip_mbtree.h"

#include <algorithm>

#pragma clang fp contract( off )

namespace x264hip {

// x264_log2's tables, reference common/tables.c:66-90 (decimal literals converted as the
// reference's are: as doubles, then to float).  The finish kernel stages them into LDS once per
// block, so the per-lane reads are ds_read_b32, not loads from a table in memory
__constant__ float k_log2_lut[128] =
{
    0.00000, 0.01123, 0.02237, 0.03342, 0.04439, 0.05528, 0.06609, 0.07682,
    0.08746, 0.09803, 0.10852, 0.11894, 0.12928, 0.13955, 0.14975, 0.15987,
    0.16993, 0.17991, 0.18982, 0.19967, 0.20945, 0.21917, 0.22882, 0.23840,
    0.24793, 0.25739, 0.26679, 0.27612, 0.28540, 0.29462, 0.30378, 0.31288,
    0.32193, 0.33092, 0.33985, 0.34873, 0.35755, 0.36632, 0.37504, 0.38370,
    0.39232, 0.40088, 0.40939, 0.41785, 0.42626, 0.43463, 0.44294, 0.45121,
    0.45943, 0.46761, 0.47573, 0.48382, 0.49185, 0.49985, 0.50779, 0.51570,
    0.52356, 0.53138, 0.53916, 0.54689, 0.55459, 0.56224, 0.56986, 0.57743,
    0.58496, 0.59246, 0.59991, 0.60733, 0.61471, 0.62205, 0.62936, 0.63662,
    0.64386, 0.65105, 0.65821, 0.66534, 0.67243, 0.67948, 0.68650, 0.69349,
    0.70044, 0.70736, 0.71425, 0.72110, 0.72792, 0.73471, 0.74147, 0.74819,
    0.75489, 0.76155, 0.76818, 0.77479, 0.78136, 0.78790, 0.79442, 0.80090,
    0.80735, 0.81378, 0.82018, 0.82655, 0.83289, 0.83920, 0.84549, 0.85175,
    0.85798, 0.86419, 0.87036, 0.87652, 0.88264, 0.88874, 0.89482, 0.90087,
    0.90689, 0.91289, 0.91886, 0.92481, 0.93074, 0.93664, 0.94251, 0.94837,
    0.95420, 0.96000, 0.96578, 0.97154, 0.97728, 0.98299, 0.98868, 0.99435,
};
__constant__ float k_log2_lz_lut[32] =
{
    31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0
};

// the steps of one launch, by value in the kernel arguments.  Their pointers come out of the
// argument block as generic pointers; the kernels name them global again (the form load_al uses)
// so the loads and atomics are global_*, not flat_*
constexpr int MBT_MAX_STEPS = 16;
constexpr int MBT_MAX_DSTS = 2 * MBT_MAX_STEPS;
// a 32-bit accumulator cannot wrap while it takes at most this many source MBs: an MB adds at
// most amount + 1 over both lists' weighted amounts plus 4 rounding units over the four
// shares, <= 32772, and 131000 * 32772 + 32767 < 2^32
constexpr int64_t MBT_ACC_MBS = 131000;

struct MbtStep
{
    const uint16_t *intra, *costs, *invq, *pin;
    const int16_t *mv[2];
    int32_t acc[2];                   // accumulator plane of each list's destination
    float fps;
    int32_t weight;
};
struct MbtBatch
{
    MbtStep s[MBT_MAX_STEPS];
};
struct MbtDsts
{
    uint16_t *p[MBT_MAX_DSTS];
};

typedef const __attribute__( ( address_space( 1 ) ) ) uint16_t g_cu16;
typedef const __attribute__( ( address_space( 1 ) ) ) int16_t g_ci16;
typedef __attribute__( ( address_space( 1 ) ) ) uint16_t g_u16;

// mbtree_propagate_cost (mc.c:511-525) of one MB
__device__ __forceinline__ int propagate_amount( int intra, int cost, int invq, int pin, float fps )
{
    if( !intra )
        return 0;                     // the reference divides 0 by 0 here
    const int inter = min( intra, cost & 0x3fff );
    const float propagate_intra = (float)( intra * invq );
    const float t = propagate_intra * fps;
    const float propagate_amount = (float)pin + t;
    const float propagate_num = (float)( intra - inter );
    const float propagate_denom = (float)intra;
    const float u = propagate_amount * propagate_num;
    const float q = u / propagate_denom;
    return min( (int)( q + 0.5f ), 32767 );
}

// one thread per (step, MB of [m0, m1)): mbtree_propagate_list (mc.c:527-598) of both lists
// into the accumulators
__global__ __launch_bounds__( 256 ) void mbtree_scatter_kernel( MbtBatch batch, uint32_t *__restrict__ acc, int mbw,
                                                                int mbh, int m0, int m1 )
{
    const int i = m0 + (int)( blockIdx.x * 256 + threadIdx.x );
    if( i >= m1 )
        return;
    const MbtStep &s = batch.s[blockIdx.y];
    const int mbc = mbw * mbh;
    g_cu16 *intra = (g_cu16 *)(uintptr_t)s.intra;
    g_cu16 *costs = (g_cu16 *)(uintptr_t)s.costs;
    const int cost = costs[i];
    int invq = 256, pin = 0;
    if( s.invq )
        invq = ( (g_cu16 *)(uintptr_t)s.invq )[i];
    if( s.pin )
        pin = ( (g_cu16 *)(uintptr_t)s.pin )[i];
    const int amount = propagate_amount( intra[i], cost, invq, pin, s.fps );
    const int lists_used = cost >> 14;
    const int mb_y = i / mbw, mb_x = i - mb_y * mbw;
#pragma unroll
    for( int l = 0; l < 2; l++ )
    {
        if( !s.mv[l] || !( lists_used & ( 1 << l ) ) )
            continue;
        int listamount = amount;
        if( lists_used == 3 )
            listamount = ( listamount * ( l ? 64 - s.weight : s.weight ) + 32 ) >> 6;
        uint32_t *a = acc + (int64_t)s.acc[l] * mbc;
        g_ci16 *mv = (g_ci16 *)(uintptr_t)s.mv[l];
        int x = mv[2 * i], y = mv[2 * i + 1];
        if( !( x | y ) )
        {
            __hip_atomic_fetch_add( a + i, (uint32_t)listamount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
            continue;
        }
        // signed coordinates with explicit bounds: the reference's unsigned compares accept
        // exactly the shares whose column and row lie inside the frame
        const int mbx = ( x >> 5 ) + mb_x, mby = ( y >> 5 ) + mb_y;
        x &= 31;
        y &= 31;
        const int w[4] = { ( ( 32 - y ) * ( 32 - x ) * listamount + 512 ) >> 10, ( ( 32 - y ) * x * listamount + 512 ) >> 10,
                           ( y * ( 32 - x ) * listamount + 512 ) >> 10, ( y * x * listamount + 512 ) >> 10 };
#pragma unroll
        for( int k = 0; k < 4; k++ )
        {
            const int cx = mbx + ( k & 1 ), cy = mby + ( k >> 1 );
            if( cx >= 0 && cx < mbw && cy >= 0 && cy < mbh )
                __hip_atomic_fetch_add( a + ( cy * mbw + cx ), (uint32_t)w[k], __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT );
        }
    }
}

// dst = min( dst + sum, 32767 ) of destination plane blockIdx.y over the MBs [0, mbc)
__global__ __launch_bounds__( 256 ) void mbtree_merge_kernel( MbtDsts dsts, const uint32_t *__restrict__ acc, int mbc )
{
    const int i = (int)( blockIdx.x * 256 + threadIdx.x );
    if( i >= mbc )
        return;
    g_u16 *dst = (g_u16 *)(uintptr_t)dsts.p[blockIdx.y];
    const uint64_t v = (uint64_t)dst[i] + acc[(int64_t)blockIdx.y * mbc + i];
    dst[i] = (uint16_t)( v < 32767 ? v : 32767 );
}

// macroblock_tree_finish (slicetype.c:1039-1048), one thread per MB
__global__ __launch_bounds__( 256 ) void mbtree_finish_kernel( const uint16_t *__restrict__ intra,
                                                               const uint16_t *__restrict__ invq,
                                                               const uint16_t *__restrict__ prop, const float *aq,
                                                               float *out, int mbc, int fps_factor, float weightdelta,
                                                               float strength )
{
    __shared__ float lut[128], lz_lut[32];
    if( threadIdx.x < 128 )
        lut[threadIdx.x] = k_log2_lut[threadIdx.x];
    else if( threadIdx.x < 160 )
        lz_lut[threadIdx.x - 128] = k_log2_lz_lut[threadIdx.x - 128];
    __syncthreads();
    const int i = (int)( blockIdx.x * 256 + threadIdx.x );
    if( i >= mbc )
        return;
    const int ic = ( (int)intra[i] * ( invq ? (int)invq[i] : 256 ) + 128 ) >> 8;
    if( !ic )
        return;
    const int pc = ( (int)prop[i] * fps_factor + 128 ) >> 8;
    // x264_log2 (common/base.h:226-230)
    auto log2 = [&]( uint32_t x ) {
        const int lz = __builtin_clz( x );
        return lut[( x << lz >> 24 ) & 0x7f] + lz_lut[lz];
    };
    const float d = log2( (uint32_t)( ic + pc ) ) - log2( (uint32_t)ic );
    const float log2_ratio = d + weightdelta;
    const float m = strength * log2_ratio;
    out[i] = aq[i] - m;
}

hipError_t launch_mbtree_propagate( const x264hip_mbtree_step_t *steps, int n, int mbw, int mbh, hipStream_t stream )
{
    const int64_t mbc = (int64_t)mbw * mbh;
    // steps per launch: the argument block's capacity and the accumulator bound; a single step
    // of more MBs than the bound is walked in MB ranges, merged between
    const int per = (int)std::min<int64_t>( MBT_MAX_STEPS, std::max<int64_t>( 1, MBT_ACC_MBS / mbc ) );
    uint32_t *acc = nullptr;
    const size_t plane = (size_t)mbc * sizeof( uint32_t );
    hipError_t e = scratch_alloc( (void **)&acc, 2 * std::min( per, n ) * plane, stream );
    if( e != hipSuccess )
        return e;
    const dim3 blk( 256 );
    for( int s0 = 0; s0 < n && e == hipSuccess; s0 += per )
    {
        const int cnt = std::min( per, n - s0 );
        MbtBatch b = {};
        MbtDsts d = {};
        int nd = 0;
        for( int k = 0; k < cnt; k++ )
        {
            const x264hip_mbtree_step_t &s = steps[s0 + k];
            MbtStep &o = b.s[k];
            o.intra = s.intra_cost; o.costs = s.lowres_costs; o.invq = s.inv_qscale; o.pin = s.propagate_in;
            o.fps = s.fps_factor; o.weight = s.bipred_weight;
            for( int l = 0; l < 2; l++ )
            {
                o.mv[l] = l && !s.mvs[1] ? nullptr : s.mvs[l];
                if( !o.mv[l] )
                    continue;
                int j = 0;
                while( j < nd && d.p[j] != s.ref_costs[l] )
                    j++;
                if( j == nd )
                    d.p[nd++] = s.ref_costs[l];
                o.acc[l] = j;
            }
        }
        const int64_t chunk = cnt == 1 ? std::min( mbc, MBT_ACC_MBS ) : mbc;
        for( int64_t m0 = 0; m0 < mbc && e == hipSuccess; m0 += chunk )
        {
            const int64_t m1 = std::min( mbc, m0 + chunk );
            e = hipMemsetAsync( acc, 0, nd * plane, stream );
            if( e != hipSuccess )
                break;
            mbtree_scatter_kernel<<<dim3( (unsigned)( ( m1 - m0 + 255 ) / 256 ), (unsigned)cnt ), blk, 0, stream>>>(
                b, acc, mbw, mbh, (int)m0, (int)m1 );
            mbtree_merge_kernel<<<dim3( (unsigned)( ( mbc + 255 ) / 256 ), (unsigned)nd ), blk, 0, stream>>>(
                d, acc, (int)mbc );
            e = hipGetLastError();
        }
    }
    const hipError_t ef = hipFreeAsync( acc, stream );
    return e != hipSuccess ? e : ef;
}

hipError_t launch_mbtree_finish( const uint16_t *intra, const uint16_t *invq, const uint16_t *prop, const float *aq,
                                 float *out, int mbc, int fps_factor, float weightdelta, float strength,
                                 hipStream_t stream )
{
    mbtree_finish_kernel<<<dim3( (unsigned)( ( mbc + 255 ) / 256 ) ), dim3( 256 ), 0, stream>>>(
        intra, invq, prop, aq, out, mbc, fps_factor, weightdelta, strength );
    return hipGetLastError();
}

} // namespace x264hip
