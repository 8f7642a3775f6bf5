// Device cores of the intra predictors shared by intra.hip (the prediction costs) and mbintra.hip
// (the intra macroblock encode): the two rounding filters of common/predict.c:531-532 and the 8x8
// directional modes on the filtered edge.
#pragma once
#include "hipcommon.h"

namespace x264hip {

__device__ __forceinline__ int f1( int a, int b ) { return (a + b + 1) >> 1; }
__device__ __forceinline__ int f2( int a, int b, int c ) { return (a + 2 * b + c + 2) >> 2; }

// ------------------------------------------------------------- 8x8 directional modes
// predict_8x8 modes 3..8 on the filtered edge e[] (e[7..14] = l7..l0, e[15] = lt,
// e[16..32] = t0..t15, t15) in closed form; oracle.c pred8x8_px is the same
// restatement, pinned to predict.c:741-883 by tests/golden/intra8x8_golden.npz.
// E: anything indexable, registers (x and y compile-time constants) or shared memory.
template <int MODE, typename E>
__device__ __forceinline__ int pred8_dir( const E &e, int x, int y )
{
    if constexpr( MODE == 3 )   // DDL
    {
        const int z = x + y;
        return f2( e[16 + z], e[17 + z], e[16 + (z + 2 < 15 ? z + 2 : 15)] );
    }
    else if constexpr( MODE == 4 )   // DDR
    {
        const int c = x > y ? 15 + x - y : 15 - (y - x);
        return f2( e[c - 1], e[c], e[c + 1] );
    }
    else if constexpr( MODE == 5 )   // VR
    {
        const int z = 2 * x - y;
        if( z < 0 )
            return f2( e[15 + z], e[16 + z], e[17 + z] );
        if( !(z & 1) )
            return f1( e[15 + z / 2], e[16 + z / 2] );
        const int c = 15 + (z + 1) / 2;
        return f2( e[c - 1], e[c], e[c + 1] );
    }
    else if constexpr( MODE == 6 )   // HD
    {
        const int z = 2 * y - x;
        if( z < 0 )
            return f2( e[13 - z], e[14 - z], e[15 - z] );
        if( !(z & 1) )
            return f1( e[15 - z / 2], e[14 - z / 2] );
        const int c = 15 - (z + 1) / 2;
        return f2( e[c - 1], e[c], e[c + 1] );
    }
    else if constexpr( MODE == 7 )   // VL
    {
        const int c = 16 + x + (y >> 1);
        return (y & 1) ? f2( e[c], e[c + 1], e[c + 2] ) : f1( e[c], e[c + 1] );
    }
    else   // HU
    {
        const int z = x + 2 * y;
        if( z > 13 )
            return e[7];
        if( z == 13 )
            return f2( e[8], e[7], e[7] );
        const int c = 14 - (z >> 1);
        return (z & 1) ? f2( e[c], e[c - 1], e[c - 2] ) : f1( e[c], e[c - 1] );
    }
}

} // namespace x264hip
