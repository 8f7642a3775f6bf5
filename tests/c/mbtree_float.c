/* TEST INFRASTRUCTURE: the float expression of MB-tree's propagate amount, restated in C so the
 * test can compile it the way the reference's C build is compiled (-O3 -ffast-math
 * -fno-tree-vectorize) and strictly (-O2 -ffp-contract=off) and compare both with the numpy
 * restatement (tests/mbtree_cases.py propagate_cost), which is the GPU kernels' contract.
 *
 * usage: mbtree_float IN OUT
 *   IN:  int32 n, int32 chunk, then uint16 propagate_in[n], intra[n], inter[n], inv_qscale[n],
 *        then float fps_factor[ceil(n / chunk)] (one per chunk of elements, as the reference passes
 *        one per MB row)
 *   OUT: int16 amount[n]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define COST_MASK ((1 << 14) - 1)

/* one row: the amount each MB passes on to its references */
__attribute__((noinline)) static void row_amounts( int16_t *amount, const uint16_t *propagate_in,
                                                   const uint16_t *intra_costs, const uint16_t *inter_costs,
                                                   const uint16_t *inv_qscales, const float *fps_factor, int len )
{
    float fps = *fps_factor;
    for( int i = 0; i < len; i++ )
    {
        int intra = intra_costs[i];
        int inter = inter_costs[i] & COST_MASK;
        if( inter > intra )
            inter = intra;
        float scaled_intra = intra * inv_qscales[i];
        float total = propagate_in[i] + scaled_intra * fps;
        float num = intra - inter;
        float denom = intra;
        int v = (int)(total * num / denom + 0.5f);
        amount[i] = v < 32767 ? v : 32767;
    }
}

static void *xread( FILE *f, size_t bytes )
{
    void *p = malloc( bytes ? bytes : 1 );
    if( !p || fread( p, 1, bytes, f ) != bytes )
    {
        fprintf( stderr, "mbtree_float: short input\n" );
        exit( 2 );
    }
    return p;
}

int main( int argc, char **argv )
{
    if( argc != 3 )
        return 2;
    FILE *in = fopen( argv[1], "rb" );
    if( !in )
        return 2;
    int32_t hdr[2];
    if( fread( hdr, sizeof(hdr), 1, in ) != 1 || hdr[0] < 1 || hdr[1] < 1 )
        return 2;
    const int n = hdr[0], chunk = hdr[1], nchunks = (n + chunk - 1) / chunk;
    uint16_t *pin = xread( in, (size_t)n * 2 ), *intra = xread( in, (size_t)n * 2 );
    uint16_t *inter = xread( in, (size_t)n * 2 ), *invq = xread( in, (size_t)n * 2 );
    float *fps = xread( in, (size_t)nchunks * sizeof(float) );
    fclose( in );
    int16_t *amount = malloc( (size_t)n * 2 );
    if( !amount )
        return 2;
    for( int c = 0; c < nchunks; c++ )
    {
        const int o = c * chunk, len = n - o < chunk ? n - o : chunk;
        row_amounts( amount + o, pin + o, intra + o, inter + o, invq + o, fps + c, len );
    }
    FILE *out = fopen( argv[2], "wb" );
    if( !out || fwrite( amount, 2, (size_t)n, out ) != (size_t)n || fclose( out ) )
        return 2;
    free( pin ); free( intra ); free( inter ); free( invq ); free( fps ); free( amount );
    return 0;
}
