// The per-bit-depth extern "C" entries and the argument validation of the public ABI.  Not a
// translation unit: capi.cpp includes this file twice, with BD defined as the literal 8 and then
// 10, the way x264 compiles its own sources once per bit depth.  BD_NAME( f ) is x264hip_<BD>_f;
// everything else used here is defined in capi.cpp above the include.

// ---- x264hip_me_bind: the SAD table the per-call pixel entries answer from
extern "C" int BD_NAME( me_bind_tables )( const PT<BD>::pixel *fenc, const PT<BD>::pixel *ref,
                                          intptr_t stride, int mb_width, int mb_height,
                                          const PT<BD>::sadt *table, const uint16_t *table8, int range )
{
    if( !fenc || !ref || !( table || table8 ) || mb_width <= 0 || mb_height <= 0 ||
        range < 1 || range > 29 || stride < 16 * (intptr_t)mb_width + 2 * BIND_PAD )
        return X264HIP_EINVAL;
    MeBind &b = t_bind;
    b.table8 = table8;
    b.bd = BD;
    b.fenc = (const uint8_t *)fenc;
    b.ref = (const uint8_t *)ref;
    b.stride = stride;
    b.mbw = mb_width;
    b.mbh = mb_height;
    b.R = range;
    b.pitch = (2 * range + 1 + 3) & ~3;
    b.table = table;
    return X264HIP_OK;
}

extern "C" int BD_NAME( me_bind )( const PT<BD>::pixel *fenc, const PT<BD>::pixel *ref, intptr_t stride,
                                   int mb_width, int mb_height, const PT<BD>::sadt *table, int range )
{
    if( !table )
        return X264HIP_EINVAL;
    return BD_NAME( me_bind_tables )( fenc, ref, stride, mb_width, mb_height, table, nullptr, range );
}

// Table initialisers.  Both forms only OVERRIDE: the entries this backend
// implements are replaced, every other entry (the trellis entries, intra_*_x9_*, the
// never-initialised ssim[7], and the encoder's mbcmp / fpelcmp aliases) keeps what the caller's
// C init put there.  Without a usable gfx950 device (or without X264HIP_CPU_HIP in
// `cpu` for the flag form) the table is left untouched, so a host without the GPU
// keeps its C entries, the convention of reference common/opencl.c:400-409; no
// entry that could reach a missing device is ever installed.
extern "C" void BD_NAME( pixel_init_hip )( BD_NAME( pixel_function_t ) *pixf )
{
    if( pixf && x264hip_available() )
    {
        fill_pixel<BD>( pixf );
        note_fill();
    }
}

extern "C" void BD_NAME( pixel_init )( uint32_t cpu, BD_NAME( pixel_function_t ) *pixf )
{
    if( cpu & X264HIP_CPU_HIP )
        BD_NAME( pixel_init_hip )( pixf );
}

extern "C" void BD_NAME( dct_init_hip )( BD_NAME( dct_function_t ) *d )
{
    if( d && x264hip_available() )
        fill_dct<BD>( d );
}

extern "C" void BD_NAME( dct_init )( uint32_t cpu, BD_NAME( dct_function_t ) *d )
{
    if( cpu & X264HIP_CPU_HIP )
        BD_NAME( dct_init_hip )( d );
}

extern "C" void BD_NAME( quant_init_hip )( BD_NAME( quant_function_t ) *q )
{
    if( q && x264hip_available() )
        fill_quant<BD>( q );
}

extern "C" void BD_NAME( quant_init )( void *h, uint32_t cpu, BD_NAME( quant_function_t ) *q )
{
    (void)h;
    if( cpu & X264HIP_CPU_HIP )
        BD_NAME( quant_init_hip )( q );
}

extern "C" void BD_NAME( zigzag_init_hip )( BD_NAME( zigzag_function_t ) *p,
                                            BD_NAME( zigzag_function_t ) *i )
{
    if( p && i && x264hip_available() )
        fill_zigzag<BD>( p, i );
}

extern "C" void BD_NAME( zigzag_init )( uint32_t cpu, BD_NAME( zigzag_function_t ) *p,
                                        BD_NAME( zigzag_function_t ) *i )
{
    if( cpu & X264HIP_CPU_HIP )
        BD_NAME( zigzag_init_hip )( p, i );
}

extern "C" int BD_NAME( cqm_init )( const uint8_t *const sl[8], int dz_inter, int dz_intra, int b8,
                                    PT<BD>::udctcoef *q4m, PT<BD>::udctcoef *q4b, PT<BD>::udctcoef *q8m,
                                    PT<BD>::udctcoef *q8b )
{
    return cqm_init<BD>( sl, dz_inter, dz_intra, b8 ? 2 : 0, q4m, q4b, q8m, q8b );
}

extern "C" int BD_NAME( pixel_cmp_batch )( int op, int i_pixel, const PT<BD>::pixel *fenc, intptr_t fs,
                                           const PT<BD>::pixel *ref, intptr_t rs, const int64_t *fo,
                                           const int64_t *ro, int n, int32_t *scores, void *stream )
{
    if( op < 0 || op > 3 || i_pixel < 0 || i_pixel > 7 || n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_cmp_batch<BD>( op, i_pixel, fenc, fs, ref, rs, fo, ro, n, scores,
                                          (hipStream_t)stream ), "pixel_cmp_batch" );
}

extern "C" int BD_NAME( pixel_stat_batch )( int op, int i_pixel, const PT<BD>::pixel *p1, intptr_t s1,
                                            const PT<BD>::pixel *p2, intptr_t s2, const int64_t *o1,
                                            const int64_t *o2, int height, int n, uint64_t *out,
                                            void *stream )
{
    if( op < 0 || op > 4 || n < 0 || ( (op == 3 || op == 4) && height < 0 ) )
        return X264HIP_EINVAL;
    return map_err( launch_stat_batch<BD>( op, i_pixel, p1, s1, p2, s2, o1, o2, height, n, out,
                                           (hipStream_t)stream ), "pixel_stat_batch" );
}

extern "C" int BD_NAME( var2_batch )( int i_pixel, const PT<BD>::pixel *fenc, intptr_t fs, intptr_t fvd,
                                      const PT<BD>::pixel *fdec, intptr_t ds, intptr_t dvd,
                                      const int64_t *fo, const int64_t *dof, int n, int32_t *out,
                                      void *stream )
{
    if( n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_var2_batch<BD>( i_pixel, fenc, fs, fvd, fdec, ds, dvd, fo, dof, n, out,
                                           (hipStream_t)stream ), "var2_batch" );
}

extern "C" int BD_NAME( ads_batch )( int i_pixel, const int32_t *enc_dc, const uint16_t *sums, int delta,
                                     const int64_t *sums_off, const uint16_t *cost, const int64_t *cost_off,
                                     const int32_t *width, const int32_t *thresh, int n, int16_t *mvs,
                                     int mvs_pitch, int32_t *nmv, void *stream )
{
    if( i_pixel < 0 || i_pixel > 6 || n < 0 || mvs_pitch < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_ads_batch( i_pixel, enc_dc, sums, delta, sums_off, cost, cost_off, width, thresh, n,
                                      mvs, mvs_pitch, nmv, (hipStream_t)stream ), "ads_batch" );
}

extern "C" int BD_NAME( intra_cmp_x3_batch )( int kind, int op, const PT<BD>::pixel *fenc, intptr_t fs,
                                              const PT<BD>::pixel *fdec, intptr_t ds, const int64_t *fo,
                                              const int64_t *dof, int n, int32_t *scores, void *stream )
{
    const bool ok = kind >= 0 && kind <= 4 &&
                    ( op == X264HIP_CMP_SAD || ( kind == 4 ? op == X264HIP_CMP_SA8D : op == X264HIP_CMP_SATD ) );
    if( !ok || n < 0 || ( n > 0 && ( !fenc || !fdec || !fo || !dof || !scores ) ) )
        return X264HIP_EINVAL;
    return map_err( launch_intra_x3<BD>( kind, op, fenc, fs, fdec, ds, fo, dof, n, scores,
                                         (hipStream_t)stream ), "intra_cmp_x3_batch" );
}

extern "C" int BD_NAME( lowres_intra_cost )( const PT<BD>::pixel *plane, intptr_t stride, intptr_t fstride,
                                             int mbw, int mbh, int nframes, int satd, int all_modes,
                                             int lambda, const uint16_t *invq, uint16_t *cost,
                                             int32_t *row_satd, int32_t *est, void *stream )
{
    if( mbw < 0 || mbh < 0 || nframes < 0 || lambda < 0 || ( (uintptr_t)plane & 3 ) ||
        ( ( stride * (intptr_t)sizeof(PT<BD>::pixel) ) & 3 ) ||
        ( ( fstride * (intptr_t)sizeof(PT<BD>::pixel) ) & 3 ) || stride < 8 * mbw + 64 ||
        ( (int64_t)mbw * mbh * nframes > 0 && ( !plane || !cost ) ) )
        return X264HIP_EINVAL;
    return map_err( launch_lowres_intra<BD>( plane, stride, fstride, mbw, mbh, nframes, satd, all_modes, lambda,
                                             invq, cost, row_satd, est, (hipStream_t)stream ),
                    "lowres_intra_cost" );
}

extern "C" int BD_NAME( lowres_inter_cost_ex )(
    const PT<BD>::pixel *fenc, intptr_t ffs, const PT<BD>::pixel *rf, const PT<BD>::pixel *rh,
    const PT<BD>::pixel *rv, const PT<BD>::pixel *rc, intptr_t stride, intptr_t rfs, int mbw, int mbh,
    int npairs, int me_method, int subme, int satd, int me_range, int mv_range, int lambda,
    const uint16_t *cost_mv, const uint16_t *intra_cost, const uint16_t *invq, int16_t *mvs, int32_t *mv_costs,
    uint16_t *lowres_costs, int32_t *row_satd, int32_t *est, const PT<BD>::pixel *ref_w, int w_scale,
    int w_denom, int w_offset, int n_slices, void *stream )
{
    if( n_slices < 1 || n_slices > 256 )
        return X264HIP_EINVAL;
    const intptr_t pb = (intptr_t)sizeof( PT<BD>::pixel );
    if( mbw < 0 || mbh < 0 || npairs < 0 || ( me_method != 0 && me_method != 1 ) ||
        ( subme != 2 && subme != 4 ) || me_range < 1 || mv_range < 1 || lambda < 0 ||
        ( (uintptr_t)fenc & 3 ) || ( ( stride * pb ) & 3 ) || ( ( ffs * pb ) & 3 ) ||
        stride < 8 * mbw + 64 ||
        ( ref_w && ( w_denom < 0 || w_denom > 7 || w_scale < -128 || w_scale > 127 || w_offset < -128 ||
                     w_offset > 127 ) ) ||
        ( (int64_t)mbw * mbh * npairs > 0 &&
          ( !fenc || !rf || !rh || !rv || !rc || !cost_mv || !intra_cost || !mvs || !mv_costs ||
            !lowres_costs ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *ref[4] = { rf, rh, rv, rc };
    return map_err( launch_lowres_inter<BD>( fenc, ffs, ref, stride, rfs, mbw, mbh, npairs, me_method, subme,
                                             satd, me_range, mv_range, lambda, cost_mv, intra_cost, invq, mvs,
                                             mv_costs, lowres_costs, row_satd, est, ref_w, w_scale, w_denom,
                                             w_offset, n_slices, (hipStream_t)stream ),
                    "lowres_inter_cost" );
}

extern "C" int BD_NAME( lowres_inter_cost )(
    const PT<BD>::pixel *fenc, intptr_t ffs, const PT<BD>::pixel *rf, const PT<BD>::pixel *rh,
    const PT<BD>::pixel *rv, const PT<BD>::pixel *rc, intptr_t stride, intptr_t rfs, int mbw, int mbh,
    int npairs, int me_method, int subme, int satd, int me_range, int mv_range, int lambda,
    const uint16_t *cost_mv, const uint16_t *intra_cost, const uint16_t *invq, int16_t *mvs, int32_t *mv_costs,
    uint16_t *lowres_costs, int32_t *row_satd, int32_t *est, void *stream )
{
    return BD_NAME( lowres_inter_cost_ex )( fenc, ffs, rf, rh, rv, rc, stride, rfs, mbw, mbh, npairs,
                                            me_method, subme, satd, me_range, mv_range, lambda, cost_mv,
                                            intra_cost, invq, mvs, mv_costs, lowres_costs, row_satd, est,
                                            nullptr, 0, 0, 0, 1, stream );
}

extern "C" int BD_NAME( weight_scale_plane )( PT<BD>::pixel *dst, intptr_t ds, intptr_t dfs,
                                              const PT<BD>::pixel *src, intptr_t ss, intptr_t sfs,
                                              int width, int height, int nframes, int scale, int denom,
                                              int offset, void *stream )
{
    if( width < 0 || height < 0 || nframes < 0 || denom < 0 || denom > 7 || scale < -128 || scale > 127 ||
        offset < -128 || offset > 127 ||
        ( (int64_t)width * height * nframes > 0 && ( !dst || !src || dst == src ) ) )
        return X264HIP_EINVAL;
    return map_err( launch_weight_plane<BD>( dst, ds, dfs, src, ss, sfs, width, height, nframes, scale, denom,
                                             offset, (hipStream_t)stream ),
                    "weight_scale_plane" );
}

extern "C" int BD_NAME( lowres_bidir_cost_ex )(
    const PT<BD>::pixel *fenc, intptr_t ffs, const PT<BD>::pixel *af, const PT<BD>::pixel *ah,
    const PT<BD>::pixel *av, const PT<BD>::pixel *ac, intptr_t afs, const PT<BD>::pixel *bf,
    const PT<BD>::pixel *bh, const PT<BD>::pixel *bv, const PT<BD>::pixel *bc, intptr_t bfs, intptr_t stride,
    int mbw, int mbh, int n, int me_method, int subme, int satd, int me_range, int mv_range, int lambda,
    const uint16_t *cost_mv, int search, int16_t *mvs0, int32_t *costs0, int16_t *mvs1, int32_t *costs1,
    const int16_t *p1mvs, int dsf, int weight, const uint16_t *invq, uint16_t *lowres_costs, int32_t *row_satd,
    int32_t *est, int n_slices, void *stream )
{
    const intptr_t pb = (intptr_t)sizeof( PT<BD>::pixel );
    if( n_slices < 1 || n_slices > 256 )
        return X264HIP_EINVAL;
    if( mbw < 0 || mbh < 0 || n < 0 || ( me_method != 0 && me_method != 1 ) || ( subme != 2 && subme != 4 ) ||
        me_range < 1 || mv_range < 1 || lambda < 0 || search < 0 || search > 3 || weight < 0 || weight > 64 ||
        ( (uintptr_t)fenc & 3 ) || ( ( stride * pb ) & 3 ) || ( ( ffs * pb ) & 3 ) || stride < 8 * mbw + 64 ||
        ( (int64_t)mbw * mbh * n > 0 && ( !fenc || !af || !ah || !av || !ac || !bf || !bh || !bv || !bc ||
                                          !cost_mv || !mvs0 || !costs0 || !mvs1 || !costs1 || !lowres_costs ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *ra[4] = { af, ah, av, ac }, *rb[4] = { bf, bh, bv, bc };
    return map_err( launch_lowres_bidir<BD>( fenc, ffs, ra, afs, rb, bfs, stride, mbw, mbh, n, me_method, subme,
                                             satd, me_range, mv_range, lambda, cost_mv, search, mvs0, costs0,
                                             mvs1, costs1, p1mvs, dsf, weight, invq, lowres_costs, row_satd,
                                             est, n_slices, (hipStream_t)stream ),
                    "lowres_bidir_cost" );
}

extern "C" int BD_NAME( lowres_bidir_cost )(
    const PT<BD>::pixel *fenc, intptr_t ffs, const PT<BD>::pixel *af, const PT<BD>::pixel *ah,
    const PT<BD>::pixel *av, const PT<BD>::pixel *ac, intptr_t afs, const PT<BD>::pixel *bf,
    const PT<BD>::pixel *bh, const PT<BD>::pixel *bv, const PT<BD>::pixel *bc, intptr_t bfs, intptr_t stride,
    int mbw, int mbh, int n, int me_method, int subme, int satd, int me_range, int mv_range, int lambda,
    const uint16_t *cost_mv, int search, int16_t *mvs0, int32_t *costs0, int16_t *mvs1, int32_t *costs1,
    const int16_t *p1mvs, int dsf, int weight, const uint16_t *invq, uint16_t *lowres_costs, int32_t *row_satd,
    int32_t *est, void *stream )
{
    return BD_NAME( lowres_bidir_cost_ex )( fenc, ffs, af, ah, av, ac, afs, bf, bh, bv, bc, bfs, stride,
                                            mbw, mbh, n, me_method, subme, satd, me_range, mv_range,
                                            lambda, cost_mv, search, mvs0, costs0, mvs1, costs1, p1mvs, dsf,
                                            weight, invq, lowres_costs, row_satd, est, 1, stream );
}

extern "C" int BD_NAME( frame_integral )( const PT<BD>::pixel *plane, intptr_t stride, intptr_t fstride,
                                          int lines, int padh, int sub8x8, int nframes, uint16_t *integral,
                                          intptr_t ifstride, void *stream )
{
    if( lines <= 0 || nframes < 0 || padh < 0 || stride < padh + 16 )
        return X264HIP_EINVAL;
    return map_err( launch_frame_integral<BD>( plane, stride, fstride, lines, padh, sub8x8, nframes, integral,
                                               ifstride, (hipStream_t)stream ), "frame_integral" );
}

extern "C" int BD_NAME( me_search_full )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                          const PT<BD>::pixel *ref, intptr_t rs, intptr_t rfs, int mbw,
                                          int mbh, int nframes, int range, PT<BD>::sadt *table,
                                          void *stream )
{
    if( mbw < 0 || mbh < 0 || nframes < 0 || !( range == 4 || range == 8 || range == 16 || range == 24 ) )
        return X264HIP_EINVAL;
    return map_err( launch_me_full<BD>( fenc, fs, ffs, ref, rs, rfs, mbw, mbh, nframes, range, table, nullptr,
                                        nullptr, (hipStream_t)stream ), "me_search_full" );
}

extern "C" int BD_NAME( me_search_centred )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                             const PT<BD>::pixel *ref, intptr_t rs, intptr_t rfs, int mbw,
                                             int mbh, int nframes, int range, const int16_t *centre,
                                             PT<BD>::sadt *table, int16_t *origin, void *stream )
{
    if( mbw < 0 || mbh < 0 || nframes < 0 || !centre || !origin ||
        !( range == 4 || range == 8 || range == 16 || range == 24 ) )
        return X264HIP_EINVAL;
    return map_err( launch_me_full<BD>( fenc, fs, ffs, ref, rs, rfs, mbw, mbh, nframes, range, table, centre,
                                        origin, (hipStream_t)stream ), "me_search_centred" );
}

extern "C" int BD_NAME( me_search_full8 )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                           const PT<BD>::pixel *ref, intptr_t rs, intptr_t rfs, int mbw,
                                           int mbh, int nframes, int range, uint16_t *table8,
                                           void *stream )
{
    if( mbw < 0 || mbh < 0 || nframes < 0 ||
        !( range == 4 || range == 8 || range == 16 || range == 24 ) ||
        ( (int64_t)mbw * mbh * nframes > 0 && ( !fenc || !ref || !table8 ) ) )
        return X264HIP_EINVAL;
    return map_err( launch_me_full8<BD>( fenc, fs, ffs, ref, rs, rfs, mbw, mbh, nframes, range, table8,
                                         (hipStream_t)stream ), "me_search_full8" );
}

extern "C" int BD_NAME( me_esa_argmin )( const PT<BD>::sadt *table, int range, int n, int me_range,
                                         const int16_t *par, const int32_t *init_cost,
                                         const uint16_t *cost_mv, int32_t *out, void *stream )
{
    if( range < 1 || range > 29 || n < 0 || me_range < 0 || 2 * me_range + 4 > 64 )
        return X264HIP_EINVAL;
    return map_err( launch_me_esa_argmin<BD>( table, range, n, me_range, nullptr, par, init_cost, cost_mv, out,
                                              (hipStream_t)stream ), "me_esa_argmin" );
}

extern "C" int BD_NAME( me_esa_argmin_at )( const PT<BD>::sadt *table, int range, int n, int me_range,
                                            const int16_t *origin, const int16_t *par,
                                            const int32_t *init_cost, const uint16_t *cost_mv, int32_t *out,
                                            void *stream )
{
    if( range < 1 || range > 29 || n < 0 || me_range < 0 || 2 * me_range + 4 > 64 || !origin ||
        range < me_range )
        return X264HIP_EINVAL;
    return map_err( launch_me_esa_argmin<BD>( table, range, n, me_range, origin, par, init_cost, cost_mv, out,
                                              (hipStream_t)stream ), "me_esa_argmin_at" );
}

extern "C" int BD_NAME( ssd_plane_batch )( const PT<BD>::pixel *pix1, intptr_t s1, intptr_t f1,
                                           const PT<BD>::pixel *pix2, intptr_t s2, intptr_t f2, int width,
                                           int height, int nframes, uint64_t *ssd, void *stream )
{
    if( width < 0 || height < 0 || nframes < 0 || (nframes && (!pix1 || !pix2 || !ssd)) )
        return X264HIP_EINVAL;
    return map_err( launch_plane_ssd<BD>( 0, pix1, s1, f1, pix2, s2, f2, width, height, nframes, ssd,
                                          (hipStream_t)stream ), "ssd_plane_batch" );
}

extern "C" int BD_NAME( ssd_nv12_batch )( const PT<BD>::pixel *pix1, intptr_t s1, intptr_t f1,
                                          const PT<BD>::pixel *pix2, intptr_t s2, intptr_t f2, int width,
                                          int height, int nframes, uint64_t *ssd_uv, void *stream )
{
    if( width < 0 || height < 0 || nframes < 0 || (nframes && (!pix1 || !pix2 || !ssd_uv)) )
        return X264HIP_EINVAL;
    return map_err( launch_plane_ssd<BD>( 1, pix1, s1, f1, pix2, s2, f2, width, height, nframes, ssd_uv,
                                          (hipStream_t)stream ), "ssd_nv12_batch" );
}

extern "C" int BD_NAME( me_search_esa )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                         const PT<BD>::pixel *ref, intptr_t rs, intptr_t rfs, int mbw,
                                         int mbh, int nframes, int range, int me_range, const int16_t *par,
                                         const int32_t *init_cost, const uint16_t *cost_mv, int32_t *out,
                                         void *stream )
{
    if( mbw < 0 || mbh < 0 || nframes < 0 || !( range == 4 || range == 8 || range == 16 || range == 24 ) ||
        me_range < 0 || 2 * me_range + 4 > 64 || range < me_range ||
        ((int64_t)nframes * mbw * mbh && (!par || !init_cost || !cost_mv || !out)) )
        return X264HIP_EINVAL;
    return map_err( launch_me_search_esa<BD>( fenc, fs, ffs, ref, rs, rfs, mbw, mbh, nframes, range, me_range,
                                              par, init_cost, cost_mv, out, (hipStream_t)stream ),
                    "me_search_esa" );
}

extern "C" int BD_NAME( me_search_esa8 )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                          const PT<BD>::pixel *ref, intptr_t rs, intptr_t rfs, int mbw,
                                          int mbh, int nframes, int range, int me_range,
                                          const int16_t *centre, const int16_t *par,
                                          const int32_t *init_cost, const uint16_t *cost_mv, int32_t *out,
                                          void *stream )
{
    if( mbw < 0 || mbh < 0 || nframes < 0 ||
        !( range == 0 || range == 4 || range == 8 || range == 16 || range == 24 ) || me_range < 0 ||
        2 * me_range + 4 > 64 || ((int64_t)nframes * mbw * mbh && (!fenc || !ref || !par || !init_cost ||
                                                                   !cost_mv || !out)) )
        return X264HIP_EINVAL;
    return map_err( launch_me_search_esa8<BD>( fenc, fs, ffs, ref, rs, rfs, mbw, mbh, nframes, range, me_range,
                                               centre, par, init_cost, cost_mv, out, (hipStream_t)stream ),
                    "me_search_esa8" );
}

extern "C" int BD_NAME( me_tesa )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                   const PT<BD>::pixel *ref, intptr_t rs, intptr_t rfs,
                                   const uint16_t *integral, intptr_t ifs, int mbw, int mbh, int nframes,
                                   int me_range, int satd, const PT<BD>::sadt *table, int range,
                                   const int16_t *origin, const int16_t *par, const int32_t *init_cost,
                                   const uint16_t *cost_mv, int32_t *out, void *stream )
{
    if( mbw < 0 || mbh < 0 || nframes < 0 || me_range < 1 || me_range > 32 || !fenc || !ref || !integral ||
        !par || !init_cost || !cost_mv || !out || ((uintptr_t)fenc & 3) || ((fs * sizeof( PT<BD>::pixel )) & 3) ||
        (table && (range < 1 || range > 29)) )
        return X264HIP_EINVAL;
    return map_err( launch_me_tesa<BD>( fenc, fs, ffs, ref, rs, rfs, integral, ifs, mbw, mbh, nframes, me_range,
                                        satd, table, range, origin, par, init_cost, cost_mv, out,
                                        (hipStream_t)stream ), "me_tesa" );
}

extern "C" int BD_NAME( hpel_filter )( const PT<BD>::pixel *src, PT<BD>::pixel *dh, PT<BD>::pixel *dv,
                                       PT<BD>::pixel *dc, intptr_t stride, intptr_t fstride, int width,
                                       int height, int nframes, void *stream )
{
    if( width <= 0 || height <= 0 || nframes < 0 || (width | height) & 15 )
        return X264HIP_EINVAL;
    return map_err( launch_hpel_filter<BD>( src, dh, dv, dc, stride, fstride, width, height, nframes,
                                            (hipStream_t)stream ), "hpel_filter" );
}

extern "C" int BD_NAME( subpel_cmp_batch )( int op, int i_pixel, const PT<BD>::pixel *fenc, intptr_t fs,
                                            const PT<BD>::pixel *p0, const PT<BD>::pixel *p1,
                                            const PT<BD>::pixel *p2, const PT<BD>::pixel *p3, intptr_t rs,
                                            const int64_t *fo, const int32_t *qxy, int n, int32_t *scores,
                                            void *stream )
{
    if( ( op != X264HIP_CMP_SAD && op != X264HIP_CMP_SATD ) || i_pixel < 0 || i_pixel > 7 || n < 0 )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *planes[4] = { p0, p1, p2, p3 };
    return map_err( launch_subpel_cmp<BD>( op, i_pixel, fenc, fs, planes, rs, fo, qxy, n, scores,
                                           (hipStream_t)stream ), "subpel_cmp_batch" );
}

extern "C" int BD_NAME( subpel_qpel9_batch )( int op, int i_pixel, const PT<BD>::pixel *fenc, intptr_t fs,
                                              const PT<BD>::pixel *p0, const PT<BD>::pixel *p1,
                                              const PT<BD>::pixel *p2, const PT<BD>::pixel *p3, intptr_t rs,
                                              const int64_t *fo, const int32_t *cxy, int n, int32_t *scores,
                                              void *stream )
{
    if( ( op != X264HIP_CMP_SAD && op != X264HIP_CMP_SATD ) || i_pixel < 0 || i_pixel > 3 || n < 0 ||
        ( n > 0 && ( !fenc || !p0 || !p1 || !p2 || !p3 || !fo || !cxy || !scores ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *planes[4] = { p0, p1, p2, p3 };
    return map_err( launch_subpel_qpel9<BD>( op, i_pixel, fenc, fs, planes, rs, fo, cxy, n, scores,
                                             (hipStream_t)stream ), "subpel_qpel9_batch" );
}

extern "C" int BD_NAME( me_refine_subpel )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                            const PT<BD>::pixel *p0, const PT<BD>::pixel *p1,
                                            const PT<BD>::pixel *p2, const PT<BD>::pixel *p3, intptr_t rs,
                                            intptr_t rfs, int i_pixel, int subme, int refine_qpel,
                                            int fpel_satd, const int32_t *pos, const int16_t *par,
                                            const int32_t *init_cost, const uint16_t *cost_mv, int n,
                                            int32_t *out, int32_t *nevals, void *stream )
{
    if( i_pixel < 0 || i_pixel > 6 || subme < 1 || subme > 11 || n < 0 ||
        ( n > 0 && ( !fenc || !p0 || !p1 || !p2 || !p3 || !pos || !par || !init_cost || !cost_mv || !out ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *planes[4] = { p0, p1, p2, p3 };
    return map_err( launch_me_refine_subpel<BD>( fenc, fs, ffs, planes, rs, rfs, i_pixel, subme, !!refine_qpel,
                                                 fpel_satd, pos, par, init_cost, cost_mv, n, out, nevals,
                                                 nullptr, nullptr, nullptr, (hipStream_t)stream ),
                    "me_refine_subpel" );
}

extern "C" int BD_NAME( me_refine_subpel_ex )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                               const PT<BD>::pixel *p0, const PT<BD>::pixel *p1,
                                               const PT<BD>::pixel *p2, const PT<BD>::pixel *p3,
                                               intptr_t rs, intptr_t rfs, int i_pixel, int subme,
                                               int refine_qpel, int fpel_satd, const int32_t *pos,
                                               const int16_t *par, const int32_t *init_cost,
                                               const uint16_t *cost_mv, int n, int32_t *out,
                                               int32_t *nevals, const x264hip_refine_ext_t *ext,
                                               void *stream )
{
    if( i_pixel < 0 || i_pixel > 6 || subme < 1 || subme > 11 || n < 0 ||
        ( n > 0 && ( !fenc || !p0 || !p1 || !p2 || !p3 || !pos || !par || !init_cost || !cost_mv || !out ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *planes[4] = { p0, p1, p2, p3 };
    return map_err( launch_me_refine_subpel<BD>( fenc, fs, ffs, planes, rs, rfs, i_pixel, subme, !!refine_qpel,
                                                 fpel_satd, pos, par, init_cost, cost_mv, n, out, nevals,
                                                 nullptr, nullptr, ext, (hipStream_t)stream ),
                    "me_refine_subpel_ex" );
}

extern "C" int BD_NAME( me_refine_qpel_refdupe )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                                  const PT<BD>::pixel *p0, const PT<BD>::pixel *p1,
                                                  const PT<BD>::pixel *p2, const PT<BD>::pixel *p3,
                                                  intptr_t rs, intptr_t rfs, int i_pixel, int subme,
                                                  int fpel_satd, const int32_t *pos, const int16_t *par,
                                                  const int32_t *init_cost, const uint16_t *cost_mv, int n,
                                                  int32_t *out, int32_t *nevals, int32_t *halfpel_thresh,
                                                  const int32_t *ref_cost, const x264hip_refine_ext_t *ext,
                                                  void *stream )
{
    if( i_pixel < 0 || i_pixel > 6 || subme < 1 || subme > 11 || n < 0 ||
        ( n > 0 && ( !fenc || !p0 || !p1 || !p2 || !p3 || !pos || !par || !init_cost || !cost_mv || !out ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *planes[4] = { p0, p1, p2, p3 };
    return map_err( launch_me_refine_subpel<BD>( fenc, fs, ffs, planes, rs, rfs, i_pixel, subme, 2, fpel_satd,
                                                 pos, par, init_cost, cost_mv, n, out, nevals, halfpel_thresh,
                                                 ref_cost, ext, (hipStream_t)stream ),
                    "me_refine_qpel_refdupe" );
}

extern "C" int BD_NAME( me_search_ref )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                         const PT<BD>::pixel *fw, const PT<BD>::pixel *p0,
                                         const PT<BD>::pixel *p1, const PT<BD>::pixel *p2,
                                         const PT<BD>::pixel *p3, intptr_t rs, intptr_t rfs, int i_pixel,
                                         int me_method, int subme, int me_range, const int32_t *pos,
                                         const int16_t *par, const int16_t *mvc, const uint16_t *cost_mv,
                                         int n, int32_t *out, int32_t *nevals,
                                         const x264hip_refine_ext_t *ext, void *stream )
{
    if( n < 0 || ( n > 0 && ( !fenc || !fw || !p0 || !p1 || !p2 || !p3 || !pos || !par || !mvc || !cost_mv ||
                              !out ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *planes[4] = { p0, p1, p2, p3 };
    return map_err( launch_me_search_ref<BD>( fenc, fs, ffs, fw, planes, rs, rfs, i_pixel, me_method, subme,
                                              me_range, pos, par, mvc, cost_mv, n, out, nevals, nullptr,
                                              nullptr, ext, (hipStream_t)stream ), "me_search_ref" );
}

extern "C" int BD_NAME( me_analyse_p16x16 )(
    const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs, const PT<BD>::pixel *fw, const PT<BD>::pixel *p0,
    const PT<BD>::pixel *p1, const PT<BD>::pixel *p2, const PT<BD>::pixel *p3, intptr_t rs, intptr_t rfs,
    int mbw, int mbh, int nframes, int me_method, int subme, int me_range, int mv_range,
    const int16_t *lowres_mv, const int16_t *ref_mv, int ref_mv_scale, const uint16_t *cost_mv, int32_t *out,
    int32_t *nevals, const x264hip_refine_ext_t *ext, void *stream )
{
    if( mbw < 0 || mbh < 0 || nframes < 0 || mv_range < 1 || mv_range > 8192 ||
        ( (int64_t)mbw * mbh * nframes > 0 && ( !fenc || !fw || !p0 || !p1 || !p2 || !p3 || !cost_mv || !out ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *planes[4] = { p0, p1, p2, p3 };
    return map_err( launch_me_analyse_p16x16<BD>( fenc, fs, ffs, fw, planes, rs, rfs, mbw, mbh, nframes,
                                                  me_method, subme, me_range, mv_range, lowres_mv, ref_mv,
                                                  ref_mv_scale, cost_mv, out, nevals, ext, (hipStream_t)stream ),
                    "me_analyse_p16x16" );
}

extern "C" int BD_NAME( me_refine_bidir_satd )(
    const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs, const PT<BD>::pixel *l0f, const PT<BD>::pixel *l0h,
    const PT<BD>::pixel *l0v, const PT<BD>::pixel *l0c, const PT<BD>::pixel *l1f, const PT<BD>::pixel *l1h,
    const PT<BD>::pixel *l1v, const PT<BD>::pixel *l1c, intptr_t rs, intptr_t rfs, int i_pixel, int mbcmp_satd,
    const int32_t *pos, const int16_t *par, const int32_t *weight, const uint16_t *cost_mv, int n, int32_t *out,
    int32_t *cost, int32_t *nevals, void *stream )
{
    if( i_pixel < 0 || i_pixel > 3 || n < 0 ||
        ( n > 0 && ( !fenc || !l0f || !l0h || !l0v || !l0c || !l1f || !l1h || !l1v || !l1c || !pos || !par ||
                     !weight || !cost_mv || !out ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *p0[4] = { l0f, l0h, l0v, l0c }, *p1[4] = { l1f, l1h, l1v, l1c };
    return map_err( launch_me_refine_bidir<BD>( fenc, fs, ffs, p0, p1, rs, rfs, i_pixel, mbcmp_satd, pos, par,
                                                weight, cost_mv, n, out, cost, nevals, (hipStream_t)stream ),
                    "me_refine_bidir_satd" );
}

extern "C" int BD_NAME( me_search_ref_thresh )( const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs,
                                                const PT<BD>::pixel *fw, const PT<BD>::pixel *p0,
                                                const PT<BD>::pixel *p1, const PT<BD>::pixel *p2,
                                                const PT<BD>::pixel *p3, intptr_t rs, intptr_t rfs,
                                                int i_pixel, int me_method, int subme, int me_range,
                                                const int32_t *pos, const int16_t *par, const int16_t *mvc,
                                                const uint16_t *cost_mv, int n, int32_t *out,
                                                int32_t *nevals, int32_t *halfpel_thresh,
                                                const int32_t *ref_cost, const x264hip_refine_ext_t *ext,
                                                void *stream )
{
    if( n < 0 || ( n > 0 && ( !fenc || !fw || !p0 || !p1 || !p2 || !p3 || !pos || !par || !mvc || !cost_mv ||
                              !out ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *planes[4] = { p0, p1, p2, p3 };
    return map_err( launch_me_search_ref<BD>( fenc, fs, ffs, fw, planes, rs, rfs, i_pixel, me_method, subme,
                                              me_range, pos, par, mvc, cost_mv, n, out, nevals, halfpel_thresh,
                                              ref_cost, ext, (hipStream_t)stream ), "me_search_ref_thresh" );
}

extern "C" int BD_NAME( me_search_ref_tesa )(
    const PT<BD>::pixel *fenc, intptr_t fs, intptr_t ffs, const PT<BD>::pixel *fw, const PT<BD>::pixel *p0,
    const PT<BD>::pixel *p1, const PT<BD>::pixel *p2, const PT<BD>::pixel *p3, intptr_t rs, intptr_t rfs,
    const uint16_t *integral8, const uint16_t *integral4, intptr_t ifs, int i_pixel, int subme, int me_range,
    const int32_t *pos, const int16_t *par, const int16_t *mvc, const uint16_t *cost_mv, int n, int32_t *out,
    int32_t *nevals, int32_t *scan, int32_t *halfpel_thresh, const int32_t *ref_cost,
    const x264hip_refine_ext_t *ext, void *stream )
{
    if( n < 0 || i_pixel < 0 || i_pixel > 6 || subme < 1 || subme > 11 || me_range < 4 || me_range > 32 ||
        ( (uintptr_t)out & 15 ) || ( i_pixel > 3 && !integral4 ) ||
        ( n > 0 && ( !fenc || !fw || !p0 || !p1 || !p2 || !p3 || !integral8 || !pos || !par || !mvc ||
                     !cost_mv || !out ) ) )
        return X264HIP_EINVAL;
    const PT<BD>::pixel *planes[4] = { p0, p1, p2, p3 };
    return map_err( launch_me_search_ref_tesa<BD>( fenc, fs, ffs, fw, planes, rs, rfs, integral8, integral4,
                                                   ifs, i_pixel, subme, me_range, pos, par, mvc, cost_mv, n,
                                                   out, nevals, scan, halfpel_thresh, ref_cost, ext,
                                                   (hipStream_t)stream ), "me_search_ref_tesa" );
}

extern "C" int BD_NAME( sub_dct_batch )( int kind, const PT<BD>::pixel *fenc, intptr_t fs,
                                         const PT<BD>::pixel *fdec, intptr_t ds, const int64_t *fo,
                                         const int64_t *dofs, int n, PT<BD>::dctcoef *dct, void *stream )
{
    if( kind < 0 || kind > 6 || n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_sub_dct<BD>( kind, fenc, fs, fdec, ds, fo, dofs, n, dct, (hipStream_t)stream ),
                    "sub_dct_batch" );
}

extern "C" int BD_NAME( dc_batch )( int kind, PT<BD>::dctcoef *dct, PT<BD>::dctcoef *dct4x4, int n,
                                    void *stream )
{
    if( kind < 0 || kind > 2 || n < 0 || ( kind == 1 && !dct4x4 ) )
        return X264HIP_EINVAL;
    if( kind == X264HIP_DC_I4x4 )
        return map_err( launch_idct4x4dc<BD>( dct, n, (hipStream_t)stream ), "dc_batch" );
    return map_err( launch_dc<BD>( kind, dct, dct4x4, n, (hipStream_t)stream ), "dc_batch" );
}

extern "C" int BD_NAME( add_idct_batch )( int kind, PT<BD>::pixel *dst, intptr_t ds, const int64_t *doff,
                                          const PT<BD>::dctcoef *dct, int n, void *stream )
{
    if( kind < 0 || kind > 6 || n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_add_idct<BD>( kind, dst, ds, doff, dct, n, (hipStream_t)stream ), "add_idct_batch" );
}

extern "C" int BD_NAME( dequant_batch )( int kind, PT<BD>::dctcoef *dct, const int32_t *dmf,
                                         const int32_t *qp, int n, void *stream )
{
    if( kind < 0 || kind > 2 || n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_dequant<BD>( kind, dct, dmf, qp, n, (hipStream_t)stream ), "dequant_batch" );
}

extern "C" int BD_NAME( idct_dequant_2x4_batch )( int dconly, PT<BD>::dctcoef *dct,
                                                  PT<BD>::dctcoef *dct4x4, const int32_t *dmf,
                                                  const int32_t *qp, int n, void *stream )
{
    if( n < 0 || ( !dconly && !dct4x4 ) )
        return X264HIP_EINVAL;
    return map_err( launch_idct_dequant_2x4<BD>( dconly, dct, dct4x4, dmf, qp, n, (hipStream_t)stream ),
                    "idct_dequant_2x4_batch" );
}

extern "C" int BD_NAME( optimize_chroma_dc_batch )( int c422, PT<BD>::dctcoef *dct, const int32_t *dmf,
                                                    int n, int32_t *nz, void *stream )
{
    if( n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_optimize_chroma<BD>( c422, dct, dmf, n, nz, (hipStream_t)stream ),
                    "optimize_chroma_dc_batch" );
}

extern "C" int BD_NAME( denoise_dct_batch )( PT<BD>::dctcoef *dct, int size, int n, uint32_t *sum,
                                             const PT<BD>::udctcoef *offset, void *stream )
{
    if( n < 0 || size < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_denoise<BD>( dct, size, n, sum, offset, (hipStream_t)stream ), "denoise_dct_batch" );
}

extern "C" int BD_NAME( coef_stat_batch )( int kind, const PT<BD>::dctcoef *dct, int64_t pitch, int n,
                                           int32_t *out, void *stream )
{
    if( kind < 0 || kind > 7 || n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_coef_stat<BD>( kind, dct, pitch, n, out, (hipStream_t)stream ), "coef_stat_batch" );
}

extern "C" int BD_NAME( coeff_level_run_batch )( int num, const PT<BD>::dctcoef *dct, int64_t pitch, int n,
                                                 int32_t *last, int32_t *mask, int32_t *count,
                                                 PT<BD>::dctcoef *level, void *stream )
{
    if( !( num == 4 || num == 8 || num == 15 || num == 16 ) || n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_level_run<BD>( num, dct, pitch, n, last, mask, count, level, (hipStream_t)stream ),
                    "coeff_level_run_batch" );
}

extern "C" int BD_NAME( zigzag_scan_batch )( int size, int field, PT<BD>::dctcoef *level,
                                             const PT<BD>::dctcoef *dct, int n, void *stream )
{
    if( !( size == 4 || size == 8 ) || n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_zigzag_scan<BD>( size, field ? 1 : 0, level, dct, n, (hipStream_t)stream ),
                    "zigzag_scan_batch" );
}

extern "C" int BD_NAME( zigzag_sub_batch )( int kind, int field, PT<BD>::dctcoef *level,
                                            PT<BD>::dctcoef *dc, const PT<BD>::pixel *src, intptr_t ss,
                                            PT<BD>::pixel *dst, intptr_t ds, const int64_t *so,
                                            const int64_t *dso, int n, int32_t *nz, void *stream )
{
    if( kind < 0 || kind > 2 || n < 0 || ( kind == 1 && !dc ) )
        return X264HIP_EINVAL;
    return map_err( launch_zigzag_sub<BD>( kind, field ? 1 : 0, level, dc, src, ss, dst, ds, so, dso, n, nz,
                                           (hipStream_t)stream ), "zigzag_sub_batch" );
}

extern "C" int BD_NAME( zigzag_interleave_batch )( PT<BD>::dctcoef *dst, const PT<BD>::dctcoef *src,
                                                   uint8_t *nnz, int n, void *stream )
{
    if( n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_interleave<BD>( dst, src, nnz, n, (hipStream_t)stream ), "zigzag_interleave_batch" );
}

extern "C" int BD_NAME( frame_init_lowres )( const PT<BD>::pixel *src, intptr_t stride, intptr_t fstride,
                                             int width, int height, int nframes,
                                             PT<BD>::pixel *const dst[4], intptr_t ds, intptr_t dfs,
                                             void *stream )
{
    if( width < 2 || height < 2 || nframes < 0 || !dst || ( (width / 2 + 64) % PT<BD>::PPD ) ||
        ( (ds * (intptr_t)sizeof(PT<BD>::pixel)) & 3 ) || ( ( (uintptr_t)dst[0] | (uintptr_t)dst[1] |
                                                                (uintptr_t)dst[2] | (uintptr_t)dst[3] ) & 3 ) )
        return X264HIP_EINVAL;
    return map_err( launch_frame_init_lowres<BD>( src, stride, fstride, width, height, nframes, dst, ds, dfs,
                                                  (hipStream_t)stream ), "frame_init_lowres" );
}

extern "C" int BD_NAME( ssim_bands )( const PT<BD>::pixel *p1, intptr_t s1, intptr_t f1,
                                      const PT<BD>::pixel *p2, intptr_t s2, intptr_t f2, int width,
                                      const int32_t *bands, int n_bands, int n_frames, float *ssim,
                                      void *stream )
{
    if( width < 0 || width > 8192 || n_bands < 0 || n_frames < 0 ||
        ( n_bands > 0 && n_frames > 0 && ( !p1 || !p2 || !bands || !ssim ) ) )
        return X264HIP_EINVAL;
    return map_err( launch_ssim_bands<BD>( p1, s1, f1, p2, s2, f2, width, bands, n_bands, n_frames, ssim,
                                           (hipStream_t)stream ), "ssim_bands" );
}

extern "C" int BD_NAME( ssim_wxh )( const PT<BD>::pixel *p1, intptr_t s1, const PT<BD>::pixel *p2,
                                    intptr_t s2, int width, int height, float *ssim, int *cnt,
                                    void *stream )
{
    if( width < 0 || height < 0 || !ssim || ( width >= 8 && height >= 8 && ( !p1 || !p2 ) ) )
        return X264HIP_EINVAL;
    if( cnt )
        *cnt = ( (height >> 2) - 1 ) * ( (width >> 2) - 1 );
    return map_err( launch_ssim_wxh<BD>( p1, s1, p2, s2, width, height, ssim, (hipStream_t)stream ),
                    "ssim_wxh" );
}

extern "C" int BD_NAME( frame_pixel_stats )( const PT<BD>::pixel *luma, intptr_t ls,
                                             const PT<BD>::pixel *cu, const PT<BD>::pixel *cv, intptr_t cs,
                                             int mbw, int mbh, int cf, uint64_t *stats, void *stream )
{
    if( mbw < 0 || mbh < 0 || cf < 0 || cf > 3 || !stats || ( mbw * mbh > 0 && !luma ) ||
        ( mbw * mbh > 0 && cf && !cu ) || ( mbw * mbh > 0 && cf == 3 && !cv ) )
        return X264HIP_EINVAL;
    return map_err( launch_frame_stats<BD>( luma, ls, cu, cv, cs, mbw, mbh, cf, stats, (hipStream_t)stream ),
                    "frame_pixel_stats" );
}

extern "C" int BD_NAME( weight_cost_batch )( int kind, const PT<BD>::pixel *fenc,
                                             const PT<BD>::pixel *const ref[4], intptr_t stride, int mbw,
                                             int mbh, const uint16_t *intra, const int16_t *mvs, int satd,
                                             int plane, int lambda, int n_slices,
                                             const x264hip_weight_t *cands, int n, uint32_t *costs,
                                             void *stream )
{
    if( kind < 0 || kind > 3 || mbw < 0 || mbh < 0 || n < 0 || lambda < 0 || n_slices < 1 ||
        ( (kind == 1 || kind == 2) && ( plane < 0 || plane > 1 ) ) )
        return X264HIP_EINVAL;
    if( n > 0 && ( !cands || !costs ) )
        return X264HIP_EINVAL;
    for( int i = 0; i < n; i++ )
        if( cands[i].weighted && ( cands[i].scale < 0 || cands[i].scale > 255 || cands[i].denom < 0 ||
                                   cands[i].denom > 7 || cands[i].offset < -128 || cands[i].offset > 127 ) )
            return X264HIP_EINVAL;
    if( n > 0 && mbw * mbh > 0 &&
        ( !fenc || !ref || !ref[0] || ( kind == 0 && !intra ) ||
          ( kind == 0 && mvs && ( !ref[1] || !ref[2] || !ref[3] ) ) ) )
        return X264HIP_EINVAL;
    return map_err( launch_weight_cost<BD>( kind, fenc, stride, ref, stride, mbw, mbh, intra, mvs, satd,
                                            kind == 1 || kind == 2 ? plane : 0, lambda, n_slices, cands, n,
                                            costs, (hipStream_t)stream ), "weight_cost_batch" );
}

extern "C" int BD_NAME( weights_analyse )(
    const PT<BD>::pixel *fenc_lr, const PT<BD>::pixel *const ref_lr[4], intptr_t lrs, int mbw, int mbh,
    const uint16_t *intra, const int16_t *mvs, int cf, const PT<BD>::pixel *const fenc_c[2],
    const PT<BD>::pixel *const ref_c[2], intptr_t cs, const uint32_t fsum[3], const uint64_t fssd[3],
    const uint32_t rsum[3], const uint64_t rssd[3], int b_lookahead, int subme, int satd, int lambda,
    int n_slices, int weightp_fake, PT<BD>::pixel *wlr, x264hip_weight_t weights[3], float *cost_delta,
    void *stream )
{
    if( mbw <= 0 || mbh <= 0 || cf < 0 || cf > 3 || subme < 0 || subme > 11 || lambda < 0 || n_slices < 1 ||
        !fenc_lr || !ref_lr || !ref_lr[0] || !intra || !fsum || !fssd || !rsum || !rssd || !weights ||
        ( mvs && ( !ref_lr[1] || !ref_lr[2] || !ref_lr[3] ) ) ||
        ( !b_lookahead && cf && ( !fenc_c || !ref_c || !fenc_c[0] || !ref_c[0] ||
                                  ( cf == 3 && ( !fenc_c[1] || !ref_c[1] ) ) ) ) )
        return X264HIP_EINVAL;
    WpInput<BD> in;
    memset( &in, 0, sizeof( in ) );
    in.fenc_lr = fenc_lr;
    for( int i = 0; i < 4; i++ )
        in.ref_lr[i] = ref_lr[i];
    in.lrs = lrs; in.mbw = mbw; in.mbh = mbh; in.intra = intra; in.mvs = mvs; in.cf = cf;
    if( !b_lookahead && cf )
        for( int i = 0; i < 2; i++ )
        {
            in.fenc_c[i] = fenc_c[i];
            in.ref_c[i] = ref_c[i];
        }
    in.cs = cs;
    for( int i = 0; i < 3; i++ )
    {
        in.fenc_sum[i] = fsum[i]; in.ref_sum[i] = rsum[i];
        in.fenc_ssd[i] = fssd[i]; in.ref_ssd[i] = rssd[i];
    }
    in.b_lookahead = !!b_lookahead; in.subme = subme; in.satd = satd; in.lambda = lambda;
    in.numslices = n_slices; in.weightp_fake = weightp_fake;
    return map_err( weights_analyse<BD>( in, weights, cost_delta, wlr, (hipStream_t)stream ),
                    "weights_analyse" );
}

extern "C" int BD_NAME( mb_dequant_idct_add )( int transform, const PT<BD>::dctcoef *dct, int mbw, int mbh,
                                               int nframes, const int32_t *dmf, const int32_t *qp,
                                               const PT<BD>::pixel *pred, intptr_t ps, intptr_t pfs,
                                               PT<BD>::pixel *recon, intptr_t rs, intptr_t rfs,
                                               void *stream )
{
    if( !( transform == 4 || transform == 8 ) || mbw < 0 || mbh < 0 || nframes < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_mb_recon<BD>( transform, dct, mbw, mbh, nframes, dmf, qp, pred, ps, pfs, recon, rs,
                                         rfs, (hipStream_t)stream ), "mb_dequant_idct_add" );
}

extern "C" int BD_NAME( quant_batch )( int kind, PT<BD>::dctcoef *dct, const PT<BD>::udctcoef *mf,
                                       const PT<BD>::udctcoef *bias, int n, int32_t *nz, void *stream )
{
    if( kind < 0 || kind > 2 || n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_quant<BD>( kind, dct, mf, bias, 0, 0, n, nz, (hipStream_t)stream ), "quant_batch" );
}

extern "C" int BD_NAME( quant_dc_batch )( int kind, PT<BD>::dctcoef *dct, int mf, int bias, int n,
                                          int32_t *nz, void *stream )
{
    if( kind < 3 || kind > 4 || n < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_quant<BD>( kind, dct, nullptr, nullptr, mf, bias, n, nz, (hipStream_t)stream ),
                    "quant_dc_batch" );
}

extern "C" int BD_NAME( mb_dct_quant )( int transform, const PT<BD>::pixel *fenc, intptr_t fs,
                                        intptr_t ffs, const PT<BD>::pixel *pred, intptr_t ps, intptr_t pfs,
                                        int mbw, int mbh, int nframes, const PT<BD>::udctcoef *mf,
                                        const PT<BD>::udctcoef *bias, PT<BD>::dctcoef *dct, int32_t *nz,
                                        void *stream )
{
    if( ( transform != 4 && transform != 8 ) || mbw < 0 || mbh < 0 || nframes < 0 )
        return X264HIP_EINVAL;
    return map_err( launch_mb_dct_quant<BD>( transform, fenc, fs, ffs, pred, ps, pfs, mbw, mbh, nframes, mf,
                                             bias, dct, nz, (hipStream_t)stream ), "mb_dct_quant" );
}
