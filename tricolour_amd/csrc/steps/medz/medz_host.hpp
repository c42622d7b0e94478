// Host side of the sliding 2-D median background and the robust z-score on it (steps/medz/kernels_medz.hpp)
#pragma once
// One route: every shape, radius and alignment runs the same kernel, k_medz_select, once per median (DESIGN.md
// §Median z-score).  No workspace: the residual and z-score images are the caller's, every element written.
namespace {
bool medz_shape_fits(int64_t n_win, int64_t ntime, int64_t nchan) {
    return ntime < (1ll << 31) && nchan < (1ll << 31) && n_win <= (INT64_MAX / 16 / ntime) / nchan;
}

// shape limits of the entry points; 0 when the shape is fine
int medz_check_shape(int64_t n_win, int64_t ntime, int64_t nchan) {
    if (!medz_shape_fits(n_win, ntime, nchan)) return set_err(TRI_EUNSUPPORTED, "window too large");
    // every launch is one-dimensional and holds fewer than 2^31 blocks
    const int64_t lim = (1ll << 31) - 1;
    if (n_win > lim / (cdiv(ntime, MEDZ_TR) * cdiv(nchan, MEDZ_TC)))
        return set_err(TRI_EUNSUPPORTED, "too many lines for one launch: pass fewer windows per call");
    return 0;
}

// the radii and min_samples; 0 when they are fine
int medz_check_radii(int64_t kt, int64_t kf, int64_t min_samples) {
    if (kt < 0 || kt > MEDZ_MAXK || kf < 0 || kf > MEDZ_MAXK || (kt == 0 && kf == 0))
        return set_err(TRI_EINVAL, "radius_time and radius_freq must be integers in [0, %d] and not both 0, got %lld and %lld",
                       MEDZ_MAXK, (long long)kt, (long long)kf);
    const int64_t area = (2 * kt + 1) * (2 * kf + 1);
    if (area > MEDZ_MAXAREA)
        return set_err(TRI_EINVAL, "(2 radius_time + 1) (2 radius_freq + 1) must be at most %d, got %lld", MEDZ_MAXAREA,
                       (long long)area);
    if (min_samples < 1 || min_samples > area)
        return set_err(TRI_EINVAL, "min_samples must be an integer in [1, %lld], got %lld", (long long)area,
                       (long long)min_samples);
    // what a block stages fits its LDS array (true of every pair the area limit lets through)
    if ((MEDZ_TR + 2 * kt) * (MEDZ_TC + 2 * kf) > MEDZ_LDS_WORDS)
        return set_err(TRI_EUNSUPPORTED, "radii %lld and %lld need more LDS than a block has", (long long)kt, (long long)kf);
    return 0;
}

struct MedzShape {
    int64_t n_win;
    int ntime, nchan, kt, kf;
    unsigned min_samples;
};

// source A: background (and residual, may be NULL) of vis under `flags`
int medz_background(hipStream_t st, const void* vis, int vis_dtype, const uint8_t* flags, const MedzShape& s,
                    float* background, float* residual) {
    const int tiles_t = (int)cdiv(s.ntime, MEDZ_TR), tiles_f = (int)cdiv(s.nchan, MEDZ_TC);
    const dim3 grid((unsigned)(s.n_win * tiles_t * tiles_f));
    if (vis_dtype == TRI_VIS_C64)
        hipLaunchKernelGGL((k_medz_select<TRI_VIS_C64, false>), grid, dim3(MEDZ_NT), 0, st, vis, flags, s.ntime, s.nchan,
                           tiles_t, tiles_f, s.kt, s.kf, s.min_samples, 0.0, background, residual,
                           (const uint8_t*)nullptr, (uint8_t*)nullptr);
    else
        hipLaunchKernelGGL((k_medz_select<TRI_VIS_F32, false>), grid, dim3(MEDZ_NT), 0, st, vis, flags, s.ntime, s.nchan,
                           tiles_t, tiles_f, s.kt, s.kf, s.min_samples, 0.0, background, residual,
                           (const uint8_t*)nullptr, (uint8_t*)nullptr);
    LAUNCHCHK();
    return TRI_OK;
}

// source B: scale (may be NULL) and z of the residual; gout = (gin != 0) | hit unless gout is NULL
int medz_zscore(hipStream_t st, const float* residual, const MedzShape& s, double nsigma, float* scale, float* zscore,
                const uint8_t* gin, uint8_t* gout) {
    const int tiles_t = (int)cdiv(s.ntime, MEDZ_TR), tiles_f = (int)cdiv(s.nchan, MEDZ_TC);
    const dim3 grid((unsigned)(s.n_win * tiles_t * tiles_f));
    hipLaunchKernelGGL((k_medz_select<TRI_VIS_F32, true>), grid, dim3(MEDZ_NT), 0, st, (const void*)residual,
                       (const uint8_t*)nullptr, s.ntime, s.nchan, tiles_t, tiles_f, s.kt, s.kf, s.min_samples, nsigma,
                       scale, zscore, gin, gout);
    LAUNCHCHK();
    return TRI_OK;
}
}  // namespace

extern "C" int tri_medfilt_background(const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_win, int64_t ntime,
                                      int64_t nchan, int64_t radius_time, int64_t radius_freq, int64_t min_samples,
                                      float* background, float* residual, void* stream) {
    if (!vis || !flags || !background) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = medz_check_radii(radius_time, radius_freq, min_samples)) return rc;
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = medz_check_shape(n_win, ntime, nchan)) return rc;
    const size_t N = (size_t)n_win * ntime * nchan, nv = N * (vis_dtype == TRI_VIS_C64 ? 8 : 4);
    if (ranges_overlap(background, N * 4, vis, nv) || ranges_overlap(background, N * 4, flags, N) ||
        (residual && (ranges_overlap(residual, N * 4, vis, nv) || ranges_overlap(residual, N * 4, flags, N) ||
                      ranges_overlap(residual, N * 4, background, N * 4))))
        return set_err(TRI_EINVAL, "background and residual must not overlap an input or each other");
    const MedzShape s{n_win, (int)ntime, (int)nchan, (int)radius_time, (int)radius_freq, (unsigned)min_samples};
    return medz_background((hipStream_t)stream, vis, vis_dtype, flags, s, background, residual);
}

extern "C" int tri_medfilt_zscore(const float* residual, int64_t n_win, int64_t ntime, int64_t nchan, int64_t radius_time,
                                  int64_t radius_freq, int64_t min_samples, float* scale, float* zscore, void* stream) {
    if (!residual || !zscore) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = medz_check_radii(radius_time, radius_freq, min_samples)) return rc;
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = medz_check_shape(n_win, ntime, nchan)) return rc;
    const size_t N = (size_t)n_win * ntime * nchan;
    if (ranges_overlap(zscore, N * 4, residual, N * 4) ||
        (scale && (ranges_overlap(scale, N * 4, residual, N * 4) || ranges_overlap(scale, N * 4, zscore, N * 4))))
        return set_err(TRI_EINVAL, "scale and zscore must not overlap residual or each other");
    const MedzShape s{n_win, (int)ntime, (int)nchan, (int)radius_time, (int)radius_freq, (unsigned)min_samples};
    return medz_zscore((hipStream_t)stream, residual, s, 0.0, scale, zscore, nullptr, nullptr);
}

extern "C" int tri_median_zscore_threshold(const void* vis, int vis_dtype, const uint8_t* flags, uint8_t* out_flags,
                                           int64_t n_win, int64_t ntime, int64_t nchan, int64_t radius_time,
                                           int64_t radius_freq, int64_t min_samples, double nsigma, int64_t rounds,
                                           float* residual, float* zscore, void* stream) {
    if (!vis || !flags || !out_flags || !residual || !zscore) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = medz_check_radii(radius_time, radius_freq, min_samples)) return rc;
    if (!(nsigma > 0.0)) return set_err(TRI_EINVAL, "nsigma must be > 0");
    if (rounds < 1 || rounds > 4) return set_err(TRI_EINVAL, "rounds must be an integer in [1, 4], got %lld", (long long)rounds);
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = medz_check_shape(n_win, ntime, nchan)) return rc;
    const size_t N = (size_t)n_win * ntime * nchan;
    const void* p[5] = {vis, flags, out_flags, residual, zscore};
    const size_t nb[5] = {N * (vis_dtype == TRI_VIS_C64 ? 8 : 4), N, N, N * 4, N * 4};
    for (int a = 2; a < 5; a++)
        for (int b = 0; b < a; b++)
            if (ranges_overlap(p[a], nb[a], p[b], nb[b]))
                return set_err(TRI_EINVAL, "out_flags, residual and zscore must not overlap an input or each other");
    hipStream_t st = (hipStream_t)stream;
    const MedzShape s{n_win, (int)ntime, (int)nchan, (int)radius_time, (int)radius_freq, (unsigned)min_samples};
    // g_0 = flags; every round reads the running flags and ORs its hits into out_flags
    const uint8_t* g = flags;
    for (int64_t k = 0; k < rounds; k++) {
        if (int rc = medz_background(st, vis, vis_dtype, g, s, nullptr, residual)) return rc;
        if (int rc = medz_zscore(st, residual, s, nsigma, nullptr, zscore, g, out_flags)) return rc;
        g = out_flags;
    }
    return TRI_OK;
}
