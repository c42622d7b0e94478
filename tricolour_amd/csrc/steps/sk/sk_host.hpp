// Host side of the spectral-kurtosis statistics and the flagging of (block, channel) cells on them
// (steps/sk/kernels_sk.hpp)
#pragma once
// One kernel per pass; two switches, by divisibility and alignment alone (DESIGN.md §Spectral kurtosis): the
// statistics pass loads 16 bytes per lane when nchan % 4 == 0 and the bases allow it, the apply pass 16 flags per lane
// when nchan % 16 == 0 and the bases allow it.  Neither changes a result.  No workspace: sk and count are the
// caller's, every element written.
namespace {
struct SkShape {
    int64_t n_win, ntime, nchan;
    int block_time, nblocks;
};

bool sk_shape_fits(int64_t n_win, int64_t ntime, int64_t nchan) {
    return ntime < (1ll << 31) && nchan < (1ll << 31) && n_win <= (INT64_MAX / 16 / ntime) / nchan;
}

// shape limits shared by the three entry points; 0 when the shape is fine
int sk_check_shape(int64_t n_win, int64_t ntime, int64_t nchan, int64_t block_time) {
    if (!sk_shape_fits(n_win, ntime, nchan)) return set_err(TRI_EUNSUPPORTED, "window too large");
    // every launch is one-dimensional and holds fewer than 2^31 blocks; the apply pass without its 16-flag lanes has
    // the most: one per (window, block of rows, SK_AR rows of it, SK_NT channels)
    const int64_t lim = (1ll << 31) - 1;
    const int64_t per_win = cdiv(ntime, block_time) * cdiv(block_time, SK_AR);     // < 2^31 * 2^12
    if (per_win > lim || n_win > lim / (per_win * cdiv(nchan, SK_NT)))
        return set_err(TRI_EUNSUPPORTED, "too many cells for one launch: pass fewer windows per call");
    return 0;
}

int sk_check_block(int64_t block_time) {
    if (block_time < 2 || block_time > SK_MAX_BLOCK)
        return set_err(TRI_EINVAL, "block_time must be an integer in [2, %d], got %lld", SK_MAX_BLOCK, (long long)block_time);
    return 0;
}

// block_time, shape and min_samples; 0 when they are fine
int sk_check_params(int64_t block_time, double shape, int64_t min_samples) {
    if (int rc = sk_check_block(block_time)) return rc;
    if (!(shape > 0.0) || std::isinf(shape)) return set_err(TRI_EINVAL, "shape must be a finite number > 0");
    if (min_samples < 2 || min_samples > block_time)
        return set_err(TRI_EINVAL, "min_samples must be an integer in [2, %lld], got %lld", (long long)block_time,
                       (long long)min_samples);
    return 0;
}

int sk_statistics(hipStream_t st, const void* vis, int vis_dtype, const uint8_t* flags, const SkShape& s, double shape,
                  int min_samples, float* sk, int32_t* count) {
    const bool c64 = vis_dtype == TRI_VIS_C64;
    const bool vec = s.nchan % 4 == 0 && (uintptr_t)vis % 16 == 0 && (uintptr_t)flags % 4 == 0;
    const int nstrip = (int)cdiv(s.nchan, SK_NT * (vec ? 4 : 1));
    const dim3 grid((unsigned)(s.n_win * s.nblocks * nstrip));
#define SK_STATS(V, VEC)                                                                                             \
    hipLaunchKernelGGL((k_sk_stats<V, VEC>), grid, dim3(SK_NT), 0, st, vis, flags, s.ntime, s.nchan, s.block_time, \
                       s.nblocks, nstrip, shape, min_samples, sk, count)
    if (c64) { if (vec) SK_STATS(TRI_VIS_C64, true); else SK_STATS(TRI_VIS_C64, false); }
    else     { if (vec) SK_STATS(TRI_VIS_F32, true); else SK_STATS(TRI_VIS_F32, false); }
#undef SK_STATS
    LAUNCHCHK();
    return TRI_OK;
}

int sk_apply(hipStream_t st, const float* sk, const int32_t* count, const uint8_t* flags, uint8_t* out_flags,
             const SkShape& s, const double* lower, const double* upper) {
    const bool vec = s.nchan % 16 == 0 && (uintptr_t)flags % 16 == 0 && (uintptr_t)out_flags % 16 == 0 &&
                     (uintptr_t)sk % 16 == 0 && (uintptr_t)count % 16 == 0;
    const int nstrip = (int)cdiv(s.nchan, SK_NT * (vec ? 16 : 1)), nchunk = (int)cdiv(s.block_time, SK_AR);
    const dim3 grid((unsigned)(s.n_win * s.nblocks * nchunk * nstrip));
    if (vec)
        hipLaunchKernelGGL(k_sk_apply<true>, grid, dim3(SK_NT), 0, st, sk, count, flags, out_flags, s.ntime, s.nchan,
                           s.block_time, s.nblocks, nchunk, nstrip, lower, upper);
    else
        hipLaunchKernelGGL(k_sk_apply<false>, grid, dim3(SK_NT), 0, st, sk, count, flags, out_flags, s.ntime, s.nchan,
                           s.block_time, s.nblocks, nchunk, nstrip, lower, upper);
    LAUNCHCHK();
    return TRI_OK;
}
}  // namespace

extern "C" int tri_sk_statistics(const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_win, int64_t ntime,
                                 int64_t nchan, int64_t block_time, double shape, int64_t min_samples, float* sk,
                                 int32_t* count, void* stream) {
    if (!vis || !flags || !sk) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = sk_check_params(block_time, shape, min_samples)) return rc;
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = sk_check_shape(n_win, ntime, nchan, block_time)) return rc;
    const SkShape s{n_win, ntime, nchan, (int)block_time, (int)cdiv(ntime, block_time)};
    const size_t N = (size_t)n_win * ntime * nchan, nc = (size_t)n_win * s.nblocks * nchan;
    const size_t nv = N * (vis_dtype == TRI_VIS_C64 ? 8 : 4);
    if (ranges_overlap(sk, nc * 4, vis, nv) || ranges_overlap(sk, nc * 4, flags, N) ||
        (count && (ranges_overlap(count, nc * 4, vis, nv) || ranges_overlap(count, nc * 4, flags, N) ||
                   ranges_overlap(count, nc * 4, sk, nc * 4))))
        return set_err(TRI_EINVAL, "sk and count must not overlap an input or each other");
    return sk_statistics((hipStream_t)stream, vis, vis_dtype, flags, s, shape, (int)min_samples, sk, count);
}

extern "C" int tri_sk_apply(const float* sk, const int32_t* count, const uint8_t* flags, uint8_t* out_flags, int64_t n_win,
                            int64_t ntime, int64_t nchan, int64_t block_time, const double* lower, const double* upper,
                            void* stream) {
    if (!sk || !count || !flags || !out_flags || !lower || !upper) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = sk_check_block(block_time)) return rc;
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = sk_check_shape(n_win, ntime, nchan, block_time)) return rc;
    const SkShape s{n_win, ntime, nchan, (int)block_time, (int)cdiv(ntime, block_time)};
    const size_t N = (size_t)n_win * ntime * nchan, nc = (size_t)n_win * s.nblocks * nchan;
    const size_t nt = (size_t)(block_time + 1) * 8;
    if (ranges_overlap(out_flags, N, flags, N) || ranges_overlap(out_flags, N, sk, nc * 4) ||
        ranges_overlap(out_flags, N, count, nc * 4) || ranges_overlap(out_flags, N, lower, nt) ||
        ranges_overlap(out_flags, N, upper, nt))
        return set_err(TRI_EINVAL, "out_flags must not overlap an input");
    return sk_apply((hipStream_t)stream, sk, count, flags, out_flags, s, lower, upper);
}

extern "C" int tri_sk_threshold(const void* vis, int vis_dtype, const uint8_t* flags, uint8_t* out_flags, int64_t n_win,
                                int64_t ntime, int64_t nchan, int64_t block_time, double shape, int64_t min_samples,
                                const double* lower, const double* upper, float* sk, int32_t* count, void* stream) {
    if (!vis || !flags || !out_flags || !lower || !upper || !sk || !count)
        return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = sk_check_params(block_time, shape, min_samples)) return rc;
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = sk_check_shape(n_win, ntime, nchan, block_time)) return rc;
    const SkShape s{n_win, ntime, nchan, (int)block_time, (int)cdiv(ntime, block_time)};
    const size_t N = (size_t)n_win * ntime * nchan, nc = (size_t)n_win * s.nblocks * nchan;
    const size_t nt = (size_t)(block_time + 1) * 8;
    // inputs first, then the outputs: an output may overlap nothing before it
    const void* p[7] = {vis, flags, lower, upper, out_flags, sk, count};
    const size_t nb[7] = {N * (vis_dtype == TRI_VIS_C64 ? 8 : 4), N, nt, nt, N, nc * 4, nc * 4};
    for (int a = 4; a < 7; a++)
        for (int b = 0; b < a; b++)
            if (ranges_overlap(p[a], nb[a], p[b], nb[b]))
                return set_err(TRI_EINVAL, "out_flags, sk and count must not overlap an input or each other");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sk_statistics(st, vis, vis_dtype, flags, s, shape, (int)min_samples, sk, count)) return rc;
    return sk_apply(st, sk, count, flags, out_flags, s, lower, upper);
}
