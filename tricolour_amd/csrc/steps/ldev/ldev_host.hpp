// Host side of the sliding-window complex deviation and its thresholding (steps/ldev/kernels_ldev.hpp)
#pragma once
// Routes, by width, divisibility and alignment alone (DESIGN.md §Local deviation): windows 3 and 5 run the compiled
// register-ring kernels, every other width the run-time one; the deviation passes load 16 bytes per lane when
// nchan % 4 == 0 and the bases allow it, the apply pass 16 flags per lane when the sample count % 16 == 0 and the bases
// allow it.  None changes a result.
namespace {
struct LdevWs {
    float *d_t, *d_f;
    uint8_t *hit_t, *hit_f;
    int64_t* ends;
    size_t bytes;
};

LdevWs ldev_carve(void* ws, int64_t n_win, int64_t ntime, int64_t nchan, int64_t n_chunk_ends) {
    LdevWs w;
    const size_t N = (size_t)n_win * ntime * nchan;
    Bump b(ws, SIZE_MAX, ws == nullptr);
    w.d_t = b.get<float>(N);
    w.d_f = b.get<float>(N);
    w.hit_t = b.get<uint8_t>(N);
    w.hit_f = b.get<uint8_t>(N);
    w.ends = b.get<int64_t>((size_t)n_chunk_ends);
    w.bytes = b.off;
    return w;
}

bool ldev_shape_fits(int64_t n_win, int64_t ntime, int64_t nchan) {
    return ntime < (1ll << 31) && nchan < (1ll << 31) && n_win <= (INT64_MAX / 16 / ntime) / nchan;
}

// shape limits of the entry points; 0 when the shape is fine
int ldev_check_shape(int64_t n_win, int64_t ntime, int64_t nchan, int64_t nchunk) {
    if (!ldev_shape_fits(n_win, ntime, nchan)) return set_err(TRI_EUNSUPPORTED, "window too large");
    // every launch is one-dimensional and holds fewer than 2^31 blocks
    const int64_t lim = (1ll << 31) - 1;
    const int64_t strips = cdiv(nchan, LDEV_CW);
    if (n_win > lim / (ntime * strips) || n_win > lim / cdiv(nchan, LDEV_LC) ||
        cdiv((int64_t)n_win * ntime * nchan, LDEV_NT) > lim || (nchunk > 0 && n_win * ntime > lim / nchunk))
        return set_err(TRI_EUNSUPPORTED, "too many lines for one launch: pass fewer windows per call");
    return 0;
}

int ldev_check_window(const char* name, int64_t w) {
    if (w < 3 || w > LDEV_MAXW || w % 2 == 0)
        return set_err(TRI_EINVAL, "%s must be an odd integer in [3, %d], got %lld", name, LDEV_MAXW, (long long)w);
    return 0;
}

// d along one axis (time: axis 0) of n_win windows into `out`
int ldev_deviation(hipStream_t st, int axis, const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_win,
                   int64_t ntime, int64_t nchan, int window, float* out) {
    const bool c64 = vis_dtype == TRI_VIS_C64;
    const bool vec = nchan % 4 == 0 && (uintptr_t)vis % 16 == 0 && (uintptr_t)flags % 4 == 0 && (uintptr_t)out % 16 == 0;
    const int nstrip = (int)cdiv(nchan, LDEV_CW);
    const int ntiles = (int)cdiv(ntime, axis == 0 ? LDEV_TR : LDEV_FR);
    const dim3 grid((unsigned)(n_win * ntiles * nstrip));
#define LDEV_PASS(K, V, VEC)                                                                                          \
    do {                                                                                                              \
        if (window == 3)                                                                                              \
            hipLaunchKernelGGL((K<V, 3, VEC>), grid, dim3(LDEV_NT), 0, st, vis, flags, ntime, nchan, nstrip, ntiles,  \
                               window, out);                                                                          \
        else if (window == 5)                                                                                         \
            hipLaunchKernelGGL((K<V, 5, VEC>), grid, dim3(LDEV_NT), 0, st, vis, flags, ntime, nchan, nstrip, ntiles,  \
                               window, out);                                                                          \
        else                                                                                                          \
            hipLaunchKernelGGL((K<V, 0, VEC>), grid, dim3(LDEV_NT), 0, st, vis, flags, ntime, nchan, nstrip, ntiles,  \
                               window, out);                                                                          \
    } while (0)
    if (axis == 0) {
        if (c64) { if (vec) LDEV_PASS(k_ldev_time, TRI_VIS_C64, true); else LDEV_PASS(k_ldev_time, TRI_VIS_C64, false); }
        else     { if (vec) LDEV_PASS(k_ldev_time, TRI_VIS_F32, true); else LDEV_PASS(k_ldev_time, TRI_VIS_F32, false); }
    } else {
        if (c64) { if (vec) LDEV_PASS(k_ldev_freq, TRI_VIS_C64, true); else LDEV_PASS(k_ldev_freq, TRI_VIS_C64, false); }
        else     { if (vec) LDEV_PASS(k_ldev_freq, TRI_VIS_F32, true); else LDEV_PASS(k_ldev_freq, TRI_VIS_F32, false); }
    }
#undef LDEV_PASS
    LAUNCHCHK();
    return TRI_OK;
}
}  // namespace

extern "C" size_t tri_local_deviation_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan,
                                                      int64_t n_chunk_ends) {
    if (n_win <= 0 || ntime <= 0 || nchan <= 0 || n_chunk_ends < 2) return 0;
    if (!ldev_shape_fits(n_win, ntime, nchan)) return 0;
    return ldev_carve(nullptr, n_win, ntime, nchan, n_chunk_ends).bytes;
}

extern "C" int tri_local_deviation(const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_win, int64_t ntime,
                                   int64_t nchan, int64_t window_time, int64_t window_freq, float* d_time,
                                   float* d_freq, void* stream) {
    if (!vis || !flags) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = ldev_check_window("window_time", window_time)) return rc;
    if (int rc = ldev_check_window("window_freq", window_freq)) return rc;
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = ldev_check_shape(n_win, ntime, nchan, 0)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (d_time)
        if (int rc = ldev_deviation(st, 0, vis, vis_dtype, flags, n_win, ntime, nchan, (int)window_time, d_time)) return rc;
    if (d_freq)
        if (int rc = ldev_deviation(st, 1, vis, vis_dtype, flags, n_win, ntime, nchan, (int)window_freq, d_freq)) return rc;
    return TRI_OK;
}

extern "C" int tri_local_deviation_threshold(const void* vis, int vis_dtype, const uint8_t* flags, uint8_t* out_flags,
                                             int64_t n_win, int64_t ntime, int64_t nchan, int64_t window_time,
                                             int64_t window_freq, double scale_time, double scale_freq,
                                             const int64_t* chunk_ends, int64_t n_chunk_ends, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    if (!vis || !flags || !out_flags || !chunk_ends) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = ldev_check_window("window_time", window_time)) return rc;
    if (int rc = ldev_check_window("window_freq", window_freq)) return rc;
    if (!(scale_time >= 0.0) || !(scale_freq >= 0.0)) return set_err(TRI_EINVAL, "scale must be >= 0");
    if (int rc = check_chunk_ends(nchan, chunk_ends, n_chunk_ends)) return rc;
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    const int64_t nchunk = n_chunk_ends - 1;
    if (int rc = ldev_check_shape(n_win, ntime, nchan, nchunk)) return rc;
    const size_t N = (size_t)n_win * ntime * nchan;
    if (ranges_overlap(out_flags, N, flags, N)) return set_err(TRI_EINVAL, "out_flags must not overlap flags");
    const size_t need = tri_local_deviation_workspace_bytes(n_win, ntime, nchan, n_chunk_ends);
    if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool on_t = scale_time > 0.0, on_f = scale_freq > 0.0;
    if (!on_t && !on_f) return launch_identity(st, flags, out_flags, N);
    const LdevWs w = ldev_carve(workspace, n_win, ntime, nchan, n_chunk_ends);
    if (on_t) {
        if (int rc = ldev_deviation(st, 0, vis, vis_dtype, flags, n_win, ntime, nchan, (int)window_time, w.d_t)) return rc;
        hipLaunchKernelGGL(k_ldev_level<0>, dim3((unsigned)(n_win * cdiv(nchan, LDEV_LC))), dim3(LDEV_NT), 0, st, w.d_t,
                           n_win, ntime, nchan, (const int64_t*)nullptr, 0, scale_time, w.hit_t);
        LAUNCHCHK();
    }
    if (on_f) {
        // (pageable host memory: the copy is staged before the call returns, so the caller's array may go)
        HIPCHK(hipMemcpyAsync(w.ends, chunk_ends, (size_t)n_chunk_ends * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (int rc = ldev_deviation(st, 1, vis, vis_dtype, flags, n_win, ntime, nchan, (int)window_freq, w.d_f)) return rc;
        hipLaunchKernelGGL(k_ldev_level<1>, dim3((unsigned)cdiv(n_win * ntime * nchunk, LDEV_LW)), dim3(LDEV_NT), 0, st,
                           w.d_f, n_win, ntime, nchan, (const int64_t*)w.ends, (int)nchunk, scale_freq, w.hit_f);
        LAUNCHCHK();
    }
    const uint8_t* ht = on_t ? w.hit_t : nullptr;
    const uint8_t* hf = on_f ? w.hit_f : nullptr;
    if (N % 16 == 0 && (uintptr_t)flags % 16 == 0 && (uintptr_t)out_flags % 16 == 0)
        hipLaunchKernelGGL(k_ldev_apply<true>, dim3((unsigned)cdiv((int64_t)N / 16, LDEV_NT)), dim3(LDEV_NT), 0, st, flags,
                           ht, hf, out_flags, (int64_t)N);
    else
        hipLaunchKernelGGL(k_ldev_apply<false>, dim3((unsigned)cdiv((int64_t)N, LDEV_NT)), dim3(LDEV_NT), 0, st, flags, ht,
                           hf, out_flags, (int64_t)N);
    LAUNCHCHK();
    return TRI_OK;
}
