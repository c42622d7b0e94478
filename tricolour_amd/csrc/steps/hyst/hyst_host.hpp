// Host side of the value-driven hysteresis growth of flags (steps/hyst/kernels_hyst.hpp)
#pragma once
// Routes, by shape, divisibility and alignment alone (DESIGN.md §Hysteresis growth): a level line of at most HYST_LN
// samples keeps its keys in LDS, a longer one is re-read for every pass (decided inside the kernel, per line); the
// growth kernel writes 16 flags per lane when nchan % 16 == 0 and the bases allow it.  None changes a result.
namespace {
struct HystWs {
    float *med_t, *mad_t, *med_f, *mad_f;
    unsigned *seed, *et, *ef;
    int64_t* ends;
    size_t bytes;
};

HystWs hyst_carve(void* ws, int64_t n_win, int64_t ntime, int64_t nchan, int64_t n_chunk_ends) {
    HystWs w;
    const size_t lines_t = (size_t)n_win * nchan, lines_f = (size_t)n_win * ntime * (size_t)(n_chunk_ends - 1);
    const size_t words = (size_t)n_win * ntime * (size_t)cdiv(nchan, 32);
    Bump b(ws, SIZE_MAX, ws == nullptr);
    w.med_t = b.get<float>(lines_t);
    w.mad_t = b.get<float>(lines_t);
    w.med_f = b.get<float>(lines_f);
    w.mad_f = b.get<float>(lines_f);
    w.seed = b.get<unsigned>(words);
    w.et = b.get<unsigned>(words);
    w.ef = b.get<unsigned>(words);
    w.ends = b.get<int64_t>((size_t)n_chunk_ends);
    w.bytes = b.off;
    return w;
}

bool hyst_shape_fits(int64_t n_win, int64_t ntime, int64_t nchan, int64_t n_chunk_ends) {
    return ntime < (1ll << 31) && nchan < (1ll << 31) && n_chunk_ends <= (1ll << 30) &&
           n_win <= (INT64_MAX / 64 / ntime) / std::max(nchan, n_chunk_ends);
}

// shape limits of the entry points; 0 when the shape is fine
int hyst_check_shape(int64_t n_win, int64_t ntime, int64_t nchan, int64_t n_chunk_ends) {
    if (!hyst_shape_fits(n_win, ntime, nchan, n_chunk_ends)) return set_err(TRI_EUNSUPPORTED, "window too large");
    // every launch is one-dimensional and holds fewer than 2^31 blocks
    const int64_t lim = (1ll << 31) - 1;
    const int64_t nchunk = n_chunk_ends - 1;
    if (n_win > lim / cdiv(nchan, HYST_LC) || cdiv(n_win * ntime * nchunk, HYST_LW) > lim ||
        n_win > lim / (cdiv(ntime, HYST_ER) * cdiv(nchan, HYST_NT)) ||
        n_win > lim / (cdiv(ntime, HYST_GR) * cdiv(cdiv(nchan, 32), HYST_GW)))
        return set_err(TRI_EUNSUPPORTED, "too many lines for one launch: pass fewer windows per call");
    return 0;
}

// the host's chunk ends; 0 when they are fine
int hyst_check_chunks(int64_t nchan, const int64_t* chunk_ends, int64_t n_chunk_ends) {
    if (!chunk_ends) return set_err(TRI_EINVAL, "NULL pointer argument");
    return check_chunk_ends(nchan, chunk_ends, n_chunk_ends);
}

int hyst_check_nsigma(double nsigma_time, double nsigma_freq) {
    if (!(nsigma_time >= 0.0) || !(nsigma_freq >= 0.0)) return set_err(TRI_EINVAL, "nsigma must be >= 0");
    return 0;
}

int hyst_check_workspace(void* workspace, size_t workspace_bytes, int64_t n_win, int64_t ntime, int64_t nchan,
                         int64_t n_chunk_ends) {
    return check_workspace(workspace, workspace_bytes, hyst_carve(nullptr, n_win, ntime, nchan, n_chunk_ends).bytes);
}

// med and mad of the lines of one axis (time: axis 0); `ends` on the device
int hyst_levels(hipStream_t st, int axis, const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_win,
                int64_t ntime, int64_t nchan, const int64_t* ends, int64_t nchunk, float* med, float* mad) {
    const bool c64 = vis_dtype == TRI_VIS_C64;
    if (axis == 0) {
        const dim3 grid((unsigned)(n_win * cdiv(nchan, HYST_LC)));
        if (c64)
            hipLaunchKernelGGL((k_hyst_level<TRI_VIS_C64, 0>), grid, dim3(HYST_NT), 0, st, vis, flags, n_win, ntime, nchan,
                               ends, (int)nchunk, med, mad);
        else
            hipLaunchKernelGGL((k_hyst_level<TRI_VIS_F32, 0>), grid, dim3(HYST_NT), 0, st, vis, flags, n_win, ntime, nchan,
                               ends, (int)nchunk, med, mad);
    } else {
        const dim3 grid((unsigned)cdiv(n_win * ntime * nchunk, HYST_LW));
        if (c64)
            hipLaunchKernelGGL((k_hyst_level<TRI_VIS_C64, 1>), grid, dim3(HYST_NT), 0, st, vis, flags, n_win, ntime, nchan,
                               ends, (int)nchunk, med, mad);
        else
            hipLaunchKernelGGL((k_hyst_level<TRI_VIS_F32, 1>), grid, dim3(HYST_NT), 0, st, vis, flags, n_win, ntime, nchan,
                               ends, (int)nchunk, med, mad);
    }
    LAUNCHCHK();
    return TRI_OK;
}

// levels of the axes that are on, then the planes and / or the byte images
int hyst_eligible(hipStream_t st, const void* vis, int vis_dtype, const uint8_t* flags, const uint8_t* missing,
                  int64_t n_win, int64_t ntime, int64_t nchan, double nsigma_time, double nsigma_freq,
                  const int64_t* chunk_ends, int64_t n_chunk_ends, const HystWs& w, bool planes, uint8_t* b_et,
                  uint8_t* b_ef) {
    const int64_t nchunk = n_chunk_ends - 1;
    // (pageable host memory: the copy is staged before the call returns, so the caller's array may go)
    HIPCHK(hipMemcpyAsync(w.ends, chunk_ends, (size_t)n_chunk_ends * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (nsigma_time > 0.0)
        if (int rc = hyst_levels(st, 0, vis, vis_dtype, flags, n_win, ntime, nchan, w.ends, nchunk, w.med_t, w.mad_t)) return rc;
    if (nsigma_freq > 0.0)
        if (int rc = hyst_levels(st, 1, vis, vis_dtype, flags, n_win, ntime, nchan, w.ends, nchunk, w.med_f, w.mad_f)) return rc;
    const int nstrip = (int)cdiv(nchan, HYST_NT), ntiles = (int)cdiv(ntime, HYST_ER), nw = (int)cdiv(nchan, 32);
    const dim3 grid((unsigned)(n_win * ntiles * nstrip));
    const double scale_t = nsigma_time * TRI_MAD_NORMAL, scale_f = nsigma_freq * TRI_MAD_NORMAL;
    unsigned *ps = planes ? w.seed : nullptr, *pt = planes ? w.et : nullptr, *pf = planes ? w.ef : nullptr;
    if (vis_dtype == TRI_VIS_C64)
        hipLaunchKernelGGL((k_hyst_eligible<TRI_VIS_C64>), grid, dim3(HYST_NT), 0, st, vis, flags, missing, ntime, nchan,
                           nstrip, ntiles, (const int64_t*)w.ends, (int)nchunk, scale_t, scale_f, (const float*)w.med_t,
                           (const float*)w.mad_t, (const float*)w.med_f, (const float*)w.mad_f, nw, ps, pt, pf, b_et, b_ef);
    else
        hipLaunchKernelGGL((k_hyst_eligible<TRI_VIS_F32>), grid, dim3(HYST_NT), 0, st, vis, flags, missing, ntime, nchan,
                           nstrip, ntiles, (const int64_t*)w.ends, (int)nchunk, scale_t, scale_f, (const float*)w.med_t,
                           (const float*)w.mad_t, (const float*)w.med_f, (const float*)w.mad_f, nw, ps, pt, pf, b_et, b_ef);
    LAUNCHCHK();
    return TRI_OK;
}

// out = (base != 0) | G_reach from the planes of the workspace
int hyst_grow(hipStream_t st, const HystWs& w, const uint8_t* base, uint8_t* out, int64_t n_win, int64_t ntime,
              int64_t nchan, int reach) {
    const int nw = (int)cdiv(nchan, 32), ntr = (int)cdiv(ntime, HYST_GR), ntw = (int)cdiv(nw, HYST_GW);
    const dim3 grid((unsigned)(n_win * ntr * ntw));
    if (nchan % 16 == 0 && (uintptr_t)base % 16 == 0 && (uintptr_t)out % 16 == 0)
        hipLaunchKernelGGL(k_hyst_grow<true>, grid, dim3(HYST_NT), 0, st, (const unsigned*)w.seed, (const unsigned*)w.et,
                           (const unsigned*)w.ef, base, out, ntime, nchan, nw, ntr, ntw, reach);
    else
        hipLaunchKernelGGL(k_hyst_grow<false>, grid, dim3(HYST_NT), 0, st, (const unsigned*)w.seed, (const unsigned*)w.et,
                           (const unsigned*)w.ef, base, out, ntime, nchan, nw, ntr, ntw, reach);
    LAUNCHCHK();
    return TRI_OK;
}
}  // namespace

extern "C" size_t tri_hyst_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan, int64_t n_chunk_ends) {
    if (n_win <= 0 || ntime <= 0 || nchan <= 0 || n_chunk_ends < 2) return 0;
    if (!hyst_shape_fits(n_win, ntime, nchan, n_chunk_ends)) return 0;
    return hyst_carve(nullptr, n_win, ntime, nchan, n_chunk_ends).bytes;
}

extern "C" int tri_hyst_levels(const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_win, int64_t ntime,
                               int64_t nchan, const int64_t* chunk_ends, int64_t n_chunk_ends, float* med_time,
                               float* mad_time, float* med_freq, float* mad_freq, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!vis || !flags || !med_time || !mad_time || !med_freq || !mad_freq)
        return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = hyst_check_chunks(nchan, chunk_ends, n_chunk_ends)) return rc;
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = hyst_check_shape(n_win, ntime, nchan, n_chunk_ends)) return rc;
    if (int rc = hyst_check_workspace(workspace, workspace_bytes, n_win, ntime, nchan, n_chunk_ends)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const HystWs w = hyst_carve(workspace, n_win, ntime, nchan, n_chunk_ends);
    HIPCHK(hipMemcpyAsync(w.ends, chunk_ends, (size_t)n_chunk_ends * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (int rc = hyst_levels(st, 0, vis, vis_dtype, flags, n_win, ntime, nchan, w.ends, n_chunk_ends - 1, med_time, mad_time)) return rc;
    return hyst_levels(st, 1, vis, vis_dtype, flags, n_win, ntime, nchan, w.ends, n_chunk_ends - 1, med_freq, mad_freq);
}

extern "C" int tri_hyst_eligible(const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_win, int64_t ntime,
                                 int64_t nchan, double nsigma_time, double nsigma_freq, const int64_t* chunk_ends,
                                 int64_t n_chunk_ends, uint8_t* e_time, uint8_t* e_freq, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!vis || !flags || !e_time || !e_freq) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = hyst_check_nsigma(nsigma_time, nsigma_freq)) return rc;
    if (int rc = hyst_check_chunks(nchan, chunk_ends, n_chunk_ends)) return rc;
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = hyst_check_shape(n_win, ntime, nchan, n_chunk_ends)) return rc;
    const size_t N = (size_t)n_win * ntime * nchan;
    if (ranges_overlap(e_time, N, flags, N) || ranges_overlap(e_freq, N, flags, N) || ranges_overlap(e_time, N, e_freq, N))
        return set_err(TRI_EINVAL, "e_time and e_freq must not overlap flags or each other");
    if (int rc = hyst_check_workspace(workspace, workspace_bytes, n_win, ntime, nchan, n_chunk_ends)) return rc;
    const HystWs w = hyst_carve(workspace, n_win, ntime, nchan, n_chunk_ends);
    return hyst_eligible((hipStream_t)stream, vis, vis_dtype, flags, nullptr, n_win, ntime, nchan, nsigma_time,
                         nsigma_freq, chunk_ends, n_chunk_ends, w, false, e_time, e_freq);
}

extern "C" int tri_hyst_grow(const uint8_t* seeds, const uint8_t* e_time, const uint8_t* e_freq, uint8_t* out,
                             int64_t n_win, int64_t ntime, int64_t nchan, int64_t reach, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (!seeds || !e_time || !e_freq || !out) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (reach < 1 || reach > HYST_MAXREACH)
        return set_err(TRI_EINVAL, "reach must be an integer in [1, %d], got %lld", HYST_MAXREACH, (long long)reach);
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = hyst_check_shape(n_win, ntime, nchan, 2)) return rc;
    const size_t N = (size_t)n_win * ntime * nchan;
    if (ranges_overlap(out, N, seeds, N) || ranges_overlap(out, N, e_time, N) || ranges_overlap(out, N, e_freq, N))
        return set_err(TRI_EINVAL, "out must not overlap an input");
    if (int rc = hyst_check_workspace(workspace, workspace_bytes, n_win, ntime, nchan, 2)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const HystWs w = hyst_carve(workspace, n_win, ntime, nchan, 2);
    const int nstrip = (int)cdiv(nchan, HYST_NT), ntiles = (int)cdiv(ntime, HYST_ER), nw = (int)cdiv(nchan, 32);
    hipLaunchKernelGGL(k_hyst_pack, dim3((unsigned)(n_win * ntiles * nstrip)), dim3(HYST_NT), 0, st, seeds, e_time, e_freq,
                       ntime, nchan, nstrip, ntiles, nw, w.seed, w.et, w.ef);
    LAUNCHCHK();
    return hyst_grow(st, w, seeds, out, n_win, ntime, nchan, (int)reach);
}

extern "C" int tri_hysteresis_growth(const void* vis, int vis_dtype, const uint8_t* flags, const uint8_t* missing,
                                     uint8_t* out_flags, int64_t n_win, int64_t ntime, int64_t nchan,
                                     double nsigma_time, double nsigma_freq, int64_t reach, const int64_t* chunk_ends,
                                     int64_t n_chunk_ends, void* workspace, size_t workspace_bytes, void* stream) {
    if (!vis || !flags || !out_flags) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = hyst_check_nsigma(nsigma_time, nsigma_freq)) return rc;
    if (reach < 1 || reach > HYST_MAXREACH)
        return set_err(TRI_EINVAL, "reach must be an integer in [1, %d], got %lld", HYST_MAXREACH, (long long)reach);
    if (int rc = hyst_check_chunks(nchan, chunk_ends, n_chunk_ends)) return rc;
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = hyst_check_shape(n_win, ntime, nchan, n_chunk_ends)) return rc;
    const size_t N = (size_t)n_win * ntime * nchan;
    if (ranges_overlap(out_flags, N, flags, N) || (missing && ranges_overlap(out_flags, N, missing, N)))
        return set_err(TRI_EINVAL, "out_flags must not overlap flags or missing");
    if (int rc = hyst_check_workspace(workspace, workspace_bytes, n_win, ntime, nchan, n_chunk_ends)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const HystWs w = hyst_carve(workspace, n_win, ntime, nchan, n_chunk_ends);
    if (int rc = hyst_eligible(st, vis, vis_dtype, flags, missing, n_win, ntime, nchan, nsigma_time, nsigma_freq,
                               chunk_ends, n_chunk_ends, w, true, nullptr, nullptr)) return rc;
    return hyst_grow(st, w, flags, out_flags, n_win, ntime, nchan, (int)reach);
}
