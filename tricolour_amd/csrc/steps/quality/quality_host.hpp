// Host side of the quality statistics of the unflagged samples (steps/quality/kernels_quality.hpp)
#pragma once
// One route per dtype, by divisibility and alignment alone: the walk loads 16 bytes per lane when nchan % QUAL_V == 0 and
// the bases allow it.  It changes no result.
namespace {
struct QualWs {
    QualRow* rows;              // (n_win, nstrips, ntime)
    long long *ccnt, *tcnt;     // (n_win, 2, nchan), (n_win, 2, ntime)
    double *csum, *tsum;        // (n_win, 4, nchan), (n_win, 4, ntime)
    size_t bytes;
};

QualWs qual_carve(void* ws, int64_t n_win, int64_t ntime, int64_t nchan) {
    QualWs w;
    const size_t nstrips = (size_t)cdiv(nchan, QUAL_SW);
    Bump b(ws, SIZE_MAX, ws == nullptr);
    w.rows = b.get<QualRow>((size_t)n_win * nstrips * (size_t)ntime);
    w.ccnt = b.get<long long>((size_t)n_win * 2 * (size_t)nchan);
    w.tcnt = b.get<long long>((size_t)n_win * 2 * (size_t)ntime);
    w.csum = b.get<double>((size_t)n_win * 4 * (size_t)nchan);
    w.tsum = b.get<double>((size_t)n_win * 4 * (size_t)ntime);
    w.bytes = b.off;
    return w;
}

// every launch is one-dimensional and holds fewer than 2^31 blocks; every index fits 63 bits
bool qual_shape_fits(int64_t n_bl, int64_t n_corr, int64_t ntime, int64_t nchan) {
    const int64_t lim = (1ll << 31) - 1;
    if (ntime > lim || nchan > lim - QUAL_SW || n_corr > lim || n_bl > lim) return false;
    const int64_t n_win = n_bl * n_corr;
    if (n_win > lim) return false;
    const int64_t ngroups = cdiv(cdiv(nchan, QUAL_SW), QUAL_WPB);
    if (n_win > lim / ngroups) return false;
    if (n_corr > lim * QUAL_NT / 6 / std::max(ntime, nchan)) return false;
    return n_win <= (INT64_MAX / 64 / ntime) / nchan;
}
}  // namespace

extern "C" size_t tri_quality_workspace_bytes(int64_t n_bl, int64_t n_corr, int64_t ntime, int64_t nchan) {
    if (n_bl <= 0 || n_corr <= 0 || ntime <= 0 || nchan <= 0) return 0;
    if (!qual_shape_fits(n_bl, n_corr, ntime, nchan)) return 0;
    return qual_carve(nullptr, n_bl * n_corr, ntime, nchan).bytes;
}

extern "C" int tri_window_quality(const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_bl, int64_t n_corr,
                                  int64_t ntime, int64_t nchan, int64_t* counts_bl, double* sums_bl,
                                  int64_t* counts_time, double* sums_time, int64_t* counts_chan, double* sums_chan,
                                  int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    if (!vis || !flags || !counts_bl || !sums_bl || !counts_time || !sums_time || !counts_chan || !sums_chan)
        return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_bl < 0 || n_corr < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EINVAL, "vis dtype must be complex64 or float32");
    hipStream_t st = (hipStream_t)stream;
    const int64_t lim = (1ll << 31) - 1;
    if (n_bl == 0 || n_corr == 0 || ntime == 0 || nchan == 0) {
        // no sample: the bl cells are zeros, the others are zeros or stay
        if (n_bl > lim || n_corr > lim || ntime > lim || nchan > lim) return set_err(TRI_EUNSUPPORTED, "window too large");
        const size_t nb = (size_t)(n_bl * n_corr), nt = (size_t)(n_corr * ntime), nc = (size_t)(n_corr * nchan);
        if (nb) {
            HIPCHK(hipMemsetAsync(counts_bl, 0, 2 * nb * sizeof(int64_t), st));
            HIPCHK(hipMemsetAsync(sums_bl, 0, 4 * nb * sizeof(double), st));
        }
        if (!accumulate && nt) {
            HIPCHK(hipMemsetAsync(counts_time, 0, 2 * nt * sizeof(int64_t), st));
            HIPCHK(hipMemsetAsync(sums_time, 0, 4 * nt * sizeof(double), st));
        }
        if (!accumulate && nc) {
            HIPCHK(hipMemsetAsync(counts_chan, 0, 2 * nc * sizeof(int64_t), st));
            HIPCHK(hipMemsetAsync(sums_chan, 0, 4 * nc * sizeof(double), st));
        }
        return TRI_OK;
    }
    if (!qual_shape_fits(n_bl, n_corr, ntime, nchan))
        return set_err(TRI_EUNSUPPORTED, "window too large for one launch: pass fewer baselines per call");
    const int64_t n_win = n_bl * n_corr;
    {
        const size_t N = (size_t)n_win * ntime * nchan;
        const void* p[8] = {vis, flags, counts_bl, sums_bl, counts_time, sums_time, counts_chan, sums_chan};
        const size_t nb[8] = {N * (vis_dtype == TRI_VIS_C64 ? 8 : 4), N, (size_t)n_win * 16, (size_t)n_win * 32,
                              (size_t)(n_corr * ntime) * 16, (size_t)(n_corr * ntime) * 32,
                              (size_t)(n_corr * nchan) * 16, (size_t)(n_corr * nchan) * 32};
        for (int a = 2; a < 8; a++)
            for (int b = 0; b < a; b++)
                if (ranges_overlap(p[a], nb[a], p[b], nb[b]))
                    return set_err(TRI_EINVAL, "outputs must not overlap the inputs or each other");
    }
    const QualWs w = qual_carve(workspace, n_win, ntime, nchan);
    if (int rc = check_workspace(workspace, workspace_bytes, w.bytes)) return rc;

    const int nstrips = (int)cdiv(nchan, QUAL_SW), ngroups = (int)cdiv(nstrips, QUAL_WPB);
    const dim3 grid((unsigned)(n_win * ngroups));
    const bool c64 = vis_dtype == TRI_VIS_C64;
    const bool vec = nchan % QUAL_V == 0 && (uintptr_t)vis % 16 == 0 && (uintptr_t)flags % 4 == 0;
    if (c64 && vec)
        hipLaunchKernelGGL((k_quality_walk<TRI_VIS_C64, true>), grid, dim3(QUAL_NT), 0, st, vis, flags, ntime, nchan, nstrips,
                           ngroups, w.rows, w.ccnt, w.csum);
    else if (c64)
        hipLaunchKernelGGL((k_quality_walk<TRI_VIS_C64, false>), grid, dim3(QUAL_NT), 0, st, vis, flags, ntime, nchan, nstrips,
                           ngroups, w.rows, w.ccnt, w.csum);
    else if (vec)
        hipLaunchKernelGGL((k_quality_walk<TRI_VIS_F32, true>), grid, dim3(QUAL_NT), 0, st, vis, flags, ntime, nchan, nstrips,
                           ngroups, w.rows, w.ccnt, w.csum);
    else
        hipLaunchKernelGGL((k_quality_walk<TRI_VIS_F32, false>), grid, dim3(QUAL_NT), 0, st, vis, flags, ntime, nchan, nstrips,
                           ngroups, w.rows, w.ccnt, w.csum);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_quality_window, dim3((unsigned)n_win), dim3(QUAL_NT), 0, st, (const QualRow*)w.rows, n_win, ntime,
                       nstrips, w.tcnt, w.tsum, (long long*)counts_bl, sums_bl);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_quality_fold, dim3((unsigned)cdiv(6 * n_corr * ntime, QUAL_NT)), dim3(QUAL_NT), 0, st,
                       (const long long*)w.tcnt, (const double*)w.tsum, n_bl, n_corr, ntime, (long long*)counts_time,
                       sums_time, accumulate);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_quality_fold, dim3((unsigned)cdiv(6 * n_corr * nchan, QUAL_NT)), dim3(QUAL_NT), 0, st,
                       (const long long*)w.ccnt, (const double*)w.csum, n_bl, n_corr, nchan, (long long*)counts_chan,
                       sums_chan, accumulate);
    LAUNCHCHK();
    return TRI_OK;
}
