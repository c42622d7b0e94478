// Host side of the line-RMS statistics and thresholding of whole timesteps / channels (kernels_linerms.hpp)
#pragma once
// One shape of the power pass for every window (tiles of 64 rows x 1024 channels); two switches, by divisibility and
// alignment alone (DESIGN.md §Line RMS): the power pass loads 16 bytes per lane when nchan % 4 == 0 and the bases
// allow it, the apply pass 16 flags per lane when nchan % 16 == 0 and the bases allow it.  Neither changes a result.
namespace {
struct LrmsWs {
    double *row_sum, *ch_sum, *rms_t, *rms_c;
    int *row_cnt, *ch_cnt;
    uint8_t *bad_t, *bad_c;
    int64_t nstrip, ntiles;
    size_t bytes;
};

LrmsWs lrms_carve(void* ws, int64_t n_win, int64_t ntime, int64_t nchan) {
    LrmsWs w;
    w.nstrip = cdiv(nchan, LRMS_CW);
    w.ntiles = cdiv(ntime, LRMS_TR);
    Bump b(ws, SIZE_MAX, ws == nullptr);
    w.row_sum = b.get<double>((size_t)n_win * ntime * w.nstrip);
    w.ch_sum = b.get<double>((size_t)n_win * w.ntiles * nchan);
    w.rms_t = b.get<double>((size_t)n_win * ntime);
    w.rms_c = b.get<double>((size_t)n_win * nchan);
    w.row_cnt = b.get<int>((size_t)n_win * ntime * w.nstrip);
    w.ch_cnt = b.get<int>((size_t)n_win * w.ntiles * nchan);
    w.bad_t = b.get<uint8_t>((size_t)n_win * ntime);
    w.bad_c = b.get<uint8_t>((size_t)n_win * nchan);
    w.bytes = b.off;
    return w;
}

bool lrms_shape_fits(int64_t n_win, int64_t ntime, int64_t nchan) {
    return ntime < (1ll << 31) && nchan < (1ll << 31) && n_win <= (INT64_MAX / 16 / ntime) / nchan;
}

// shape limits shared by the three entry points; 0 when the shape is fine
int lrms_check_shape(int64_t n_win, int64_t ntime, int64_t nchan) {
    if (!lrms_shape_fits(n_win, ntime, nchan)) return set_err(TRI_EUNSUPPORTED, "window too large");
    // a launch holds fewer than 2^32 threads: 256 per time row in the apply pass, 256 per tile in the power pass
    if (n_win * ntime >= (1ll << 24) || n_win * cdiv(ntime, LRMS_TR) * cdiv(nchan, LRMS_CW) >= (1ll << 24) ||
        n_win * (ntime + nchan) >= (1ll << 31) || cdiv(nchan, 256) > 65535)
        return set_err(TRI_EUNSUPPORTED, "too many lines for one launch: pass fewer windows per call");
    return 0;
}

// power pass and combine: rms (and counts, when asked for) of every line of n_win windows
int lrms_statistics(hipStream_t st, const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_win, int64_t ntime,
                    int64_t nchan, const LrmsWs& w, double* rms_t, double* rms_c, int* cnt_t, int* cnt_c) {
    const bool c64 = vis_dtype == TRI_VIS_C64;
    const bool vec = nchan % 4 == 0 && (uintptr_t)vis % 16 == 0 && (uintptr_t)flags % 4 == 0;
    const dim3 grid((unsigned)(n_win * w.ntiles * w.nstrip));
#define LRMS_POWER(V, VEC)                                                                                        \
    hipLaunchKernelGGL((k_lrms_power<V, VEC>), grid, dim3(LRMS_NT), 0, st, vis, flags, ntime, nchan, (int)w.nstrip, \
                       (int)w.ntiles, w.row_sum, w.row_cnt, w.ch_sum, w.ch_cnt)
    if (c64) { if (vec) LRMS_POWER(TRI_VIS_C64, true); else LRMS_POWER(TRI_VIS_C64, false); }
    else     { if (vec) LRMS_POWER(TRI_VIS_F32, true); else LRMS_POWER(TRI_VIS_F32, false); }
#undef LRMS_POWER
    LAUNCHCHK();
    const int64_t lines = n_win * (ntime + nchan);
    hipLaunchKernelGGL(k_lrms_combine, dim3((unsigned)cdiv(lines, 256)), dim3(256), 0, st, w.row_sum, w.row_cnt,
                       w.ch_sum, w.ch_cnt, n_win, ntime, nchan, (int)w.nstrip, (int)w.ntiles, rms_t, rms_c, cnt_t, cnt_c);
    LAUNCHCHK();
    return TRI_OK;
}
}  // namespace

extern "C" size_t tri_line_rms_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan) {
    if (n_win <= 0 || ntime <= 0 || nchan <= 0) return 0;
    if (!lrms_shape_fits(n_win, ntime, nchan)) return 0;
    return lrms_carve(nullptr, n_win, ntime, nchan).bytes;
}

extern "C" int tri_line_rms(const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_win, int64_t ntime,
                            int64_t nchan, double* rms_time, double* rms_chan, int32_t* count_time,
                            int32_t* count_chan, void* workspace, size_t workspace_bytes, void* stream) {
    if (!vis || !flags || !rms_time || !rms_chan) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = lrms_check_shape(n_win, ntime, nchan)) return rc;
    if (int rc = check_workspace(workspace, workspace_bytes, tri_line_rms_workspace_bytes(n_win, ntime, nchan))) return rc;
    const LrmsWs w = lrms_carve(workspace, n_win, ntime, nchan);
    return lrms_statistics((hipStream_t)stream, vis, vis_dtype, flags, n_win, ntime, nchan, w, rms_time, rms_chan,
                           count_time, count_chan);
}

extern "C" int tri_line_rms_threshold(const void* vis, int vis_dtype, const uint8_t* flags, uint8_t* out_flags,
                                      int64_t n_win, int64_t ntime, int64_t nchan, double nsigma_time,
                                      double nsigma_freq, int flag_low, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    if (!vis || !flags || !out_flags) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (!(nsigma_time >= 0.0) || !(nsigma_freq >= 0.0)) return set_err(TRI_EINVAL, "nsigma must be >= 0");
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = lrms_check_shape(n_win, ntime, nchan)) return rc;
    const size_t N = (size_t)n_win * ntime * nchan;
    if (ranges_overlap(out_flags, N, flags, N)) return set_err(TRI_EINVAL, "out_flags must not overlap flags");
    if (int rc = check_workspace(workspace, workspace_bytes, tri_line_rms_workspace_bytes(n_win, ntime, nchan))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (nsigma_time == 0.0 && nsigma_freq == 0.0) return launch_identity(st, flags, out_flags, N);
    const LrmsWs w = lrms_carve(workspace, n_win, ntime, nchan);
    if (int rc = lrms_statistics(st, vis, vis_dtype, flags, n_win, ntime, nchan, w, w.rms_t, w.rms_c, nullptr, nullptr))
        return rc;
    hipLaunchKernelGGL(k_lrms_decide, dim3((unsigned)n_win, 2), dim3(LRMS_DT), 0, st, w.rms_t, w.rms_c, ntime, nchan,
                       nsigma_time, nsigma_freq, flag_low ? 1 : 0, w.bad_t, w.bad_c);
    LAUNCHCHK();
    const unsigned rows = (unsigned)(n_win * ntime);
    if (nchan % 16 == 0 && (uintptr_t)flags % 16 == 0 && (uintptr_t)out_flags % 16 == 0)
        hipLaunchKernelGGL(k_lrms_apply<true>, dim3(rows, (unsigned)cdiv(nchan, 4096)), dim3(256), 0, st, flags, w.bad_t,
                           w.bad_c, out_flags, ntime, nchan);
    else
        hipLaunchKernelGGL(k_lrms_apply<false>, dim3(rows, (unsigned)cdiv(nchan, 256)), dim3(256), 0, st, flags, w.bad_t,
                           w.bad_c, out_flags, ntime, nchan);
    LAUNCHCHK();
    return TRI_OK;
}
