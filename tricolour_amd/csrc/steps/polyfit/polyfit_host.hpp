// Host side of the piecewise-polynomial fit background and the flagging on it (steps/polyfit/kernels_polyfit.hpp)
#pragma once
// The visibilities are read once (k_pf_prepare) into the workspace's amplitude and state images; the passes work on
// those and k_pf_finish writes the flags (DESIGN.md §Polynomial fit).  Three switches, none of which changes a result:
// the prepare pass handles 4 samples per lane when nchan % 4 == 0 and the bases allow 16-byte accesses, the finish pass
// 16 per lane when nchan % 16 == 0 and the bases allow it, and the frequency pass keeps lines of up to 4096 channels in
// a quarter of the LDS that longer ones need.  A fitted line holds at most PF_MAX_LINE samples.
namespace {
enum { PF_ORDER_FREQTIME = 0, PF_ORDER_TIMEFREQ = 1, PF_ORDER_FREQ = 2, PF_ORDER_TIME = 3 };
enum { PF_AXIS_TIME = 0, PF_AXIS_FREQ = 1 };

struct PfWs {
    float* amp;
    uint8_t* state;
    double* coef;
    size_t bytes;
};

PfWs pf_carve(void* ws, int64_t n_win, int64_t ntime, int64_t nchan, int64_t time_pieces) {
    PfWs w;
    const size_t N = (size_t)n_win * ntime * nchan;
    Bump b(ws, SIZE_MAX, ws == nullptr);
    w.amp = b.get<float>(N);
    w.state = b.get<uint8_t>(N);
    w.coef = b.get<double>((size_t)n_win * time_pieces * PF_CS * nchan);
    w.bytes = b.off;
    return w;
}

bool pf_shape_fits(int64_t n_win, int64_t ntime, int64_t nchan) {
    return ntime < (1ll << 31) && nchan < (1ll << 31) && n_win <= (INT64_MAX / 16 / ntime) / nchan;
}

// shape limits of the entry points, `time` / `freq`: whether that axis is fitted; 0 when the shape is fine
int pf_check_shape(int64_t n_win, int64_t ntime, int64_t nchan, bool time, bool freq) {
    if (!pf_shape_fits(n_win, ntime, nchan)) return set_err(TRI_EUNSUPPORTED, "window too large");
    if ((time && ntime > PF_MAX_LINE) || (freq && nchan > PF_MAX_LINE))
        return set_err(TRI_EUNSUPPORTED, "a fitted line holds at most %d samples, got %lld times and %lld channels",
                       PF_MAX_LINE, (long long)ntime, (long long)nchan);
    // every launch is one-dimensional and holds fewer than 2^31 blocks: one per row in the frequency pass, one per
    // PF_NT samples in the prepare and finish passes
    const int64_t lim = (1ll << 31) - 1;
    if (n_win > lim / ntime || n_win > lim / (ntime * cdiv(nchan, PF_NT)))
        return set_err(TRI_EUNSUPPORTED, "too many lines for one launch: pass fewer windows per call");
    return 0;
}

int pf_check_fit(const char* axis, int64_t degree, int64_t pieces) {
    if (degree < 0 || degree > 3)
        return set_err(TRI_EINVAL, "%s_degree must be an integer in [0, 3], got %lld", axis, (long long)degree);
    if (pieces < 1 || pieces > PF_MAX_PIECES)
        return set_err(TRI_EINVAL, "%s_pieces must be an integer in [1, %d], got %lld", axis, PF_MAX_PIECES, (long long)pieces);
    return 0;
}

int pf_check_cutoff(const char* axis, double cutoff) {
    if (!(cutoff > 0.0) || std::isinf(cutoff)) return set_err(TRI_EINVAL, "%s_cutoff must be a finite number > 0", axis);
    return 0;
}

struct PfShape {
    int64_t n_win;
    int ntime, nchan;
};

int pf_prepare(hipStream_t st, const void* vis, int vis_dtype, const uint8_t* flags, const PfShape& s, const PfWs& w) {
    const int64_t N = s.n_win * s.ntime * s.nchan;
    const bool vec = s.nchan % 4 == 0 && (uintptr_t)vis % 16 == 0 && (uintptr_t)flags % 4 == 0 &&
                     (uintptr_t)w.amp % 16 == 0 && (uintptr_t)w.state % 4 == 0;
    const dim3 grid((unsigned)cdiv(cdiv(N, vec ? 4 : 1), PF_NT));
#define PF_PREPARE(V, VEC) hipLaunchKernelGGL((k_pf_prepare<V, VEC>), grid, dim3(PF_NT), 0, st, vis, flags, N, w.amp, w.state)
    if (vis_dtype == TRI_VIS_C64) { if (vec) PF_PREPARE(TRI_VIS_C64, true); else PF_PREPARE(TRI_VIS_C64, false); }
    else                          { if (vec) PF_PREPARE(TRI_VIS_F32, true); else PF_PREPARE(TRI_VIS_F32, false); }
#undef PF_PREPARE
    LAUNCHCHK();
    return TRI_OK;
}

// one pass along time; bg != NULL: the background call
int pf_time(hipStream_t st, const PfShape& s, const PfWs& w, int pieces_alloc, int pieces, int degree, double cutoff,
            int rounds, int min_samples, float* bg) {
    const int nstrip = (int)cdiv(s.nchan, PF_NT);
    const dim3 grid((unsigned)(s.n_win * nstrip));
    if (bg)
        hipLaunchKernelGGL(k_pf_time<true>, grid, dim3(PF_NT), 0, st, w.amp, w.state, s.ntime, s.nchan, nstrip,
                           pieces_alloc, pieces, degree, cutoff, rounds, min_samples, w.coef, bg);
    else
        hipLaunchKernelGGL(k_pf_time<false>, grid, dim3(PF_NT), 0, st, w.amp, w.state, s.ntime, s.nchan, nstrip,
                           pieces_alloc, pieces, degree, cutoff, rounds, min_samples, w.coef, bg);
    LAUNCHCHK();
    return TRI_OK;
}

// one pass along frequency; bg != NULL: the background call
int pf_freq(hipStream_t st, const PfShape& s, const PfWs& w, int pieces, int degree, double cutoff, int rounds,
            int min_samples, float* bg) {
    const dim3 grid((unsigned)(s.n_win * s.ntime));
    const bool small = s.nchan <= 4096;
#define PF_FREQ(CAP, BG)                                                                                             \
    hipLaunchKernelGGL((k_pf_freq<CAP, BG>), grid, dim3(PF_NT), 0, st, w.amp, w.state, s.nchan, pieces, degree, cutoff, \
                       rounds, min_samples, bg)
    if (bg) { if (small) PF_FREQ(4096, true); else PF_FREQ(16384, true); }
    else    { if (small) PF_FREQ(4096, false); else PF_FREQ(16384, false); }
#undef PF_FREQ
    LAUNCHCHK();
    return TRI_OK;
}

int pf_finish(hipStream_t st, const PfShape& s, const PfWs& w, uint8_t* out) {
    const int64_t N = s.n_win * s.ntime * s.nchan;
    const bool vec = s.nchan % 16 == 0 && (uintptr_t)w.state % 16 == 0 && (uintptr_t)out % 16 == 0;
    const dim3 grid((unsigned)cdiv(cdiv(N, vec ? 16 : 1), PF_NT));
    if (vec) hipLaunchKernelGGL(k_pf_finish<true>, grid, dim3(PF_NT), 0, st, w.state, out, N);
    else     hipLaunchKernelGGL(k_pf_finish<false>, grid, dim3(PF_NT), 0, st, w.state, out, N);
    LAUNCHCHK();
    return TRI_OK;
}
}  // namespace

extern "C" size_t tri_polyfit_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan, int64_t time_pieces) {
    if (n_win <= 0 || ntime <= 0 || nchan <= 0 || time_pieces < 0 || time_pieces > PF_MAX_PIECES) return 0;
    if (!pf_shape_fits(n_win, ntime, nchan)) return 0;
    return pf_carve(nullptr, n_win, ntime, nchan, time_pieces).bytes;
}

extern "C" int tri_polyfit_background(const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_win, int64_t ntime,
                                      int64_t nchan, int axis, int64_t pieces, int64_t degree, float* background,
                                      void* scratch, size_t scratch_bytes, void* stream) {
    if (!vis || !flags || !background) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (axis != PF_AXIS_TIME && axis != PF_AXIS_FREQ) return set_err(TRI_EINVAL, "axis must be 0 (time) or 1 (frequency)");
    if (int rc = pf_check_fit(axis == PF_AXIS_TIME ? "time" : "freq", degree, pieces)) return rc;
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    const bool time = axis == PF_AXIS_TIME;
    if (int rc = pf_check_shape(n_win, ntime, nchan, time, !time)) return rc;
    const size_t N = (size_t)n_win * ntime * nchan, nv = N * (vis_dtype == TRI_VIS_C64 ? 8 : 4);
    if (ranges_overlap(background, N * 4, vis, nv) || ranges_overlap(background, N * 4, flags, N))
        return set_err(TRI_EINVAL, "background must not overlap an input");
    const int64_t tp = time ? pieces : 0;
    const size_t need = tri_polyfit_workspace_bytes(n_win, ntime, nchan, tp);
    if (int rc = check_workspace(scratch, scratch_bytes, need)) return rc;
    if (ranges_overlap(scratch, need, vis, nv) || ranges_overlap(scratch, need, flags, N) ||
        ranges_overlap(scratch, need, background, N * 4))
        return set_err(TRI_EINVAL, "the scratch buffer must not overlap an input or the output");
    hipStream_t st = (hipStream_t)stream;
    const PfWs w = pf_carve(scratch, n_win, ntime, nchan, tp);
    const PfShape s{n_win, (int)ntime, (int)nchan};
    if (int rc = pf_prepare(st, vis, vis_dtype, flags, s, w)) return rc;
    if (time) return pf_time(st, s, w, (int)tp, (int)pieces, (int)degree, 0.0, 1, 0, background);
    return pf_freq(st, s, w, (int)pieces, (int)degree, 0.0, 1, 0, background);
}

extern "C" int tri_polyfit_threshold(const void* vis, int vis_dtype, const uint8_t* flags, uint8_t* out_flags,
                                     int64_t n_win, int64_t ntime, int64_t nchan, int order, double time_cutoff,
                                     int64_t time_degree, int64_t time_pieces, double freq_cutoff, int64_t freq_degree,
                                     int64_t freq_pieces, int64_t rounds, int64_t min_samples, void* scratch,
                                     size_t scratch_bytes, void* stream) {
    if (!vis || !flags || !out_flags) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (order < PF_ORDER_FREQTIME || order > PF_ORDER_TIME)
        return set_err(TRI_EINVAL, "order must be 0 (freqtime), 1 (timefreq), 2 (freq) or 3 (time)");
    if (int rc = pf_check_cutoff("time", time_cutoff)) return rc;
    if (int rc = pf_check_cutoff("freq", freq_cutoff)) return rc;
    if (int rc = pf_check_fit("time", time_degree, time_pieces)) return rc;
    if (int rc = pf_check_fit("freq", freq_degree, freq_pieces)) return rc;
    if (rounds < 1 || rounds > PF_MAX_ROUNDS)
        return set_err(TRI_EINVAL, "rounds must be an integer in [1, %d], got %lld", PF_MAX_ROUNDS, (long long)rounds);
    if (min_samples < 2 || min_samples > INT32_MAX)
        return set_err(TRI_EINVAL, "min_samples must be an integer >= 2, got %lld", (long long)min_samples);
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    const bool time = order != PF_ORDER_FREQ, freq = order != PF_ORDER_TIME;
    if (int rc = pf_check_shape(n_win, ntime, nchan, time, freq)) return rc;
    const size_t N = (size_t)n_win * ntime * nchan, nv = N * (vis_dtype == TRI_VIS_C64 ? 8 : 4);
    if (ranges_overlap(out_flags, N, vis, nv) || ranges_overlap(out_flags, N, flags, N))
        return set_err(TRI_EINVAL, "out_flags must not overlap an input");
    const size_t need = tri_polyfit_workspace_bytes(n_win, ntime, nchan, time_pieces);
    if (int rc = check_workspace(scratch, scratch_bytes, need)) return rc;
    if (ranges_overlap(scratch, need, vis, nv) || ranges_overlap(scratch, need, flags, N) ||
        ranges_overlap(scratch, need, out_flags, N))
        return set_err(TRI_EINVAL, "the scratch buffer must not overlap an input or the output");
    hipStream_t st = (hipStream_t)stream;
    const PfWs w = pf_carve(scratch, n_win, ntime, nchan, time_pieces);
    const PfShape s{n_win, (int)ntime, (int)nchan};
    if (int rc = pf_prepare(st, vis, vis_dtype, flags, s, w)) return rc;
    // the second pass finds the first one's hits in the state image: its mask is valid & ~hits_first
    const bool time_first = order == PF_ORDER_TIMEFREQ || order == PF_ORDER_TIME;
    const int npass = time && freq ? 2 : 1;
    for (int pass = 0; pass < npass; pass++) {
        if ((pass == 0) == time_first) {
            if (int rc = pf_time(st, s, w, (int)time_pieces, (int)time_pieces, (int)time_degree, time_cutoff, (int)rounds,
                                 (int)min_samples, nullptr))
                return rc;
        } else {
            if (int rc = pf_freq(st, s, w, (int)freq_pieces, (int)freq_degree, freq_cutoff, (int)rounds, (int)min_samples,
                                 nullptr))
                return rc;
        }
    }
    return pf_finish(st, s, w, out_flags);
}
