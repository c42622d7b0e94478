// Host side of the scale-invariant rank operator (kernels_sir.hpp): out = f | SIR_time(f) | SIR_freq(f) per (bl, corr) window
#pragma once
// Routes, by line length alone:
//   time  (n = ntime, 64 adjacent channels per block):  n <= 64: 256 threads x 1 sub-chunk;  n <= 256: 1024 x 1;
//         n <= 1024: 1024 x 4;  longer: segments of 1024 samples (1024 x 4), three launches through the workspace
//   freq  (n = nchan):  n <= 256: 16 lines per block, 256 threads x 1;  n <= 4096: one line per block, 256 x 1;
//         n <= 16384: 1024 x 1;  n <= 65536: 512 x 8;  longer: segments of 65536 (512 x 8) through the workspace
// The masked operator (tri_scale_invariant_rank_masked, k_sir<..., MISSING = true>) takes the same routes with the same
// geometry; per (line, segment) its workspace holds one 64-bit (U, M) count where the unmasked one holds an int.
#define SIR_TIME_SEG 1024
#define SIR_FREQ_SEG 65536

static size_t sir_ws_part(int64_t lines, int64_t n, int64_t seglen, size_t count_bytes) {
    if (n <= seglen) return 0;
    size_t e = (size_t)lines * (size_t)cdiv(n, seglen);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    return al(e * count_bytes) + 2 * al(e * sizeof(double));
}

extern "C" size_t tri_sir_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan) {
    if (n_win <= 0 || ntime <= 0 || nchan <= 0) return 0;
    // the two axes run one after the other and share the workspace
    return std::max(sir_ws_part(n_win * nchan, ntime, SIR_TIME_SEG, sizeof(int)),
                    sir_ws_part(n_win * ntime, nchan, SIR_FREQ_SEG, sizeof(int)));
}

extern "C" size_t tri_sir_masked_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan) {
    if (n_win <= 0 || ntime <= 0 || nchan <= 0) return 0;
    return std::max(sir_ws_part(n_win * nchan, ntime, SIR_TIME_SEG, sizeof(unsigned long long)),
                    sir_ws_part(n_win * ntime, nchan, SIR_FREQ_SEG, sizeof(unsigned long long)));
}

// miss == nullptr: the unmasked operator (penalty unused)
struct SirMissing {
    const uint8_t* miss;
    double penalty;
};

template <int NT, int CB, int K, bool TIME, bool VEC, bool OR, bool MISSING>
static int launch_sir(hipStream_t st, const uint8_t* in, uint8_t* out, int64_t nlines, int64_t ntime, int64_t nchan,
                      double eta, void* ws, SirMissing mi) {
    constexpr int SPAN = NT / CB * 16 * K;
    const int64_t n = TIME ? ntime : nchan;
    const int64_t gx = cdiv(nlines, CB);
    if (gx >= (1ll << 31)) return set_err(TRI_EUNSUPPORTED, "too many lines for one launch");
    if (n <= SPAN) {
        hipLaunchKernelGGL((k_sir<NT, CB, K, SIR_FULL, TIME, VEC, OR, MISSING>), dim3((unsigned)gx), dim3(NT), 0, st, in,
                           out, nlines, ntime, nchan, eta, 1, nullptr, nullptr, nullptr, mi.miss, mi.penalty);
        LAUNCHCHK();
        return TRI_OK;
    }
    const int64_t nseg = cdiv(n, SPAN);
    if (nseg > 65535) return set_err(TRI_EUNSUPPORTED, "line too long");
    const size_t e = (size_t)nlines * nseg;
    Bump b(ws, SIZE_MAX, false);
    int* cnt = MISSING ? (int*)b.get<unsigned long long>(e) : b.get<int>(e);
    double* mn = b.get<double>(e);
    double* mx = b.get<double>(e);
    dim3 grid((unsigned)gx, (unsigned)nseg);
    hipLaunchKernelGGL((k_sir<NT, CB, K, SIR_COUNT, TIME, VEC, OR, MISSING>), grid, dim3(NT), 0, st, in, out, nlines,
                       ntime, nchan, eta, (int)nseg, cnt, mn, mx, mi.miss, mi.penalty);
    hipLaunchKernelGGL((k_sir<NT, CB, K, SIR_MINMAX, TIME, VEC, OR, MISSING>), grid, dim3(NT), 0, st, in, out, nlines,
                       ntime, nchan, eta, (int)nseg, cnt, mn, mx, mi.miss, mi.penalty);
    hipLaunchKernelGGL((k_sir<NT, CB, K, SIR_FINAL, TIME, VEC, OR, MISSING>), grid, dim3(NT), 0, st, in, out, nlines,
                       ntime, nchan, eta, (int)nseg, cnt, mn, mx, mi.miss, mi.penalty);
    LAUNCHCHK();
    return TRI_OK;
}

template <bool VEC, bool OR, bool MISSING>
static int launch_sir_freq(hipStream_t st, const uint8_t* in, uint8_t* out, int64_t n_win, int64_t ntime,
                           int64_t nchan, double eta, void* ws, SirMissing mi) {
    const int64_t lines = n_win * ntime;
    if (nchan <= 256) return launch_sir<256, 16, 1, false, VEC, OR, MISSING>(st, in, out, lines, ntime, nchan, eta, ws, mi);
    if (nchan <= 4096) return launch_sir<256, 1, 1, false, VEC, OR, MISSING>(st, in, out, lines, ntime, nchan, eta, ws, mi);
    if (nchan <= 16384) return launch_sir<1024, 1, 1, false, VEC, OR, MISSING>(st, in, out, lines, ntime, nchan, eta, ws, mi);
    // 512 x 8 rather than 1024 x 4: the latter needs more than the 128 VGPRs a 1024-thread block allows and spills
    return launch_sir<512, 1, 8, false, VEC, OR, MISSING>(st, in, out, lines, ntime, nchan, eta, ws, mi);   // segments beyond 65536
}

template <bool MISSING>
static int launch_sir_time(hipStream_t st, const uint8_t* in, uint8_t* out, int64_t n_win, int64_t ntime,
                           int64_t nchan, double eta, void* ws, SirMissing mi) {
    const int64_t lines = n_win * nchan;
    if (ntime <= 64) return launch_sir<256, 64, 1, true, false, false, MISSING>(st, in, out, lines, ntime, nchan, eta, ws, mi);
    if (ntime <= 256) return launch_sir<1024, 64, 1, true, false, false, MISSING>(st, in, out, lines, ntime, nchan, eta, ws, mi);
    return launch_sir<1024, 64, 4, true, false, false, MISSING>(st, in, out, lines, ntime, nchan, eta, ws, mi);   // segments beyond 1024
}
static_assert(SIR_TIME_SEG == 1024 / 64 * 16 * 4 && SIR_FREQ_SEG == 512 * 16 * 8, "segment lengths follow the widest routes");

// both entry points; MISSING: `mi.miss` has been checked by the caller
template <bool MISSING>
static int sir_run(const uint8_t* flags, uint8_t* out_flags, int64_t n_win, int64_t ntime, int64_t nchan,
                   double eta_time, double eta_freq, SirMissing mi, void* workspace, size_t workspace_bytes, void* stream) {
    if (!flags || !out_flags) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (!(eta_time >= 0.0 && eta_time < 1.0) || !(eta_freq >= 0.0 && eta_freq < 1.0))
        return set_err(TRI_EINVAL, "eta must lie in [0, 1)");
    if (n_win == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (ntime >= (1ll << 31) || nchan >= (1ll << 31) || n_win > (INT64_MAX / ntime) / nchan)
        return set_err(TRI_EUNSUPPORTED, "window too large");
    const size_t N = (size_t)n_win * ntime * nchan;
    if (ranges_overlap(out_flags, N, flags, N)) return set_err(TRI_EINVAL, "out_flags must not overlap flags");
    if (MISSING && ranges_overlap(out_flags, N, mi.miss, N))
        return set_err(TRI_EINVAL, "out_flags must not overlap missing");
    const size_t need = MISSING ? tri_sir_masked_workspace_bytes(n_win, ntime, nchan) : tri_sir_workspace_bytes(n_win, ntime, nchan);
    // short lines need no workspace: NULL is fine then
    if (need > 0)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool t = eta_time > 0.0, f = eta_freq > 0.0;
    if (!t && !f) return launch_identity(st, flags, out_flags, N);
    if (t) {
        int rc = launch_sir_time<MISSING>(st, flags, out_flags, n_win, ntime, nchan, eta_time, workspace, mi);
        if (rc) return rc;
    }
    if (f) {
        // both axes read the INPUT mask; the frequency pass ORs into the time pass's result
        const bool vec = nchan % 16 == 0 && (uintptr_t)flags % 16 == 0 && (uintptr_t)out_flags % 16 == 0 &&
                         (!MISSING || (uintptr_t)mi.miss % 16 == 0);
        int rc = vec ? (t ? launch_sir_freq<true, true, MISSING>(st, flags, out_flags, n_win, ntime, nchan, eta_freq, workspace, mi)
                          : launch_sir_freq<true, false, MISSING>(st, flags, out_flags, n_win, ntime, nchan, eta_freq, workspace, mi))
                     : (t ? launch_sir_freq<false, true, MISSING>(st, flags, out_flags, n_win, ntime, nchan, eta_freq, workspace, mi)
                          : launch_sir_freq<false, false, MISSING>(st, flags, out_flags, n_win, ntime, nchan, eta_freq, workspace, mi));
        if (rc) return rc;
    }
    return TRI_OK;
}

extern "C" int tri_scale_invariant_rank(const uint8_t* flags, uint8_t* out_flags, int64_t n_win, int64_t ntime,
                                        int64_t nchan, double eta_time, double eta_freq, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    return sir_run<false>(flags, out_flags, n_win, ntime, nchan, eta_time, eta_freq, SirMissing{nullptr, 0.0}, workspace,
                          workspace_bytes, stream);
}

extern "C" int tri_scale_invariant_rank_masked(const uint8_t* flags, const uint8_t* missing, uint8_t* out_flags,
                                               int64_t n_win, int64_t ntime, int64_t nchan, double eta_time,
                                               double eta_freq, double penalty, void* workspace, size_t workspace_bytes,
                                               void* stream) {
    if (!missing) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (!(penalty >= 0.0) || !std::isfinite(penalty)) return set_err(TRI_EINVAL, "penalty must be finite and >= 0");
    return sir_run<true>(flags, out_flags, n_win, ntime, nchan, eta_time, eta_freq, SirMissing{missing, penalty}, workspace,
                         workspace_bytes, stream);
}
