// Host side of the log-binned amplitude histograms of the kept and the flagged samples (steps/hist/kernels_hist.hpp)
#pragma once
// One route per dtype, by divisibility and alignment alone (16-byte loads when nchan % HIST_V == 0 and the bases allow
// it).  It changes no result.  No workspace: the chunk ends travel as kernel arguments, HIST_CPL chunks per launch.
namespace {
template <int VIS, bool VEC>
void hist_launch(hipStream_t st, dim3 grid, size_t lds, const void* vis, const uint8_t* flags, int64_t ntime, int64_t nchan,
                 int n_corr, int nbands, int64_t nchunks, const HistChunks& ch, int ebase, int shift, int nb,
                 int64_t* hist_bl, int64_t* hist_chunk) {
    hipLaunchKernelGGL((k_hist_fill<VIS, VEC>), grid, dim3(HIST_NT), lds, st, vis, flags, ntime, nchan, n_corr, nbands, nchunks,
                       ch, ebase, shift, nb, (unsigned long long*)hist_bl, (unsigned long long*)hist_chunk);
}
}  // namespace

extern "C" int64_t tri_histogram_slots(int emin, int emax, int sub_bits) {
    if (emin < -126 || emax > 128 || emin >= emax || sub_bits < 0 || sub_bits > 5) return 0;
    const int64_t nb = (int64_t)(emax - emin) << sub_bits;
    return nb <= TRI_MAX_HIST_BINS ? nb + 3 : 0;
}

extern "C" int tri_amplitude_histogram(const void* vis, int vis_dtype, const uint8_t* flags, int64_t n_bl, int64_t n_corr,
                                       int64_t ntime, int64_t nchan, const int64_t* chunk_ends, int64_t n_chunk_ends,
                                       int emin, int emax, int sub_bits, int64_t* hist_bl, int64_t* hist_chunk,
                                       int accumulate, void* stream) {
    if (!vis || !flags || !chunk_ends || !hist_bl || !hist_chunk) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_bl < 0 || n_corr < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EINVAL, "vis dtype must be complex64 or float32");
    const int64_t slots = tri_histogram_slots(emin, emax, sub_bits);
    if (slots == 0)
        return set_err(TRI_EINVAL, "bins must have -126 <= emin < emax <= 128, 0 <= sub_bits <= 5 and at most %d bins",
                       TRI_MAX_HIST_BINS);
    // (too many ends are unsupported here, not invalid: answered ahead of the shared check, which excludes fewer than 2)
    if (n_chunk_ends > (1ll << 30)) return set_err(TRI_EUNSUPPORTED, "at most 2^30 chunk ends");
    int64_t widest = 0;
    if (int rc = check_chunk_ends(nchan, chunk_ends, n_chunk_ends, &widest)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t lim = (1ll << 31) - 1, nchunks = n_chunk_ends - 1, cells = 2 * slots;
    if (n_bl > lim || n_corr > lim || ntime > lim || nchan > lim || n_bl * n_corr > lim ||
        n_corr > (INT64_MAX / 64 / cells) / nchunks)
        return set_err(TRI_EUNSUPPORTED, "window too large");
    const int64_t n_win = n_bl * n_corr;
    const size_t bytes_bl = (size_t)(n_win * cells) * sizeof(int64_t);
    const size_t bytes_chunk = (size_t)(n_corr * nchunks * cells) * sizeof(int64_t);
    if (n_win == 0 || ntime == 0 || nchan == 0) {
        // no sample: the bl cells are zeros, the chunk cells are zeros or stay
        if (bytes_bl) HIPCHK(hipMemsetAsync(hist_bl, 0, bytes_bl, st));
        if (!accumulate && bytes_chunk) HIPCHK(hipMemsetAsync(hist_chunk, 0, bytes_chunk, st));
        return TRI_OK;
    }
    const int64_t nbands = cdiv(ntime, HIST_ROWS);
    if (n_win > HIST_MAX_GRID_X / nbands)
        return set_err(TRI_EUNSUPPORTED, "window too large for one launch: pass fewer baselines per call");
    if (cdiv(widest, HIST_SPAN) > 65535) return set_err(TRI_EUNSUPPORTED, "a frequency chunk is too wide");
    if (n_win > (INT64_MAX / 64 / ntime) / nchan) return set_err(TRI_EUNSUPPORTED, "window too large");
    {
        const size_t N = (size_t)n_win * ntime * nchan;
        const void* p[4] = {vis, flags, hist_bl, hist_chunk};
        const size_t nby[4] = {N * (vis_dtype == TRI_VIS_C64 ? 8 : 4), N, bytes_bl, bytes_chunk};
        for (int a = 2; a < 4; a++)
            for (int b = 0; b < a; b++)
                if (ranges_overlap(p[a], nby[a], p[b], nby[b]))
                    return set_err(TRI_EINVAL, "outputs must not overlap the inputs or each other");
    }
    HIPCHK(hipMemsetAsync(hist_bl, 0, bytes_bl, st));
    if (!accumulate) HIPCHK(hipMemsetAsync(hist_chunk, 0, bytes_chunk, st));

    const int nb = (int)slots - 3, ebase = (emin + 127) << sub_bits, shift = 23 - sub_bits;
    const size_t lds = (size_t)cells * sizeof(unsigned);
    const bool c64 = vis_dtype == TRI_VIS_C64;
    const bool vec = nchan % HIST_V == 0 && (uintptr_t)vis % 16 == 0 && (uintptr_t)flags % 4 == 0;
    for (int64_t g0 = 0; g0 < nchunks; g0 += HIST_CPL) {
        HistChunks ch;
        const int n = (int)std::min<int64_t>(HIST_CPL, nchunks - g0);
        int64_t wide = 0;
        for (int j = 0; j < HIST_CPL; j++) {
            const int64_t g = g0 + (j < n ? j : 0);             // the unused rows repeat the first: never indexed
            ch.lo[j] = (int)chunk_ends[g];
            ch.hi[j] = (int)chunk_ends[g + 1];
            ch.idx[j] = (int)g;
            if (j < n) wide = std::max(wide, chunk_ends[g + 1] - chunk_ends[g]);
        }
        if (wide == 0) continue;                                // nothing but empty chunks
        const dim3 grid((unsigned)(n_win * nbands), (unsigned)n, (unsigned)cdiv(wide, HIST_SPAN));
        if (c64 && vec)
            hist_launch<TRI_VIS_C64, true>(st, grid, lds, vis, flags, ntime, nchan, (int)n_corr, (int)nbands, nchunks, ch,
                                           ebase, shift, nb, hist_bl, hist_chunk);
        else if (c64)
            hist_launch<TRI_VIS_C64, false>(st, grid, lds, vis, flags, ntime, nchan, (int)n_corr, (int)nbands, nchunks, ch,
                                            ebase, shift, nb, hist_bl, hist_chunk);
        else if (vec)
            hist_launch<TRI_VIS_F32, true>(st, grid, lds, vis, flags, ntime, nchan, (int)n_corr, (int)nbands, nchunks, ch,
                                           ebase, shift, nb, hist_bl, hist_chunk);
        else
            hist_launch<TRI_VIS_F32, false>(st, grid, lds, vis, flags, ntime, nchan, (int)n_corr, (int)nbands, nchunks, ch,
                                            ebase, shift, nb, hist_bl, hist_chunk);
        LAUNCHCHK();
    }
    return TRI_OK;
}
