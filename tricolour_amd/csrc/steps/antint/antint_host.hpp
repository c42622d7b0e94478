// Host side of antenna integration: one mean-amplitude image per antenna, flagged as a block of windows, and the
// flag excess of an antenna's baselines (steps/antint/kernels_antint.hpp)
#pragma once
// Two switches, by divisibility and alignment alone (DESIGN.md §Antenna integration): the accumulate owns 4 positions
// per thread when n % 4 == 0 and the bases allow 16-byte loads (4-byte for flags), the apply pass 16 flags per thread
// when n % 16 == 0 and the bases allow it.  Neither changes a result.

// the shape checks the four entry points share: 0 when fine; *empty is set when there is nothing to do
static int ant_check_shape(int64_t nbl, int64_t nant, int64_t n, bool* empty) {
    if (nbl < 0 || nant < 0 || n < 0) return set_err(TRI_EINVAL, "bad shape");
    *empty = nbl == 0 || nant == 0 || n == 0;
    if (*empty) return 0;
    // the antenna is the grid's second dimension; list entries and antenna numbers are int32
    if (nant > 65535) return set_err(TRI_EUNSUPPORTED, "more than 65535 antennas");
    if (n >= (1ll << 38) || nbl >= (1ll << 31) || nbl > (INT64_MAX / 16) / n || nant > (INT64_MAX / 16) / n)
        return set_err(TRI_EUNSUPPORTED, "image too large");
    return 0;
}

extern "C" int tri_antenna_accumulate(const void* vis, int vis_dtype, const uint8_t* flags, const int32_t* offsets,
                                      const int32_t* baselines, int64_t nbl, int64_t nant, int64_t n, double* sum,
                                      int32_t* count, void* stream) {
    // vis == NULL: the flags-only form, which neither reads vis_dtype nor touches sum
    if (!flags || !offsets || !baselines || !count || (vis && !sum)) return set_err(TRI_EINVAL, "NULL pointer argument");
    bool empty;
    if (int rc = ant_check_shape(nbl, nant, n, &empty)) return rc;
    if (vis && !vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (empty) return TRI_OK;
    const bool vec = n % 4 == 0 && (uintptr_t)flags % 4 == 0 && (uintptr_t)count % 16 == 0 &&
                     (!vis || ((uintptr_t)vis % 16 == 0 && (uintptr_t)sum % 16 == 0));
    const int64_t npiece = vec ? n / 4 : n;
    const dim3 grid((unsigned)cdiv(npiece, ANT_NT), (unsigned)nant);
    hipStream_t st = (hipStream_t)stream;
#define ANT_ACCUMULATE(V, VEC)                                                                                    \
    hipLaunchKernelGGL((k_ant_accumulate<V, VEC>), grid, dim3(ANT_NT), 0, st, vis, flags, offsets, baselines, nbl, n, \
                       npiece, sum, count)
    // (-1 is ANT_NO_VIS, written as the kernel log spells it)
    if (!vis)                          { if (vec) ANT_ACCUMULATE(-1, 4); else ANT_ACCUMULATE(-1, 1); }
    else if (vis_dtype == TRI_VIS_C64) { if (vec) ANT_ACCUMULATE(TRI_VIS_C64, 4); else ANT_ACCUMULATE(TRI_VIS_C64, 1); }
    else                               { if (vec) ANT_ACCUMULATE(TRI_VIS_F32, 4); else ANT_ACCUMULATE(TRI_VIS_F32, 1); }
#undef ANT_ACCUMULATE
    LAUNCHCHK();
    return TRI_OK;
}

extern "C" int tri_antenna_mean(const double* sum, const int32_t* count, const int32_t* min_count, int64_t nant,
                                int64_t n, float* amp, uint8_t* flag, void* stream) {
    if (!sum || !count || !min_count || !amp || !flag) return set_err(TRI_EINVAL, "NULL pointer argument");
    bool empty;
    if (int rc = ant_check_shape(1, nant, n, &empty)) return rc;
    if (empty) return TRI_OK;
    hipLaunchKernelGGL(k_ant_finish, dim3((unsigned)cdiv(n, ANT_NT), (unsigned)nant), dim3(ANT_NT), 0,
                       (hipStream_t)stream, sum, count, min_count, n, amp, flag);
    LAUNCHCHK();
    return TRI_OK;
}

extern "C" int tri_antenna_flag_excess(const int32_t* count, const int32_t* members, const int32_t* max_flagged,
                                       int64_t nant, int64_t n, uint8_t* det, void* stream) {
    if (!count || !members || !max_flagged || !det) return set_err(TRI_EINVAL, "NULL pointer argument");
    bool empty;
    if (int rc = ant_check_shape(1, nant, n, &empty)) return rc;
    if (empty) return TRI_OK;
    if (ranges_overlap(det, (size_t)nant * n, count, (size_t)nant * n * sizeof(int32_t)))
        return set_err(TRI_EINVAL, "det must not overlap count");
    hipLaunchKernelGGL(k_ant_excess, dim3((unsigned)cdiv(n, ANT_NT), (unsigned)nant), dim3(ANT_NT), 0,
                       (hipStream_t)stream, count, members, max_flagged, n, det);
    LAUNCHCHK();
    return TRI_OK;
}

extern "C" int tri_antenna_broadcast_or(const uint8_t* flags, const uint8_t* det, const int32_t* ant1,
                                        const int32_t* ant2, uint8_t* out, int64_t nbl, int64_t nant, int64_t n,
                                        void* stream) {
    // nant == 0: no antenna number is inside, det is not read and may be NULL; out = (flags != 0)
    if (!flags || !ant1 || !ant2 || !out || (nant > 0 && !det)) return set_err(TRI_EINVAL, "NULL pointer argument");
    bool empty;
    if (nant < 0) return set_err(TRI_EINVAL, "bad shape");
    if (int rc = ant_check_shape(nbl, std::max<int64_t>(nant, 1), n, &empty)) return rc;
    if (empty) return TRI_OK;
    const size_t N = (size_t)nbl * n;
    if (ranges_overlap(out, N, det, (size_t)nant * n)) return set_err(TRI_EINVAL, "out must not overlap det");
    // in place (out == flags) is fine: every byte is read and written by one thread; a shifted overlap is not
    if (out != flags && ranges_overlap(out, N, flags, N))
        return set_err(TRI_EINVAL, "out must be flags itself or not overlap it");
    hipStream_t st = (hipStream_t)stream;
    const unsigned gy = (unsigned)std::min<int64_t>(nbl, 65535);
    if (n % 16 == 0 && (uintptr_t)flags % 16 == 0 && (uintptr_t)det % 16 == 0 && (uintptr_t)out % 16 == 0)
        hipLaunchKernelGGL(k_ant_apply<true>, dim3((unsigned)cdiv(n / 16, ANT_NT), gy), dim3(ANT_NT), 0, st, flags, det,
                           ant1, ant2, out, nbl, nant, n);
    else
        hipLaunchKernelGGL(k_ant_apply<false>, dim3((unsigned)cdiv(n, ANT_NT), gy), dim3(ANT_NT), 0, st, flags, det,
                           ant1, ant2, out, nbl, nant, n);
    LAUNCHCHK();
    return TRI_OK;
}
