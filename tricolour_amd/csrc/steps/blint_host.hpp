// Host side of baseline integration: mean amplitude over baselines, flagged as one image (steps/kernels_blint.hpp)
#pragma once
// Two switches, by divisibility and alignment alone (DESIGN.md §Baseline integration): the accumulate owns 4 positions
// per thread when n % 4 == 0 and the bases allow 16-byte loads, the apply pass 16 flags per thread when n % 16 == 0 and
// the bases allow it.  Neither changes a result.
extern "C" int tri_baseline_accumulate(const void* vis, int vis_dtype, const uint8_t* flags, const uint8_t* select,
                                       int64_t nbl, int64_t n, double* sum, int32_t* count, void* stream) {
    if (!vis || !flags || !sum || !count) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (nbl < 0 || n < 0) return set_err(TRI_EINVAL, "bad shape");
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (nbl == 0 || n == 0) return TRI_OK;
    if (n >= (1ll << 38) || nbl > (INT64_MAX / 16) / n) return set_err(TRI_EUNSUPPORTED, "image too large");
    const bool vec = n % 4 == 0 && (uintptr_t)vis % 16 == 0 && (uintptr_t)flags % 4 == 0 && (uintptr_t)sum % 16 == 0 &&
                     (uintptr_t)count % 16 == 0;
    const int64_t npiece = vec ? n / 4 : n;
    const dim3 grid((unsigned)cdiv(npiece, BLI_NT));
    hipStream_t st = (hipStream_t)stream;
#define BLI_ACCUMULATE(V, VEC)                                                                                   \
    hipLaunchKernelGGL((k_bli_accumulate<V, VEC>), grid, dim3(BLI_NT), 0, st, vis, flags, select, nbl, n, npiece, sum, \
                       count)
    if (vis_dtype == TRI_VIS_C64) { if (vec) BLI_ACCUMULATE(TRI_VIS_C64, 4); else BLI_ACCUMULATE(TRI_VIS_C64, 1); }
    else                          { if (vec) BLI_ACCUMULATE(TRI_VIS_F32, 4); else BLI_ACCUMULATE(TRI_VIS_F32, 1); }
#undef BLI_ACCUMULATE
    LAUNCHCHK();
    return TRI_OK;
}

extern "C" int tri_baseline_mean(const double* sum, const int32_t* count, int64_t n, int64_t min_count, float* amp,
                                 uint8_t* flag, void* stream) {
    if (!sum || !count || !amp || !flag) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n < 0) return set_err(TRI_EINVAL, "bad shape");
    if (min_count < 1) return set_err(TRI_EINVAL, "min_count must be >= 1");
    if (n == 0) return TRI_OK;
    if (n >= (1ll << 38)) return set_err(TRI_EUNSUPPORTED, "image too large");
    hipLaunchKernelGGL(k_bli_finish, dim3((unsigned)cdiv(n, BLI_NT)), dim3(BLI_NT), 0, (hipStream_t)stream, sum, count, n,
                       min_count, amp, flag);
    LAUNCHCHK();
    return TRI_OK;
}

extern "C" int tri_broadcast_or(const uint8_t* flags, const uint8_t* line, uint8_t* out, int64_t nbl, int64_t n,
                                void* stream) {
    if (!flags || !line || !out) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (nbl < 0 || n < 0) return set_err(TRI_EINVAL, "bad shape");
    if (nbl == 0 || n == 0) return TRI_OK;
    if (n >= (1ll << 38) || nbl > (INT64_MAX / 16) / n) return set_err(TRI_EUNSUPPORTED, "image too large");
    const size_t N = (size_t)nbl * n;
    if (ranges_overlap(out, N, line, (size_t)n)) return set_err(TRI_EINVAL, "out must not overlap line");
    // in place (out == flags) is fine: every byte is read and written by one thread; a shifted overlap is not
    if (out != flags && ranges_overlap(out, N, flags, N))
        return set_err(TRI_EINVAL, "out must be flags itself or not overlap it");
    hipStream_t st = (hipStream_t)stream;
    const unsigned gy = (unsigned)std::min<int64_t>(nbl, 65535);
    if (n % 16 == 0 && (uintptr_t)flags % 16 == 0 && (uintptr_t)line % 16 == 0 && (uintptr_t)out % 16 == 0)
        hipLaunchKernelGGL(k_bli_apply<true>, dim3((unsigned)cdiv(n / 16, BLI_NT), gy), dim3(BLI_NT), 0, st, flags, line,
                           out, nbl, n);
    else
        hipLaunchKernelGGL(k_bli_apply<false>, dim3((unsigned)cdiv(n, BLI_NT), gy), dim3(BLI_NT), 0, st, flags, line, out,
                           nbl, n);
    LAUNCHCHK();
    return TRI_OK;
}
