// Host side of the sky-subtracted incoherent noise spectrum (steps/ins/kernels_ins.hpp)
#pragma once
// Three switches, by size, divisibility and alignment alone (DESIGN.md §Incoherent noise spectrum): the accumulate
// owns strips of 8 difference rows when the image then still fills the device and single rows otherwise, and 4 channels
// per thread when nchan % 4 == 0 and the bases allow 16-byte loads; the apply pass owns 16 flags per thread when
// nchan % 16 == 0 and the bases allow it.  None changes a result.
namespace {
struct InsWs {
    float *x, *level;
    uint8_t *live, *valid;
    int32_t* q;
    size_t bytes;
};

// nimg = ncorr * (ntime - 1) * nchan positions, nline = ncorr * nchan lines
InsWs ins_carve(void* ws, size_t nimg, size_t nline) {
    InsWs w;
    Bump b(ws, SIZE_MAX, ws == nullptr);
    w.x = b.get<float>(nimg);
    w.live = b.get<uint8_t>(nline);
    w.level = b.get<float>(nline);
    w.q = b.get<int32_t>(nimg);
    w.valid = b.get<uint8_t>(nimg);
    w.bytes = b.off;
    return w;
}

bool ins_image_fits(int64_t ncorr, int64_t ntime, int64_t nchan) {
    return ntime < (1ll << 31) && nchan < (1ll << 31) && ncorr <= ((1ll << 38) / ntime) / nchan;
}

// shape limits of the entry points (every launch is one-dimensional in x and holds fewer than 2^31 blocks); 0 when
// the shape is fine.  Called with all three sizes > 0.
int ins_check_shape(int64_t nbl, int64_t ncorr, int64_t ntime, int64_t nchan) {
    if (!ins_image_fits(ncorr, ntime, nchan)) return set_err(TRI_EUNSUPPORTED, "image too large");
    if (nbl > (INT64_MAX / 16) / (ncorr * ntime * nchan)) return set_err(TRI_EUNSUPPORTED, "image too large");
    if (ncorr * ntime >= (1ll << 31)) return set_err(TRI_EUNSUPPORTED, "too many rows for one launch");
    return 0;
}

// level, q and valid of one round from x / count / mask
int ins_round(hipStream_t st, const float* x, const int32_t* count, const uint8_t* mask, int64_t ncorr, int64_t nd,
              int64_t nchan, int64_t min_count, float* level, uint8_t* live, int32_t* q, uint8_t* valid) {
    const int64_t nimg = ncorr * nd * nchan;
    hipLaunchKernelGGL(k_ins_level, dim3((unsigned)(ncorr * cdiv(nchan, INS_LC))), dim3(INS_NT), 0, st, x, mask, nd, nchan,
                       level, live);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_ins_zq, dim3((unsigned)cdiv(nimg, INS_NT)), dim3(INS_NT), 0, st, x, count, mask,
                       (const float*)level, (const uint8_t*)live, nd, nchan, nimg, min_count, q, valid);
    LAUNCHCHK();
    return TRI_OK;
}
}  // namespace

extern "C" int tri_ins_accumulate(const void* vis, int vis_dtype, const uint8_t* flags, const uint8_t* select,
                                  int64_t nbl, int64_t ncorr, int64_t ntime, int64_t nchan, double* sum,
                                  int32_t* count, void* stream) {
    if (!vis || !flags || !sum || !count) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (nbl < 0 || ncorr < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (!vis_dtype_ok(vis_dtype)) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (nbl == 0 || ncorr == 0 || ntime < 2 || nchan == 0) return TRI_OK;
    if (int rc = ins_check_shape(nbl, ncorr, ntime, nchan)) return rc;
    const size_t nimg = (size_t)ncorr * (ntime - 1) * nchan;
    if (ranges_overlap(sum, nimg * sizeof(double), count, nimg * sizeof(int32_t)))
        return set_err(TRI_EINVAL, "sum and count must not overlap");
    const bool vec = nchan % 4 == 0 && (uintptr_t)vis % 16 == 0 && (uintptr_t)flags % 4 == 0 && (uintptr_t)sum % 16 == 0 &&
                     (uintptr_t)count % 16 == 0;
    // strips of INS_STRIP rows when those fill the device, else one row per thread
    static_assert(INS_STRIP == 8 && INS_UNROLL == 4, "the launch sites below spell the two forms out");
    const int64_t npc = vec ? nchan / 4 : nchan;
    const bool strips = ncorr * cdiv(ntime - 1, INS_STRIP) * npc >= INS_FILL;
    const int64_t ntile = strips ? cdiv(ntime - 1, INS_STRIP) : ntime - 1;
    const dim3 grid((unsigned)cdiv(ncorr * ntile * npc, INS_NT));
    hipStream_t st = (hipStream_t)stream;
#define INS_ACCUMULATE(V, VEC)                                                                                        \
    do {                                                                                                              \
        if (strips)                                                                                                   \
            hipLaunchKernelGGL((k_ins_accumulate<V, VEC, 8, 1>), grid, dim3(INS_NT), 0, st, vis, flags, select, nbl,  \
                               ncorr, ntime, nchan, npc, ntile, sum, count);                                          \
        else                                                                                                          \
            hipLaunchKernelGGL((k_ins_accumulate<V, VEC, 1, 4>), grid, dim3(INS_NT), 0, st, vis, flags, select, nbl,  \
                               ncorr, ntime, nchan, npc, ntile, sum, count);                                          \
    } while (0)
    if (vis_dtype == TRI_VIS_C64) { if (vec) INS_ACCUMULATE(TRI_VIS_C64, 4); else INS_ACCUMULATE(TRI_VIS_C64, 1); }
    else                          { if (vec) INS_ACCUMULATE(TRI_VIS_F32, 4); else INS_ACCUMULATE(TRI_VIS_F32, 1); }
#undef INS_ACCUMULATE
    LAUNCHCHK();
    return TRI_OK;
}

extern "C" size_t tri_ins_workspace_bytes(int64_t ncorr, int64_t ntime, int64_t nchan) {
    if (ncorr <= 0 || ntime < 2 || nchan <= 0) return 0;
    if (!ins_image_fits(ncorr, ntime, nchan)) return 0;
    return ins_carve(nullptr, (size_t)ncorr * (ntime - 1) * nchan, (size_t)ncorr * nchan).bytes;
}

extern "C" int tri_ins_zscore(const double* sum, const int32_t* count, const uint8_t* mask, int64_t ncorr,
                              int64_t ntime, int64_t nchan, int64_t min_count, float* level, int32_t* q,
                              uint8_t* valid, void* workspace, size_t workspace_bytes, void* stream) {
    if (!sum || !count || !mask || !level || !q || !valid) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (ncorr < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (min_count < 1) return set_err(TRI_EINVAL, "min_count must be >= 1");
    if (ncorr == 0 || ntime < 2 || nchan == 0) return TRI_OK;
    if (int rc = ins_check_shape(1, ncorr, ntime, nchan)) return rc;
    const int64_t nd = ntime - 1;
    const size_t nimg = (size_t)ncorr * nd * nchan, nline = (size_t)ncorr * nchan;
    const void* ptr[6] = {level, q, valid, sum, count, mask};
    const size_t len[6] = {nline * 4, nimg * 4, nimg, nimg * 8, nimg * 4, nimg};
    for (int a = 0; a < 3; a++)                              // every output against everything after it
        for (int b = a + 1; b < 6; b++)
            if (ranges_overlap(ptr[a], len[a], ptr[b], len[b]))
                return set_err(TRI_EINVAL, "level, q and valid must not overlap each other or the inputs");
    if (int rc = check_workspace(workspace, workspace_bytes, tri_ins_workspace_bytes(ncorr, ntime, nchan))) return rc;
    const InsWs w = ins_carve(workspace, nimg, nline);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ins_mean, dim3((unsigned)cdiv((int64_t)nimg, INS_NT)), dim3(INS_NT), 0, st, sum, count,
                       (int64_t)nimg, min_count, w.x);
    LAUNCHCHK();
    return ins_round(st, w.x, count, mask, ncorr, nd, nchan, min_count, level, w.live, q, valid);
}

extern "C" int tri_ins_match(const double* sum, const int32_t* count, int64_t ncorr, int64_t ntime, int64_t nchan,
                             int64_t min_count, const int64_t* shape_lo, const int64_t* shape_hi,
                             const double* shape_nsigma, int64_t n_shapes, double nsigma_narrow, int64_t rounds,
                             uint8_t* mask, void* workspace, size_t workspace_bytes, void* stream) {
    if (!sum || !count || !mask) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (ncorr < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (min_count < 1) return set_err(TRI_EINVAL, "min_count must be >= 1");
    if (n_shapes < 0 || n_shapes > INS_MAX_SHAPES)
        return set_err(TRI_EINVAL, "at most %d shapes, got %lld", INS_MAX_SHAPES, (long long)n_shapes);
    if (n_shapes > 0 && (!shape_lo || !shape_hi || !shape_nsigma)) return set_err(TRI_EINVAL, "NULL pointer argument");
    InsShapes sh;
    memset(&sh, 0, sizeof(sh));
    for (int64_t i = 0; i < n_shapes; i++) {
        if (!(0 <= shape_lo[i] && shape_lo[i] < shape_hi[i] && shape_hi[i] <= nchan))
            return set_err(TRI_EINVAL, "shape %lld: channels [%lld, %lld) do not lie in [0, %lld)", (long long)i,
                           (long long)shape_lo[i], (long long)shape_hi[i], (long long)nchan);
        if (!(shape_nsigma[i] > 0.0)) return set_err(TRI_EINVAL, "shape %lld: nsigma must be > 0", (long long)i);
    }
    if (!(nsigma_narrow >= 0.0)) return set_err(TRI_EINVAL, "nsigma_narrow must be >= 0 (0 switches it off)");
    if (rounds < 1 || rounds > 16) return set_err(TRI_EINVAL, "rounds must lie in [1, 16], got %lld", (long long)rounds);
    if (ncorr == 0 || ntime < 2 || nchan == 0) return TRI_OK;
    if (int rc = ins_check_shape(1, ncorr, ntime, nchan)) return rc;
    const int64_t nd = ntime - 1;
    const size_t nimg = (size_t)ncorr * nd * nchan, nline = (size_t)ncorr * nchan;
    if (ranges_overlap(mask, nimg, sum, nimg * 8) || ranges_overlap(mask, nimg, count, nimg * 4))
        return set_err(TRI_EINVAL, "mask must not overlap sum or count");
    if (int rc = check_workspace(workspace, workspace_bytes, tri_ins_workspace_bytes(ncorr, ntime, nchan))) return rc;
    sh.n = (int)n_shapes;
    for (int64_t i = 0; i < n_shapes; i++) {
        sh.lo[i] = (int)shape_lo[i];
        sh.hi[i] = (int)shape_hi[i];
        sh.nsigma[i] = shape_nsigma[i];
    }
    sh.nsigma_narrow = nsigma_narrow;
    const InsWs w = ins_carve(workspace, nimg, nline);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(mask, 0, nimg, st));
    hipLaunchKernelGGL(k_ins_mean, dim3((unsigned)cdiv((int64_t)nimg, INS_NT)), dim3(INS_NT), 0, st, sum, count,
                       (int64_t)nimg, min_count, w.x);
    LAUNCHCHK();
    // a fixed number of rounds, nothing read back: a round that finds nothing changes nothing
    for (int64_t r = 0; r < rounds; r++) {
        if (int rc = ins_round(st, w.x, count, mask, ncorr, nd, nchan, min_count, w.level, w.live, w.q, w.valid)) return rc;
        hipLaunchKernelGGL(k_ins_match, dim3((unsigned)(ncorr * nd)), dim3(INS_NT), 0, st, (const int32_t*)w.q,
                           (const uint8_t*)w.valid, nchan, sh, mask);
        LAUNCHCHK();
    }
    return TRI_OK;
}

extern "C" int tri_ins_apply(const uint8_t* flags, const uint8_t* mask, uint8_t* out, int64_t nbl, int64_t ncorr,
                             int64_t ntime, int64_t nchan, void* stream) {
    if (!flags || !mask || !out) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (nbl < 0 || ncorr < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (nbl == 0 || ncorr == 0 || ntime == 0 || nchan == 0) return TRI_OK;
    if (int rc = ins_check_shape(nbl, ncorr, ntime, nchan)) return rc;
    const int64_t n = ncorr * ntime * nchan;
    const size_t N = (size_t)nbl * n, nimg = (size_t)ncorr * (ntime - 1) * nchan;
    if (ranges_overlap(out, N, mask, nimg)) return set_err(TRI_EINVAL, "out must not overlap mask");
    // in place (out == flags) is fine: every byte is read and written by one thread; a shifted overlap is not
    if (out != flags && ranges_overlap(out, N, flags, N))
        return set_err(TRI_EINVAL, "out must be flags itself or not overlap it");
    const unsigned gy = (unsigned)std::min<int64_t>(nbl, 65535);
    hipStream_t st = (hipStream_t)stream;
    if (nchan % 16 == 0 && (uintptr_t)flags % 16 == 0 && (uintptr_t)mask % 16 == 0 && (uintptr_t)out % 16 == 0)
        hipLaunchKernelGGL(k_ins_apply<true>, dim3((unsigned)cdiv(n / 16, INS_NT), gy), dim3(INS_NT), 0, st, flags, mask,
                           out, nbl, ntime, nchan, n);
    else
        hipLaunchKernelGGL(k_ins_apply<false>, dim3((unsigned)cdiv(n, INS_NT), gy), dim3(INS_NT), 0, st, flags, mask, out,
                           nbl, ntime, nchan, n);
    LAUNCHCHK();
    return TRI_OK;
}
