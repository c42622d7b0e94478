// step_host.hpp -- what the host files of the stand-alone device steps (steps/**/*_host.hpp) share.
// Part of the single translation unit tricolour_amd.hip, included there once, ahead of the step host files.
// Plain static functions, each used by at least two steps.  A check that fails has set the error (set_err) and
// hands back its status; 0 when the argument is fine.  The order of an entry point's checks is that entry point's
// own: the first failing one decides status and message.
#pragma once

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte; an empty range overlaps nothing
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    return na > 0 && nb > 0 && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

// The vis dtypes every step reads.  The status of a wrong one is the caller's: TRI_EINVAL from the quality statistics
// and the histograms, TRI_EUNSUPPORTED from every other step.
static bool vis_dtype_ok(int vis_dtype) { return vis_dtype == TRI_VIS_C64 || vis_dtype == TRI_VIS_F32; }

// The host's frequency chunk ends (non-NULL: hysteresis checks that just before, the others with their other
// pointers): at least one chunk, from 0 to nchan, never decreasing.  `widest`, if asked for, gets the widest chunk.
// More than 2^30 ends are TRI_EINVAL here; the histograms answer those themselves, with TRI_EUNSUPPORTED, first.
static int check_chunk_ends(int64_t nchan, const int64_t* chunk_ends, int64_t n_chunk_ends, int64_t* widest = nullptr) {
    if (n_chunk_ends < 2 || n_chunk_ends > (1ll << 30)) return set_err(TRI_EINVAL, "freq_chunks must be >= 1");
    if (chunk_ends[0] != 0 || chunk_ends[n_chunk_ends - 1] != nchan)
        return set_err(TRI_EINVAL, "freq chunk ends must start at 0 and end at the channel count");
    int64_t w = 0;
    for (int64_t g = 1; g < n_chunk_ends; g++) {
        if (chunk_ends[g] < chunk_ends[g - 1]) return set_err(TRI_EINVAL, "freq chunk ends must not decrease");
        w = std::max(w, chunk_ends[g] - chunk_ends[g - 1]);
    }
    if (widest) *widest = w;
    return 0;
}

// a workspace of at least `need` bytes; NULL is refused whatever `need` (the rank operator, which needs none for
// short lines, asks only when need > 0)
static int check_workspace(const void* workspace, size_t workspace_bytes, size_t need) {
    if (!workspace || workspace_bytes < need)
        return set_err(TRI_EWORKSPACE, "workspace of %zu bytes is smaller than the %zu needed", workspace_bytes, need);
    return 0;
}

// out_flags = (flags != 0): what a thresholding step with both of its axes off answers
static int launch_identity(hipStream_t st, const uint8_t* flags, uint8_t* out_flags, size_t N) {
    hipLaunchKernelGGL(k_normalise_flags, dim3((unsigned)cdiv((int64_t)N, 256)), dim3(256), 0, st, flags, out_flags, N);
    LAUNCHCHK();
    return TRI_OK;
}
