// kernels_sk.hpp -- spectral kurtosis of (time, chan) windows in tiled blocks of time rows, and the flagging of whole
// (block, channel) cells on it (the estimator is Nita & Gary 2010; the definition, with its operation order, is this
// project's own: include/tricolour_amd.h).
//
// Per window, visibilities v, input flags f, block length M = block_time, d = shape:
//   p      = (double)re * (double)re + (double)im * (double)im     (float32 input: (double)x * (double)x)
//   valid  = f == 0 and p is finite
//   block b holds the rows [b M, min(T, (b + 1) M)); per (block, channel), rows in ascending order, from n = 0,
//            S1 = S2 = +0.0:  n += 1, S1 = S1 + p, S2 = S2 + (p * p) for every valid sample -- a sequential chain
//   q      = ((double)n * S2) / (S1 * S1);  k = (((double)n * d + 1.0) / ((double)n - 1.0)) * (q - 1.0);  sk = (float)k
//            NaN (0x7FC00000) when n < min_samples, when !(S1 * S1 > 0) and for any other NaN
//   hit    = (double)sk < lower[n] || (double)sk > upper[n]  (a NaN on either side never hits; neither does a count
//            outside [0, M]);  out[t, c] = (f[t, c] != 0) | hit[t / M, c]
//
// Two launches, no LDS, no atomics, no scratch.
//   k_sk_stats  the only pass over the visibilities (8 B + 1 B per sample; 4 B + 1 B for float32).  A lane owns the
//               channels [c0, c0 + CH) of one (window, block) and walks the block's rows with n, S1, S2 in registers;
//               adjacent lanes hold adjacent channels, so every row access is coalesced.  VEC: CH = 4, two 16-byte
//               loads (one for float32) and one 4-byte flag load per row; otherwise CH = 1.  The adds are a dependent
//               chain but the loads are not: SK_RB rows are loaded before their arithmetic starts.
//   k_sk_apply  a lane owns CH channels of SK_AR rows of one (window, block): it decides its cells once (sk, count and
//               the two table entries) and ORs the hit into the flags of its rows.  VEC: CH = 16, 16-byte accesses.
#pragma once

#define SK_NT 256           // threads per block, both kernels
#define SK_RB 4             // rows loaded ahead of their arithmetic (statistics) / of their stores (apply)
#define SK_AR 16            // apply: rows of a block one lane walks
#define SK_MAX_BLOCK 65536  // largest block_time

// R rows from row `s` (sample index of the lane's first channel) on: all loads first, then the chain.
template <int VIS, bool VEC, int R>
__device__ __forceinline__ void sk_rows(const float* __restrict__ vf, const uint8_t* __restrict__ flags, int64_t s,
                                        int64_t nchan, double* s1, double* s2, int* n) {
    constexpr bool CPLX = VIS == TRI_VIS_C64;
    constexpr int CH = VEC ? 4 : 1;
    float re[R][CH], im[R][CH];
    unsigned fl[R];                                 // byte j = flag of channel j
#pragma unroll
    for (int q = 0; q < R; q++) {
        const int64_t i = s + q * nchan;
        if (VEC) {
            fl[q] = *reinterpret_cast<const unsigned*>(flags + i);
            if (CPLX) {
                const float4 a = *reinterpret_cast<const float4*>(vf + 2 * i);
                const float4 b = *reinterpret_cast<const float4*>(vf + 2 * i + 4);
                re[q][0] = a.x; im[q][0] = a.y; re[q][1] = a.z; im[q][1] = a.w;
                re[q][2] = b.x; im[q][2] = b.y; re[q][3] = b.z; im[q][3] = b.w;
            } else {
                const float4 a = *reinterpret_cast<const float4*>(vf + i);
                re[q][0] = a.x; re[q][1] = a.y; re[q][2] = a.z; re[q][3] = a.w;
#pragma unroll
                for (int j = 0; j < CH; j++) im[q][j] = 0.0f;
            }
        } else {
            fl[q] = flags[i];
            if (CPLX) {
                const float2 a = *reinterpret_cast<const float2*>(vf + 2 * i);
                re[q][0] = a.x; im[q][0] = a.y;
            } else {
                re[q][0] = vf[i]; im[q][0] = 0.0f;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < R; q++) {
#pragma unroll
        for (int j = 0; j < CH; j++) {
            const double a = (double)re[q][j], b = (double)im[q][j];
            const double p = CPLX ? a * a + b * b : a * a;
            const bool valid = ((fl[q] >> (8 * j)) & 0xFFu) == 0 && p < (double)INFINITY;     // p >= 0 or NaN
            n[j] += valid ? 1 : 0;
            s1[j] = valid ? s1[j] + p : s1[j];
            s2[j] = valid ? s2[j] + (p * p) : s2[j];
        }
    }
}

// VIS: TRI_VIS_C64 or TRI_VIS_F32.  VEC: nchan % 4 == 0 and the bases aligned for the 16-byte / 4-byte loads; the
// arithmetic and its order are the same either way.  Grid: one block per (window, block of rows, strip of SK_NT * CH
// channels), strips fastest.  count may be null.
template <int VIS, bool VEC>
__global__ void __launch_bounds__(SK_NT)
k_sk_stats(const void* __restrict__ vis_, const uint8_t* __restrict__ flags, int64_t ntime, int64_t nchan,
           int block_time, int nblocks, int nstrip, double shape, int min_samples, float* __restrict__ sk,
           int* __restrict__ count) {
    constexpr int CH = VEC ? 4 : 1;
    const int64_t blk = blockIdx.x;
    const int strip = (int)(blk % nstrip);
    const int b = (int)(blk / nstrip % nblocks);
    const int64_t win = blk / nstrip / nblocks;
    const int64_t c0 = ((int64_t)strip * SK_NT + threadIdx.x) * CH;
    if (c0 >= nchan) return;                        // VEC: nchan % 4 == 0, a lane has all of its channels or none
    const int64_t t0 = (int64_t)b * block_time;
    const int nrows = (int)min((int64_t)block_time, ntime - t0);
    const float* vf = reinterpret_cast<const float*>(vis_);

    double s1[CH], s2[CH];
    int n[CH];
#pragma unroll
    for (int j = 0; j < CH; j++) { s1[j] = 0.0; s2[j] = 0.0; n[j] = 0; }

    int64_t s = (win * ntime + t0) * nchan + c0;
    int r = 0;
    for (; r + SK_RB <= nrows; r += SK_RB, s += SK_RB * nchan) sk_rows<VIS, VEC, SK_RB>(vf, flags, s, nchan, s1, s2, n);
    for (; r < nrows; r++, s += nchan) sk_rows<VIS, VEC, 1>(vf, flags, s, nchan, s1, s2, n);

    const int64_t o = (win * nblocks + b) * nchan + c0;
#pragma unroll
    for (int j = 0; j < CH; j++) {
        const double dn = (double)n[j], den = s1[j] * s1[j];
        float v = __uint_as_float(0x7FC00000u);
        if (n[j] >= min_samples && den > 0.0) {
            const double q = (dn * s2[j]) / den;
            const double k = ((dn * shape + 1.0) / (dn - 1.0)) * (q - 1.0);
            const float f = (float)k;
            if (f == f) v = f;
        }
        sk[o + j] = v;
        if (count) count[o + j] = n[j];
    }
}

// 0x01 in byte j of the result where byte j of w is nonzero
__device__ __forceinline__ unsigned sk_nonzero_bytes(unsigned w) {
    return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) >> 7 & 0x01010101u;
}

__device__ __forceinline__ bool sk_hit(float s, int n, int block_time, const double* __restrict__ lower,
                                       const double* __restrict__ upper) {
    if (n < 0 || n > block_time) return false;      // the tables hold block_time + 1 entries
    const double v = (double)s;
    return v < lower[n] || v > upper[n];            // false for a NaN on either side
}

// VEC: nchan % 16 == 0 and 16-byte aligned bases, 16 channels per lane; otherwise one.  Grid: one block per (window,
// block of rows, chunk of SK_AR rows, strip of SK_NT * CH channels), strips fastest.
template <bool VEC>
__global__ void __launch_bounds__(SK_NT)
k_sk_apply(const float* __restrict__ sk, const int* __restrict__ count, const uint8_t* __restrict__ flags,
           uint8_t* __restrict__ out, int64_t ntime, int64_t nchan, int block_time, int nblocks, int nchunk, int nstrip,
           const double* __restrict__ lower, const double* __restrict__ upper) {
    constexpr int CH = VEC ? 16 : 1;
    const int64_t blk = blockIdx.x;
    const int strip = (int)(blk % nstrip);
    const int chunk = (int)(blk / nstrip % nchunk);
    const int b = (int)(blk / nstrip / nchunk % nblocks);
    const int64_t win = blk / nstrip / nchunk / nblocks;
    const int64_t c0 = ((int64_t)strip * SK_NT + threadIdx.x) * CH;
    if (c0 >= nchan) return;
    const int64_t t0 = (int64_t)b * block_time + (int64_t)chunk * SK_AR;
    const int64_t t1 = min(ntime, min((int64_t)(b + 1) * block_time, t0 + SK_AR));
    if (t0 >= t1) return;                           // a short last block has fewer chunks
    const int64_t cell = (win * nblocks + b) * nchan + c0;
    int64_t i = (win * ntime + t0) * nchan + c0;
    const int rows = (int)(t1 - t0);
    int r = 0;
    if (VEC) {
        unsigned hit[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 s = *reinterpret_cast<const float4*>(sk + cell + 4 * g);
            const int4 n = *reinterpret_cast<const int4*>(count + cell + 4 * g);
            hit[g] = (sk_hit(s.x, n.x, block_time, lower, upper) ? 0x00000001u : 0u) |
                     (sk_hit(s.y, n.y, block_time, lower, upper) ? 0x00000100u : 0u) |
                     (sk_hit(s.z, n.z, block_time, lower, upper) ? 0x00010000u : 0u) |
                     (sk_hit(s.w, n.w, block_time, lower, upper) ? 0x01000000u : 0u);
        }
        for (; r + SK_RB <= rows; r += SK_RB, i += SK_RB * nchan) {
            uint4 f[SK_RB];
#pragma unroll
            for (int q = 0; q < SK_RB; q++) f[q] = *reinterpret_cast<const uint4*>(flags + i + q * nchan);
#pragma unroll
            for (int q = 0; q < SK_RB; q++)
                *reinterpret_cast<uint4*>(out + i + q * nchan) =
                    make_uint4(sk_nonzero_bytes(f[q].x) | hit[0], sk_nonzero_bytes(f[q].y) | hit[1],
                               sk_nonzero_bytes(f[q].z) | hit[2], sk_nonzero_bytes(f[q].w) | hit[3]);
        }
        for (; r < rows; r++, i += nchan) {
            const uint4 f = *reinterpret_cast<const uint4*>(flags + i);
            *reinterpret_cast<uint4*>(out + i) = make_uint4(sk_nonzero_bytes(f.x) | hit[0], sk_nonzero_bytes(f.y) | hit[1],
                                                            sk_nonzero_bytes(f.z) | hit[2], sk_nonzero_bytes(f.w) | hit[3]);
        }
    } else {
        const unsigned hit = sk_hit(sk[cell], count[cell], block_time, lower, upper) ? 1u : 0u;
        for (; r + SK_RB <= rows; r += SK_RB, i += SK_RB * nchan) {
            unsigned f[SK_RB];
#pragma unroll
            for (int q = 0; q < SK_RB; q++) f[q] = flags[i + q * nchan];
#pragma unroll
            for (int q = 0; q < SK_RB; q++) out[i + q * nchan] = (uint8_t)((f[q] ? 1u : 0u) | hit);
        }
        for (; r < rows; r++, i += nchan) out[i] = (uint8_t)((flags[i] ? 1u : 0u) | hit);
    }
}
