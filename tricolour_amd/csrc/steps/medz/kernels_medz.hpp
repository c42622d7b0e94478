// kernels_medz.hpp -- sliding 2-D median background of (time, chan) windows and the robust z-score on it (the model is
// detrend_medfilt of HERA's xrfi; the definition is this project's own, include/tricolour_amd.h).
//
// Per window, with radii Kt, Kf and the neighbourhood W(t, f) = the samples within Kt rows and Kf channels, cut at the
// window's edges:
//   a  = the flagger's amplitude (tri_hypotf / fabsf); a sample is valid iff its flag is 0 and a is finite
//   b  = median of the valid a over W              (n < min_samples: NaN; even n: (float)(((double)x + (double)y) / 2.0))
//   r  = a - b where the centre is valid and b is not NaN, else NaN
//   m  = median, by the same rule, of fabsf(r) over the non-NaN r of W
//   z  = (float)((double)r / ((double)m * 1.4826)) where r and m are not NaN, else NaN;  hit = (double)fabsf(z) > nsigma
// Every NaN written is 0x7FC00000.
//
// One kernel, k_medz_select<VIS, RES>, does both medians.  A block of MEDZ_NT threads owns a tile of MEDZ_TR rows x
// MEDZ_TC channels of one window.  It stages the tile with Kt rows above and below and Kf channels on either side into
// LDS as keys: the bit pattern of the non-negative float32 (unsigned order = float order), MEDZ_NOKEY for a sample
// that is invalid, outside the window's image or (RES) NaN.  Rows and channels beyond the image are never read, so a
// tile never sees the neighbouring window.
//   <VIS, false>  source A: keys from vis and flags; writes b and, if asked, r.
//   <1, true>     source B: keys from fabsf of the residual image; writes m (if asked), z and, if asked,
//                 gout = (gin != 0) | hit.  A thread reads and writes the flags of its own samples only, so gout may
//                 be gin.
// Selection: a thread owns MEDZ_PT consecutive rows of one channel and finds each one's k-th smallest key,
// k = (n - 1) / 2, by bisection on the 31 key bits from the top: with prefix p and t = p | bit it counts the keys
// below t in the neighbourhood and keeps the bit iff the count is at most k.  One pass counts n, 31 find the lower
// middle x, one counts the keys <= x and, only where a lane has an even n whose upper middle is another value, one
// more finds the smallest key above x.  The MEDZ_PT neighbourhoods of a thread overlap in all but MEDZ_PT - 1 rows at
// either end, so every key is read from LDS once per pass and compared with up to MEDZ_PT pivots: a quarter of the
// LDS reads of one output per thread, and the 64 lanes of a wave read 64 consecutive words (no bank conflict for any
// row length).  The cost is 2 vector operations per key, pivot and pass; nothing depends on the data but the last,
// wave-uniformly skipped pass, and no route changes a bit of any output.
#pragma once

#define MEDZ_NT 256                 // threads per block
#define MEDZ_TR 16                  // rows of a tile
#define MEDZ_TC 64                  // channels of a tile: one wave's lanes
#define MEDZ_PT 4                   // consecutive rows per thread (MEDZ_TR * MEDZ_TC == MEDZ_NT * MEDZ_PT)
#define MEDZ_MAXK 32                // largest radius
#define MEDZ_MAXAREA 625            // largest neighbourhood
// staged keys of a block: (MEDZ_TR + 2 Kt) * (MEDZ_TC + 2 Kf) is largest, under the area limit, at Kt = 32, Kf = 4
// (the host checks every pair of radii against it: medz_check_radii)
#define MEDZ_LDS_WORDS ((MEDZ_TR + 2 * MEDZ_MAXK) * (MEDZ_TC + 2 * 4))
#define MEDZ_NOKEY 0xFFFFFFFFu      // a sample that enters no median
#define MEDZ_NAN 0x7FC00000u

static_assert(MEDZ_TR * MEDZ_TC == MEDZ_NT * MEDZ_PT && MEDZ_TC == 64 && MEDZ_PT == 4, "k_medz_select's thread map");

// cnt[o] = the keys below piv[o] in the neighbourhood of the thread's output o.  `col`: the thread's first staged key
// (staged row 0 of its outputs, its channel's left edge); output o's rows are the staged rows o ... o + 2 Kt.
__device__ __forceinline__ void medz_count(const unsigned* __restrict__ col, int lw, int kt2, int kf2,
                                           const unsigned (&piv)[MEDZ_PT], unsigned (&cnt)[MEDZ_PT]) {
#pragma unroll
    for (int o = 0; o < MEDZ_PT; o++) cnt[o] = 0;
    for (int i = 0; i < kt2 + MEDZ_PT; i++) {
        const unsigned* __restrict__ row = col + i * lw;
        if (i >= MEDZ_PT - 1 && i <= kt2) {             // a row of all four neighbourhoods
#pragma unroll 4
            for (int j = 0; j <= kf2; j++) {
                const unsigned key = row[j];
#pragma unroll
                for (int o = 0; o < MEDZ_PT; o++) cnt[o] += key < piv[o] ? 1u : 0u;
            }
        } else {                                        // the first and last rows: a pivot of 0 counts nothing
            unsigned q[MEDZ_PT];
#pragma unroll
            for (int o = 0; o < MEDZ_PT; o++) q[o] = (i >= o && i - o <= kt2) ? piv[o] : 0u;
#pragma unroll 4
            for (int j = 0; j <= kf2; j++) {
                const unsigned key = row[j];
#pragma unroll
                for (int o = 0; o < MEDZ_PT; o++) cnt[o] += key < q[o] ? 1u : 0u;
            }
        }
    }
}

// nxt[o] = the smallest key above x[o] in the neighbourhood of output o (a key: there is one where this is used).
// key - (x + 1) wraps to the top of the range for the keys <= x, and MEDZ_NOKEY stays above every key.
__device__ __forceinline__ void medz_next(const unsigned* __restrict__ col, int lw, int kt2, int kf2,
                                          const unsigned (&x)[MEDZ_PT], unsigned (&nxt)[MEDZ_PT]) {
    unsigned d[MEDZ_PT];
#pragma unroll
    for (int o = 0; o < MEDZ_PT; o++) d[o] = 0xFFFFFFFFu;
    for (int i = 0; i < kt2 + MEDZ_PT; i++) {
        const unsigned* __restrict__ row = col + i * lw;
        for (int j = 0; j <= kf2; j++) {
            const unsigned key = row[j];
#pragma unroll
            for (int o = 0; o < MEDZ_PT; o++)
                if (i >= o && i - o <= kt2) d[o] = min(d[o], key - (x[o] + 1u));
        }
    }
#pragma unroll
    for (int o = 0; o < MEDZ_PT; o++) nxt[o] = d[o] + (x[o] + 1u);
}

// grid: n_win * tiles_t * tiles_f blocks of MEDZ_NT threads, tile-of-channels fastest.
//   <VIS, false>: src = vis, flags; out0 = background, out1 = residual (either may be NULL); gin, gout unused.
//   <1, true>:    src = residual, flags unused; out0 = scale (may be NULL), out1 = z; gout = (gin != 0) | hit when
//                 gout is not NULL.
template <int VIS, bool RES>
__global__ void __launch_bounds__(MEDZ_NT)
k_medz_select(const void* __restrict__ src, const uint8_t* __restrict__ flags, int ntime, int nchan, int tiles_t,
              int tiles_f, int kt, int kf, unsigned min_samples, double nsigma, float* __restrict__ out0,
              float* __restrict__ out1, const uint8_t* gin, uint8_t* gout) {
    __shared__ unsigned s_key[MEDZ_LDS_WORDS];
    const int64_t blk = blockIdx.x;
    const int tile_f = (int)(blk % tiles_f);
    const int tile_t = (int)(blk / tiles_f % tiles_t);
    const int64_t win = blk / tiles_f / tiles_t;
    const int64_t base = win * (int64_t)ntime * nchan;
    const int t0 = tile_t * MEDZ_TR, f0 = tile_f * MEDZ_TC;
    const int kt2 = 2 * kt, kf2 = 2 * kf;
    const int lh = MEDZ_TR + kt2, lw = MEDZ_TC + kf2;       // lh * lw <= MEDZ_LDS_WORDS: medz_check_radii

    // stage: staged (i, j) is the image's (t0 - kt + i, f0 - kf + j)
    for (int e = threadIdx.x; e < lh * lw; e += MEDZ_NT) {
        const int i = e / lw, j = e - i * lw;
        const int t = t0 - kt + i, f = f0 - kf + j;
        unsigned key = MEDZ_NOKEY;
        if (t >= 0 && t < ntime && f >= 0 && f < nchan) {
            const int64_t s = base + (int64_t)t * nchan + f;
            if (RES) {
                const unsigned k = __float_as_uint(fabsf(reinterpret_cast<const float*>(src)[s]));
                if (k <= 0x7F800000u) key = k;              // every non-NaN residual counts, an infinite one too
            } else if (flags[s] == 0) {
                const unsigned k = __float_as_uint(load_amp<VIS>(src, (size_t)s));
                if (k < 0x7F800000u) key = k;               // amplitudes carry no sign: +inf and NaN lie at and above
            }
        }
        s_key[e] = key;
    }
    __syncthreads();

    const int c = threadIdx.x & (MEDZ_TC - 1), r0 = (threadIdx.x >> 6) * MEDZ_PT;
    const unsigned* col = s_key + r0 * lw + c;

    unsigned piv[MEDZ_PT], n[MEDZ_PT], k[MEDZ_PT], x[MEDZ_PT], cnt[MEDZ_PT];
#pragma unroll
    for (int o = 0; o < MEDZ_PT; o++) piv[o] = 0x80000000u;  // above every key, below MEDZ_NOKEY
    medz_count(col, lw, kt2, kf2, piv, n);
#pragma unroll
    for (int o = 0; o < MEDZ_PT; o++) { k[o] = n[o] ? (n[o] - 1) / 2 : 0; x[o] = 0; }
    for (int bit = 30; bit >= 0; bit--) {
#pragma unroll
        for (int o = 0; o < MEDZ_PT; o++) piv[o] = x[o] | 1u << bit;
        medz_count(col, lw, kt2, kf2, piv, cnt);
#pragma unroll
        for (int o = 0; o < MEDZ_PT; o++) x[o] = cnt[o] <= k[o] ? piv[o] : x[o];
    }
    // the upper middle of an even n: x again if more than k + 1 keys are <= x, else the next key above
    unsigned y[MEDZ_PT];
#pragma unroll
    for (int o = 0; o < MEDZ_PT; o++) piv[o] = x[o] + 1u;
    medz_count(col, lw, kt2, kf2, piv, cnt);
    bool other = false;
#pragma unroll
    for (int o = 0; o < MEDZ_PT; o++) {
        y[o] = x[o];
        other = other || (n[o] != 0 && n[o] % 2 == 0 && cnt[o] == k[o] + 1);
    }
    if (__any(other)) {
        unsigned nxt[MEDZ_PT];
        medz_next(col, lw, kt2, kf2, x, nxt);
#pragma unroll
        for (int o = 0; o < MEDZ_PT; o++)
            if (n[o] != 0 && n[o] % 2 == 0 && cnt[o] == k[o] + 1) y[o] = nxt[o];
    }

    const int f = f0 + c;
#pragma unroll
    for (int o = 0; o < MEDZ_PT; o++) {
        const int t = t0 + r0 + o;
        if (t >= ntime || f >= nchan) continue;
        const int64_t s = base + (int64_t)t * nchan + f;
        float med = __uint_as_float(MEDZ_NAN);
        if (n[o] >= min_samples) {
            med = __uint_as_float(x[o]);
            if (n[o] % 2 == 0) med = (float)(((double)med + (double)__uint_as_float(y[o])) / 2.0);
        }
        const bool has = n[o] >= min_samples;
        if (!RES) {
            if (out0) out0[s] = med;
            if (out1) {
                const unsigned ck = col[(o + kt) * lw + kf];    // the centre's key
                float r = __uint_as_float(MEDZ_NAN);
                if (ck != MEDZ_NOKEY && has) r = __uint_as_float(ck) - med;
                out1[s] = r;
            }
        } else {
            if (out0) out0[s] = med;
            const float r = reinterpret_cast<const float*>(src)[s];
            float z = __uint_as_float(MEDZ_NAN);
            if (r == r && has) {
                z = (float)((double)r / ((double)med * TRI_MAD_NORMAL));
                if (z != z) z = __uint_as_float(MEDZ_NAN);      // 0 / 0, inf / inf: one NaN
            }
            out1[s] = z;
            if (gout) gout[s] = (gin[s] != 0 || (double)fabsf(z) > nsigma) ? 1 : 0;
        }
    }
}
