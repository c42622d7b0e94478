// kernels_ldev.hpp -- sliding-window complex deviation of (time, chan) windows and the thresholding of single samples
// on it (the model is CASA's rflag; the definition is this project's own, include/tricolour_amd.h).
//
// Per window, visibilities v and input flags f; one axis (the window slides along time, or along channels):
//   counts = f == 0 and neither part of v is NaN                  (float32 amplitudes: re = a, im = 0)
//   over the counting samples of the 2h + 1 samples around (t, c), clipped at the window's edge, in ascending order,
//   in float64 from +0.0 without FMA:
//     n, sr += re, si += im;  mr = sr / n, mi = si / n;  acc += (re - mr)^2, then acc += (im - mi)^2
//     d = (float)sqrt(acc / n)
//   usable = the sample counts and n >= 2; an unusable sample has d = NaN (0x7FC00000); a usable sample whose window
//   holds a counting sample with an infinite part has d = +inf
//   level  = per line -- time axis: (window, channel); channel axis: (window, time row, frequency chunk) -- the median
//            of the finite d (even count: float32(a + b) / 2); the line is live with >= 3 of them and a level > 0
//   hit    = usable and (d == +inf or (live and (double)d > (double)level * scale))
//   out    = f | hit_time | hit_freq
//
// Four kernels.
//   k_ldev_time   d along time.  A block of 256 threads owns LDEV_TR = 64 rows x 1024 channels; a thread owns 4
//                 adjacent channels (two 16-byte loads and one flag word per row) and walks down the rows with a
//                 register ring of W rows, so every sample is loaded once (plus 2h halo rows per 64).  W = 3 and 5 are
//                 compiled; W = 0 is the route for every other width: no ring, the window re-read from memory.
//   k_ldev_freq   d along channels.  The same thread layout, one row at a time; a thread holds its 4 samples and h on
//                 either side (the neighbours' loads hit the same cache lines).  W as above.
//   k_ldev_level  the level of every line by an exact 8-bit radix select over the bit patterns of the non-negative
//                 float32 d (4 counting passes and one for the upper middle of an even count), then the hit bytes.
//                 <0>: 32 adjacent channels of one window per block, 8 threads per channel (rows of 128 bytes);
//                 <1>: one wave per (row, chunk), 4 lines per block.  Integer LDS atomics only.
//   k_ldev_apply  out = f | hit_time | hit_freq, 16 flags per thread (VEC) or one.
// VEC in the first two: nchan % 4 == 0 and the bases aligned for 16-byte / 4-byte accesses.  Neither W nor VEC changes
// the arithmetic or its order: the same bits on every route, for every batch size and on every run.
#pragma once

#define LDEV_NT 256                 // threads per block, all kernels
#define LDEV_V 4                    // channels per thread
#define LDEV_CW (LDEV_NT * LDEV_V)  // channels per strip
#define LDEV_TR 64                  // k_ldev_time: rows per tile
#define LDEV_FR 8                   // k_ldev_freq: rows per block
#define LDEV_MAXW 31                // widest window
#define LDEV_LC 32                  // k_ldev_level<0>: channels per block
#define LDEV_LW 4                   // k_ldev_level<1>: lines per block

#define LDEV_COUNTS 1u              // sample state: it counts
#define LDEV_INF 2u                 //               it counts and a part is infinite

__device__ __forceinline__ unsigned ldev_state(unsigned flag, float re, float im) {
    if (flag != 0 || re != re || im != im) return 0u;
    return LDEV_COUNTS | ((isinf(re) || isinf(im)) ? LDEV_INF : 0u);
}

// d of one sample.  get(k, re, im) gives the state and the value of slot k of the window, k = 0 .. w - 1 in ascending
// position (state 0 for a slot beyond the edge); the sample itself is slot `centre`.
template <bool CPLX, class Get>
__device__ __forceinline__ float ldev_eval(int w, int centre, Get get) {
    int n = 0;
    unsigned any = 0, self = 0;
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int k = 0; k < w; k++) {
        float re, im;
        const unsigned s = get(k, re, im);
        const bool c = (s & LDEV_COUNTS) != 0;
        any |= s;
        self = k == centre ? s : self;
        n += c ? 1 : 0;
        sr = c ? sr + (double)re : sr;
        if (CPLX) si = c ? si + (double)im : si;
    }
    const double dn = (double)n;
    const double mr = sr / dn, mi = CPLX ? si / dn : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < w; k++) {
        float re, im;
        const bool c = (get(k, re, im) & LDEV_COUNTS) != 0;
        const double dr = (double)re - mr;
        acc = c ? acc + dr * dr : acc;
        if (CPLX) {                                 // amplitudes: im - mi = +0.0 and acc + 0.0 = acc
            const double di = (double)im - mi;
            acc = c ? acc + di * di : acc;
        }
    }
    float d = (float)sqrt(acc / dn);
    if (any & LDEV_INF) d = INFINITY;
    if (!(self & LDEV_COUNTS) || n < 2) d = __uint_as_float(0x7FC00000u);
    return d;
}

// the LDEV_V samples of a thread at sample index s (row start + channel): state per channel (0 where there is none)
template <bool CPLX, bool VEC>
__device__ __forceinline__ void ldev_load4(const float* __restrict__ vf, const uint8_t* __restrict__ flags, int64_t s,
                                           int nv, float (&re)[LDEV_V], float (&im)[LDEV_V], unsigned (&st)[LDEV_V]) {
#pragma unroll
    for (int j = 0; j < LDEV_V; j++) { re[j] = 0.0f; im[j] = 0.0f; st[j] = 0u; }
    if (nv <= 0) return;
    if (VEC) {
        const unsigned fl = *reinterpret_cast<const unsigned*>(flags + s);
        if (CPLX) {
            const float4 a = *reinterpret_cast<const float4*>(vf + 2 * s);
            const float4 b = *reinterpret_cast<const float4*>(vf + 2 * s + 4);
            re[0] = a.x; im[0] = a.y; re[1] = a.z; im[1] = a.w;
            re[2] = b.x; im[2] = b.y; re[3] = b.z; im[3] = b.w;
        } else {
            const float4 a = *reinterpret_cast<const float4*>(vf + s);
            re[0] = a.x; re[1] = a.y; re[2] = a.z; re[3] = a.w;
        }
#pragma unroll
        for (int j = 0; j < LDEV_V; j++) st[j] = ldev_state((fl >> (8 * j)) & 0xFFu, re[j], im[j]);
    } else {
#pragma unroll
        for (int j = 0; j < LDEV_V; j++) {
            if (j < nv) {
                if (CPLX) {
                    const float2 a = *reinterpret_cast<const float2*>(vf + 2 * (s + j));
                    re[j] = a.x; im[j] = a.y;
                } else {
                    re[j] = vf[s + j];
                }
                st[j] = ldev_state(flags[s + j], re[j], im[j]);
            }
        }
    }
}

// one sample at index s
template <bool CPLX>
__device__ __forceinline__ unsigned ldev_load1(const float* __restrict__ vf, const uint8_t* __restrict__ flags,
                                               int64_t s, float& re, float& im) {
    if (CPLX) {
        const float2 a = *reinterpret_cast<const float2*>(vf + 2 * s);
        re = a.x; im = a.y;
    } else {
        re = vf[s]; im = 0.0f;
    }
    return ldev_state(flags[s], re, im);
}

template <bool VEC>
__device__ __forceinline__ void ldev_store4(float* __restrict__ out, int64_t s, int nv, const float (&d)[LDEV_V]) {
    if (VEC) {
        *reinterpret_cast<float4*>(out + s) = make_float4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int j = 0; j < LDEV_V; j++)
            if (j < nv) out[s + j] = d[j];
    }
}

// VIS: TRI_VIS_C64 or TRI_VIS_F32.  W: 3, 5, or 0 for the width `window` read at run time.
// grid: n_win * ntiles * nstrip blocks.
template <int VIS, int W, bool VEC>
__global__ void __launch_bounds__(LDEV_NT)
k_ldev_time(const void* __restrict__ vis_, const uint8_t* __restrict__ flags, int64_t ntime, int64_t nchan, int nstrip,
            int ntiles, int window, float* __restrict__ d_time) {
    constexpr bool CPLX = VIS == TRI_VIS_C64;
    const int64_t blk = blockIdx.x;
    const int strip = (int)(blk % nstrip);
    const int tile = (int)(blk / nstrip % ntiles);
    const int64_t win = blk / nstrip / ntiles;
    const int64_t c0 = (int64_t)strip * LDEV_CW + threadIdx.x * LDEV_V;
    const int64_t t0 = (int64_t)tile * LDEV_TR;
    const int nrows = (int)min((int64_t)LDEV_TR, ntime - t0);
    const int nv = (int)max((int64_t)0, min((int64_t)LDEV_V, nchan - c0));
    const float* vf = reinterpret_cast<const float*>(vis_);
    if (nv <= 0) return;

    if constexpr (W > 0) {
        constexpr int H = (W - 1) / 2;
        constexpr int WW = W;
        float re[WW][LDEV_V], im[WW][LDEV_V];
        unsigned st[WW][LDEV_V];
        auto fetch = [&](int64_t t, float (&r)[LDEV_V], float (&i)[LDEV_V], unsigned (&s)[LDEV_V]) {
            const bool there = t >= 0 && t < ntime;
            ldev_load4<CPLX, VEC>(vf, flags, (win * ntime + (there ? t : 0)) * nchan + c0, there ? nv : 0, r, i, s);
        };
        // slots 1 .. W - 1 hold rows t0 - H .. t0 + H - 1; every step shifts down and loads row t + H into the last
#pragma unroll
        for (int k = 1; k < WW; k++) fetch(t0 - H + (k - 1), re[k], im[k], st[k]);
        for (int r = 0; r < nrows; r++) {
#pragma unroll
            for (int k = 0; k + 1 < WW; k++) {
#pragma unroll
                for (int j = 0; j < LDEV_V; j++) { re[k][j] = re[k + 1][j]; im[k][j] = im[k + 1][j]; st[k][j] = st[k + 1][j]; }
            }
            fetch(t0 + r + H, re[WW - 1], im[WW - 1], st[WW - 1]);
            float d[LDEV_V];
#pragma unroll
            for (int j = 0; j < LDEV_V; j++)
                d[j] = ldev_eval<CPLX>(WW, H, [&](int k, float& a, float& b) { a = re[k][j]; b = im[k][j]; return st[k][j]; });
            ldev_store4<VEC>(d_time, (win * ntime + t0 + r) * nchan + c0, nv, d);
        }
    } else {
        const int h = (window - 1) / 2;
        for (int r = 0; r < nrows; r++) {
            const int64_t t = t0 + r;
            float d[LDEV_V];
#pragma unroll
            for (int j = 0; j < LDEV_V; j++) {
                d[j] = __uint_as_float(0x7FC00000u);
                if (j >= nv) continue;
                d[j] = ldev_eval<CPLX>(window, h, [&](int k, float& a, float& b) {
                    const int64_t tt = t - h + k;
                    a = 0.0f; b = 0.0f;
                    if (tt < 0 || tt >= ntime) return 0u;
                    return ldev_load1<CPLX>(vf, flags, (win * ntime + tt) * nchan + c0 + j, a, b);
                });
            }
            ldev_store4<VEC>(d_time, (win * ntime + t) * nchan + c0, nv, d);
        }
    }
}

// grid: n_win * cdiv(ntime, LDEV_FR) * nstrip blocks.
template <int VIS, int W, bool VEC>
__global__ void __launch_bounds__(LDEV_NT)
k_ldev_freq(const void* __restrict__ vis_, const uint8_t* __restrict__ flags, int64_t ntime, int64_t nchan, int nstrip,
            int ntiles, int window, float* __restrict__ d_freq) {
    constexpr bool CPLX = VIS == TRI_VIS_C64;
    const int64_t blk = blockIdx.x;
    const int strip = (int)(blk % nstrip);
    const int tile = (int)(blk / nstrip % ntiles);
    const int64_t win = blk / nstrip / ntiles;
    const int64_t c0 = (int64_t)strip * LDEV_CW + threadIdx.x * LDEV_V;
    const int64_t t0 = (int64_t)tile * LDEV_FR;
    const int nrows = (int)min((int64_t)LDEV_FR, ntime - t0);
    const int nv = (int)max((int64_t)0, min((int64_t)LDEV_V, nchan - c0));
    const float* vf = reinterpret_cast<const float*>(vis_);
    if (nv <= 0) return;

    for (int r = 0; r < nrows; r++) {
        const int64_t row = (win * ntime + t0 + r) * nchan;
        float d[LDEV_V];
        if constexpr (W > 0) {
            constexpr int H = (W - 1) / 2;
            constexpr int NS = LDEV_V + 2 * H;      // slot i holds channel c0 - H + i
            float re[NS], im[NS];
            unsigned st[NS];
            {
                float r4[LDEV_V], i4[LDEV_V];
                unsigned s4[LDEV_V];
                ldev_load4<CPLX, VEC>(vf, flags, row + c0, nv, r4, i4, s4);
#pragma unroll
                for (int j = 0; j < LDEV_V; j++) { re[H + j] = r4[j]; im[H + j] = i4[j]; st[H + j] = s4[j]; }
            }
#pragma unroll
            for (int i = 0; i < NS; i++) {
                if (i >= H && i < H + LDEV_V) continue;
                const int64_t c = c0 - H + i;
                re[i] = 0.0f; im[i] = 0.0f; st[i] = 0u;
                if (c >= 0 && c < nchan) st[i] = ldev_load1<CPLX>(vf, flags, row + c, re[i], im[i]);
            }
#pragma unroll
            for (int j = 0; j < LDEV_V; j++)
                d[j] = ldev_eval<CPLX>(W, H, [&](int k, float& a, float& b) { a = re[j + k]; b = im[j + k]; return st[j + k]; });
        } else {
            const int h = (window - 1) / 2;
#pragma unroll
            for (int j = 0; j < LDEV_V; j++) {
                d[j] = __uint_as_float(0x7FC00000u);
                if (j >= nv) continue;
                d[j] = ldev_eval<CPLX>(window, h, [&](int k, float& a, float& b) {
                    const int64_t c = c0 + j - h + k;
                    a = 0.0f; b = 0.0f;
                    if (c < 0 || c >= nchan) return 0u;
                    return ldev_load1<CPLX>(vf, flags, row + c, a, b);
                });
            }
        }
        ldev_store4<VEC>(d_freq, row + c0, nv, d);
    }
}

// Bit pattern of a d that enters the level: finite and >= +0, so the values order like their bit patterns.
__device__ __forceinline__ bool ldev_key(float d, unsigned& key) {
    key = __float_as_uint(d);
    return key < 0x7F800000u;
}

// One wave: the bin of the 256-bin histogram h that holds the k-th smallest (k from 0) and the count below that bin;
// `total` is the histogram's sum.  found is false when k >= total.
__device__ __forceinline__ bool ldev_pick(const unsigned* h, unsigned k, int lane, unsigned& bin, unsigned& below,
                                          unsigned& total) {
    const unsigned h0 = h[4 * lane], h1 = h[4 * lane + 1], h2 = h[4 * lane + 2], h3 = h[4 * lane + 3];
    const unsigned mine = h0 + h1 + h2 + h3;
    unsigned incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d, 64);
        incl += lane >= d ? up : 0u;
    }
    total = __shfl(incl, 63, 64);
    const unsigned excl = incl - mine;
    const bool here = excl <= k && k < incl;
    unsigned b = 0, bl = 0;
    if (here) {
        const unsigned r = k - excl;
        if (r < h0) { b = 0; bl = 0; }
        else if (r < h0 + h1) { b = 1; bl = h0; }
        else if (r < h0 + h1 + h2) { b = 2; bl = h0 + h1; }
        else { b = 3; bl = h0 + h1 + h2; }
        b += 4 * lane;
        bl += excl;
    }
    const unsigned long long who = __ballot(here);
    if (who == 0) return false;
    const int src = __ffsll((long long)who) - 1;
    bin = __shfl(b, src, 64);
    below = __shfl(bl, src, 64);
    return true;
}

// AXIS 0: lines are (window, channel) of d (n_win, ntime, nchan), LDEV_LC adjacent channels per block;
//         grid n_win * cdiv(nchan, LDEV_LC).
// AXIS 1: lines are (window, row, chunk), chunk k = channels [ends[k], ends[k + 1]), one wave per line;
//         grid cdiv(n_win * ntime * nchunk, LDEV_LW).
// hit (n_win, ntime, nchan) receives 0 / 1 for every sample.
template <int AXIS>
__global__ void __launch_bounds__(LDEV_NT)
k_ldev_level(const float* __restrict__ d, int64_t n_win, int64_t ntime, int64_t nchan,
             const int64_t* __restrict__ ends, int nchunk, double scale, uint8_t* __restrict__ hit) {
    constexpr int NL = AXIS == 0 ? LDEV_LC : LDEV_LW;       // lines per block
    constexpr int G = LDEV_NT / NL;                         // threads per line
    __shared__ unsigned hist[NL][257];                      // 257: a line's bins start on another bank
    __shared__ unsigned s_prefix[NL], s_k[NL], s_m[NL], s_le[NL], s_nxt[NL];
    const int line = AXIS == 0 ? (int)threadIdx.x % NL : (int)threadIdx.x / G;
    const int sub = AXIS == 0 ? (int)threadIdx.x / NL : (int)threadIdx.x % G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    int64_t base = 0, stride = 1;
    int len = 0;
    if (AXIS == 0) {
        const int64_t nstrip = (nchan + NL - 1) / NL;
        const int64_t win = (int64_t)blockIdx.x / nstrip;
        const int64_t c = ((int64_t)blockIdx.x % nstrip) * NL + line;
        if (c < nchan) { base = win * ntime * nchan + c; stride = nchan; len = (int)ntime; }
    } else {
        const int64_t l = (int64_t)blockIdx.x * NL + line;
        if (l < n_win * ntime * nchunk) {
            const int64_t row = l / nchunk;
            const int k = (int)(l % nchunk);
            base = row * nchan + ends[k];
            len = (int)(ends[k + 1] - ends[k]);
        }
    }
    if (threadIdx.x < NL) { s_prefix[threadIdx.x] = 0; s_k[threadIdx.x] = 0; s_m[threadIdx.x] = 0; s_le[threadIdx.x] = 0; s_nxt[threadIdx.x] = 0xFFFFFFFFu; }

    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < NL * 257; i += LDEV_NT) (&hist[0][0])[i] = 0;
        __syncthreads();
        const unsigned prefix = s_prefix[line];
        const unsigned mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int i0 = 0; i0 < len; i0 += G) {
            const int i = i0 + sub;
            unsigned key = 0;
            const bool in = i < len && ldev_key(d[base + i * stride], key) && (key & mask) == prefix;
            const int b = in ? (int)(key >> shift & 255u) : -1;
            if (AXIS == 1) {
                // the wave is one line and its leading digits mostly agree: those lanes add as one
                const unsigned long long live = __ballot(in);
                if (live == 0) continue;
                const int src = __ffsll((long long)live) - 1;
                const int ref = __shfl(b, src, 64);
                const unsigned long long same = __ballot(b == ref);
                if (lane == src) atomicAdd(&hist[line][ref], (unsigned)__popcll(same));
                else if (in && b != ref) atomicAdd(&hist[line][b], 1u);
            } else if (in) {
                atomicAdd(&hist[line][b], 1u);
            }
        }
        __syncthreads();
        for (int l = wave; l < NL; l += LDEV_NT / 64) {
            unsigned k = s_k[l], bin = 0, below = 0, total = 0;
            if (shift == 24) {
                // the first histogram holds every value of the line: its sum is m
                unsigned none = 0, z = 0;
                ldev_pick(hist[l], 0xFFFFFFFFu, lane, none, z, total);
                k = total ? (total - 1) / 2 : 0;
            }
            const bool found = ldev_pick(hist[l], k, lane, bin, below, total);
            if (lane == 0) {
                if (shift == 24) s_m[l] = total;
                if (found) {
                    s_prefix[l] |= bin << shift;
                    s_k[l] = k - below;
                }
            }
        }
        __syncthreads();
    }

    // even count: the upper middle is lo again when enough values are <= lo, else the smallest value above lo
    const unsigned lo = s_prefix[line], m = s_m[line];
    {
        unsigned le = 0, nxt = 0xFFFFFFFFu;
        for (int i = sub; i < len; i += G) {
            unsigned key;
            if (!ldev_key(d[base + i * stride], key)) continue;
            if (key <= lo) le++;
            else nxt = key < nxt ? key : nxt;
        }
        if (le) atomicAdd(&s_le[line], le);
        if (nxt != 0xFFFFFFFFu) atomicMin(&s_nxt[line], nxt);
    }
    __syncthreads();
    float med = __uint_as_float(lo);
    if (!(m & 1u) && m) {
        const unsigned hi = s_le[line] >= m / 2 + 1 ? lo : s_nxt[line];
        const float sum = __uint_as_float(lo) + __uint_as_float(hi);
        med = sum / 2.0f;
    }
    const bool live = m >= 3 && med > 0.0f;
    const double thr = (double)med * scale;
    for (int i = sub; i < len; i += G) {
        const float v = d[base + i * stride];
        const bool usable = v == v;
        hit[base + i * stride] = usable && (v == INFINITY || (live && (double)v > thr)) ? 1 : 0;
    }
}

// n bytes; either hit image may be null (that axis is switched off).  VEC: n % 16 == 0 and 16-byte aligned bases.
template <bool VEC>
__global__ void __launch_bounds__(LDEV_NT)
k_ldev_apply(const uint8_t* __restrict__ flags, const uint8_t* __restrict__ hit_t, const uint8_t* __restrict__ hit_f,
             uint8_t* __restrict__ out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * LDEV_NT + threadIdx.x) * (VEC ? 16 : 1);
    if (i >= n) return;
    if (VEC) {
        const uint4 f = *reinterpret_cast<const uint4*>(flags + i);
        const uint4 z = make_uint4(0, 0, 0, 0);
        const uint4 a = hit_t ? *reinterpret_cast<const uint4*>(hit_t + i) : z;
        const uint4 b = hit_f ? *reinterpret_cast<const uint4*>(hit_f + i) : z;
        auto one = [](unsigned w, unsigned x, unsigned y) {
            return ((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) >> 7 & 0x01010101u) | x | y;
        };
        *reinterpret_cast<uint4*>(out + i) = make_uint4(one(f.x, a.x, b.x), one(f.y, a.y, b.y), one(f.z, a.z, b.z),
                                                         one(f.w, a.w, b.w));
    } else {
        out[i] = (flags[i] ? 1u : 0u) | (hit_t ? hit_t[i] : 0u) | (hit_f ? hit_f[i] : 0u);
    }
}
