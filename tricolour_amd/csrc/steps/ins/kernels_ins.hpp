// kernels_ins.hpp -- sky-subtracted incoherent noise spectrum: the amplitudes of the time differences of every
// baseline averaged over baselines into one (corr, ntime - 1, chan) image, z-scored against the channel's median over
// time and matched against channel ranges (the model is SSINS, Wilensky et al. 2019; the definition is this project's
// own, include/tricolour_amd.h, and identity with SSINS is not claimed).
//
// vis (nbl, ncorr, ntime, nchan) complex64 or float32 amplitudes (re = a, im = 0), flags uint8, select[nbl] or null;
// nd = ntime - 1 difference rows, image position i = (k, t, c), t in [0, nd):
//   d        = tri_hypotf(re[t+1] - re[t], im[t+1] - im[t]); the pair counts if its baseline is selected, both flags
//              are 0 and d is not NaN;  sum[i] += (double)d, count[i] += 1 for b = 0 .. nbl - 1 in that order
//   x        = count >= min_count ? (float)(sum / (double)count) : NaN
//   level    = per line (k, c) the median of the finite x of its unmasked rows (even count: float32(a + b) / 2);
//              live with >= 3 of them and a level > 0
//   q        = fixed-point z-score, rint(clamp((x / med - 1) * sqrt(count / (4/pi - 1)), +-16384) * 65536); 2^30 for
//              x = +inf; 0 where the position is not valid
//   match    = per row (k, t): the channel range (or the single position) with the largest sum(q) / sqrt(m) / nsigma
//              above 1 goes into the mask; rounds repeat level, q and match on the mask so far
//   out      = (flags != 0) | mask[t - 1] | mask[t]
//
// Six kernels; no floating-point atomics, integer LDS atomics in the level kernel only.
//   k_ins_accumulate  the only pass over the visibilities (8 B + 1 B per sample).  A thread owns VEC adjacent channels
//                     of INS_STRIP consecutive difference rows: per baseline it loads INS_STRIP + 1 rows (each row
//                     feeds two differences and is fetched once, plus one halo row per strip), all loads issued
//                     together, and walks the baselines in memory order, so a position's float64 sum has one order
//                     whatever the grid or the split of the baselines over calls.  An image too small to fill the
//                     device with strips takes the single-row form: one difference row per thread, two rows loaded,
//                     INS_UNROLL baselines in flight.
//   k_ins_mean        sum / count -> x; one pass over the image.
//   k_ins_level       the level of every line by an exact 8-bit radix select over order-preserving keys of x
//                     (4 counting passes and one for the upper middle of an even count); 32 adjacent channels per
//                     block, 8 threads per channel (rows of 128 bytes).
//   k_ins_zq          valid and q of every position.
//   k_ins_match       one block per row: integer sums per shape (wave shuffles, then LDS), the narrow maximum, the
//                     pick, and its range into the mask.  The sums are exact, so their order is free.
//   k_ins_apply       out = flags | mask[t - 1] | mask[t], 16 flags per thread (VEC16) or one, for every baseline.
// VEC in the accumulate: nchan % 4 == 0 and the bases aligned for 16-byte / 4-byte accesses.  It changes neither the
// arithmetic nor its order.
#pragma once

#define INS_NT 256          // threads per block, all kernels
#define INS_STRIP 8         // k_ins_accumulate: difference rows per thread of the strip form
#define INS_UNROLL 4        //                   baselines in flight of the single-row form
#define INS_FILL 131072     //                   threads that fill the device at the strip form's 2 waves per SIMD
#define INS_LC 32           // k_ins_level: channels per block
#define INS_MAX_SHAPES 32
#define INS_QNAN 0x7FC00000u

// VEC samples of one visibility row: parts (im only for complex64) and the flag bytes, byte j = flag of sample j.
template <int VD, int VEC>
struct InsRow {
    float re[VEC], im[VEC];
    unsigned fl;
};

template <int VD, int VEC>
__device__ __forceinline__ void ins_load(const float* vp, const uint8_t* fp, InsRow<VD, VEC>& s) {
    constexpr bool CPLX = VD == TRI_VIS_C64;
    if constexpr (VEC == 4) {
        s.fl = *reinterpret_cast<const unsigned*>(fp);
        const float4 a = *reinterpret_cast<const float4*>(vp);
        if constexpr (CPLX) {
            const float4 b = *reinterpret_cast<const float4*>(vp + 4);
            s.re[0] = a.x; s.im[0] = a.y; s.re[1] = a.z; s.im[1] = a.w;
            s.re[2] = b.x; s.im[2] = b.y; s.re[3] = b.z; s.im[3] = b.w;
        } else {
            s.re[0] = a.x; s.re[1] = a.y; s.re[2] = a.z; s.re[3] = a.w;
        }
    } else {
        s.fl = fp[0];
        if constexpr (CPLX) {
            const float2 a = *reinterpret_cast<const float2*>(vp);
            s.re[0] = a.x; s.im[0] = a.y;
        } else {
            s.re[0] = vp[0];
        }
    }
}

// the differences of row `b` (time t + 1) and row `a` (time t) into the accumulators of difference row t
template <int VD, int VEC>
__device__ __forceinline__ void ins_add(const InsRow<VD, VEC>& a, const InsRow<VD, VEC>& b, double (&sum)[VEC],
                                        int (&cnt)[VEC]) {
    const unsigned fl = a.fl | b.fl;
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        const float dr = b.re[j] - a.re[j];
        float d;
        if constexpr (VD == TRI_VIS_C64) d = tri_hypotf(dr, b.im[j] - a.im[j]);
        else d = fabsf(dr);                                  // tri_hypotf(dr, 0)
        const bool counts = ((fl >> (8 * j)) & 0xFFu) == 0 && d == d;
        sum[j] = counts ? sum[j] + (double)d : sum[j];
        cnt[j] += counts ? 1 : 0;
    }
}

// VD: TRI_VIS_C64 or TRI_VIS_F32.  STRIP difference rows per thread, BU baselines whose loads are in flight
// together: <INS_STRIP, 1> for an image that fills the device with strips (one halo row per 8), <1, INS_UNROLL> for a
// smaller one, where a strip would leave SIMDs idle and the second read of every row comes from cache.  npc =
// nchan / VEC pieces per row, ntile = cdiv(ntime - 1, STRIP) strips; ncorr * ntile * npc threads, adjacent threads on
// adjacent pieces.  select: one byte per baseline (nonzero: takes part) or null; the branches on it are the same in
// every lane.  Whatever the form, a position's sum takes the baselines in ascending order.
template <int VD, int VEC, int STRIP, int BU>
__global__ void __launch_bounds__(INS_NT)
k_ins_accumulate(const void* __restrict__ vis_, const uint8_t* __restrict__ flags, const uint8_t* __restrict__ select,
                 int64_t nbl, int64_t ncorr, int64_t ntime, int64_t nchan, int64_t npc, int64_t ntile,
                 double* __restrict__ sum_, int* __restrict__ count_) {
    constexpr int W = VD == TRI_VIS_C64 ? 2 : 1;          // floats per sample
    const int64_t g = (int64_t)blockIdx.x * INS_NT + threadIdx.x;
    if (g >= ncorr * ntile * npc) return;
    const int64_t piece = g % npc, tile = g / npc % ntile, k = g / npc / ntile;
    const int64_t nd = ntime - 1, t0 = tile * STRIP, c0 = piece * VEC;
    const int nrows = (int)min((int64_t)STRIP, nd - t0);                   // difference rows of this strip, >= 1
    const int64_t n = ncorr * ntime * nchan;                               // samples per baseline
    // 64-bit steps: baseline b starts b * n samples on, past 2^32 bytes for any real scan
    const float* vp = reinterpret_cast<const float*>(vis_) + ((k * ntime + t0) * nchan + c0) * W;
    const uint8_t* fp = flags + (k * ntime + t0) * nchan + c0;
    double* sp = sum_ + (k * nd + t0) * nchan + c0;
    int* cp = count_ + (k * nd + t0) * nchan + c0;

    double sum[STRIP][VEC];
    int cnt[STRIP][VEC];
#pragma unroll
    for (int r = 0; r < STRIP; r++) {
#pragma unroll
        for (int j = 0; j < VEC; j++) { sum[r][j] = 0.0; cnt[r][j] = 0; }
        if (r < nrows) {
            if constexpr (VEC == 4) {
                const double2 s0 = *reinterpret_cast<const double2*>(sp + r * nchan);
                const double2 s1 = *reinterpret_cast<const double2*>(sp + r * nchan + 2);
                const int4 c = *reinterpret_cast<const int4*>(cp + r * nchan);
                sum[r][0] = s0.x; sum[r][1] = s0.y; sum[r][2] = s1.x; sum[r][3] = s1.y;
                cnt[r][0] = c.x; cnt[r][1] = c.y; cnt[r][2] = c.z; cnt[r][3] = c.w;
            } else {
                sum[r][0] = sp[r * nchan];
                cnt[r][0] = cp[r * nchan];
            }
        }
    }

    // bit q: baseline b0 + q exists and takes part
    auto group = [&](int64_t b0) {
        unsigned m = 0;
#pragma unroll
        for (int q = 0; q < BU; q++)
            if (b0 + q < nbl) m |= (!select || select[b0 + q] != 0 ? 1u : 0u) << q;
        return m;
    };
    unsigned on = group(0);
    for (int64_t b = 0; b < nbl; b += BU) {
        // the next group's select bytes are asked for before this group's rows, so their wait is the rows' own
        const unsigned next = group(b + BU);
        const unsigned cur = __builtin_amdgcn_readfirstlane(on);
        InsRow<VD, VEC> row[BU][STRIP + 1];
#pragma unroll
        for (int q = 0; q < BU; q++) {
#pragma unroll
            for (int r = 0; r <= STRIP; r++) {
#pragma unroll
                for (int j = 0; j < VEC; j++) { row[q][r].re[j] = 0.0f; row[q][r].im[j] = 0.0f; }
                row[q][r].fl = 0xFFFFFFFFu;
            }
            if (cur >> q & 1u) {
#pragma unroll
                for (int r = 0; r <= STRIP; r++)
                    if (r <= nrows) ins_load<VD, VEC>(vp + (q * n + r * nchan) * W, fp + q * n + r * nchan, row[q][r]);
            }
        }
#pragma unroll
        for (int q = 0; q < BU; q++) {                       // strictly in baseline order
            if (cur >> q & 1u) {
#pragma unroll
                for (int r = 0; r < STRIP; r++)
                    if (r < nrows) ins_add<VD, VEC>(row[q][r], row[q][r + 1], sum[r], cnt[r]);
            }
        }
        on = next;
        vp += BU * n * W;
        fp += BU * n;
    }

#pragma unroll
    for (int r = 0; r < STRIP; r++) {
        if (r < nrows) {
            if constexpr (VEC == 4) {
                *reinterpret_cast<double2*>(sp + r * nchan) = make_double2(sum[r][0], sum[r][1]);
                *reinterpret_cast<double2*>(sp + r * nchan + 2) = make_double2(sum[r][2], sum[r][3]);
                *reinterpret_cast<int4*>(cp + r * nchan) = make_int4(cnt[r][0], cnt[r][1], cnt[r][2], cnt[r][3]);
            } else {
                sp[r * nchan] = sum[r][0];
                cp[r * nchan] = cnt[r][0];
            }
        }
    }
}

// One thread per position of the image: x = the mean of a usable position, NaN otherwise.
__global__ void __launch_bounds__(INS_NT)
k_ins_mean(const double* __restrict__ sum, const int* __restrict__ count, int64_t n, int64_t min_count,
           float* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * INS_NT + threadIdx.x;
    if (i >= n) return;
    const int c = count[i];
    x[i] = (int64_t)c >= min_count ? (float)(sum[i] / (double)c) : __uint_as_float(INS_QNAN);
}

// Order-preserving key of a float32 (negative values below positive ones); false for a value that does not enter the
// level: masked, NaN or infinite.
__device__ __forceinline__ bool ins_key(float x, unsigned masked, unsigned& key) {
    const unsigned u = __float_as_uint(x);
    key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return masked == 0 && (u & 0x7FFFFFFFu) < 0x7F800000u;
}

__device__ __forceinline__ float ins_unkey(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// One wave: the bin of the 256-bin histogram h that holds the k-th smallest (k from 0) and the count below that bin;
// `total` is the histogram's sum.  false when k >= total.
__device__ __forceinline__ bool ins_pick(const unsigned* h, unsigned k, int lane, unsigned& bin, unsigned& below,
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

// Lines are (corr, channel) of x (ncorr, nd, nchan), INS_LC adjacent channels per block; grid ncorr * cdiv(nchan,
// INS_LC).  level / live (ncorr, nchan): the median (NaN for an empty line) and whether the line is live.
__global__ void __launch_bounds__(INS_NT)
k_ins_level(const float* __restrict__ x, const uint8_t* __restrict__ mask, int64_t nd, int64_t nchan,
            float* __restrict__ level, uint8_t* __restrict__ live) {
    constexpr int NL = INS_LC;                              // lines per block
    constexpr int G = INS_NT / NL;                          // threads per line
    __shared__ unsigned hist[NL][257];                      // 257: a line's bins start on another bank
    __shared__ unsigned s_prefix[NL], s_k[NL], s_m[NL], s_le[NL], s_nxt[NL];
    const int line = (int)threadIdx.x % NL, sub = (int)threadIdx.x / NL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    const int64_t nstrip = (nchan + NL - 1) / NL;
    const int64_t k = (int64_t)blockIdx.x / nstrip;
    const int64_t c = ((int64_t)blockIdx.x % nstrip) * NL + line;
    const int64_t base = k * nd * nchan + c;
    const int len = c < nchan ? (int)nd : 0;
    if (threadIdx.x < NL) { s_prefix[threadIdx.x] = 0; s_k[threadIdx.x] = 0; s_m[threadIdx.x] = 0; s_le[threadIdx.x] = 0; s_nxt[threadIdx.x] = 0xFFFFFFFFu; }

    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < NL * 257; i += INS_NT) (&hist[0][0])[i] = 0;
        __syncthreads();
        const unsigned prefix = s_prefix[line];
        const unsigned high = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int i = sub; i < len; i += G) {
            unsigned key;
            if (ins_key(x[base + i * nchan], mask[base + i * nchan], key) && (key & high) == prefix)
                atomicAdd(&hist[line][key >> shift & 255u], 1u);
        }
        __syncthreads();
        for (int l = wave; l < NL; l += INS_NT / 64) {
            unsigned kk = s_k[l], bin = 0, below = 0, total = 0;
            if (shift == 24) {
                // the first histogram holds every value of the line: its sum is m
                unsigned none = 0, z = 0;
                ins_pick(hist[l], 0xFFFFFFFFu, lane, none, z, total);
                kk = total ? (total - 1) / 2 : 0;
            }
            const bool found = ins_pick(hist[l], kk, lane, bin, below, total);
            if (lane == 0) {
                if (shift == 24) s_m[l] = total;
                if (found) {
                    s_prefix[l] |= bin << shift;
                    s_k[l] = kk - below;
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
            if (!ins_key(x[base + i * nchan], mask[base + i * nchan], key)) continue;
            if (key <= lo) le++;
            else nxt = key < nxt ? key : nxt;
        }
        if (le) atomicAdd(&s_le[line], le);
        if (nxt != 0xFFFFFFFFu) atomicMin(&s_nxt[line], nxt);
    }
    __syncthreads();
    if (sub == 0 && c < nchan) {
        float med = __uint_as_float(INS_QNAN);
        if (m) {
            med = ins_unkey(lo);
            if (!(m & 1u)) {
                const unsigned hi = s_le[line] >= m / 2 + 1 ? lo : s_nxt[line];
                const float two = ins_unkey(lo) + ins_unkey(hi);
                med = two / 2.0f;
            }
        }
        level[k * nchan + c] = med;
        live[k * nchan + c] = m >= 3 && med > 0.0f ? 1 : 0;
    }
}

// One thread per position: valid and q.
__global__ void __launch_bounds__(INS_NT)
k_ins_zq(const float* __restrict__ x, const int* __restrict__ count, const uint8_t* __restrict__ mask,
         const float* __restrict__ level, const uint8_t* __restrict__ live, int64_t nd, int64_t nchan, int64_t n,
         int64_t min_count, int* __restrict__ q, uint8_t* __restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * INS_NT + threadIdx.x;
    if (i >= n) return;
    const int64_t line = i / (nd * nchan) * nchan + i % nchan;
    const int cnt = count[i];
    const bool ok = (int64_t)cnt >= min_count && mask[i] == 0 && live[line] != 0;
    int qq = 0;
    if (ok) {
        const float xv = x[i];
        if (xv == INFINITY) {
            qq = 1 << 30;
        } else {
            const double z = ((double)xv / (double)level[line] - 1.0) * sqrt((double)cnt / 0.2732395447351628);
            qq = (int)rint(fmin(fmax(z, -16384.0), 16384.0) * 65536.0);
        }
    }
    q[i] = qq;
    valid[i] = ok ? 1 : 0;
}

// the shapes of a match, by value in the kernel arguments
struct InsShapes {
    int n;
    int lo[INS_MAX_SHAPES], hi[INS_MAX_SHAPES];
    double nsigma[INS_MAX_SHAPES];
    double nsigma_narrow;
};

// grid: ncorr * nd rows, one block each.  Adds the row's pick to mask.
__global__ void __launch_bounds__(INS_NT)
k_ins_match(const int* __restrict__ q, const uint8_t* __restrict__ valid, int64_t nchan, InsShapes sh,
            uint8_t* __restrict__ mask) {
    __shared__ long long s_sum[INS_MAX_SHAPES][INS_NT / 64], s_key[INS_NT / 64];
    __shared__ int s_cnt[INS_MAX_SHAPES][INS_NT / 64];
    __shared__ int s_lo, s_hi;
    const int64_t row = (int64_t)blockIdx.x * nchan;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long none = INT64_MIN;

    for (int i = 0; i < sh.n; i++) {
        long long s = 0;
        int m = 0;
        for (int c = sh.lo[i] + (int)threadIdx.x; c < sh.hi[i]; c += INS_NT) {
            s += q[row + c];                                // q is 0 where the position is not valid
            m += valid[row + c];
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            s += __shfl_down(s, d, 64);
            m += __shfl_down(m, d, 64);
        }
        if (lane == 0) { s_sum[i][wave] = s; s_cnt[i][wave] = m; }
    }
    long long key = none;
    if (sh.nsigma_narrow > 0.0) {
        // largest q, lowest channel on ties: q in the high word, the complement of the channel in the low one
        for (int64_t c = threadIdx.x; c < nchan; c += INS_NT)
            if (valid[row + c]) {
                const long long kq = (long long)q[row + c] * 4294967296ll + (long long)(0xFFFFFFFFu - (unsigned)c);
                key = kq > key ? kq : key;
            }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const long long o = __shfl_down(key, d, 64);
            key = o > key ? o : key;
        }
    }
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        double best = 1.0;                                   // only r > 1 is a pick
        int lo = 0, hi = 0;
        for (int i = 0; i < sh.n; i++) {
            long long s = 0;
            int m = 0;
            for (int w = 0; w < INS_NT / 64; w++) { s += s_sum[i][w]; m += s_cnt[i][w]; }
            if (m == 0) continue;
            const double r = ((double)s / 65536.0) / sqrt((double)m) / sh.nsigma[i];
            if (r > best) { best = r; lo = sh.lo[i]; hi = sh.hi[i]; }
        }
        long long kk = none;
        for (int w = 0; w < INS_NT / 64; w++) kk = s_key[w] > kk ? s_key[w] : kk;
        if (kk != none) {
            const int qq = (int)(kk >> 32);
            const int c = (int)(0xFFFFFFFFu - (unsigned)(kk & 0xFFFFFFFFll));
            const double r = ((double)qq / 65536.0) / sh.nsigma_narrow;
            if (r > best) { best = r; lo = c; hi = c + 1; }
        }
        s_lo = lo;
        s_hi = hi;
    }
    __syncthreads();
    for (int c = s_lo + (int)threadIdx.x; c < s_hi; c += INS_NT) mask[row + c] = 1;
}

// grid (pieces of one baseline's (ncorr, ntime, nchan) flags, baselines): a thread reads its piece of the two mask
// rows once and walks the baselines blockIdx.y, blockIdx.y + gridDim.y, ...  VEC16: nchan % 16 == 0 and 16-byte
// aligned bases, 16 flags per thread.  out may be flags itself: every byte is read and written by one thread.
template <bool VEC16>
__global__ void __launch_bounds__(INS_NT)
k_ins_apply(const uint8_t* flags, const uint8_t* __restrict__ mask, uint8_t* out, int64_t nbl, int64_t ntime,
            int64_t nchan, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * INS_NT + threadIdx.x) * (VEC16 ? 16 : 1);
    if (i >= n) return;
    const int64_t nd = ntime - 1, c = i % nchan, t = i / nchan % ntime, k = i / nchan / ntime;
    const uint8_t* up = mask + (k * nd + t - 1) * nchan + c;      // difference row t - 1; read only when it exists
    const uint8_t* dn = mask + (k * nd + t) * nchan + c;
    // byte-wise "!= 0" of a dword
    auto norm = [](unsigned w) { return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) >> 7 & 0x01010101u; };
    if constexpr (VEC16) {
        uint4 l = make_uint4(0, 0, 0, 0);
        if (t >= 1) {
            const uint4 a = *reinterpret_cast<const uint4*>(up);
            l = make_uint4(norm(a.x), norm(a.y), norm(a.z), norm(a.w));
        }
        if (t < nd) {
            const uint4 a = *reinterpret_cast<const uint4*>(dn);
            l = make_uint4(l.x | norm(a.x), l.y | norm(a.y), l.z | norm(a.z), l.w | norm(a.w));
        }
        for (int64_t b = blockIdx.y; b < nbl; b += gridDim.y) {
            const uint4 f = *reinterpret_cast<const uint4*>(flags + b * n + i);
            *reinterpret_cast<uint4*>(out + b * n + i) =
                make_uint4(norm(f.x) | l.x, norm(f.y) | l.y, norm(f.z) | l.z, norm(f.w) | l.w);
        }
    } else {
        unsigned l = 0;
        if (t >= 1) l |= up[0] ? 1u : 0u;
        if (t < nd) l |= dn[0] ? 1u : 0u;
        for (int64_t b = blockIdx.y; b < nbl; b += gridDim.y)
            out[b * n + i] = (uint8_t)((flags[b * n + i] ? 1u : 0u) | l);
    }
}
