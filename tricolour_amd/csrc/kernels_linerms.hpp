// kernels_linerms.hpp -- line-RMS statistics of (time, chan) windows and the thresholding of whole timesteps and
// whole channels on them (the model is AOFlagger's threshold_timestep_rms / threshold_channel_rms; the definition is
// this project's own, include/tricolour_amd.h).
//
// Per window, visibilities v and input flags f:
//   p      = (double)re * (double)re + (double)im * (double)im     (float32 amplitudes: (double)a * (double)a)
//   counts = f == 0 and p is not NaN
//   rms    = sqrt(sum p / n) over the n counting samples of a time row (over channels) or a channel (over times);
//            NaN for an empty line (n == 0)
//   med, sigma = median and 1.4826 * median(|rms - med|) of the finite rms of one axis;  a finite line is bad when
//            |rms - med| > nsigma * sigma (flag_low) or rms - med > nsigma * sigma;  a non-empty, non-finite line is
//            always bad;  fewer than 3 finite lines or !(sigma > 1e-9 * med): nothing else is
//   out    = f | bad_time[t] | bad_chan[c]
//
// Four launches.
//   k_lrms_power    the only pass over the visibilities (8 B + 1 B per sample; 4 B + 1 B for amplitudes).  A block of
//                   256 threads owns a tile of LRMS_TR = 64 rows x LRMS_CW = 1024 channels; a thread owns 4 adjacent
//                   channels (two 16-byte loads and one 4-byte flag load per row).  Row sums: the thread's 4 samples
//                   in channel order, an xor butterfly over the wave, the wave's value parked in LDS; after the last
//                   row the 4 waves are added in wave order -> one partial per (row, 1024-channel strip).  Channel
//                   sums: per-thread accumulators carried down the tile's rows in row order -> one partial per
//                   (64-row tile, channel).  No atomics; the order depends on the shape alone (not on the batch, the
//                   alignment or the run), so the sums are reproducible bit for bit.
//   k_lrms_combine  one thread per line: the partials in strip / tile order, rms = sqrt(sum / n).
//   k_lrms_decide   one block per (window, axis): exact medians by an 8-bit radix select over the bit patterns of the
//                   non-negative float64 values in global memory (any line count), then the bad-line bytes.
//   k_lrms_apply    out = f | bad_time | bad_chan, 16 flags per thread (VEC) or one.
#pragma once

#define LRMS_NT 256                 // power pass: threads per block
#define LRMS_V 4                    //             channels per thread
#define LRMS_CW (LRMS_NT * LRMS_V)  //             channels per strip
#define LRMS_TR 64                  //             rows per tile
#define LRMS_RB 4                   //             rows loaded ahead of their arithmetic
#define LRMS_DT 512                 // decision: threads per block

// VIS: TRI_VIS_C64 or TRI_VIS_F32.  VEC: nchan % 4 == 0 and the bases aligned for the 16-byte / 4-byte loads; the
// arithmetic and its order are the same either way.
template <int VIS, bool VEC>
__global__ void __launch_bounds__(LRMS_NT)
k_lrms_power(const void* __restrict__ vis_, const uint8_t* __restrict__ flags, int64_t ntime, int64_t nchan,
             int nstrip, int ntiles, double* __restrict__ row_sum, int* __restrict__ row_cnt,
             double* __restrict__ ch_sum, int* __restrict__ ch_cnt) {
    constexpr bool CPLX = VIS == TRI_VIS_C64;
    __shared__ double sh_sum[LRMS_TR][LRMS_NT / 64];
    __shared__ int sh_cnt[LRMS_TR][LRMS_NT / 64];

    const int64_t blk = blockIdx.x;
    const int strip = (int)(blk % nstrip);
    const int tile = (int)(blk / nstrip % ntiles);
    const int64_t win = blk / nstrip / ntiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)strip * LRMS_CW + threadIdx.x * LRMS_V;
    const int64_t t0 = (int64_t)tile * LRMS_TR;
    const int nrows = (int)min((int64_t)LRMS_TR, ntime - t0);
    const int nv = (int)max((int64_t)0, min((int64_t)LRMS_V, nchan - c0));     // channels this thread has
    const float* vf = reinterpret_cast<const float*>(vis_);

    double cs[LRMS_V];
    int cc[LRMS_V];
#pragma unroll
    for (int j = 0; j < LRMS_V; j++) { cs[j] = 0.0; cc[j] = 0; }

    for (int r0 = 0; r0 < nrows; r0 += LRMS_RB) {
        float re[LRMS_RB][LRMS_V], im[LRMS_RB][LRMS_V];
        unsigned fl[LRMS_RB];                       // byte j = flag of channel j; 0xFF where there is no sample
        // ---- loads of LRMS_RB rows
#pragma unroll
        for (int q = 0; q < LRMS_RB; q++) {
            const bool live = r0 + q < nrows && nv > 0;
            const int64_t s = ((win * ntime + t0 + r0 + q) * nchan + c0);
            fl[q] = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < LRMS_V; j++) { re[q][j] = 0.0f; im[q][j] = 0.0f; }
            if (!live) continue;
            if (VEC) {
                fl[q] = *reinterpret_cast<const unsigned*>(flags + s);
                if (CPLX) {
                    const float4 a = *reinterpret_cast<const float4*>(vf + 2 * s);
                    const float4 b = *reinterpret_cast<const float4*>(vf + 2 * s + 4);
                    re[q][0] = a.x; im[q][0] = a.y; re[q][1] = a.z; im[q][1] = a.w;
                    re[q][2] = b.x; im[q][2] = b.y; re[q][3] = b.z; im[q][3] = b.w;
                } else {
                    const float4 a = *reinterpret_cast<const float4*>(vf + s);
                    re[q][0] = a.x; re[q][1] = a.y; re[q][2] = a.z; re[q][3] = a.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < LRMS_V; j++) {
                    if (j < nv) {
                        fl[q] = (fl[q] & ~(0xFFu << (8 * j))) | ((unsigned)flags[s + j] << (8 * j));
                        if (CPLX) {
                            const float2 a = *reinterpret_cast<const float2*>(vf + 2 * (s + j));
                            re[q][j] = a.x; im[q][j] = a.y;
                        } else {
                            re[q][j] = vf[s + j];
                        }
                    }
                }
            }
        }
        // ---- arithmetic
#pragma unroll
        for (int q = 0; q < LRMS_RB; q++) {
            double rsum = 0.0;
            int rcnt = 0;
#pragma unroll
            for (int j = 0; j < LRMS_V; j++) {
                const double a = (double)re[q][j], b = (double)im[q][j];
                double p = CPLX ? a * a + b * b : a * a;
                const bool counts = ((fl[q] >> (8 * j)) & 0xFFu) == 0 && p == p;
                p = counts ? p : 0.0;
                rsum += p;
                cs[j] += p;
                rcnt += counts ? 1 : 0;
                cc[j] += counts ? 1 : 0;
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                rsum += __shfl_xor(rsum, d, 64);
                rcnt += __shfl_xor(rcnt, d, 64);
            }
            if (lane == 0 && r0 + q < nrows) {
                sh_sum[r0 + q][wave] = rsum;
                sh_cnt[r0 + q][wave] = rcnt;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nrows) {
        double s = sh_sum[threadIdx.x][0];
        int n = sh_cnt[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < LRMS_NT / 64; w++) {
            s += sh_sum[threadIdx.x][w];
            n += sh_cnt[threadIdx.x][w];
        }
        const int64_t o = (win * ntime + t0 + threadIdx.x) * nstrip + strip;
        row_sum[o] = s;
        row_cnt[o] = n;
    }
    const int64_t oc = (win * ntiles + tile) * nchan + c0;
#pragma unroll
    for (int j = 0; j < LRMS_V; j++) {
        if (j < nv) {
            ch_sum[oc + j] = cs[j];
            ch_cnt[oc + j] = cc[j];
        }
    }
}

// One thread per line: lines [0, n_win * ntime) are the time rows, the rest the channels.  cnt_t / cnt_c may be null.
__global__ void k_lrms_combine(const double* __restrict__ row_sum, const int* __restrict__ row_cnt,
                               const double* __restrict__ ch_sum, const int* __restrict__ ch_cnt, int64_t n_win,
                               int64_t ntime, int64_t nchan, int nstrip, int ntiles, double* __restrict__ rms_t,
                               double* __restrict__ rms_c, int* __restrict__ cnt_t, int* __restrict__ cnt_c) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nt = n_win * ntime;
    double s = 0.0;
    int64_t n = 0;
    if (i < nt) {
        for (int k = 0; k < nstrip; k++) {
            s += row_sum[i * nstrip + k];
            n += row_cnt[i * nstrip + k];
        }
        rms_t[i] = n ? sqrt(s / (double)n) : (double)NAN;
        if (cnt_t) cnt_t[i] = (int)n;
    } else if (i - nt < n_win * nchan) {
        const int64_t l = i - nt, win = l / nchan, c = l % nchan;
        for (int k = 0; k < ntiles; k++) {
            s += ch_sum[(win * ntiles + k) * nchan + c];
            n += ch_cnt[(win * ntiles + k) * nchan + c];
        }
        rms_c[l] = n ? sqrt(s / (double)n) : (double)NAN;
        if (cnt_c) cnt_c[l] = (int)n;
    }
}

// Bit pattern of the value line i enters a median with: rms, or |rms - med| for the second median.  False for a line
// that is not usable (empty: NaN; unflagged inf: inf).  The values are >= +0, so they order like their bit patterns.
__device__ __forceinline__ bool lrms_key(const double* __restrict__ v, int i, bool dev, double med,
                                         unsigned long long& key) {
    const double r = v[i];
    if ((__double_as_longlong(r) & 0x7FF0000000000000ll) == 0x7FF0000000000000ll) return false;
    key = (unsigned long long)__double_as_longlong(dev ? fabs(r - med) : r);
    return true;
}

// k-th smallest (k from 0) of the m usable values, exact, and the median from it; all threads of the block call this
// and all get the result.  hist: 256 counters; red: two 64-bit words.
__device__ double lrms_median(const double* __restrict__ v, int n, bool dev, double med, unsigned m,
                              unsigned* hist, unsigned long long* red) {
    unsigned k = (m - 1) / 2;
    unsigned long long prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int b = threadIdx.x; b < 256; b += LRMS_DT) hist[b] = 0;
        __syncthreads();
        // runs of one digit (the leading digits of a line's values mostly agree) go to LDS as one add
        int cur = -1;
        unsigned run = 0;
        for (int i = threadIdx.x; i < n; i += LRMS_DT) {
            unsigned long long key;
            if (!lrms_key(v, i, dev, med, key) || (key & mask) != prefix) continue;
            const int b = (int)(key >> shift & 255);
            if (b != cur) {
                if (run) atomicAdd(&hist[cur], run);
                cur = b;
                run = 0;
            }
            run++;
        }
        if (run) atomicAdd(&hist[cur], run);
        __syncthreads();
        unsigned below = 0;
        int b = 0;
        for (; b < 255; b++) {
            const unsigned h = hist[b];
            if (below + h > k) break;
            below += h;
        }
        k -= below;
        prefix |= (unsigned long long)b << shift;
        mask |= 0xFFull << shift;
        __syncthreads();
    }
    const double lo = __longlong_as_double((long long)prefix);
    if (m & 1u) return lo;
    // even count: the upper middle is lo again when enough values are <= lo, else the smallest value above lo
    if (threadIdx.x == 0) {
        red[0] = 0;
        red[1] = ~0ull;
    }
    __syncthreads();
    unsigned le = 0;
    unsigned long long nxt = ~0ull;
    for (int i = threadIdx.x; i < n; i += LRMS_DT) {
        unsigned long long key;
        if (!lrms_key(v, i, dev, med, key)) continue;
        if (key <= prefix) le++;
        else nxt = key < nxt ? key : nxt;
    }
    if (le) atomicAdd(&red[0], (unsigned long long)le);
    if (nxt != ~0ull) atomicMin(&red[1], nxt);
    __syncthreads();
    const unsigned long long hi = red[0] >= (unsigned long long)(m / 2 + 1) ? prefix : red[1];
    __syncthreads();
    return (lo + __longlong_as_double((long long)hi)) / 2.0;
}

// grid (n_win, 2): y = 0 the time rows of the window, y = 1 its channels.
__global__ void __launch_bounds__(LRMS_DT)
k_lrms_decide(const double* __restrict__ rms_t, const double* __restrict__ rms_c, int64_t ntime, int64_t nchan,
              double nsigma_time, double nsigma_freq, int flag_low, uint8_t* __restrict__ bad_t,
              uint8_t* __restrict__ bad_c) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long red[2];
    const bool chan = blockIdx.y == 1;
    const int n = (int)(chan ? nchan : ntime);
    const double nsigma = chan ? nsigma_freq : nsigma_time;
    const double* v = (chan ? rms_c : rms_t) + (int64_t)blockIdx.x * n;
    uint8_t* bad = (chan ? bad_c : bad_t) + (int64_t)blockIdx.x * n;
    if (!(nsigma > 0.0)) {                          // the axis is switched off
        for (int i = threadIdx.x; i < n; i += LRMS_DT) bad[i] = 0;
        return;
    }
    if (threadIdx.x == 0) red[0] = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int i = threadIdx.x; i < n; i += LRMS_DT) {
        unsigned long long key;
        mine += lrms_key(v, i, false, 0.0, key) ? 1u : 0u;
    }
    if (mine) atomicAdd(&red[0], (unsigned long long)mine);
    __syncthreads();
    const unsigned m = (unsigned)red[0];
    __syncthreads();
    bool live = false;
    double med = 0.0, thr = 0.0;
    if (m >= 3) {
        med = lrms_median(v, n, false, 0.0, m, hist, red);
        const double sigma = 1.4826 * lrms_median(v, n, true, med, m, hist, red);
        live = sigma > 1e-9 * med;
        thr = nsigma * sigma;
    }
    for (int i = threadIdx.x; i < n; i += LRMS_DT) {
        const double r = v[i];
        bool b = false;
        if (r == r) {                               // NaN: empty line
            const double d = r - med;
            if ((__double_as_longlong(r) & 0x7FF0000000000000ll) == 0x7FF0000000000000ll) b = true;
            else if (live) b = flag_low ? fabs(d) > thr : d > thr;
        }
        bad[i] = b ? 1 : 0;
    }
}

// grid (n_win * ntime rows, pieces of a row).  VEC: nchan % 16 == 0 and 16-byte aligned bases, 16 flags per thread.
template <bool VEC>
__global__ void __launch_bounds__(256)
k_lrms_apply(const uint8_t* __restrict__ flags, const uint8_t* __restrict__ bad_t, const uint8_t* __restrict__ bad_c,
             uint8_t* __restrict__ out, int64_t ntime, int64_t nchan) {
    const int64_t row = blockIdx.x;
    const int64_t win = row / ntime;
    const int64_t c = ((int64_t)blockIdx.y * 256 + threadIdx.x) * (VEC ? 16 : 1);
    if (c >= nchan) return;
    const unsigned bt = bad_t[row];
    if (VEC) {
        const uint4 f = *reinterpret_cast<const uint4*>(flags + row * nchan + c);
        const uint4 bc = *reinterpret_cast<const uint4*>(bad_c + win * nchan + c);
        auto one = [bt](unsigned w, unsigned b) {
            return ((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) >> 7 & 0x01010101u) | b | bt * 0x01010101u;
        };
        *reinterpret_cast<uint4*>(out + row * nchan + c) = make_uint4(one(f.x, bc.x), one(f.y, bc.y), one(f.z, bc.z),
                                                                       one(f.w, bc.w));
    } else {
        out[row * nchan + c] = (flags[row * nchan + c] ? 1u : 0u) | bad_c[win * nchan + c] | bt;
    }
}
