// kernels_quality.hpp -- quality statistics of the unflagged samples of (bl, corr, time, chan) windows, after AOFlagger's
// quality statistics (the definition is this project's own: include/tricolour_amd.h).
//
// A sample is valid iff its flag is 0 and both parts are finite; a pair (t, c), c < nchan - 1, is valid iff samples
// (t, c) and (t, c + 1) are.  Six numbers per cell: n, sum_re, sum_im, sum_p (p = re * re + im * im), dn, dsum_p
// (dp = dre * dre + dim * dim of the pair's difference), float64 and integers throughout, no FMA.  Cells: one per window
// (bl), per (corr, t) over baselines and channels (time), per (corr, c) over baselines and times (chan).
//
// Three kernels.
//   k_quality_walk    stage 1, the one pass over the slab.  A wave owns one window and one strip of QUAL_SW channels and
//                     walks every time row, QUAL_ROWS rows per trip (their loads are issued together); a block is
//                     QUAL_NT / 64 adjacent strips, and its waves never meet: no LDS, no barrier.  A lane holds QUAL_V
//                     consecutive channels (VEC: 16-byte loads of the visibilities, the flags as one word) and their
//                     column accumulators in registers for the whole walk.  The pair of a lane's last channel takes the
//                     right neighbour's first sample by a cross-lane move; the last lane re-reads that one sample (the
//                     halo) from memory.  Per row the lanes' partials (channels in ascending order) are summed by the
//                     xor butterfly 1, 2, 4, 8, 16, 32 -- a fixed tree; the counts come from ballots -- and lane 0
//                     writes the strip's row partial.  After the walk every lane writes its column cells.
//   k_quality_window  per window (one block): the strips' row partials summed in ascending strip order give the window's
//                     time contribution; those, each thread taking t = i, i + QUAL_NT, ... in ascending order and the
//                     threads' sums folded by a halving tree, give the window's bl cell.
//   k_quality_fold    time and chan cells: one thread per (number, corr, index) adds the windows' contributions
//                     sequentially in ascending baseline order onto the cell, QUAL_AHEAD loads issued ahead of the adds.
// Every order depends on (ntime, nchan) alone: never on how many windows a call holds nor on where a window sits.  VEC
// changes no result.  No floating-point atomics, no integer atomics either.
#pragma once

#define QUAL_NT 256                     // threads per block, all kernels
#define QUAL_V 4                        // channels per lane
#define QUAL_SW (64 * QUAL_V)           // channels per strip (one wave)
#define QUAL_WPB (QUAL_NT / 64)         // strips per block
#define QUAL_ROWS 2                     // rows per trip of the walk
#define QUAL_AHEAD 8                    // k_quality_fold: loads in flight per thread

// one strip's partial of one time row
struct QualRow {
    double s[4];                        // sum_re, sum_im, sum_p, dsum_p
    int n, dn;
};

// The QUAL_V samples of a lane (channels c0 .. c0 + QUAL_V - 1 of the row that starts at sample `row`): parts and validity.
// VEC: nchan % QUAL_V == 0 and 16-byte (visibilities) / 4-byte (flags) aligned bases, so a lane is whole or absent.
template <int VIS, bool VEC>
__device__ __forceinline__ void qual_load(const void* __restrict__ vis, const uint8_t* __restrict__ flags, int64_t row,
                                          int64_t c0, int64_t nchan, float (&re)[QUAL_V], float (&im)[QUAL_V],
                                          unsigned (&fl)[QUAL_V]) {
#pragma unroll
    for (int k = 0; k < QUAL_V; k++) { re[k] = 0.0f; im[k] = 0.0f; fl[k] = 1u; }
    if (VEC) {
        if (c0 < nchan) {
            const int64_t s = row + c0;
            if (VIS == TRI_VIS_C64) {
                const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float2*>(vis) + s);
                const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float2*>(vis) + s + 2);
                re[0] = a.x; im[0] = a.y; re[1] = a.z; im[1] = a.w;
                re[2] = b.x; im[2] = b.y; re[3] = b.z; im[3] = b.w;
            } else {
                const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(vis) + s);
                re[0] = a.x; re[1] = a.y; re[2] = a.z; re[3] = a.w;
            }
            const unsigned w = *reinterpret_cast<const unsigned*>(flags + s);
            fl[0] = w & 0xFFu; fl[1] = w >> 8 & 0xFFu; fl[2] = w >> 16 & 0xFFu; fl[3] = w >> 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < QUAL_V; k++) {
            if (c0 + k < nchan) {
                const int64_t s = row + c0 + k;
                if (VIS == TRI_VIS_C64) {
                    const float2 z = reinterpret_cast<const float2*>(vis)[s];
                    re[k] = z.x; im[k] = z.y;
                } else {
                    re[k] = reinterpret_cast<const float*>(vis)[s];
                }
                fl[k] = flags[s];
            }
        }
    }
}

// both parts finite: neither exponent field is all ones
__device__ __forceinline__ bool qual_finite(float re, float im) {
    return (__float_as_uint(re) & 0x7F800000u) != 0x7F800000u && (__float_as_uint(im) & 0x7F800000u) != 0x7F800000u;
}

// sum over the wave by the xor butterfly, the same bits in every lane
__device__ __forceinline__ double qual_wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double o = __shfl_xor(v, m, 64);
        v = v + o;
    }
    return v;
}

// grid: n_win * ngroups blocks, ngroups = cdiv(nstrips, QUAL_WPB), nstrips = cdiv(nchan, QUAL_SW).
// rows   (n_win, nstrips, ntime) QualRow
// ccnt   (n_win, 2, nchan) int64: n, dn            csum  (n_win, 4, nchan) float64: sum_re, sum_im, sum_p, dsum_p
template <int VIS, bool VEC>
__global__ void __launch_bounds__(QUAL_NT, 4)       // 4 waves per SIMD: 123 registers, nothing spilt
k_quality_walk(const void* __restrict__ vis, const uint8_t* __restrict__ flags, int64_t ntime, int64_t nchan, int nstrips,
               int ngroups, QualRow* __restrict__ rows, long long* __restrict__ ccnt, double* __restrict__ csum) {
    const int lane = threadIdx.x & 63;
    const int64_t win = (int64_t)blockIdx.x / ngroups;
    const int strip = (int)((int64_t)blockIdx.x % ngroups) * QUAL_WPB + ((int)threadIdx.x >> 6);
    if (strip >= nstrips) return;                               // the whole wave: its strip does not exist
    const int64_t c0 = (int64_t)strip * QUAL_SW + (int64_t)lane * QUAL_V;
    const int64_t ch = (int64_t)(strip + 1) * QUAL_SW;          // the halo channel: the next strip's first
    const bool halo = lane == 63 && ch < nchan;
    const int64_t base = win * ntime * nchan;

    double a_re[QUAL_V], a_im[QUAL_V], a_p[QUAL_V], a_dp[QUAL_V];
    int a_n[QUAL_V], a_dn[QUAL_V];
#pragma unroll
    for (int k = 0; k < QUAL_V; k++) { a_re[k] = 0.0; a_im[k] = 0.0; a_p[k] = 0.0; a_dp[k] = 0.0; a_n[k] = 0; a_dn[k] = 0; }
    QualRow* __restrict__ out = rows + (win * nstrips + strip) * ntime;

    for (int64_t t0 = 0; t0 < ntime; t0 += QUAL_ROWS) {
        float re[QUAL_ROWS][QUAL_V], im[QUAL_ROWS][QUAL_V], hre[QUAL_ROWS], him[QUAL_ROWS];
        unsigned fl[QUAL_ROWS][QUAL_V], hfl[QUAL_ROWS];
        // every load of the trip first
#pragma unroll
        for (int r = 0; r < QUAL_ROWS; r++) {
            const int64_t t = t0 + r < ntime ? t0 + r : ntime - 1;      // a row past the end re-reads the last (and is dropped)
            const int64_t row = base + t * nchan;
            qual_load<VIS, VEC>(vis, flags, row, c0, nchan, re[r], im[r], fl[r]);
            hre[r] = 0.0f; him[r] = 0.0f; hfl[r] = 1u;
            if (halo) {
                if (VIS == TRI_VIS_C64) {
                    const float2 z = reinterpret_cast<const float2*>(vis)[row + ch];
                    hre[r] = z.x; him[r] = z.y;
                } else {
                    hre[r] = reinterpret_cast<const float*>(vis)[row + ch];
                }
                hfl[r] = flags[row + ch];
            }
        }
#pragma unroll
        for (int r = 0; r < QUAL_ROWS; r++) {
            if (t0 + r >= ntime) break;                         // uniform
            bool ok[QUAL_V + 1];
            double dre[QUAL_V + 1], dim[QUAL_V + 1];
#pragma unroll
            for (int k = 0; k < QUAL_V; k++) {
                ok[k] = fl[r][k] == 0u && qual_finite(re[r][k], im[r][k]);
                dre[k] = (double)re[r][k];
                dim[k] = (double)im[r][k];
            }
            // the right neighbour's first sample: lane + 1, or the halo for the last lane
            const unsigned long long ok0 = __ballot(ok[0]);
            const float nre = __shfl_down(re[r][0], 1, 64), nim = __shfl_down(im[r][0], 1, 64);
            if (lane == 63) {
                ok[QUAL_V] = hfl[r] == 0u && qual_finite(hre[r], him[r]);
                dre[QUAL_V] = (double)hre[r];
                dim[QUAL_V] = (double)him[r];
            } else {
                ok[QUAL_V] = (ok0 >> (lane + 1) & 1ull) != 0;
                dre[QUAL_V] = (double)nre;
                dim[QUAL_V] = (double)nim;
            }
            double r_re = 0.0, r_im = 0.0, r_p = 0.0, r_dp = 0.0;
            int r_n = 0, r_dn = 0;
#pragma unroll
            for (int k = 0; k < QUAL_V; k++) {
                const double x = ok[k] ? dre[k] : 0.0, y = ok[k] ? dim[k] : 0.0;
                const double xx = x * x, yy = y * y;
                const double p = xx + yy;
                const bool pair = ok[k] && ok[k + 1];
                const double ex = dre[k + 1] - dre[k], ey = dim[k + 1] - dim[k];
                const double exx = ex * ex, eyy = ey * ey;
                const double q = exx + eyy;
                const double dp = pair ? q : 0.0;
                a_re[k] = a_re[k] + x; a_im[k] = a_im[k] + y; a_p[k] = a_p[k] + p; a_dp[k] = a_dp[k] + dp;
                a_n[k] += ok[k] ? 1 : 0; a_dn[k] += pair ? 1 : 0;
                r_re = r_re + x; r_im = r_im + y; r_p = r_p + p; r_dp = r_dp + dp;
                r_n += __popcll(__ballot(ok[k]));
                r_dn += __popcll(__ballot(pair));
            }
            r_re = qual_wave_sum(r_re);
            r_im = qual_wave_sum(r_im);
            r_p = qual_wave_sum(r_p);
            r_dp = qual_wave_sum(r_dp);
            if (lane == 0) {
                QualRow o;
                o.s[0] = r_re; o.s[1] = r_im; o.s[2] = r_p; o.s[3] = r_dp; o.n = r_n; o.dn = r_dn;
                out[t0 + r] = o;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < QUAL_V; k++) {
        const int64_t c = c0 + k;
        if (c < nchan) {
            ccnt[(win * 2 + 0) * nchan + c] = a_n[k];
            ccnt[(win * 2 + 1) * nchan + c] = a_dn[k];
            csum[(win * 4 + 0) * nchan + c] = a_re[k];
            csum[(win * 4 + 1) * nchan + c] = a_im[k];
            csum[(win * 4 + 2) * nchan + c] = a_p[k];
            csum[(win * 4 + 3) * nchan + c] = a_dp[k];
        }
    }
}

// grid: n_win blocks.  tcnt (n_win, 2, ntime) int64, tsum (n_win, 4, ntime) float64: the windows' time contributions;
// counts_bl (2, n_win) int64 and sums_bl (4, n_win) float64: the bl cells.
__global__ void __launch_bounds__(QUAL_NT)
k_quality_window(const QualRow* __restrict__ rows, int64_t n_win, int64_t ntime, int nstrips, long long* __restrict__ tcnt,
                 double* __restrict__ tsum, long long* __restrict__ counts_bl, double* __restrict__ sums_bl) {
    __shared__ double sh_s[4][QUAL_NT];
    __shared__ long long sh_n[2][QUAL_NT];
    const int64_t win = blockIdx.x;
    const int i = threadIdx.x;
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    long long wn = 0, wdn = 0;
    for (int64_t t = i; t < ntime; t += QUAL_NT) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        long long n = 0, dn = 0;
        for (int k = 0; k < nstrips; k++) {
            const QualRow r = rows[(win * nstrips + k) * ntime + t];
#pragma unroll
            for (int j = 0; j < 4; j++) s[j] = s[j] + r.s[j];
            n += r.n; dn += r.dn;
        }
        tcnt[(win * 2 + 0) * ntime + t] = n;
        tcnt[(win * 2 + 1) * ntime + t] = dn;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            tsum[(win * 4 + j) * ntime + t] = s[j];
            w[j] = w[j] + s[j];
        }
        wn += n; wdn += dn;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) sh_s[j][i] = w[j];
    sh_n[0][i] = wn; sh_n[1][i] = wdn;
    __syncthreads();
    for (int h = QUAL_NT / 2; h > 0; h >>= 1) {
        if (i < h) {
#pragma unroll
            for (int j = 0; j < 4; j++) sh_s[j][i] = sh_s[j][i] + sh_s[j][i + h];
            sh_n[0][i] += sh_n[0][i + h];
            sh_n[1][i] += sh_n[1][i + h];
        }
        __syncthreads();
    }
    if (i == 0) {
        counts_bl[0 * n_win + win] = sh_n[0][0];
        counts_bl[1 * n_win + win] = sh_n[1][0];
#pragma unroll
        for (int j = 0; j < 4; j++) sums_bl[j * n_win + win] = sh_s[j][0];
    }
}

// acc = acc + in[b] for b = 0 .. n_bl - 1 in this order; QUAL_AHEAD values are loaded before their adds
template <class T>
__device__ __forceinline__ T qual_fold(const T* __restrict__ in, int64_t stride, int64_t n_bl, T acc) {
    int64_t b = 0;
    for (; b + QUAL_AHEAD <= n_bl; b += QUAL_AHEAD) {
        T v[QUAL_AHEAD];
#pragma unroll
        for (int u = 0; u < QUAL_AHEAD; u++) v[u] = in[(b + u) * stride];
#pragma unroll
        for (int u = 0; u < QUAL_AHEAD; u++) acc = acc + v[u];
    }
    for (; b < n_bl; b++) acc = acc + in[b * stride];
    return acc;
}

// grid: cdiv(6 * ncorr * len, QUAL_NT) blocks.  cnt (n_bl * ncorr, 2, len) int64 and sum (n_bl * ncorr, 4, len) float64:
// the windows' contributions; counts (2, ncorr * len) and sums (4, ncorr * len): the cells, continued when accumulate != 0.
__global__ void __launch_bounds__(QUAL_NT)
k_quality_fold(const long long* __restrict__ cnt, const double* __restrict__ sum, int64_t n_bl, int64_t ncorr, int64_t len,
               long long* __restrict__ counts, double* __restrict__ sums, int accumulate) {
    const int64_t cells = ncorr * len;
    const int64_t j = (int64_t)blockIdx.x * QUAL_NT + threadIdx.x;
    if (j >= 6 * cells) return;
    const int64_t k = j / cells, cell = j % cells;
    const int64_t corr = cell / len, i = cell % len;
    if (k < 2) {
        const long long* in = cnt + (corr * 2 + k) * len + i;
        long long* o = counts + k * cells + cell;
        *o = qual_fold<long long>(in, ncorr * 2 * len, n_bl, accumulate ? *o : 0ll);
    } else {
        const double* in = sum + (corr * 4 + (k - 2)) * len + i;
        double* o = sums + (k - 2) * cells + cell;
        *o = qual_fold<double>(in, ncorr * 4 * len, n_bl, accumulate ? *o : 0.0);
    }
}
