// kernels_hyst.hpp -- value-driven hysteresis growth of the flags of (time, chan) windows (the model is the watershed
// of HERA's xrfi; the definition is this project's own, include/tricolour_amd.h).
//
// Per window, visibilities v, running flags f and a mask `missing`:
//   a        = the flagger's amplitude (tri_hypotf / fabsf); a sample counts iff f == 0 and a is not NaN
//   levels   = per line -- time axis: (window, channel); frequency axis: (window, time row, frequency chunk) -- over the
//              m counting samples with finite a: med = their median (even m: float32(x + y) / 2), dev = fabsf(a - med),
//              mad = the median of dev; the line is live iff m >= 3, med and mad are finite and mad > 0
//   e_axis   = counts && (a == +inf || (live && (double)a > (double)med + scale_axis * (double)mad)), float64, no FMA;
//              scale = nsigma * 1.4826 (the host's product); scale == 0: the axis is off
//   G_0      = (f != 0) & ~missing
//   G_{k+1}  = G_k | (e_time & (G_k[t - 1] | G_k[t + 1])) | (e_freq & (G_k[c - 1] | G_k[c + 1])), `reach` rounds, 0 outside
//   out      = (f != 0) | G_reach
//
// Four kernels, all of HYST_NT threads.
//   k_hyst_level     med and mad of every line (NaN, NaN for a line that is not live) by two exact 8-bit radix selects
//                    over the bit patterns of non-negative float32 (4 counting passes and one for the upper middle of
//                    an even count, each), integer LDS atomics only.  <VIS, 0>: HYST_LC adjacent channels of one window
//                    per block, 32 threads per channel; <VIS, 1>: one wave per (row, chunk), HYST_LW lines per block.
//                    A line of at most HYST_LN samples is read from memory once and its keys stay in LDS for all ten
//                    passes (the deviations replace the amplitudes in place); a longer line is re-read for every pass.
//   k_hyst_eligible  one pass over vis and flags: the three bit planes G_0, e_time, e_freq (words of 32 channels, rows
//                    padded to whole words, bits at channels >= nchan are 0) by the wave-wide ballot, and / or the two
//                    eligibility images as bytes.
//   k_hyst_pack      three byte images into the three bit planes (the entry of tri_hyst_grow).
//   k_hyst_grow      all `reach` rounds in one launch.  A block owns HYST_GR rows x HYST_GW words; it stages them with
//                    `reach` rows above and below and one word on either side (32 bits >= reach), keeps e_time, e_freq
//                    and G in registers and G also in two LDS tiles that alternate, and runs the rounds on the whole
//                    staged tile: a cell at distance d from the tile's rim is exact for d rounds, so after `reach`
//                    rounds the core is.  Cells outside the window are zeros, never the next window's rows.  Then
//                    out = f | G_reach for the core, 16 flags per lane (VEC: nchan % 16 == 0 and 16-byte aligned
//                    bases) or one word's 32 bytes one by one.
// Neither the LDS route of the levels nor VEC changes a result: the same bits on every route, for every batch size and
// on every run.
#pragma once

#include "../ldev/kernels_ldev.hpp"    // ldev_pick: a wave's pick of the bin of a 256-bin histogram

#define HYST_NT 256                 // threads per block, all kernels
#define HYST_LC 8                   // k_hyst_level<, 0>: channels per block
#define HYST_LW 4                   // k_hyst_level<, 1>: lines per block
#ifndef HYST_LN
#define HYST_LN 1024                // longest line whose keys stay in LDS (-DHYST_LN=1: every line is re-read, the A/B build)
#endif
#define HYST_ER 8                   // k_hyst_eligible / k_hyst_pack: rows per block
#define HYST_GR 64                  // k_hyst_grow: core rows per tile
#define HYST_GW 16                  //              core words per tile
#define HYST_MAXREACH 32
#define HYST_TW (HYST_GW + 2)                                   // staged words per row
#define HYST_TR (HYST_GR + 2 * HYST_MAXREACH)                   // most staged rows
#define HYST_CPT ((HYST_TR * HYST_TW + HYST_NT - 1) / HYST_NT)  // staged cells per thread
#define HYST_NOKEY 0xFFFFFFFFu      // a sample that enters no level

// Key of sample s for the levels: the bit pattern of its amplitude if it counts and the amplitude is finite.
template <int VIS>
__device__ __forceinline__ unsigned hyst_key(const void* __restrict__ vis, const uint8_t* __restrict__ flags, int64_t s) {
    if (flags[s] != 0) return HYST_NOKEY;
    const unsigned k = __float_as_uint(load_amp<VIS>(vis, (size_t)s));
    return k < 0x7F800000u ? k : HYST_NOKEY;        // amplitudes carry no sign: +inf and NaN lie at and above 0x7F800000
}

// Median of the keys below 0x7F800000 of every line of the block (key_at(i), i in [0, len), of the calling thread's
// line; a thread only asks for i = sub + j * G), m of them; the whole block calls it.  NaN when m == 0.
// WAVE: a wave is one line, so lanes with the same digit add as one.
template <int NL, int G, bool WAVE, class KeyAt>
__device__ __forceinline__ float hyst_median(KeyAt key_at, int len, int line, int sub, unsigned (*hist)[257],
                                             unsigned* s_prefix, unsigned* s_k, unsigned* s_m, unsigned* s_le,
                                             unsigned* s_nxt, unsigned& m) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (threadIdx.x < NL) { s_prefix[threadIdx.x] = 0; s_k[threadIdx.x] = 0; s_m[threadIdx.x] = 0; s_le[threadIdx.x] = 0; s_nxt[threadIdx.x] = 0xFFFFFFFFu; }
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < NL * 257; i += HYST_NT) (&hist[0][0])[i] = 0;
        __syncthreads();
        const unsigned prefix = s_prefix[line];
        const unsigned mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int i0 = 0; i0 < len; i0 += G) {
            const int i = i0 + sub;
            const unsigned key = i < len ? key_at(i) : HYST_NOKEY;
            const bool in = key < 0x7F800000u && (key & mask) == prefix;
            const int b = in ? (int)(key >> shift & 255u) : -1;
            if (WAVE) {
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
        for (int l = wave; l < NL; l += HYST_NT / 64) {
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
    const unsigned lo = s_prefix[line];
    m = s_m[line];
    {
        unsigned le = 0, nxt = 0xFFFFFFFFu;
        for (int i = sub; i < len; i += G) {
            const unsigned key = key_at(i);
            if (key >= 0x7F800000u) continue;
            if (key <= lo) le++;
            else nxt = key < nxt ? key : nxt;
        }
        if (le) atomicAdd(&s_le[line], le);
        if (nxt != 0xFFFFFFFFu) atomicMin(&s_nxt[line], nxt);
    }
    __syncthreads();
    if (m == 0) return __uint_as_float(0x7FC00000u);
    float med = __uint_as_float(lo);
    if (!(m & 1u)) {
        const unsigned hi = s_le[line] >= m / 2 + 1 ? lo : s_nxt[line];
        const float sum = __uint_as_float(lo) + __uint_as_float(hi);
        med = sum / 2.0f;
    }
    return med;
}

// VIS: TRI_VIS_C64 or TRI_VIS_F32.
// AXIS 0: lines are (window, channel), HYST_LC adjacent channels per block; grid n_win * cdiv(nchan, HYST_LC);
//         med / mad (n_win, nchan).
// AXIS 1: lines are (window, row, chunk), chunk k = channels [ends[k], ends[k + 1]), one wave per line;
//         grid cdiv(n_win * ntime * nchunk, HYST_LW); med / mad (n_win, ntime, nchunk).
template <int VIS, int AXIS>
__global__ void __launch_bounds__(HYST_NT)
k_hyst_level(const void* __restrict__ vis, const uint8_t* __restrict__ flags, int64_t n_win, int64_t ntime, int64_t nchan,
             const int64_t* __restrict__ ends, int nchunk, float* __restrict__ med_out, float* __restrict__ mad_out) {
    constexpr int NL = AXIS == 0 ? HYST_LC : HYST_LW;       // lines per block
    constexpr int G = HYST_NT / NL;                         // threads per line
    __shared__ unsigned keys[NL * HYST_LN];
    __shared__ unsigned hist[NL][257];                      // 257: a line's bins start on another bank
    __shared__ unsigned s_prefix[NL], s_k[NL], s_m[NL], s_le[NL], s_nxt[NL];
    const int line = AXIS == 0 ? (int)threadIdx.x % NL : (int)threadIdx.x / G;
    const int sub = AXIS == 0 ? (int)threadIdx.x / NL : (int)threadIdx.x % G;

    int64_t base = 0, stride = 1, oi = -1;
    int len = 0;
    if (AXIS == 0) {
        const int64_t nstrip = (nchan + NL - 1) / NL;
        const int64_t win = (int64_t)blockIdx.x / nstrip;
        const int64_t c = ((int64_t)blockIdx.x % nstrip) * NL + line;
        if (c < nchan) { base = win * ntime * nchan + c; stride = nchan; len = (int)ntime; oi = win * nchan + c; }
    } else {
        const int64_t l = (int64_t)blockIdx.x * NL + line;
        if (l < n_win * ntime * nchunk) {
            const int64_t row = l / nchunk;
            const int k = (int)(l % nchunk);
            base = row * nchan + ends[k];
            len = (int)(ends[k + 1] - ends[k]);
            oi = l;
        }
    }
    const bool staged = len <= HYST_LN;
    // the thread's own slots of the LDS copy: no other thread reads or writes them
    auto slot = [&](int i) -> unsigned& { return keys[AXIS == 0 ? i * NL + line : line * HYST_LN + i]; };
    if (staged)
        for (int i = sub; i < len; i += G) slot(i) = hyst_key<VIS>(vis, flags, base + i * stride);

    unsigned m = 0;
    const float med = hyst_median<NL, G, AXIS == 1>(
        [&](int i) { return staged ? slot(i) : hyst_key<VIS>(vis, flags, base + i * stride); },
        len, line, sub, hist, s_prefix, s_k, s_m, s_le, s_nxt, m);
    const bool alive = m >= 3 && __float_as_uint(med) < 0x7F800000u;

    // dev = fabsf(a - med): finite and >= +0, since a and med are
    auto dev_key = [&](unsigned key) {
        return key < 0x7F800000u && alive ? __float_as_uint(fabsf(__uint_as_float(key) - med)) : HYST_NOKEY;
    };
    if (staged)
        for (int i = sub; i < len; i += G) slot(i) = dev_key(slot(i));
    unsigned m2 = 0;
    const float mad = hyst_median<NL, G, AXIS == 1>(
        [&](int i) { return staged ? slot(i) : dev_key(hyst_key<VIS>(vis, flags, base + i * stride)); },
        len, line, sub, hist, s_prefix, s_k, s_m, s_le, s_nxt, m2);
    const bool live = alive && __float_as_uint(mad) < 0x7F800000u && mad > 0.0f;
    if (sub == 0 && oi >= 0) {
        const float nan = __uint_as_float(0x7FC00000u);
        med_out[oi] = live ? med : nan;
        mad_out[oi] = live ? mad : nan;
    }
}

// The two words of the wave's 64 channels (channel of lane 0 a multiple of 64) into row `row` of a bit plane.
__device__ __forceinline__ void hyst_put(unsigned* __restrict__ plane, int64_t row, int64_t c_wave, int nw, bool bit) {
    const unsigned long long b = __ballot(bit);
    const int lane = threadIdx.x & 63;
    if (plane && (lane == 0 || lane == 32)) {
        const int64_t w = c_wave / 32 + (lane >> 5);
        if (w < nw) plane[row * nw + w] = lane == 0 ? (unsigned)b : (unsigned)(b >> 32);
    }
}

// grid: n_win * ntiles * nstrip blocks of HYST_ER rows x HYST_NT channels.  scale_t / scale_f: nsigma * 1.4826, 0 = off
// (its levels are then not read).  missing and each output may be null; levels of a line that is not live are NaN.
template <int VIS>
__global__ void __launch_bounds__(HYST_NT)
k_hyst_eligible(const void* __restrict__ vis, const uint8_t* __restrict__ flags, const uint8_t* __restrict__ missing,
                int64_t ntime, int64_t nchan, int nstrip, int ntiles, const int64_t* __restrict__ ends, int nchunk,
                double scale_t, double scale_f, const float* __restrict__ med_t, const float* __restrict__ mad_t,
                const float* __restrict__ med_f, const float* __restrict__ mad_f, int nw, unsigned* __restrict__ p_seed,
                unsigned* __restrict__ p_et, unsigned* __restrict__ p_ef, uint8_t* __restrict__ b_et,
                uint8_t* __restrict__ b_ef) {
    const int64_t blk = blockIdx.x;
    const int strip = (int)(blk % nstrip);
    const int tile = (int)(blk / nstrip % ntiles);
    const int64_t win = blk / nstrip / ntiles;
    const int64_t c = (int64_t)strip * HYST_NT + threadIdx.x;
    const int64_t c_wave = c - (threadIdx.x & 63);
    const int64_t t0 = (int64_t)tile * HYST_ER;
    const int nrows = (int)min((int64_t)HYST_ER, ntime - t0);
    const bool in = c < nchan;
    const bool on_t = scale_t > 0.0, on_f = scale_f > 0.0;

    bool live_t = false;
    double thr_t = 0.0;
    if (in && on_t) {
        const float med = med_t[win * nchan + c], mad = mad_t[win * nchan + c];
        live_t = med == med;
        const double spread = scale_t * (double)mad;
        thr_t = (double)med + spread;
    }
    int k = 0;                                      // the chunk of channel c: the last k with ends[k] <= c
    if (in && on_f) {
        int hi = nchunk;                            // ends[hi] = nchan > c
        while (hi - k > 1) {
            const int mid = (k + hi) >> 1;
            if (ends[mid] <= c) k = mid; else hi = mid;
        }
    }
    for (int r = 0; r < nrows; r++) {
        const int64_t row = win * ntime + t0 + r;
        const int64_t s = row * nchan + c;
        bool seed = false, et = false, ef = false;
        if (in) {
            const unsigned f = flags[s];
            const float a = load_amp<VIS>(vis, (size_t)s);
            const bool counts = f == 0 && a == a;
            seed = f != 0 && !(missing && missing[s] != 0);
            et = counts && on_t && (a == INFINITY || (live_t && (double)a > thr_t));
            if (counts && on_f) {
                const float med = med_f[row * nchunk + k], mad = mad_f[row * nchunk + k];
                const double spread = scale_f * (double)mad;
                const double thr = (double)med + spread;
                ef = a == INFINITY || (med == med && (double)a > thr);
            }
            if (b_et) b_et[s] = et ? 1 : 0;
            if (b_ef) b_ef[s] = ef ? 1 : 0;
        }
        hyst_put(p_seed, row, c_wave, nw, seed);
        hyst_put(p_et, row, c_wave, nw, et);
        hyst_put(p_ef, row, c_wave, nw, ef);
    }
}

// Three byte images (nonzero = set) into the three bit planes; the grid of k_hyst_eligible.
__global__ void __launch_bounds__(HYST_NT)
k_hyst_pack(const uint8_t* __restrict__ seeds, const uint8_t* __restrict__ e_time, const uint8_t* __restrict__ e_freq,
            int64_t ntime, int64_t nchan, int nstrip, int ntiles, int nw, unsigned* __restrict__ p_seed,
            unsigned* __restrict__ p_et, unsigned* __restrict__ p_ef) {
    const int64_t blk = blockIdx.x;
    const int strip = (int)(blk % nstrip);
    const int tile = (int)(blk / nstrip % ntiles);
    const int64_t win = blk / nstrip / ntiles;
    const int64_t c = (int64_t)strip * HYST_NT + threadIdx.x;
    const int64_t c_wave = c - (threadIdx.x & 63);
    const int64_t t0 = (int64_t)tile * HYST_ER;
    const int nrows = (int)min((int64_t)HYST_ER, ntime - t0);
    const bool in = c < nchan;
    for (int r = 0; r < nrows; r++) {
        const int64_t row = win * ntime + t0 + r;
        const int64_t s = row * nchan + c;
        hyst_put(p_seed, row, c_wave, nw, in && seeds[s] != 0);
        hyst_put(p_et, row, c_wave, nw, in && e_time[s] != 0);
        hyst_put(p_ef, row, c_wave, nw, in && e_freq[s] != 0);
    }
}

// 4 bits into 4 bytes of 0 / 1, lowest bit in the lowest byte
__device__ __forceinline__ unsigned hyst_spread4(unsigned nib) { return ((nib & 15u) * 0x00204081u) & 0x01010101u; }
// 4 bytes into 0 / 1 each: nonzero -> 1
__device__ __forceinline__ unsigned hyst_one4(unsigned w) { return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) >> 7 & 0x01010101u; }

// grid: n_win * ntr * ntw blocks, ntr = cdiv(ntime, HYST_GR), ntw = cdiv(nw, HYST_GW); reach in [1, HYST_MAXREACH].
// out = (base != 0) | G_reach, bytes (n_win, ntime, nchan).
template <bool VEC>
__global__ void __launch_bounds__(HYST_NT)
k_hyst_grow(const unsigned* __restrict__ p_seed, const unsigned* __restrict__ p_et, const unsigned* __restrict__ p_ef,
            const uint8_t* __restrict__ base, uint8_t* __restrict__ out, int64_t ntime, int64_t nchan, int nw, int ntr,
            int ntw, int reach) {
    __shared__ unsigned tile[2][HYST_TR * HYST_TW];
    const int64_t blk = blockIdx.x;
    const int wt = (int)(blk % ntw);
    const int rt = (int)(blk / ntw % ntr);
    const int64_t win = blk / ntw / ntr;
    const int rows = HYST_GR + 2 * reach;           // staged rows: row r is time rt * HYST_GR - reach + r
    const int cells = rows * HYST_TW;               // word j of a row is word wt * HYST_GW - 1 + j
    const int64_t t_first = (int64_t)rt * HYST_GR - reach;
    const int64_t w_first = (int64_t)wt * HYST_GW - 1;

    unsigned g[HYST_CPT], et[HYST_CPT], ef[HYST_CPT];
#pragma unroll
    for (int k = 0; k < HYST_CPT; k++) {
        const int i = (int)threadIdx.x + k * HYST_NT;
        g[k] = 0; et[k] = 0; ef[k] = 0;
        if (i < cells) {
            const int64_t t = t_first + i / HYST_TW, w = w_first + i % HYST_TW;
            if (t >= 0 && t < ntime && w >= 0 && w < nw) {
                const int64_t at = (win * ntime + t) * nw + w;
                g[k] = p_seed[at]; et[k] = p_et[at]; ef[k] = p_ef[at];
            }
            tile[0][i] = g[k];
        }
    }
    __syncthreads();
    for (int round = 0; round < reach; round++) {
        const unsigned* src = tile[round & 1];
        unsigned* dst = tile[(round & 1) ^ 1];
#pragma unroll
        for (int k = 0; k < HYST_CPT; k++) {
            const int i = (int)threadIdx.x + k * HYST_NT;
            if (i < cells) {
                const int r = i / HYST_TW, j = i % HYST_TW;
                const unsigned up = r > 0 ? src[i - HYST_TW] : 0u;
                const unsigned dn = r + 1 < rows ? src[i + HYST_TW] : 0u;
                const unsigned lf = j > 0 ? src[i - 1] : 0u;
                const unsigned rg = j + 1 < HYST_TW ? src[i + 1] : 0u;
                const unsigned cur = g[k];
                // bit b of a word is channel 32 * w + b: channel c - 1 arrives by a shift up, with the carry of the word before
                const unsigned side = (cur << 1) | (lf >> 31) | (cur >> 1) | (rg << 31);
                g[k] = cur | (et[k] & (up | dn)) | (ef[k] & side);
                dst[i] = g[k];
            }
        }
        __syncthreads();
    }
    const unsigned* fin = tile[reach & 1];
    if (VEC) {
        // 16 channels per lane: one half of a word, 16 bytes
        for (int q = threadIdx.x; q < HYST_GR * HYST_GW * 2; q += HYST_NT) {
            const int r = q / (HYST_GW * 2), h = q % (HYST_GW * 2);
            const int64_t t = (int64_t)rt * HYST_GR + r;
            const int64_t w = (int64_t)wt * HYST_GW + h / 2;
            if (t >= ntime || w >= nw) continue;
            const int64_t c = w * 32 + (h & 1) * 16;
            if (c >= nchan) continue;               // nchan % 16 == 0: the half is whole or absent
            const unsigned bits = fin[(r + reach) * HYST_TW + h / 2 + 1] >> ((h & 1) * 16);
            const int64_t s = (win * ntime + t) * nchan + c;
            const uint4 f = *reinterpret_cast<const uint4*>(base + s);
            *reinterpret_cast<uint4*>(out + s) =
                make_uint4(hyst_one4(f.x) | hyst_spread4(bits), hyst_one4(f.y) | hyst_spread4(bits >> 4),
                           hyst_one4(f.z) | hyst_spread4(bits >> 8), hyst_one4(f.w) | hyst_spread4(bits >> 12));
        }
    } else {
        for (int q = threadIdx.x; q < HYST_GR * HYST_GW; q += HYST_NT) {
            const int r = q / HYST_GW, j = q % HYST_GW;
            const int64_t t = (int64_t)rt * HYST_GR + r;
            const int64_t w = (int64_t)wt * HYST_GW + j;
            if (t >= ntime || w >= nw) continue;
            const unsigned bits = fin[(r + reach) * HYST_TW + j + 1];
            const int64_t s = (win * ntime + t) * nchan + w * 32;
            const int nb = (int)min((int64_t)32, nchan - w * 32);
            for (int b = 0; b < nb; b++) out[s + b] = (base[s + b] ? 1u : 0u) | (bits >> b & 1u);
        }
    }
}
