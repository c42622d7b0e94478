// kernels_hist.hpp -- log-binned amplitude histograms of the kept and of the flagged samples of (bl, corr, time, chan)
// windows, after the "log N - log S" histogram AOFlagger keeps beside its quality statistics (the definition is this
// project's own: include/tricolour_amd.h).
//
// Every sample is counted exactly once, in one population (0 = kept: its flag is 0; 1 = flagged) and one slot.  Bins are
// three integers: emin, emax (-126 <= emin < emax <= 128) and sub_bits (0 .. 5); nb = (emax - emin) << sub_bits bins, at
// most TRI_MAX_HIST_BINS, and nb + 3 slots: 0 underflow (zero included), 1 .. nb the bins, nb + 1 overflow, nb + 2
// non-finite.  The slot of a sample:
//   1. either part NaN or +-Inf (qual_finite's rule; a float32 input has one part): slot nb + 2;
//   2. otherwise a = tri_hypotf(re, im) = (float)sqrt((double)re * re + (double)im * im) for complex64, |x| for float32;
//   3. u = the bit pattern of a, k = (u >> (23 - sub_bits)) - ((emin + 127) << sub_bits);
//   4. k < 0: slot 0; k >= nb: slot nb + 1 (finite parts whose amplitude rounds to +Inf land here); else slot k + 1.
// No logarithm, no floating-point comparison.  Bin k covers [2^(emin + (k >> s)) * (1 + (k mod 2^s) / 2^s), next edge),
// s = sub_bits.
//
// One kernel, k_hist_fill<VIS, VEC>.  A block owns one window, one span of at most HIST_SPAN channels of one frequency
// chunk and one band of at most HIST_ROWS time rows -- at most HIST_SPAN * HIST_ROWS samples, so its 32-bit counters
// cannot wrap.  Its threads walk the region flat, (row, item) = (i / items, i % items): VEC (nchan % HIST_V == 0 and
// 16-byte / 4-byte aligned bases) takes the span's aligned interior HIST_V channels at a time, 16-byte loads of the
// visibilities and the flags as one word, and the unaligned edges of the span (chunk ends such as 409 and 819) one sample
// at a time; without VEC every sample takes the scalar path.  Each sample is one LDS atomic add into the block's private
// histogram of 2 * (nb + 3) 32-bit counters (16 KB at most).  At the end the block's non-zero counters are added to the
// window's hist_bl cell and to the (corr, chunk) hist_chunk cell with 64-bit integer atomic adds.  Integer adds commute:
// the counts do not depend on arrival order, on the number of windows of a call or on where a window sits.  VEC changes
// no result.  No floating-point atomics.
//
// Launch geometry: grid (n_win * nbands, chunks of this launch, spans), nbands = cdiv(ntime, HIST_ROWS); the host passes
// the ends of up to HIST_CPL chunks per launch by value (the call takes no workspace) and skips launches whose chunks
// are all empty.  Limits (TRI_EUNSUPPORTED beyond them): n_win * nbands <= HIST_MAX_GRID_X (the threads of a launch
// along x stay below 2^32), a chunk of at most 65535 * HIST_SPAN channels, at most 2^30 chunk ends.
#pragma once

#include "../quality/kernels_quality.hpp"       // qual_finite

#define HIST_NT 256                             // threads per block
#define HIST_V 4                                // channels per wide load
#define HIST_SPAN (HIST_NT * HIST_V)            // channels of one chunk a block covers
#define HIST_ROWS 64                            // time rows per band
#define HIST_CPL 64                             // chunks per launch
#define HIST_MAX_GRID_X ((1 << 24) - 1)         // blocks along x

// the chunks of one launch: channels [lo, hi) of chunk idx
struct HistChunks {
    int lo[HIST_CPL], hi[HIST_CPL], idx[HIST_CPL];
};

// one sample into the block's histogram h[2][slots]
template <int VIS>
__device__ __forceinline__ void hist_count(unsigned* __restrict__ h, float re, float im, unsigned fl, int ebase, int shift,
                                           int nb) {
    int slot = nb + 2;
    if (qual_finite(re, im)) {
        const float a = VIS == TRI_VIS_C64 ? tri_hypotf(re, im) : fabsf(re);
        const int k = (int)(__float_as_uint(a) >> shift) - ebase;
        slot = k < 0 ? 0 : (k >= nb ? nb + 1 : k + 1);
    }
    atomicAdd(&h[(fl ? nb + 3 : 0) + slot], 1u);
}

// grid: (n_win * nbands, chunks of this launch, spans of the widest of them); dynamic LDS: 2 * (nb + 3) counters.
// hist_bl    (n_win, 2, nb + 3) int64          hist_chunk  (n_corr, nchunks, 2, nb + 3) int64
// ebase = (emin + 127) << sub_bits, shift = 23 - sub_bits
template <int VIS, bool VEC>
__global__ void __launch_bounds__(HIST_NT)
k_hist_fill(const void* __restrict__ vis, const uint8_t* __restrict__ flags, int64_t ntime, int64_t nchan, int n_corr,
            int nbands, int64_t nchunks, HistChunks ch, int ebase, int shift, int nb,
            unsigned long long* __restrict__ hist_bl, unsigned long long* __restrict__ hist_chunk) {
    extern __shared__ unsigned hist_lds[];
    const int g = blockIdx.y;
    const int64_t lo = (int64_t)ch.lo[g] + (int64_t)blockIdx.z * HIST_SPAN;
    if (lo >= ch.hi[g]) return;                                 // the whole block: this chunk has no such span
    const int64_t hi = lo + HIST_SPAN < ch.hi[g] ? lo + HIST_SPAN : (int64_t)ch.hi[g];
    const int64_t win = (int64_t)blockIdx.x / nbands;
    const int64_t t0 = ((int64_t)blockIdx.x % nbands) * HIST_ROWS;
    const unsigned rows = (unsigned)(ntime - t0 < HIST_ROWS ? ntime - t0 : HIST_ROWS);
    const int cells = 2 * (nb + 3);
    for (int i = threadIdx.x; i < cells; i += HIST_NT) hist_lds[i] = 0u;
    __syncthreads();

    const int64_t base = (win * ntime + t0) * nchan;
    // the aligned interior [alo, ahi) in steps of HIST_V; the rest of [lo, hi) one sample at a time
    int64_t alo = hi, ahi = hi;
    if (VEC) {
        alo = (lo + HIST_V - 1) / HIST_V * HIST_V;
        ahi = hi / HIST_V * HIST_V;
        if (ahi <= alo) { alo = hi; ahi = hi; }
    }
    if (VEC) {
        const unsigned nvec = (unsigned)((ahi - alo) / HIST_V), total = rows * nvec;
#pragma unroll 2
        for (unsigned i = threadIdx.x; i < total; i += HIST_NT) {
            const unsigned r = i / nvec, v = i - r * nvec;
            const int64_t s = base + (int64_t)r * nchan + alo + (int64_t)v * HIST_V;
            const unsigned w = *reinterpret_cast<const unsigned*>(flags + s);
            if (VIS == TRI_VIS_C64) {
                const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float2*>(vis) + s);
                const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float2*>(vis) + s + 2);
                hist_count<VIS>(hist_lds, a.x, a.y, w & 0xFFu, ebase, shift, nb);
                hist_count<VIS>(hist_lds, a.z, a.w, w >> 8 & 0xFFu, ebase, shift, nb);
                hist_count<VIS>(hist_lds, b.x, b.y, w >> 16 & 0xFFu, ebase, shift, nb);
                hist_count<VIS>(hist_lds, b.z, b.w, w >> 24, ebase, shift, nb);
            } else {
                const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(vis) + s);
                hist_count<VIS>(hist_lds, a.x, 0.0f, w & 0xFFu, ebase, shift, nb);
                hist_count<VIS>(hist_lds, a.y, 0.0f, w >> 8 & 0xFFu, ebase, shift, nb);
                hist_count<VIS>(hist_lds, a.z, 0.0f, w >> 16 & 0xFFu, ebase, shift, nb);
                hist_count<VIS>(hist_lds, a.w, 0.0f, w >> 24, ebase, shift, nb);
            }
        }
    }
    {
        const unsigned nleft = (unsigned)(alo - lo), nedge = nleft + (unsigned)(hi - ahi), total = rows * nedge;
        for (unsigned i = threadIdx.x; i < total; i += HIST_NT) {
            const unsigned r = i / nedge, e = i - r * nedge;
            const int64_t c = e < nleft ? lo + e : ahi + (e - nleft);
            const int64_t s = base + (int64_t)r * nchan + c;
            float re, im = 0.0f;
            if (VIS == TRI_VIS_C64) {
                const float2 z = reinterpret_cast<const float2*>(vis)[s];
                re = z.x; im = z.y;
            } else {
                re = reinterpret_cast<const float*>(vis)[s];
            }
            hist_count<VIS>(hist_lds, re, im, flags[s], ebase, shift, nb);
        }
    }
    __syncthreads();

    unsigned long long* __restrict__ ob = hist_bl + win * cells;
    unsigned long long* __restrict__ oc = hist_chunk + ((win % n_corr) * nchunks + ch.idx[g]) * cells;
    for (int i = threadIdx.x; i < cells; i += HIST_NT) {
        const unsigned c = hist_lds[i];
        if (c) {
            atomicAdd(ob + i, (unsigned long long)c);
            atomicAdd(oc + i, (unsigned long long)c);
        }
    }
}
