// kernels_blint.hpp -- baseline integration: the amplitudes of all baselines averaged into one (corr, time, chan)
// image, which the ordinary flagger then flags, and the detections given back to every baseline (the model is
// AOFlagger's baseline integration; the definition is this project's own, include/tricolour_amd.h).
//
// vis (nbl, n) complex64 or float32 amplitudes, flags (nbl, n) uint8, select[nbl] or null; n = ncorr * ntime * nchan:
//   a        = tri_hypotf(re, im)   (float32 amplitudes: fabsf(v));  a sample counts if its baseline is selected, its
//              flag is 0 and a is not NaN
//   sum[i]  += (double)a, count[i] += 1 for b = 0 .. nbl - 1 in that order over the counting samples
//   flag[i]  = count[i] < min_count;  amp[i] = flag[i] ? 0 : (float)(sum[i] / (double)count[i])
//   out[b,i] = (flags[b,i] != 0) | line[i]
//
// Three kernels, no LDS, no cross-lane work, no atomics.
//   k_bli_accumulate  the only pass over the visibilities (8 B + 1 B per sample; 4 B + 1 B for amplitudes).  One
//                     thread owns VEC consecutive positions and walks the baselines in memory order, so the float64
//                     sum of a position has one order whatever the grid, the batch or the split of the baselines over
//                     calls.  The loads of BLI_UNROLL baselines are issued together and consumed strictly in baseline
//                     order.  Parallelism is over n alone: a short image with many baselines under-fills the device.
//   k_bli_finish      count -> flag, sum / count -> amplitude; one pass over n.
//   k_bli_apply       out = flags | line, 16 flags per thread (VEC16) or one.
#pragma once

#define BLI_NT 256      // threads per block, all three kernels
#define BLI_UNROLL 4    // baselines whose loads are in flight together

// VEC positions of one baseline: parts (im only for complex64) and the flag bytes, byte j = flag of position j.
template <int VD, int VEC>
struct BliSamples {
    float re[VEC], im[VEC];
    unsigned fl;
};

// vp / fp: the thread's first position in this baseline.  VEC == 4: n % 4 == 0 and the bases are 16-byte (flags:
// 4-byte) aligned, so every baseline's piece is.
template <int VD, int VEC>
__device__ __forceinline__ void bli_load(const float* vp, const uint8_t* fp, BliSamples<VD, VEC>& s) {
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

// one baseline's samples into the accumulators, position by position
template <int VD, int VEC>
__device__ __forceinline__ void bli_add(const BliSamples<VD, VEC>& s, double (&sum)[VEC], int (&cnt)[VEC]) {
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        const float a = VD == TRI_VIS_C64 ? tri_hypotf(s.re[j], s.im[j]) : fabsf(s.re[j]);
        const bool counts = ((s.fl >> (8 * j)) & 0xFFu) == 0 && a == a;
        sum[j] = counts ? sum[j] + (double)a : sum[j];
        cnt[j] += counts ? 1 : 0;
    }
}

// VD: TRI_VIS_C64 or TRI_VIS_F32.  npiece = n / VEC threads.  select: one byte per baseline (nonzero: takes part) or
// null; the branches on it are the same in every lane.
template <int VD, int VEC>
__global__ void __launch_bounds__(BLI_NT)
k_bli_accumulate(const void* __restrict__ vis_, const uint8_t* __restrict__ flags, const uint8_t* __restrict__ select,
                 int64_t nbl, int64_t n, int64_t npiece, double* __restrict__ sum_, int* __restrict__ count_) {
    constexpr int W = VD == TRI_VIS_C64 ? 2 : 1;          // floats per sample
    const int64_t piece = (int64_t)blockIdx.x * BLI_NT + threadIdx.x;
    if (piece >= npiece) return;
    const int64_t i0 = piece * VEC;
    // 64-bit steps: baseline b starts b * n samples on, past 2^32 bytes for any real scan
    const float* vp = reinterpret_cast<const float*>(vis_) + i0 * W;
    const uint8_t* fp = flags + i0;
    const int64_t vstep = n * W;

    double sum[VEC];
    int cnt[VEC];
    if constexpr (VEC == 4) {
        const double2 s0 = *reinterpret_cast<const double2*>(sum_ + i0);
        const double2 s1 = *reinterpret_cast<const double2*>(sum_ + i0 + 2);
        const int4 c = *reinterpret_cast<const int4*>(count_ + i0);
        sum[0] = s0.x; sum[1] = s0.y; sum[2] = s1.x; sum[3] = s1.y;
        cnt[0] = c.x; cnt[1] = c.y; cnt[2] = c.z; cnt[3] = c.w;
    } else {
        sum[0] = sum_[i0];
        cnt[0] = count_[i0];
    }

    int64_t b = 0;
    for (; b + BLI_UNROLL <= nbl; b += BLI_UNROLL) {
        BliSamples<VD, VEC> s[BLI_UNROLL];
        // the group's select bytes first, as one scalar: the data loads below then issue back to back instead of
        // each waiting for its own byte (bytes have no scalar load, and a wait for one is a wait for all loads)
        unsigned on = (1u << BLI_UNROLL) - 1;
        if (select) {
            unsigned m = 0;
#pragma unroll
            for (int q = 0; q < BLI_UNROLL; q++) m |= (select[b + q] != 0 ? 1u : 0u) << q;
            on = __builtin_amdgcn_readfirstlane(m);
        }
#pragma unroll
        for (int q = 0; q < BLI_UNROLL; q++)
            if (on >> q & 1u) bli_load<VD, VEC>(vp + q * vstep, fp + q * n, s[q]);
#pragma unroll
        for (int q = 0; q < BLI_UNROLL; q++)
            if (on >> q & 1u) bli_add<VD, VEC>(s[q], sum, cnt);
        vp += BLI_UNROLL * vstep;
        fp += BLI_UNROLL * n;
    }
    for (; b < nbl; b++) {                                  // the last nbl % BLI_UNROLL baselines
        if (!select || select[b] != 0) {
            BliSamples<VD, VEC> s;
            bli_load<VD, VEC>(vp, fp, s);
            bli_add<VD, VEC>(s, sum, cnt);
        }
        vp += vstep;
        fp += n;
    }

    if constexpr (VEC == 4) {
        *reinterpret_cast<double2*>(sum_ + i0) = make_double2(sum[0], sum[1]);
        *reinterpret_cast<double2*>(sum_ + i0 + 2) = make_double2(sum[2], sum[3]);
        *reinterpret_cast<int4*>(count_ + i0) = make_int4(cnt[0], cnt[1], cnt[2], cnt[3]);
    } else {
        sum_[i0] = sum[0];
        count_[i0] = cnt[0];
    }
}

// One thread per position.
__global__ void __launch_bounds__(BLI_NT)
k_bli_finish(const double* __restrict__ sum, const int* __restrict__ count, int64_t n, int64_t min_count,
             float* __restrict__ amp, uint8_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * BLI_NT + threadIdx.x;
    if (i >= n) return;
    const int c = count[i];
    const bool f = (int64_t)c < min_count;
    flag[i] = f ? 1 : 0;
    amp[i] = f ? 0.0f : (float)(sum[i] / (double)c);
}

// grid (pieces of the image, baselines): a block's threads read their piece of `line` once and walk the baselines
// blockIdx.y, blockIdx.y + gridDim.y, ...  VEC16: n % 16 == 0 and 16-byte aligned bases, 16 flags per thread.
// out may be flags itself (in place).
template <bool VEC16>
__global__ void __launch_bounds__(BLI_NT)
k_bli_apply(const uint8_t* flags, const uint8_t* __restrict__ line, uint8_t* out, int64_t nbl, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * BLI_NT + threadIdx.x) * (VEC16 ? 16 : 1);
    if (i >= n) return;
    // byte-wise "!= 0" of a dword of flags
    auto norm = [](unsigned w) { return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) >> 7 & 0x01010101u; };
    if constexpr (VEC16) {
        uint4 l = *reinterpret_cast<const uint4*>(line + i);
        l = make_uint4(norm(l.x), norm(l.y), norm(l.z), norm(l.w));
        for (int64_t b = blockIdx.y; b < nbl; b += gridDim.y) {
            const uint4 f = *reinterpret_cast<const uint4*>(flags + b * n + i);
            *reinterpret_cast<uint4*>(out + b * n + i) =
                make_uint4(norm(f.x) | l.x, norm(f.y) | l.y, norm(f.z) | l.z, norm(f.w) | l.w);
        }
    } else {
        const unsigned l = line[i] ? 1u : 0u;
        for (int64_t b = blockIdx.y; b < nbl; b += gridDim.y)
            out[b * n + i] = (uint8_t)((flags[b * n + i] ? 1u : 0u) | l);
    }
}
