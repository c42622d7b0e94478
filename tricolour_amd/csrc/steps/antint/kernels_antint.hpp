// kernels_antint.hpp -- antenna integration: baseline integration (steps/kernels_blint.hpp) with one image per
// antenna instead of one for all baselines, and the flags-only variant that extends the flags of an antenna whose
// baselines are mostly flagged (the models are CASA's antint mode and AOFlagger's antenna selection; the definition
// is this project's own, include/tricolour_amd.h).
//
// vis (nbl, n) complex64 or float32 amplitudes, flags (nbl, n) uint8; n = ncorr * ntime * nchan.  The members of
// antenna a are baselines[offsets[a] .. offsets[a + 1]) in ascending order (built on the host from ubl, select and
// exclude_autos):
//   a         = tri_hypotf(re, im)   (float32 amplitudes: fabsf(v));  a sample counts if its flag is 0 and a is not
//               NaN (without visibilities: if its flag is 0)
//   sum[a,i] += (double)a, count[a,i] += 1 over the members of a in list order, over the counting samples
//   flag[a,i] = count[a,i] < min_count[a];  amp[a,i] = flag ? 0 : (float)(sum[a,i] / (double)count[a,i])
//   det[a,i]  = members[a] > 0 && members[a] - count[a,i] > max_flagged[a]            (flag excess)
//   out[b,i]  = (flags[b,i] != 0) | det[ant1[b],i] | det[ant2[b],i]
//
// Four kernels, no LDS, no cross-lane work, no atomics.
//   k_ant_accumulate  grid (pieces of n, antennas).  One thread owns VEC consecutive positions of the antenna
//                     blockIdx.y and walks its member list, so the float64 sum of a position has one order whatever
//                     the grid, the batch or the split of the baselines over calls.  The list is the same for every
//                     lane of a block: its reads are uniform.  The loads of ANT_UNROLL members are issued together and
//                     consumed strictly in list order.  Every sample is read once per antenna it belongs to: twice.
//   k_ant_finish      count -> flag, sum / count -> amplitude; one thread per (a, i).
//   k_ant_excess      count -> det, integers only; one thread per (a, i).
//   k_ant_apply       out = flags | det[ant1] | det[ant2], 16 flags per thread (VEC16) or one.
#pragma once

#define ANT_NT 256      // threads per block, all four kernels
#define ANT_UNROLL 4    // members whose loads are in flight together
#define ANT_NO_VIS (-1) // k_ant_accumulate's VD without visibilities: counts flags == 0, leaves the sum alone

// VEC positions of one member: the parts (none without visibilities) and the flag bytes, byte j = flag of position j.
// With visibilities the load and the add are those of baseline integration, so the arithmetic is the same code.
template <int VD, int VEC>
struct AntSamples : BliSamples<VD, VEC> {};
template <int VEC>
struct AntSamples<ANT_NO_VIS, VEC> {
    unsigned fl;
};

template <int VD, int VEC>
__device__ __forceinline__ void ant_load(const float* vp, const uint8_t* fp, AntSamples<VD, VEC>& s) {
    if constexpr (VD == ANT_NO_VIS) {
        if constexpr (VEC == 4) s.fl = *reinterpret_cast<const unsigned*>(fp);
        else                    s.fl = fp[0];
    } else {
        bli_load<VD, VEC>(vp, fp, s);
    }
}

template <int VD, int VEC>
__device__ __forceinline__ void ant_add(const AntSamples<VD, VEC>& s, double (&sum)[VEC], int (&cnt)[VEC]) {
    if constexpr (VD == ANT_NO_VIS) {
#pragma unroll
        for (int j = 0; j < VEC; j++) cnt[j] += ((s.fl >> (8 * j)) & 0xFFu) == 0 ? 1 : 0;
    } else {
        bli_add<VD, VEC>(s, sum, cnt);
    }
}

// VD: TRI_VIS_C64, TRI_VIS_F32 or ANT_NO_VIS (vis_ and sum_ are then not touched and may be null).  npiece = n / VEC
// threads per antenna.  A list entry outside [0, nbl) is skipped, never dereferenced; the branches on the entries are
// the same in every lane.
template <int VD, int VEC>
__global__ void __launch_bounds__(ANT_NT)
k_ant_accumulate(const void* __restrict__ vis_, const uint8_t* __restrict__ flags, const int* __restrict__ offsets,
                 const int* __restrict__ baselines, int64_t nbl, int64_t n, int64_t npiece, double* __restrict__ sum_,
                 int* __restrict__ count_) {
    constexpr bool VIS = VD != ANT_NO_VIS;
    constexpr int W = VD == TRI_VIS_C64 ? 2 : 1;          // floats per sample
    const int64_t piece = (int64_t)blockIdx.x * ANT_NT + threadIdx.x;
    if (piece >= npiece) return;
    const int64_t i0 = piece * VEC;
    const int64_t a = blockIdx.y;
    // 64-bit steps: baseline b starts b * n samples on, antenna a's image a * n positions on
    const float* vp = VIS ? reinterpret_cast<const float*>(vis_) + i0 * W : nullptr;
    const uint8_t* fp = flags + i0;
    const int64_t vstep = n * W;
    double* sp = VIS ? sum_ + a * n + i0 : nullptr;
    int* cp = count_ + a * n + i0;

    double sum[VEC];
    int cnt[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) sum[j] = 0.0;
    if constexpr (VEC == 4) {
        if constexpr (VIS) {
            const double2 s0 = *reinterpret_cast<const double2*>(sp);
            const double2 s1 = *reinterpret_cast<const double2*>(sp + 2);
            sum[0] = s0.x; sum[1] = s0.y; sum[2] = s1.x; sum[3] = s1.y;
        }
        const int4 c = *reinterpret_cast<const int4*>(cp);
        cnt[0] = c.x; cnt[1] = c.y; cnt[2] = c.z; cnt[3] = c.w;
    } else {
        if constexpr (VIS) sum[0] = sp[0];
        cnt[0] = cp[0];
    }

    const int k1 = offsets[a + 1];
    int k = offsets[a];
    for (; k + ANT_UNROLL <= k1; k += ANT_UNROLL) {
        AntSamples<VD, VEC> s[ANT_UNROLL];
        // the group's list entries first, as scalars: the data loads below then issue back to back
        int b[ANT_UNROLL];
#pragma unroll
        for (int q = 0; q < ANT_UNROLL; q++) b[q] = __builtin_amdgcn_readfirstlane(baselines[k + q]);
#pragma unroll
        for (int q = 0; q < ANT_UNROLL; q++)
            if (b[q] >= 0 && b[q] < nbl) ant_load<VD, VEC>(VIS ? vp + b[q] * vstep : nullptr, fp + b[q] * n, s[q]);
#pragma unroll
        for (int q = 0; q < ANT_UNROLL; q++)
            if (b[q] >= 0 && b[q] < nbl) ant_add<VD, VEC>(s[q], sum, cnt);
    }
    for (; k < k1; k++) {                                   // the last members % ANT_UNROLL of the list
        const int b = __builtin_amdgcn_readfirstlane(baselines[k]);
        if (b >= 0 && b < nbl) {
            AntSamples<VD, VEC> s;
            ant_load<VD, VEC>(VIS ? vp + b * vstep : nullptr, fp + b * n, s);
            ant_add<VD, VEC>(s, sum, cnt);
        }
    }

    if constexpr (VEC == 4) {
        if constexpr (VIS) {
            *reinterpret_cast<double2*>(sp) = make_double2(sum[0], sum[1]);
            *reinterpret_cast<double2*>(sp + 2) = make_double2(sum[2], sum[3]);
        }
        *reinterpret_cast<int4*>(cp) = make_int4(cnt[0], cnt[1], cnt[2], cnt[3]);
    } else {
        if constexpr (VIS) sp[0] = sum[0];
        cp[0] = cnt[0];
    }
}

// One thread per (a, i), a = blockIdx.y.  min_count[a] below 1 counts as 1: a position nothing counts at is flagged.
__global__ void __launch_bounds__(ANT_NT)
k_ant_finish(const double* __restrict__ sum, const int* __restrict__ count, const int* __restrict__ min_count,
             int64_t n, float* __restrict__ amp, uint8_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * ANT_NT + threadIdx.x;
    if (i >= n) return;
    const int64_t at = (int64_t)blockIdx.y * n + i;
    const int mc = max(min_count[blockIdx.y], 1);
    const int c = count[at];
    const bool f = c < mc;
    flag[at] = f ? 1 : 0;
    amp[at] = f ? 0.0f : (float)(sum[at] / (double)c);
}

// One thread per (a, i), a = blockIdx.y: more than max_flagged[a] of the members[a] baselines are flagged here.
__global__ void __launch_bounds__(ANT_NT)
k_ant_excess(const int* __restrict__ count, const int* __restrict__ members, const int* __restrict__ max_flagged,
             int64_t n, uint8_t* __restrict__ det) {
    const int64_t i = (int64_t)blockIdx.x * ANT_NT + threadIdx.x;
    if (i >= n) return;
    const int64_t at = (int64_t)blockIdx.y * n + i;
    const int m = members[blockIdx.y];
    det[at] = (m > 0 && m - count[at] > max_flagged[blockIdx.y]) ? 1 : 0;
}

// grid (pieces of the image, baselines): a block walks the baselines blockIdx.y, blockIdx.y + gridDim.y, ... and ORs
// the det lines of the baseline's two antennas into its normalised flags; an antenna number outside [0, nant)
// contributes nothing.  VEC16: n % 16 == 0 and 16-byte aligned bases, 16 flags per thread.  out may be flags itself.
template <bool VEC16>
__global__ void __launch_bounds__(ANT_NT)
k_ant_apply(const uint8_t* flags, const uint8_t* __restrict__ det, const int* __restrict__ ant1,
            const int* __restrict__ ant2, uint8_t* out, int64_t nbl, int64_t nant, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * ANT_NT + threadIdx.x) * (VEC16 ? 16 : 1);
    if (i >= n) return;
    // byte-wise "!= 0" of a dword of flags
    auto norm = [](unsigned w) { return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) >> 7 & 0x01010101u; };
    for (int64_t b = blockIdx.y; b < nbl; b += gridDim.y) {
        const int a1 = ant1[b], a2 = ant2[b];
        const bool in1 = a1 >= 0 && a1 < nant, in2 = a2 >= 0 && a2 < nant && a2 != a1;
        if constexpr (VEC16) {
            const uint4 f = *reinterpret_cast<const uint4*>(flags + b * n + i);
            uint4 o = make_uint4(norm(f.x), norm(f.y), norm(f.z), norm(f.w));
            if (in1) {
                const uint4 l = *reinterpret_cast<const uint4*>(det + a1 * n + i);
                o = make_uint4(o.x | norm(l.x), o.y | norm(l.y), o.z | norm(l.z), o.w | norm(l.w));
            }
            if (in2) {
                const uint4 l = *reinterpret_cast<const uint4*>(det + a2 * n + i);
                o = make_uint4(o.x | norm(l.x), o.y | norm(l.y), o.z | norm(l.z), o.w | norm(l.w));
            }
            *reinterpret_cast<uint4*>(out + b * n + i) = o;
        } else {
            unsigned o = flags[b * n + i] ? 1u : 0u;
            if (in1) o |= det[a1 * n + i] ? 1u : 0u;
            if (in2) o |= det[a2 * n + i] ? 1u : 0u;
            out[b * n + i] = (uint8_t)o;
        }
    }
}
