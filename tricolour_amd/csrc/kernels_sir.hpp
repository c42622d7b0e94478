// kernels_sir.hpp -- scale-invariant rank (SIR) operator (Offringa, van de Gronde & Roerdink 2012, A&A 539, A95)
// over uint8 flag windows, along either window axis.
//
// One line f[0..n) (nonzero = flagged), 0 <= eta < 1:
//   U(i) = number of unflagged samples in [0, i)                  (integer, i = 0..n)
//   W(i) = eta * (double)i - (double)U(i)                          (one IEEE multiply, one IEEE subtract; no FMA)
//   out[x] = max_{x < j <= n} W(j) >= min_{0 <= k <= x} W(k)
// Prefix counts are integers and min / max are exact, so any decomposition of a line gives the same bits.
//
// Decomposition used here.  A workgroup holds CB lines side by side (CB = 1: one line per block, contiguous along
// frequency; CB = 64: 64 adjacent channels, one time line each, so a wave reads 64 consecutive bytes of a row).  The
// S = NT / CB threads of one line each own K sub-chunks of 16 consecutive samples, held as 16-bit flag masks.
//   1. count unflagged samples per thread; exclusive column scan (wave shuffles + one LDS round) -> U at the
//      thread's first sample; the column total gives U(n) and so W(n);
//   2. W of every owned position i (W(n) is the suffix seed): the thread's minimum and each sub-chunk's maximum;
//      exclusive prefix-min and suffix-max column scans -> the carries from the samples before / after the thread;
//   3. per sub-chunk, a forward sweep builds min W(k<=x) in registers and a backward sweep carries max W(j>x): bit x.
// A line longer than one block's span (S * 16 * K samples) is cut into segments along blockIdx.y and run in three
// launches of the same kernel: SIR_COUNT writes each segment's unflagged count, SIR_MINMAX each segment's W minimum
// and maximum (its U offset summed from the counts), SIR_FINAL folds the other segments' aggregates into the carries.
//
// MISSING: the masked operator.  A second mask m[0..n) (nonzero = missing) and a finite penalty >= 0:
//   M(i) = missing samples in [0, i),  P(i) = i - M(i),  U(i) = present and unflagged samples in [0, i)   (integers)
//   W(i) = (eta * (double)P(i) - (double)U(i)) - penalty * (double)M(i)       (four IEEE operations in that order)
//   out[x] = present x: max_{x < j <= n} W(j) >= min_{0 <= k <= x} W(k);  missing x: f[x] != 0
// Same decomposition: the column scan carries U and M as the two halves of one 64-bit count (so do the segment
// counts of long lines), a second 16-bit mask per sub-chunk holds the missing samples.  With m all zero W is the
// unmasked W (x - 0.0 == x), so the result is the unmasked operator's bit for bit.  All of it sits behind
// `if constexpr (MISSING)`: the unmasked instantiations compile to what they were without it.
#pragma once

#define SIR_FULL 0     // the block spans the whole line
#define SIR_COUNT 1    // long lines: per-segment unflagged counts -> ws_cnt
#define SIR_MINMAX 2   // long lines: per-segment min / max of W -> ws_mn / ws_mx
#define SIR_FINAL 3    // long lines: the operator, with the other segments' aggregates as carries

// 16 flag bytes -> 16-bit mask (bit i = byte i != 0)
__device__ __forceinline__ unsigned sir_mask4(unsigned w) {
    unsigned t = (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) >> 7 & 0x01010101u;   // byte != 0 -> 1
    return (t * 0x01020408u) >> 24 & 0xFu;                                     // gather the four low bits
}
__device__ __forceinline__ unsigned sir_mask16(uint4 v) {
    return sir_mask4(v.x) | sir_mask4(v.y) << 4 | sir_mask4(v.z) << 8 | sir_mask4(v.w) << 12;
}
// 4-bit mask -> four 0/1 bytes
__device__ __forceinline__ unsigned sir_bytes4(unsigned m) { return ((m & 0xFu) * 0x00204081u) & 0x01010101u; }

// count carried through the column scan: U, or with a missing mask U (low word) and M (high word) in one add
template <bool MISSING> struct sir_count { typedef int type; };
template <> struct sir_count<true> { typedef unsigned long long type; };

// W(i) from the integer prefix counts: u = U(i), mc = M(i) (MISSING only)
template <bool MISSING>
__device__ __forceinline__ double sir_w(double eta, double penalty, int i, int u, int mc) {
    if constexpr (MISSING) return (eta * (double)(i - mc) - (double)u) - penalty * (double)mc;
    else return eta * (double)i - (double)u;
}

// Exclusive scan of v over the S = NT / CB threads of one column (tid % CB) in thread order (REV: from the last
// thread down), with `total` the column's full reduction.  sh: NT / 64 * CB entries, used by this call alone.
template <int NT, int CB, bool REV, class T, class Op>
__device__ __forceinline__ T sir_col_scan(T v, T ident, Op op, T* sh, T& total) {
    static_assert(64 % CB == 0 && NT % 64 == 0, "columns must tile a wave");
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = threadIdx.x % CB;
#pragma unroll
    for (int d = CB; d < 64; d <<= 1) {
        T t = REV ? __shfl_down(v, d, 64) : __shfl_up(v, d, 64);
        if (REV ? lane + d < 64 : lane >= d) v = op(v, t);
    }
    if (REV ? lane < CB : lane >= 64 - CB) sh[wave * CB + c] = v;     // the wave's column total
    T e = REV ? __shfl_down(v, CB, 64) : __shfl_up(v, CB, 64);
    if (REV ? lane >= 64 - CB : lane < CB) e = ident;
    __syncthreads();
    T before = ident;
    total = ident;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        T t = sh[w * CB + c];
        if (REV ? w > wave : w < wave) before = op(before, t);
        total = op(total, t);
    }
    return op(before, e);
}

// NT threads, CB lines per block, K sub-chunks of 16 samples per thread.
// TIME: line L = (window, channel), sample x at L's window base + x * nchan + channel; else line L = (window, time
// row), sample x at L * nchan + x.  VEC (frequency only, nchan % 16 == 0 and a 16-byte aligned base): uint4 loads and
// stores.  OR: out |= result (the second axis of a two-axis call) instead of out = result.  MISSING: `miss` (laid
// out as `in`) and `penalty` are read, ws_cnt holds one 64-bit (U, M) count per (line, segment); neither is touched
// otherwise.
template <int NT, int CB, int K, int PHASE, bool TIME, bool VEC, bool OR, bool MISSING = false>
__global__ void __launch_bounds__(NT)
k_sir(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t nlines, int64_t ntime, int64_t nchan,
      double eta, int nseg, int* __restrict__ ws_cnt, double* __restrict__ ws_mn, double* __restrict__ ws_mx,
      const uint8_t* __restrict__ miss, double penalty) {
    static_assert(!(TIME && VEC), "time lines are strided");
    constexpr int S = NT / CB;
    constexpr int SPAN = S * 16 * K;
    typedef typename sir_count<MISSING>::type cnt_t;
    __shared__ cnt_t sh_cnt[NT / 64 * CB];
    __shared__ double sh_mn[NT / 64 * CB];
    __shared__ double sh_mx[NT / 64 * CB];

    const int c = threadIdx.x % CB, s = threadIdx.x / CB;
    const int64_t L = (int64_t)blockIdx.x * CB + c;
    const bool active = L < nlines;
    const int n = (int)(TIME ? ntime : nchan);
    const int64_t ss = TIME ? nchan : 1;
    const int64_t base = TIME ? (L / nchan) * ntime * nchan + L % nchan : L * nchan;
    const int seg = blockIdx.y;
    const int x0 = seg * SPAN + s * 16 * K;

    // ---- load: 16-bit flag masks, nothing set at or past n
    // (MISSING: m = flagged or missing, i.e. not counted in U; mm = missing, and in its high half flagged and missing)
    unsigned m[K];
    unsigned mm[MISSING ? K : 1];
    int nv[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int xs = x0 + 16 * k;
        nv[k] = active ? min(max(n - xs, 0), 16) : 0;
        m[k] = 0;
        if (VEC) {
            if (nv[k] > 0) m[k] = sir_mask16(*reinterpret_cast<const uint4*>(in + base + xs));
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (i < nv[k] && in[base + (int64_t)(xs + i) * ss]) m[k] |= 1u << i;
        }
        if constexpr (MISSING) {
            unsigned q = 0;
            if (VEC) {
                if (nv[k] > 0) q = sir_mask16(*reinterpret_cast<const uint4*>(miss + base + xs));
            } else {
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if (i < nv[k] && miss[base + (int64_t)(xs + i) * ss]) q |= 1u << i;
            }
            mm[k] = q | (m[k] & q) << 16;
            m[k] |= q;
        }
    }
    cnt_t mine = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        mine += nv[k] - __popc(m[k]);
        if constexpr (MISSING) mine += (cnt_t)__popc(mm[k] & 0xFFFFu) << 32;
    }

    // ---- U (and M) at the thread's first sample, U(n) (and M(n))
    cnt_t col_total;
    cnt_t c0 = sir_col_scan<NT, CB, false>(mine, (cnt_t)0, [](cnt_t a, cnt_t b) { return a + b; }, sh_cnt, col_total);
    cnt_t* __restrict__ ws_c = reinterpret_cast<cnt_t*>(ws_cnt);
    if (PHASE == SIR_COUNT) {
        if (active && s == 0) ws_c[L * nseg + seg] = col_total;
        return;
    }
    cnt_t cseg = 0, call = col_total;
    if (PHASE != SIR_FULL && active) {
        call = 0;
        for (int g = 0; g < nseg; g++) {
            cnt_t t = ws_c[L * nseg + g];
            if (g < seg) cseg += t;
            call += t;
        }
    }
    c0 += cseg;
    int u0 = (int)c0, uall = (int)call, m0 = 0, mall = 0;
    if constexpr (MISSING) {
        u0 = (int)(c0 & 0xFFFFFFFFu), uall = (int)(call & 0xFFFFFFFFu);
        m0 = (int)(c0 >> 32), mall = (int)(call >> 32);
    }

    // ---- W minimum / maximum: the thread's minimum, each sub-chunk's maximum (the backward sweeps need those)
    double mx[K];
    double tmn = INFINITY, tmx = -INFINITY;
    {
        int u = u0, mc = m0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int xs = x0 + 16 * k;
            mx[k] = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if (i < nv[k]) {
                    double w = sir_w<MISSING>(eta, penalty, xs + i, u, mc);
                    tmn = fmin(tmn, w);
                    mx[k] = fmax(mx[k], w);
                    u += (m[k] >> i & 1u) ? 0 : 1;
                    if constexpr (MISSING) mc += mm[k] >> i & 1u;
                }
            }
            tmx = fmax(tmx, mx[k]);
        }
    }
    double bmn, bmx;
    double pcar = sir_col_scan<NT, CB, false>(tmn, (double)INFINITY, [](double a, double b) { return fmin(a, b); }, sh_mn, bmn);
    double scar = sir_col_scan<NT, CB, true>(tmx, (double)-INFINITY, [](double a, double b) { return fmax(a, b); }, sh_mx, bmx);
    if (PHASE == SIR_MINMAX) {
        if (active && s == 0) {
            ws_mn[L * nseg + seg] = bmn;
            ws_mx[L * nseg + seg] = bmx;
        }
        return;
    }
    if (!active) return;                    // no barrier follows
    scar = fmax(scar, sir_w<MISSING>(eta, penalty, n, uall, mall));      // W(n)
    if (PHASE == SIR_FINAL) {
        for (int g = 0; g < nseg; g++) {
            if (g < seg) pcar = fmin(pcar, ws_mn[L * nseg + g]);
            if (g > seg) scar = fmax(scar, ws_mx[L * nseg + g]);
        }
    }
#pragma unroll
    for (int k = K - 2; k >= 0; k--) mx[k] = fmax(mx[k], mx[k + 1]);   // suffix maxima over the sub-chunks

    // ---- per sub-chunk: forward sweep -> min W(k <= x), backward sweep carrying max W(j > x)
    unsigned r[K];
    int u = u0, mc = m0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int xs = x0 + 16 * k;
        double P[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (i < nv[k]) {
                pcar = fmin(pcar, sir_w<MISSING>(eta, penalty, xs + i, u, mc));
                u += (m[k] >> i & 1u) ? 0 : 1;
                if constexpr (MISSING) mc += mm[k] >> i & 1u;
            }
            P[i] = pcar;
        }
        double sc = k + 1 < K ? fmax(scar, mx[k + 1 < K ? k + 1 : k]) : scar;   // max W(j), j past the sub-chunk
        int ub = u, mb = mc;                 // U(xs + nv), M(xs + nv)
        unsigned bits = 0;
#pragma unroll
        for (int i = 15; i >= 0; i--) {
            if (i < nv[k]) {
                if (sc >= P[i]) bits |= 1u << i;
                ub -= (m[k] >> i & 1u) ? 0 : 1;
                if constexpr (MISSING) mb -= mm[k] >> i & 1u;
                sc = fmax(sc, sir_w<MISSING>(eta, penalty, xs + i, ub, mb));
            }
        }
        if constexpr (MISSING) bits = (bits & ~mm[k]) | mm[k] >> 16;    // a missing sample keeps its flag
        r[k] = bits;
    }

    // ---- store 0/1 bytes
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int xs = x0 + 16 * k;
        if (nv[k] <= 0) continue;
        if (VEC) {
            uint4 o = make_uint4(sir_bytes4(r[k]), sir_bytes4(r[k] >> 4), sir_bytes4(r[k] >> 8), sir_bytes4(r[k] >> 12));
            uint4* dst = reinterpret_cast<uint4*>(out + base + xs);
            if (OR) {
                uint4 a = *dst;
                o.x |= a.x; o.y |= a.y; o.z |= a.z; o.w |= a.w;
            }
            *dst = o;
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if (i < nv[k]) {
                    uint8_t* d = out + base + (int64_t)(xs + i) * ss;
                    uint8_t b = (uint8_t)(r[k] >> i & 1u);
                    *d = OR ? (uint8_t)(*d | b) : b;
                }
            }
        }
    }
}
