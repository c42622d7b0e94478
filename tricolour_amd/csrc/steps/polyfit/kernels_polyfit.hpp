// kernels_polyfit.hpp -- piecewise-polynomial fits along the lines of (time, chan) windows and the flagging of what
// stands off them (after CASA's tfcrop; the definition, with its operation order, is this project's own:
// include/tricolour_amd.h).
//
// Per line a[0..n) with mask m, P pieces, degree D: piece p covers [e_p, e_{p+1}), e_p = (p n) / P; in a piece of
// length L the sample j has x = (double)(2 j + 1 - L) / (double)L.  Moments are two-level sums: cells of PF_CELL = 32
// consecutive samples counted from the piece start, a sequential chain inside a cell (s_k += x^k, b_k += x^k a over the
// masked samples), then the cell sums added in ascending cell order.  Cholesky with degree truncation, Horner, r = a - f.
// A round: fit, Q = two-level sum of r r, sigma = sqrt(Q / n_m), hit = |r| > cutoff sigma && |r| > |f| 2^-20.
//
// The visibilities are read once, by k_pf_prepare; every later sweep works on its two images in the workspace:
//   amp    float32 amplitude (load_amp)
//   state  one byte per sample: PF_VALID (flag 0 and a finite amplitude), PF_HIT (hit by a pass so far), PF_FLAG (the
//          input flag was set).  The mask of every round of every pass is state == PF_VALID.
//   k_pf_prepare  VEC: 4 samples per lane, 16-byte loads and stores; otherwise 1.
//   k_pf_freq     one workgroup per time row, the line in LDS (amplitudes padded by a word per 32 against bank
//                 conflicts, valid and hit bits as words).  A lane owns a cell (moments, Q); a (piece, moment) pair
//                 owns the chain over that piece's cells; a lane per piece solves; the mark sweep is a lane per sample
//                 and gathers its hits with a wave ballot.  CAP: the longest line the LDS arrays hold.
//   k_pf_time     a lane per channel (adjacent lanes, adjacent channels: every access coalesced), sequential along time;
//                 the fits of the line's pieces go through the workspace (PF_CS doubles per piece and channel).
//   k_pf_finish   out = (state & (PF_HIT | PF_FLAG)) != 0.  VEC: 16 samples per lane.
// BG (both line kernels): one fit with the mask `valid`, (float)f written at every sample; no rounds.
// No atomics; nothing depends on the wave count or the launch geometry.
#pragma once

#define PF_NT 256            // threads per block, every kernel
#define PF_CELL 32           // samples per cell of the two-level sums
#define PF_MAX_PIECES 32
#define PF_MAX_LINE 16384    // longest fitted line, either axis
#define PF_MAX_ROUNDS 16
#define PF_NM 11             // moments of a cell: s_0 .. s_6, b_0 .. b_3
#define PF_CS 5              // doubles of a stored fit: c_0 .. c_3 and the degree used (-1: the piece holds no sample)
#define PF_VALID 1u
#define PF_HIT 2u
#define PF_FLAG 4u

template <int VIS, bool VEC>
__global__ void __launch_bounds__(PF_NT)
k_pf_prepare(const void* __restrict__ vis_, const uint8_t* __restrict__ flags, int64_t N, float* __restrict__ amp,
             uint8_t* __restrict__ state) {
    constexpr int CH = VEC ? 4 : 1;
    const int64_t i = ((int64_t)blockIdx.x * PF_NT + threadIdx.x) * CH;
    if (i >= N) return;                             // VEC: N % 4 == 0, a lane has all of its samples or none
    if (VEC) {
        const float* vf = reinterpret_cast<const float*>(vis_);
        const unsigned fl = *reinterpret_cast<const unsigned*>(flags + i);
        float a[4];
        if (VIS == TRI_VIS_C64) {
            const float4 u = *reinterpret_cast<const float4*>(vf + 2 * i);
            const float4 v = *reinterpret_cast<const float4*>(vf + 2 * i + 4);
            a[0] = tri_hypotf(u.x, u.y); a[1] = tri_hypotf(u.z, u.w);
            a[2] = tri_hypotf(v.x, v.y); a[3] = tri_hypotf(v.z, v.w);
        } else {
            const float4 u = *reinterpret_cast<const float4*>(vf + i);
            a[0] = fabsf(u.x); a[1] = fabsf(u.y); a[2] = fabsf(u.z); a[3] = fabsf(u.w);
        }
        unsigned s = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool flagged = ((fl >> (8 * j)) & 0xFFu) != 0;
            const unsigned b = flagged ? PF_FLAG : (a[j] < INFINITY ? PF_VALID : 0u);      // false for a NaN
            s |= b << (8 * j);
        }
        *reinterpret_cast<float4*>(amp + i) = make_float4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<unsigned*>(state + i) = s;
    } else {
        const float a = load_amp<VIS>(vis_, (size_t)i);
        amp[i] = a;
        state[i] = (uint8_t)(flags[i] != 0 ? PF_FLAG : (a < INFINITY ? PF_VALID : 0u));
    }
}

// one masked sample into the moments of its cell: pw_0 = 1, pw_k = pw_{k-1} x; s_k += pw_k, b_k += pw_k a
__device__ __forceinline__ void pf_accumulate(double x, double a, double* s, double* b) {
    double pw = 1.0;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        s[k] = s[k] + pw;
        if (k < 4) b[k] = b[k] + pw * a;
        pw = pw * x;
    }
}

__device__ __forceinline__ double pf_x(int j, int L) { return (double)(2 * j + 1 - L) / (double)L; }

// The fit of one piece from its moments S_0 .. S_6, B_0 .. B_3 and masked count np at degree D: c[0 .. 3] and the
// degree used, -1 when the piece holds no sample.  Every loop has constant bounds and guards: the arrays stay registers.
__device__ __forceinline__ int pf_solve(const double* S, const double* B, int np, int D, double* c) {
#pragma unroll
    for (int k = 0; k < 4; k++) c[k] = 0.0;
    if (np <= 0) return -1;
    int d = min(D, np - 1);
    double l[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) l[i][j] = 0.0;
    const double least = 0x1p-20 * S[0];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j <= d) {
            double v = S[2 * j];
#pragma unroll
            for (int k = 0; k < j; k++) v = v - l[j][k] * l[j][k];
            if (!(v > least)) {
                d = j - 1;                          // the leading factor stays; the columns from j on are not formed
            } else {
                l[j][j] = sqrt(v);
#pragma unroll
                for (int i = j + 1; i < 4; i++) {   // rows beyond d are formed too and never read
                    double t = S[i + j];
#pragma unroll
                    for (int k = 0; k < j; k++) t = t - l[i][k] * l[j][k];
                    l[i][j] = t / l[j][j];
                }
            }
        }
    }
    double y[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i <= d) {
            double t = B[i];
#pragma unroll
            for (int k = 0; k < i; k++) t = t - l[i][k] * y[k];
            y[i] = t / l[i][i];
        }
    }
#pragma unroll
    for (int i = 3; i >= 0; i--) {
        if (i <= d) {
            double t = y[i];
#pragma unroll
            for (int k = i + 1; k < 4; k++)
                if (k <= d) t = t - l[k][i] * c[k];
            c[i] = t / l[i][i];
        }
    }
    return d;
}

// Horner from c_d down (d >= 0): f = c_d, then f = f x + c_k for k = d - 1 .. 0
__device__ __forceinline__ double pf_eval(const double* c, int d, double x) {
    double f = c[3];
    f = d == 2 ? c[2] : (d > 2 ? f * x + c[2] : f);
    f = d == 1 ? c[1] : (d > 1 ? f * x + c[1] : f);
    f = d == 0 ? c[0] : f * x + c[0];
    return f;
}

__device__ __forceinline__ bool pf_is_hit(double r, double f, double limit) {
    return fabs(r) > limit && fabs(r) > fabs(f) * 0x1p-20;
}

// pieces and degree of round r of a pass
__device__ __forceinline__ void pf_round(int r, int max_pieces, int degree, int* P, int* D) {
    *P = min(2 * r + 1, max_pieces);
    *D = r == 0 ? min(1, degree) : degree;
}

__device__ __forceinline__ float pf_nan() { return __uint_as_float(0x7FC00000u); }

// ---------------------------------------------------------------------------
// time axis: a lane per channel
// ---------------------------------------------------------------------------
// Grid: one block per (window, strip of PF_NT channels), strips fastest.  coef: (window, piece < pieces_alloc,
// PF_CS, channel) doubles.  BG: max_pieces is the number of pieces, degree the degree, rounds / cutoff / min_samples
// are not read, bg is written; otherwise state gains PF_HIT where a round hits.
template <bool BG>
__global__ void __launch_bounds__(PF_NT)
k_pf_time(const float* __restrict__ amp, uint8_t* state, int ntime, int nchan, int nstrip, int pieces_alloc,
          int max_pieces, int degree, double cutoff, int rounds, int min_samples, double* __restrict__ coef,
          float* __restrict__ bg) {
    const int64_t blk = blockIdx.x;
    const int strip = (int)(blk % nstrip);
    const int64_t win = blk / nstrip;
    const int ch = strip * PF_NT + (int)threadIdx.x;
    if (ch >= nchan) return;
    const int64_t base = win * ntime * nchan + ch;
    double* cf = coef + win * pieces_alloc * PF_CS * (int64_t)nchan + ch;
    const int n = ntime;
    const int nrounds = BG ? 1 : rounds;
    for (int r = 0; r < nrounds; r++) {
        int P, D;
        if (BG) { P = max_pieces; D = degree; } else pf_round(r, max_pieces, degree, &P, &D);
        // moments and fit of every piece
        int nm = 0;
        for (int p = 0; p < P; p++) {
            const int e0 = (p * n) / P, L = ((p + 1) * n) / P - e0;
            double S[7], B[4];
#pragma unroll
            for (int k = 0; k < 7; k++) S[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) B[k] = 0.0;
            int np = 0;
            for (int j0 = 0; j0 < L; j0 += PF_CELL) {
                double s[7], b[4];
#pragma unroll
                for (int k = 0; k < 7; k++) s[k] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) b[k] = 0.0;
                const int j1 = min(j0 + PF_CELL, L);
                int64_t i = base + (int64_t)(e0 + j0) * nchan;
#pragma unroll 4
                for (int j = j0; j < j1; j++, i += nchan) {
                    const unsigned sv = state[i];           // both loads whatever the mask: they can run ahead
                    const float av = amp[i];
                    if ((sv & (PF_VALID | PF_HIT)) == PF_VALID) {
                        pf_accumulate(pf_x(j, L), (double)av, s, b);
                        np++;
                    }
                }
#pragma unroll
                for (int k = 0; k < 7; k++) S[k] = S[k] + s[k];
#pragma unroll
                for (int k = 0; k < 4; k++) B[k] = B[k] + b[k];
            }
            double c[4];
            const int d = pf_solve(S, B, np, D, c);
            double* o = cf + (int64_t)p * PF_CS * nchan;
#pragma unroll
            for (int k = 0; k < 4; k++) o[(int64_t)k * nchan] = c[k];
            o[(int64_t)4 * nchan] = (double)d;
            nm += np;
        }
        if (BG) {
            for (int p = 0; p < P; p++) {
                const int e0 = (p * n) / P, L = ((p + 1) * n) / P - e0;
                const double* o = cf + (int64_t)p * PF_CS * nchan;
                double c[4];
#pragma unroll
                for (int k = 0; k < 4; k++) c[k] = o[(int64_t)k * nchan];
                const int d = (int)o[(int64_t)4 * nchan];
                int64_t i = base + (int64_t)e0 * nchan;
                for (int j = 0; j < L; j++, i += nchan) bg[i] = d < 0 ? pf_nan() : (float)pf_eval(c, d, pf_x(j, L));
            }
            return;
        }
        if (nm < min_samples) return;
        // Q: cell sums of r r, added in (piece, cell) order
        double Q = 0.0;
        for (int p = 0; p < P; p++) {
            const int e0 = (p * n) / P, L = ((p + 1) * n) / P - e0;
            const double* o = cf + (int64_t)p * PF_CS * nchan;
            double c[4];
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = o[(int64_t)k * nchan];
            const int d = (int)o[(int64_t)4 * nchan];
            if (d < 0) continue;                    // no masked sample in the piece: its cells add +0.0
            for (int j0 = 0; j0 < L; j0 += PF_CELL) {
                double q = 0.0;
                const int j1 = min(j0 + PF_CELL, L);
                int64_t i = base + (int64_t)(e0 + j0) * nchan;
#pragma unroll 4
                for (int j = j0; j < j1; j++, i += nchan) {
                    const unsigned sv = state[i];
                    const float av = amp[i];
                    if ((sv & (PF_VALID | PF_HIT)) == PF_VALID) {
                        const double res = (double)av - pf_eval(c, d, pf_x(j, L));
                        q = q + res * res;
                    }
                }
                Q = Q + q;
            }
        }
        const double limit = cutoff * sqrt(Q / (double)nm);
        // mark
        for (int p = 0; p < P; p++) {
            const int e0 = (p * n) / P, L = ((p + 1) * n) / P - e0;
            const double* o = cf + (int64_t)p * PF_CS * nchan;
            double c[4];
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = o[(int64_t)k * nchan];
            const int d = (int)o[(int64_t)4 * nchan];
            if (d < 0) continue;
            int64_t i = base + (int64_t)e0 * nchan;
            for (int j = 0; j < L; j++, i += nchan) {
                const unsigned sv = state[i];
                const float av = amp[i];
                if ((sv & (PF_VALID | PF_HIT)) == PF_VALID) {
                    const double f = pf_eval(c, d, pf_x(j, L));
                    if (pf_is_hit((double)av - f, f, limit)) state[i] = (uint8_t)(sv | PF_HIT);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// frequency axis: a workgroup per row, the line in LDS
// ---------------------------------------------------------------------------
__device__ __forceinline__ int pf_pad(int i) { return i + (i >> 5); }

// the mask bits (valid and not hit) of the `len` <= 32 samples from i0 on
__device__ __forceinline__ unsigned pf_bits(const unsigned* V, const unsigned* H, int i0, int len) {
    const int w = i0 >> 5, sh = i0 & 31;
    unsigned v = V[w] >> sh, h = H[w] >> sh;
    if (sh) { v |= V[w + 1] << (32 - sh); h |= H[w + 1] << (32 - sh); }
    const unsigned m = v & ~h;
    return len < 32 ? m & ((1u << len) - 1u) : m;
}

// the 64 predicates of a wave's aligned group of samples from i0 on into two words of a bit array
__device__ __forceinline__ void pf_store_ballot(unsigned* W, int i0, bool pred, bool merge) {
    const unsigned long long b = __ballot(pred);
    if ((threadIdx.x & 63) == 0) {
        const int w = i0 >> 5;
        if (merge) { W[w] |= (unsigned)b; W[w + 1] |= (unsigned)(b >> 32); }
        else       { W[w] = (unsigned)b;  W[w + 1] = (unsigned)(b >> 32); }
    }
}

// Grid: one block per (window, time row).  CAP >= nchan, a multiple of PF_NT.  BG as in k_pf_time.
template <int CAP, bool BG>
__global__ void __launch_bounds__(PF_NT)
k_pf_freq(const float* __restrict__ amp, uint8_t* state, int nchan, int max_pieces, int degree, double cutoff,
          int rounds, int min_samples, float* __restrict__ bg) {
    constexpr int NCELL = CAP / PF_CELL + PF_MAX_PIECES;        // cells of a line, whatever its pieces
    __shared__ float a[CAP + CAP / 32];
    __shared__ unsigned V[CAP / 32 + 2], H[CAP / 32 + 2];
    __shared__ double cm[NCELL][PF_NM];                        // cell moments; [cell][0] is reused for the cell's r r
    __shared__ int cn[NCELL];                                   // masked count of a cell
    __shared__ double pm[PF_MAX_PIECES][PF_NM];
    __shared__ int pn[PF_MAX_PIECES];
    __shared__ double coef[PF_MAX_PIECES][PF_CS];
    __shared__ int pe[PF_MAX_PIECES + 1], pc[PF_MAX_PIECES + 1];  // first sample and first cell of a piece
    __shared__ double sh_limit;
    __shared__ int sh_nm;

    const int tid = (int)threadIdx.x;
    const int n = nchan;
    const int64_t base = (int64_t)blockIdx.x * nchan;

    for (int b0 = 0; b0 < n; b0 += PF_NT) {
        const int i = b0 + tid;
        const unsigned sv = i < n ? state[base + i] : 0u;
        if (i < n) a[pf_pad(i)] = amp[base + i];
        pf_store_ballot(V, i & ~63, (sv & PF_VALID) != 0, false);
        pf_store_ballot(H, i & ~63, (sv & PF_HIT) != 0, false);
    }
    if (tid == 0) {                                             // the word after the last group (read, then masked off)
        const int w = (int)(((int64_t)n + PF_NT - 1) / PF_NT) * (PF_NT / 32);
        V[w] = 0u; H[w] = 0u;
    }
    __syncthreads();

    const int nrounds = BG ? 1 : rounds;
    for (int r = 0; r < nrounds; r++) {
        int P, D;
        if (BG) { P = max_pieces; D = degree; } else pf_round(r, max_pieces, degree, &P, &D);
        if (tid <= P) pe[tid] = (tid * n) / P;
        __syncthreads();
        if (tid == 0) {
            pc[0] = 0;
            for (int p = 0; p < P; p++) pc[p + 1] = pc[p] + (pe[p + 1] - pe[p] + PF_CELL - 1) / PF_CELL;
        }
        __syncthreads();
        const int ncell = pc[P];
        // a lane per cell: its moments
        for (int cell = tid; cell < ncell; cell += PF_NT) {
            int p = 0;
            while (pc[p + 1] <= cell) p++;
            const int L = pe[p + 1] - pe[p], j0 = (cell - pc[p]) * PF_CELL, len = min(PF_CELL, L - j0), i0 = pe[p] + j0;
            const unsigned bits = pf_bits(V, H, i0, len);
            double s[7], b[4];
#pragma unroll
            for (int k = 0; k < 7; k++) s[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) b[k] = 0.0;
            for (int jj = 0; jj < len; jj++)
                if ((bits >> jj) & 1u) pf_accumulate(pf_x(j0 + jj, L), (double)a[pf_pad(i0 + jj)], s, b);
#pragma unroll
            for (int k = 0; k < 7; k++) cm[cell][k] = s[k];
#pragma unroll
            for (int k = 0; k < 4; k++) cm[cell][7 + k] = b[k];
            cn[cell] = __popc(bits);
        }
        __syncthreads();
        // a lane per (piece, moment): the chain over the piece's cells
        for (int task = tid; task < P * PF_NM; task += PF_NT) {
            const int p = task / PF_NM, k = task % PF_NM;
            double sum = 0.0;
            int cnt = 0;
            for (int cell = pc[p]; cell < pc[p + 1]; cell++) {
                sum = sum + cm[cell][k];
                if (k == 0) cnt += cn[cell];
            }
            pm[p][k] = sum;
            if (k == 0) pn[p] = cnt;
        }
        __syncthreads();
        if (tid < P) {
            double S[7], B[4], c[4];
#pragma unroll
            for (int k = 0; k < 7; k++) S[k] = pm[tid][k];
#pragma unroll
            for (int k = 0; k < 4; k++) B[k] = pm[tid][7 + k];
            const int d = pf_solve(S, B, pn[tid], D, c);
#pragma unroll
            for (int k = 0; k < 4; k++) coef[tid][k] = c[k];
            coef[tid][4] = (double)d;
        }
        if (tid == PF_NT - 1) {
            int nm = 0;
            for (int p = 0; p < P; p++) nm += pn[p];
            sh_nm = nm;
        }
        __syncthreads();
        if (BG) {
            for (int i = tid; i < n; i += PF_NT) {
                int p = 0;
                while (pe[p + 1] <= i) p++;
                const int d = (int)coef[p][4];
                double c[4];
#pragma unroll
                for (int k = 0; k < 4; k++) c[k] = coef[p][k];
                bg[base + i] = d < 0 ? pf_nan() : (float)pf_eval(c, d, pf_x(i - pe[p], pe[p + 1] - pe[p]));
            }
            return;
        }
        const int nm = sh_nm;
        if (nm < min_samples) break;                            // the same for every lane
        // a lane per cell: its sum of r r
        for (int cell = tid; cell < ncell; cell += PF_NT) {
            int p = 0;
            while (pc[p + 1] <= cell) p++;
            const int L = pe[p + 1] - pe[p], j0 = (cell - pc[p]) * PF_CELL, len = min(PF_CELL, L - j0), i0 = pe[p] + j0;
            const unsigned bits = pf_bits(V, H, i0, len);
            const int d = (int)coef[p][4];
            double c[4];
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = coef[p][k];
            double q = 0.0;
            if (d >= 0)
                for (int jj = 0; jj < len; jj++)
                    if ((bits >> jj) & 1u) {
                        const double res = (double)a[pf_pad(i0 + jj)] - pf_eval(c, d, pf_x(j0 + jj, L));
                        q = q + res * res;
                    }
            cm[cell][0] = q;
        }
        __syncthreads();
        if (tid == 0) {
            double Q = 0.0;
            for (int cell = 0; cell < ncell; cell++) Q = Q + cm[cell][0];
            sh_limit = cutoff * sqrt(Q / (double)nm);
        }
        __syncthreads();
        const double limit = sh_limit;
        // a lane per sample: mark
        for (int b0 = 0; b0 < n; b0 += PF_NT) {
            const int i = b0 + tid;
            bool hit = false;
            if (i < n && ((V[i >> 5] & ~H[i >> 5]) >> (i & 31) & 1u)) {
                int p = 0;
                while (pe[p + 1] <= i) p++;
                const int d = (int)coef[p][4];
                if (d >= 0) {
                    double c[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) c[k] = coef[p][k];
                    const double f = pf_eval(c, d, pf_x(i - pe[p], pe[p + 1] - pe[p]));
                    hit = pf_is_hit((double)a[pf_pad(i)] - f, f, limit);
                }
            }
            pf_store_ballot(H, i & ~63, hit, true);
        }
        __syncthreads();
    }
    // a hit sample was valid and unflagged
    for (int i = tid; i < n; i += PF_NT)
        if ((H[i >> 5] >> (i & 31)) & 1u) state[base + i] = (uint8_t)(PF_VALID | PF_HIT);
}

// 0x01 in byte j of the result where byte j of w is nonzero
__device__ __forceinline__ unsigned pf_nonzero_bytes(unsigned w) {
    return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) >> 7 & 0x01010101u;
}

template <bool VEC>
__global__ void __launch_bounds__(PF_NT)
k_pf_finish(const uint8_t* __restrict__ state, uint8_t* __restrict__ out, int64_t N) {
    constexpr int CH = VEC ? 16 : 1;
    constexpr unsigned KEEP = (PF_HIT | PF_FLAG) * 0x01010101u;
    const int64_t i = ((int64_t)blockIdx.x * PF_NT + threadIdx.x) * CH;
    if (i >= N) return;
    if (VEC) {
        const uint4 s = *reinterpret_cast<const uint4*>(state + i);
        *reinterpret_cast<uint4*>(out + i) = make_uint4(pf_nonzero_bytes(s.x & KEEP), pf_nonzero_bytes(s.y & KEEP),
                                                        pf_nonzero_bytes(s.z & KEEP), pf_nonzero_bytes(s.w & KEEP));
    } else {
        out[i] = (uint8_t)((state[i] & (PF_HIT | PF_FLAG)) != 0 ? 1u : 0u);
    }
}
