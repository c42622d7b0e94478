// kernels_scan.hpp -- the per-scan steps of the application around the window pipeline
// (apps/tricolour/app.py:389-457 and :475-480) fused into one pass each way:
//   k_pack_scan    residual (data - model), Stokes intensity, any-over-corr flags, scatter into windows
//   k_unpack_scan  gather of the flag windows, any over the window correlations, broadcast to the MS's ncorr
// and their row-list variants (k_pack_scan_rows*, k_unpack_scan_rows), which run one baseline chunk of a scan through
// the same per-sample code
#pragma once

// ---------------------------------------------------------------------------
// Fused scan pack.  One thread per (row, chan): the NC correlations of a sample are one contiguous
// NC * 8-byte piece of the row, loaded as float4 pieces (16 B / lane, consecutive lanes on consecutive
// channels), the flags as one NC-byte word.  Each window correlation is then stored as one float2 + one
// byte per lane, consecutive lanes on consecutive channels of the (bl, wcorr, time, chan) window.
//   STOKES = false (mode 0): window correlation c = residual of correlation c, flag c copied
//   STOKES = true  (modes 1 / 2): one window correlation = polarised intensity of the residual
//                  (stokes_intensity_sample, the arithmetic of k_stokes_intensity), flag = any over corr
// Residual: (d.x - m.x, d.y - m.y) in float32, numpy's complex64 subtraction.  flag == nullptr (ignore
// flags): the window flags of mapped cells are 0.  Cells no row maps to keep tri_fill_windows' NaN / 1.
//
// Bandwidth model (the kernel does no other work worth counting), per mapped MS row:
//   read   nchan * ncorr * (8 data + 8 model if any + 1 flag if any) + 8 (row_bl, row_time)
//   write  nchan * wcorr * (8 vis + 1 flag),   wcorr = ncorr (mode 0) or 1 (modes 1 / 2)
// plus tri_fill_windows' nbl * ntime * nchan * wcorr * 9 bytes written before it.  The unfused chain it
// replaces (data - model in HBM, tri_stokes_intensity, any over corr, tri_pack_data) additionally writes and
// re-reads the (row, chan, corr) residual (16 B / sample), the intensity (16 B / (row, chan)) and the
// reduced flags (2 B / (row, chan)).
// ---------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ float2 pick_corr(const float2 (&v)[NC], int c) {
    // register-resident select (a dynamic index would put the array in scratch)
    float2 r = v[0];
#pragma unroll
    for (int k = 1; k < NC; k++) r = (c == k) ? v[k] : r;
    return r;
}

template <int NC>
__device__ __forceinline__ void load_corrs(const float2* __restrict__ p, float2 (&v)[NC]) {
    if (NC == 4) {
        const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
        v[0] = make_float2(a.x, a.y); v[1 % NC] = make_float2(a.z, a.w);
        v[2 % NC] = make_float2(b.x, b.y); v[3 % NC] = make_float2(b.z, b.w);
    } else if (NC == 2) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        v[0] = make_float2(a.x, a.y); v[1 % NC] = make_float2(a.z, a.w);
    } else {
        v[0] = p[0];
    }
}

template <int NC>
__device__ __forceinline__ void load_flags(const uint8_t* __restrict__ p, uint8_t (&fl)[NC]) {
    if (NC == 4) {
        const uchar4 q = *reinterpret_cast<const uchar4*>(p);
        fl[0] = q.x; fl[1 % NC] = q.y; fl[2 % NC] = q.z; fl[3 % NC] = q.w;
    } else if (NC == 2) {
        const uchar2 q = *reinterpret_cast<const uchar2*>(p);
        fl[0] = q.x; fl[1 % NC] = q.y;
    } else {
        fl[0] = p[0];
    }
}

// One sample of the fused pack: the NC correlations at data / model / flag + i go to cell (bl, t, f) of the
// (nbl, wcorr, ntime, nchan) windows.  Shared by the whole-scan kernel and the row-list kernel.
template <int NC, bool STOKES, bool MODEL, bool FLAGS>
__device__ __forceinline__ void pack_scan_sample_v(const float2* __restrict__ data, const float2* __restrict__ model,
                                                   const uint8_t* __restrict__ flag, size_t i, int bl, int t, int f,
                                                   int nchan, int ntime, const StokesTerms& terms,
                                                   float2* __restrict__ vw, uint8_t* __restrict__ fw) {
    float2 v[NC];
    load_corrs<NC>(data + i, v);
    if (MODEL) {
        float2 m[NC];
        load_corrs<NC>(model + i, m);
#pragma unroll
        for (int c = 0; c < NC; c++) v[c] = make_float2(v[c].x - m[c].x, v[c].y - m[c].y);
    }
    uint8_t fl[NC];
    if (FLAGS) {
        load_flags<NC>(flag + i, fl);
    } else {
#pragma unroll
        for (int c = 0; c < NC; c++) fl[c] = 0;
    }
    if (STOKES) {
        const double res = stokes_intensity_sample(terms, 0, [&](int c) {
            const float2 x = pick_corr<NC>(v, c);
            return make_double2((double)x.x, (double)x.y);
        });
        uint8_t any = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) any |= fl[c];
        const size_t o = ((size_t)bl * ntime + t) * (size_t)nchan + f;
        vw[o] = make_float2((float)res, 0.0f);
        fw[o] = any ? 1 : 0;
    } else {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const size_t o = (((size_t)bl * NC + c) * ntime + t) * (size_t)nchan + f;
            vw[o] = v[c];
            fw[o] = fl[c];
        }
    }
}

// NC = 1, 2 or 4 with 16-byte aligned rows.  grid (ceil(nchan / 256), rows of the slab)
template <int NC, bool STOKES, bool MODEL, bool FLAGS>
__global__ void __launch_bounds__(256) k_pack_scan_v(const float2* __restrict__ data, const float2* __restrict__ model,
                                                     const uint8_t* __restrict__ flag, const int32_t* __restrict__ row_bl,
                                                     const int32_t* __restrict__ row_time, int nchan, int nbl, int ntime,
                                                     StokesTerms terms, float2* __restrict__ vw, uint8_t* __restrict__ fw) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t r = blockIdx.y;
    if (f >= nchan) return;
    const int bl = row_bl[r], t = row_time[r];
    if (bl < 0 || bl >= nbl || t < 0 || t >= ntime) return;
    pack_scan_sample_v<NC, STOKES, MODEL, FLAGS>(data, model, flag, (r * nchan + f) * (size_t)NC, bl, t, f, nchan, ntime,
                                                 terms, vw, fw);
}

// Row-list variant: entry e = e0 + blockIdx.y of a list reads source row src_row[e] (nullptr: e) of a
// (src_rows, nchan, NC) slab and scatters it to (row_bl[e], row_time[e]) of the windows.  The grid covers the list
// only: a baseline chunk of a scan launches its own rows, not every row of the scan.
template <int NC, bool STOKES, bool MODEL, bool FLAGS>
__global__ void __launch_bounds__(256) k_pack_scan_rows_v(const float2* __restrict__ data, const float2* __restrict__ model,
                                                          const uint8_t* __restrict__ flag, const int64_t* __restrict__ src_row,
                                                          int64_t src_rows, const int32_t* __restrict__ row_bl,
                                                          const int32_t* __restrict__ row_time, int64_t e0, int nchan,
                                                          int nbl, int ntime, StokesTerms terms, float2* __restrict__ vw,
                                                          uint8_t* __restrict__ fw) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e = e0 + blockIdx.y;
    if (f >= nchan) return;
    const int64_t r = src_row ? src_row[e] : e;
    const int bl = row_bl[e], t = row_time[e];
    if (r < 0 || r >= src_rows || bl < 0 || bl >= nbl || t < 0 || t >= ntime) return;
    pack_scan_sample_v<NC, STOKES, MODEL, FLAGS>(data, model, flag, ((size_t)r * nchan + f) * (size_t)NC, bl, t, f, nchan,
                                                 ntime, terms, vw, fw);
}

// any ncorr / alignment: correlations read one at a time
__device__ __forceinline__ void pack_scan_sample(const float2* __restrict__ data, const float2* __restrict__ model,
                                                 const uint8_t* __restrict__ flag, size_t i, int bl, int t, int f,
                                                 int nchan, int ncorr, int ntime, int stokes, const StokesTerms& terms,
                                                 float2* __restrict__ vw, uint8_t* __restrict__ fw) {
    auto resid = [&](int c) {
        const float2 d = data[i + c];
        if (!model) return d;
        const float2 m = model[i + c];
        return make_float2(d.x - m.x, d.y - m.y);
    };
    if (stokes) {
        const double res = stokes_intensity_sample(terms, 0, [&](int c) {
            const float2 x = resid(c);
            return make_double2((double)x.x, (double)x.y);
        });
        uint8_t any = 0;
        if (flag)
            for (int c = 0; c < ncorr; c++) any |= flag[i + c];
        const size_t o = ((size_t)bl * ntime + t) * (size_t)nchan + f;
        vw[o] = make_float2((float)res, 0.0f);
        fw[o] = any ? 1 : 0;
    } else {
        for (int c = 0; c < ncorr; c++) {
            const size_t o = (((size_t)bl * ncorr + c) * ntime + t) * (size_t)nchan + f;
            vw[o] = resid(c);
            fw[o] = flag ? flag[i + c] : 0;
        }
    }
}

__global__ void __launch_bounds__(256) k_pack_scan(const float2* __restrict__ data, const float2* __restrict__ model,
                                                   const uint8_t* __restrict__ flag, const int32_t* __restrict__ row_bl,
                                                   const int32_t* __restrict__ row_time, int nchan, int ncorr, int nbl,
                                                   int ntime, int stokes, StokesTerms terms, float2* __restrict__ vw,
                                                   uint8_t* __restrict__ fw) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t r = blockIdx.y;
    if (f >= nchan) return;
    const int bl = row_bl[r], t = row_time[r];
    if (bl < 0 || bl >= nbl || t < 0 || t >= ntime) return;
    pack_scan_sample(data, model, flag, (r * nchan + f) * (size_t)ncorr, bl, t, f, nchan, ncorr, ntime, stokes, terms,
                     vw, fw);
}

__global__ void __launch_bounds__(256) k_pack_scan_rows(const float2* __restrict__ data, const float2* __restrict__ model,
                                                        const uint8_t* __restrict__ flag, const int64_t* __restrict__ src_row,
                                                        int64_t src_rows, const int32_t* __restrict__ row_bl,
                                                        const int32_t* __restrict__ row_time, int64_t e0, int nchan,
                                                        int ncorr, int nbl, int ntime, int stokes, StokesTerms terms,
                                                        float2* __restrict__ vw, uint8_t* __restrict__ fw) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e = e0 + blockIdx.y;
    if (f >= nchan) return;
    const int64_t r = src_row ? src_row[e] : e;
    const int bl = row_bl[e], t = row_time[e];
    if (r < 0 || r >= src_rows || bl < 0 || bl >= nbl || t < 0 || t >= ntime) return;
    pack_scan_sample(data, model, flag, ((size_t)r * nchan + f) * (size_t)ncorr, bl, t, f, nchan, ncorr, ntime, stokes,
                     terms, vw, fw);
}

// ---------------------------------------------------------------------------
// Broadcast unpack.  One thread per (row, chan): any over the wcorr window correlations of the cell (each a
// load contiguous along chan across the wave), written to all OC output correlations (one OC-byte word).
// OC = 4: vector store; OC = 0: runtime out_ncorr.  Rows of no baseline get 0.
// ---------------------------------------------------------------------------
template <int OC>
__device__ __forceinline__ void unpack_scan_sample(const uint8_t* __restrict__ fw, int bl, int t, int f, int nchan,
                                                   int wcorr, int out_ncorr, int nbl, int ntime,
                                                   uint8_t* __restrict__ out_row) {
    uint8_t any = 0;
    if (!(bl < 0 || bl >= nbl || t < 0 || t >= ntime))
        for (int c = 0; c < wcorr; c++) any |= fw[(((size_t)bl * wcorr + c) * ntime + t) * (size_t)nchan + f];
    any = any ? 1 : 0;
    if (OC == 4) {
        *reinterpret_cast<uchar4*>(out_row + (size_t)f * 4) = make_uchar4(any, any, any, any);
    } else {
        for (int c = 0; c < out_ncorr; c++) out_row[(size_t)f * out_ncorr + c] = any;
    }
}

template <int OC>
__global__ void __launch_bounds__(256) k_unpack_scan(const uint8_t* __restrict__ fw, const int32_t* __restrict__ row_bl,
                                                     const int32_t* __restrict__ row_time, int nchan, int wcorr,
                                                     int out_ncorr, int nbl, int ntime, uint8_t* __restrict__ out) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t r = blockIdx.y;
    if (f >= nchan) return;
    unpack_scan_sample<OC>(fw, row_bl[r], row_time[r], f, nchan, wcorr, out_ncorr, nbl, ntime,
                           out + r * nchan * (size_t)(OC == 4 ? 4 : out_ncorr));
}

// Row-list variant: entry e = e0 + blockIdx.y writes destination row dst_row[e] (nullptr: e) of the
// (out_rows, nchan, out_ncorr) flags from cell (row_bl[e], row_time[e]); rows not in the list are not touched.
template <int OC>
__global__ void __launch_bounds__(256) k_unpack_scan_rows(const uint8_t* __restrict__ fw, const int64_t* __restrict__ dst_row,
                                                          int64_t out_rows, const int32_t* __restrict__ row_bl,
                                                          const int32_t* __restrict__ row_time, int64_t e0, int nchan,
                                                          int wcorr, int out_ncorr, int nbl, int ntime,
                                                          uint8_t* __restrict__ out) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e = e0 + blockIdx.y;
    if (f >= nchan) return;
    const int64_t r = dst_row ? dst_row[e] : e;
    if (r < 0 || r >= out_rows) return;
    unpack_scan_sample<OC>(fw, row_bl[e], row_time[e], f, nchan, wcorr, out_ncorr, nbl, ntime,
                           out + (size_t)r * nchan * (size_t)(OC == 4 ? 4 : out_ncorr));
}
