// tricolour_amd.hip -- host orchestration and C ABI of the MI355X SumThreshold flagger.
// The kernels live in the headers included below (one translation unit):
//   tri_common.hpp            overview, error plumbing, device helpers
//   kernels_elementwise.hpp   K1, K2, K5, K6, K8, pack / unpack, strategy steps
//   kernels_median.hpp        K3  exact medians
//   kernels_reject.hpp        K3r block median + rejection of the background loop in one pass (one workgroup per block; the redo path)
//   kernels_reject_tile.hpp   K3t the same, tile-parallel: predict / pass / finish
//   kernels_boxfilter.hpp     K4  box-Gaussian filter (four forms)
//   kernels_boxline.hpp / kernels_boxpipe.hpp   K4r register delay lines, K4p / K4q / K4qf stage pipelines
//   kernels_boxweight.hpp     K4w integer weight image of the time-axis stage (bit / byte / halfword-packed delay lines)
//   kernels_boxexact.hpp      K4x exact row filter for any radius (LDS-resident line, checked exactness)
//   kernels_sumthreshold.hpp  K7  fused SumThreshold
//   kernels_scan.hpp          fused scan pack (residual, Stokes, scatter) and broadcast unpack
//   kernels_sir.hpp           scale-invariant rank operator
//   kernels_linerms.hpp       line-RMS statistics and thresholding of whole timesteps / channels
#include <unordered_set>
#include "tri_common.hpp"
#include "kernels_elementwise.hpp"
#include "kernels_median.hpp"
#include "kernels_reject.hpp"
#include "kernels_reject_tile.hpp"
#include "kernels_boxfilter.hpp"
#include "kernels_boxline.hpp"
#include "kernels_boxpipe.hpp"
#include "kernels_boxweight.hpp"
#include "kernels_boxexact.hpp"
#include "kernels_sumthreshold.hpp"
#include "kernels_scan.hpp"
#include "kernels_sir.hpp"
#include "kernels_linerms.hpp"
#include "steps/kernels_blint.hpp"
#include "steps/ldev/kernels_ldev.hpp"
#include "steps/ins/kernels_ins.hpp"
#include "steps/hyst/kernels_hyst.hpp"
#include "steps/quality/kernels_quality.hpp"
#include "steps/hist/kernels_hist.hpp"
#include "steps/medz/kernels_medz.hpp"
#include "steps/antint/kernels_antint.hpp"
#include "steps/sk/kernels_sk.hpp"
#include "steps/polyfit/kernels_polyfit.hpp"

// ===========================================================================
// host side
// ===========================================================================
namespace {

// Opt-in to more than 64 KB of dynamic LDS for one kernel.  The attribute belongs to the (kernel, device) pair and a
// process may drive several devices (one calling thread per device): it is set once per calling thread, kernel
// and device -- not once per process -- and a transient failure is not cached.
static hipError_t lds_optin(const void* fn, hipFuncAttribute attr, int value) {
    thread_local std::unordered_set<uint64_t> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t key = (uint64_t)(uintptr_t)fn * 64u + (uint64_t)(dev & 63);
    if (done.count(key)) return hipSuccess;
    e = hipFuncSetAttribute(fn, attr, value);
    if (e == hipSuccess) done.insert(key);
    return e;
}

// a switch of the environment is on when its value starts with '1'
static inline bool is1(const char* e) { return e && e[0] == '1'; }

// ... for several kernels: stops at the first failure
template <class... K>
static hipError_t lds_optin_all(int bytes, K... kernels) {
    hipError_t e = hipSuccess;
    ((e = e != hipSuccess ? e : lds_optin(reinterpret_cast<const void*>(kernels), hipFuncAttributeMaxDynamicSharedMemorySize, bytes)), ...);
    return e;
}

struct Bump {
    char* base;
    size_t cap, off;
    bool dry;
    Bump(void* b, size_t c, bool d) : base((char*)b), cap(c), off(0), dry(d) {}
    template <typename T>
    T* get(size_t count) {
        size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
        size_t o = off;
        off += bytes;
        if (dry) return nullptr;
        return reinterpret_cast<T*>(base + o);
    }
};

// int(0.5 * sqrt(12 sigma^2 / passes + 1)), flagging.py:451
int64_t box_radius(double sigma) {
    return (int64_t)(0.5 * std::sqrt(12.0 * (sigma * sigma) / 4.0 + 1.0));
}

// float32(d) ** 4 as numba evaluates it: square-and-multiply in float32
// (numba cpython/numbers.py:207-245)
float box_denominator(int64_t r) {
    volatile float a = (float)(2 * r + 1);
    volatile float a2 = a * a;
    volatile float a4 = a2 * a2;
    volatile float res = 1.0f * a4;
    return res;
}

// RN(1 / b) for the reciprocal-based exact division of the register-ring filter kernels
// (box_divide): b and the candidates are 24-bit, so b * y is exact in float64 and the
// candidate closest to 1 / b is found without rounding.
BoxDenom box_reciprocal(float b) {
    float y = (float)(1.0 / (double)b);
    const float cand[3] = {std::nextafterf(y, 0.0f), y, std::nextafterf(y, INFINITY)};
    double best = INFINITY;
    for (float c : cand) {
        const double e = std::fabs(1.0 - (double)b * (double)c);
        if (e < best) { best = e; y = c; }
    }
    return BoxDenom{b, y};
}

struct Plan {
    int64_t T, F, Fa, avg, G;
    int64_t r0max, r1max;   // largest box radii along time / frequency
    int64_t PT, PF;         // padded line lengths
    int nit;                // background_iterations
    bool vec;               // 16-byte vectorised elementwise kernels usable
    int64_t maxchunk;       // longest frequency chunk (averaged channels)
    StWin swT, swF;
};

int make_stwin(const int64_t* w, int64_t nw, double rho, StWin* s) {
    memset(s, 0, sizeof(*s));
    if (nw <= 0) return set_err(TRI_EINVAL, "no SumThreshold window fits the data (np.max of an empty window list)");
    if (nw > TRI_MAX_WINDOWS) return set_err(TRI_EINVAL, "too many windows");
    s->nw = (int)nw;
    int off = 0, d = 0, maxw = 0;
    for (int j = 0; j < nw; j++) {
        if (w[j] <= 0) return set_err(TRI_EINVAL, "SumThreshold window of size %lld (the reference fails here with a broadcasting ValueError)", (long long)w[j]);
        s->w[j] = (int)w[j];
        s->tf[j] = std::pow(rho, std::log2((double)w[j]));
        s->scale[j] = (double)(float)(1.0 / (double)w[j]);
        s->ringoff[j] = off;
        off += (int)w[j];
        s->delay[j] = d;
        d += (int)w[j] - 1;
        maxw = std::max(maxw, (int)w[j]);
    }
    s->delay[nw] = d;
    s->ringtot = off;
    s->acccap = d + 1;
    s->maxw = maxw;
    return TRI_OK;
}

int make_plan(int64_t T, int64_t F, const tri_params* p, Plan* pl) {
    if (T <= 0 || F <= 0) return set_err(TRI_EINVAL, "empty window (ntime=%lld, nchan=%lld)", (long long)T, (long long)F);
    if (p->average_freq < 1 || p->average_freq > 255) return set_err(TRI_EUNSUPPORTED, "average_freq must be in [1, 255]");
    if (p->n_chunk_ends < 2 || !p->chunk_ends) return set_err(TRI_EINVAL, "freq_chunks must be >= 1");
    if (p->background_iterations < 0 || p->num_major_iterations < 0) return set_err(TRI_EINVAL, "negative iteration count");
    pl->T = T; pl->F = F; pl->avg = p->average_freq;
    pl->Fa = (F + pl->avg - 1) / pl->avg;
    pl->G = p->n_chunk_ends - 1;
    for (int64_t g = 0; g < p->n_chunk_ends; g++) {
        if (p->chunk_ends[g] < 0 || p->chunk_ends[g] > pl->Fa || (g > 0 && p->chunk_ends[g] < p->chunk_ends[g - 1]))
            return set_err(TRI_EINVAL, "freq chunk ends must be non-decreasing within [0, averaged channels]");
    }
    if (p->chunk_ends[0] != 0 || p->chunk_ends[pl->G] != pl->Fa) return set_err(TRI_EINVAL, "freq chunk ends must start at 0 and end at the averaged channel count");
    pl->nit = (int)p->background_iterations;
    pl->maxchunk = 0;
    for (int64_t g = 0; g + 1 < p->n_chunk_ends; g++) pl->maxchunk = std::max(pl->maxchunk, p->chunk_ends[g + 1] - p->chunk_ends[g]);
    pl->vec = (pl->avg == 1 && F % 16 == 0 && T % 4 == 0);
    int64_t emax = std::max<int64_t>(pl->nit, 1);
    pl->r0max = box_radius((double)emax * p->spike_width_time);
    pl->r1max = box_radius((double)emax * p->spike_width_freq);
    if (pl->r0max > (1 << 20) || pl->r1max > (1 << 20)) return set_err(TRI_EUNSUPPORTED, "spike width too large");
    pl->PT = T + 4 * pl->r0max;
    pl->PF = pl->Fa + 4 * pl->r1max;
    // with no major iteration the reference never looks at its window lists
    int rc = TRI_OK;
    memset(&pl->swT, 0, sizeof(pl->swT));
    memset(&pl->swF, 0, sizeof(pl->swF));
    if (p->num_major_iterations > 0) {
        rc = make_stwin(p->windows_time, p->n_windows_time, p->rho, &pl->swT);
        if (rc) return rc;
        rc = make_stwin(p->windows_freq, p->n_windows_freq, p->rho, &pl->swF);
        if (rc) return rc;
    }
    if (T * pl->Fa >= ((int64_t)1 << 31) || T * F >= ((int64_t)1 << 31))
        return set_err(TRI_EUNSUPPORTED, "a single window must hold fewer than 2^31 samples");
    return TRI_OK;
}

// Workspace carve-up for a batch of Wb windows.  `dry` only measures.
#define TRI_MAX_CHUNKS 255
struct ChunkTab {
    int n;                       // number of chunk ends
    int64_t ends[TRI_MAX_CHUNKS + 1];
};

struct Ws {
    // per-window images
    float *dataTF, *dataFT, *Aw, *Ao, *Bw, *Bo;
    uint8_t *iter, *flagsTF, *flagsFT, *bgfTF, *bgfFT, *tflTF, *fflFT, *fflTF, *comb, *dil;
    // Time-major residual as column panels, written by the final frequency stage (window stride T * Fa).  No memory of
    // its own: it lies over bgfTF | bgfFT | comb | dil, four byte images that are dead from the final pass's frequency
    // stage until the combine / dilate pass where it is used (IterStep::fused_resid, so Finish::FusedDilate: ws.comb is
    // never read and ws.dil is written after the last reader).
    float* residP;
    int *rowcnt, *colcnt;
    double* med;      // medians: max(Fa, T*G) per window
    // spectrum layout [Fa][Wb]
    float *sdata, *sw, *so, *sres;
    uint8_t *sflags, *sbgf, *sout, *srows;   // srows: sout as rows [Wb][Fa]
    uint16_t* nanmask;                       // cached-amplitude path: one NaN bit per sample, 16 samples per word
    int* itab;                               // segment table of the interpolation (K6p)
    float* srowsf;                           // spectrum residuals as rows [Wb][Fa] (median input)
    uint8_t* srowsu;                         // their flags as rows
    double* smed;     // [Wb][G]
    // SumThreshold scratch
    double* ring;
    uint8_t* acc;
    // small tables (device)
    int64_t* d_chunk_ends;   // G+1, averaged-channel units
    int64_t* d_tends;        // {0, T}
    int64_t *segC_start, *segC_len;   // chunk segments in line units
    int64_t *segB_start, *segB_len;   // chunk blocks of the FT layout (x T)
    int64_t *segT_start, *segT_len;   // the single segment [0, T)
    int* d_chunk_of;         // Fa
    size_t total;
};

static void carve(const Plan& pl, int64_t Wb, void* base, size_t cap, bool dry, Ws* ws) {
    Bump b(base, cap, dry);
    size_t W = (size_t)Wb, T = (size_t)pl.T, F = (size_t)pl.F, Fa = (size_t)pl.Fa, G = (size_t)pl.G;
    size_t N = T * Fa;
    // small tables first so that their addresses do not depend on the batch
    ws->d_chunk_ends = b.get<int64_t>(G + 1);
    ws->d_tends = b.get<int64_t>(2);
    ws->segC_start = b.get<int64_t>(G);
    ws->segC_len = b.get<int64_t>(G);
    ws->segB_start = b.get<int64_t>(G);
    ws->segB_len = b.get<int64_t>(G);
    ws->segT_start = b.get<int64_t>(1);
    ws->segT_len = b.get<int64_t>(1);
    ws->d_chunk_of = b.get<int>(Fa);
    ws->iter = b.get<uint8_t>(W * T * F);
    ws->dataTF = b.get<float>(W * N);
    ws->dataFT = b.get<float>(W * N);
    // time-axis scratch: the weight and the weight * data image of a window sit next to each other
    // (window stride 2 * PT * Fa), so one buffer descriptor of the fused frequency stage reaches both
    ws->Aw = b.get<float>(W * 2 * (size_t)pl.PT * Fa);
    ws->Ao = dry ? nullptr : ws->Aw + (size_t)pl.PT * Fa;
    ws->Bw = b.get<float>(W * (size_t)pl.PF * T);
    ws->Bo = b.get<float>(W * (size_t)pl.PF * T);
    ws->flagsTF = b.get<uint8_t>(W * N);
    ws->flagsFT = b.get<uint8_t>(W * N);
    ws->tflTF = b.get<uint8_t>(W * N);
    ws->fflFT = b.get<uint8_t>(W * N);
    ws->fflTF = b.get<uint8_t>(W * N);
    // (these four next to each other: together they hold ws->residP, T * F >= N)
    ws->bgfTF = b.get<uint8_t>(W * N);
    ws->bgfFT = b.get<uint8_t>(W * N);
    ws->comb = b.get<uint8_t>(W * N);
    ws->dil = b.get<uint8_t>(W * T * F);
    ws->residP = dry ? nullptr : reinterpret_cast<float*>(ws->bgfTF);
    ws->rowcnt = b.get<int>(W * T);
    ws->colcnt = b.get<int>(W * F);
    ws->nanmask = b.get<uint16_t>(W * N / 16 + 8);
    ws->itab = b.get<int>(3 * W * (size_t)cdiv(Fa, INTERP_SEG) * std::max<size_t>(T, 1));
    ws->med = b.get<double>(W * std::max(Fa, T * G));
    size_t PS = (size_t)pl.PF;  // spectrum padded length
    ws->sdata = b.get<float>(Fa * W);
    ws->sw = b.get<float>(PS * W);
    ws->so = b.get<float>(PS * W);
    ws->sres = b.get<float>(Fa * W);
    ws->sflags = b.get<uint8_t>(Fa * W);
    ws->sbgf = b.get<uint8_t>(Fa * W);
    ws->sout = b.get<uint8_t>(Fa * W);
    ws->srows = b.get<uint8_t>(Fa * W);
    ws->srowsf = b.get<float>(Fa * W);
    ws->srowsu = b.get<uint8_t>(Fa * W);
    ws->smed = b.get<double>(W * G);
    // SumThreshold scratch: one slot set per (window, chunk, column) thread
    size_t thrT = W * Fa, thrF = W * T * G;
    size_t ringn = std::max(thrT * (size_t)pl.swT.ringtot, thrF * (size_t)pl.swF.ringtot);
    size_t accn = std::max(thrT * (size_t)pl.swT.acccap, thrF * (size_t)pl.swF.acccap);
    ws->ring = b.get<double>(ringn);
    ws->acc = b.get<uint8_t>(accn);
    ws->total = b.off;
}

static inline dim3 grid1(size_t n, size_t W) { return dim3((unsigned)cdiv((int64_t)n, 256), (unsigned)W, 1); }

}  // namespace

__global__ void k_tables(ChunkTab ct, int T, int Fa, int64_t* chunk_ends, int64_t* tends,
                         int64_t* segC_start, int64_t* segC_len, int64_t* segB_start,
                         int64_t* segB_len, int64_t* segT_start, int64_t* segT_len,
                         int* chunk_of) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int G = ct.n - 1;
    if (i <= G) chunk_ends[i] = ct.ends[i];
    if (i < G) {
        segC_start[i] = ct.ends[i];
        segC_len[i] = ct.ends[i + 1] - ct.ends[i];
        segB_start[i] = ct.ends[i] * T;
        segB_len[i] = (ct.ends[i + 1] - ct.ends[i]) * T;
    }
    if (i == 0) { tends[0] = 0; tends[1] = T; segT_start[0] = 0; segT_len[0] = T; }
    if (i < Fa) {
        int g = 0;
        // chunk containing channel i: ends[g] <= i < ends[g+1] (skips empty chunks)
        while (g < G - 1 && !(i >= ct.ends[g] && i < ct.ends[g + 1])) g++;
        chunk_of[i] = g;
    }
}

// copies column `col` of a [L][C] array into a contiguous vector (debug taps)
__global__ void k_gather_col_f32(const float* __restrict__ a, float* __restrict__ out, int L, int C, int col) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < L) out[i] = a[(size_t)i * C + col];
}
__global__ void k_gather_col_u8(const uint8_t* __restrict__ a, uint8_t* __restrict__ out, int L, int C, int col) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < L) out[i] = a[(size_t)i * C + col];
}
__global__ void k_normalise_flags(const uint8_t* __restrict__ a, uint8_t* __restrict__ b, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[i] = a[i] ? 1 : 0;
}

extern "C" size_t tri_workspace_bytes(int64_t batch_windows, int64_t ntime, int64_t nchan,
                                      const tri_params* p) {
    Plan pl;
    if (!p || batch_windows <= 0 || make_plan(ntime, nchan, p, &pl) != TRI_OK) return 0;
    Ws ws;
    carve(pl, batch_windows, nullptr, 0, true, &ws);
    return ws.total;
}

extern "C" int tri_prepare_params(int64_t ntime, int64_t nchan, double outlier_nsigma,
                                  const double* windows_time, int64_t n_windows_time,
                                  const double* windows_freq, int64_t n_windows_freq,
                                  double background_reject, int64_t background_iterations,
                                  double spike_width_time, double spike_width_freq,
                                  int64_t time_extend, int64_t freq_extend, int64_t freq_chunks,
                                  int64_t average_freq, double flag_all_time_frac,
                                  double flag_all_freq_frac, double rho,
                                  int64_t num_major_iterations, int64_t* chunk_ends_buf,
                                  int64_t chunk_cap, tri_params* out) {
    if (!out || !chunk_ends_buf) return set_err(TRI_EINVAL, "NULL output");
    if (ntime <= 0 || nchan <= 0) return set_err(TRI_EINVAL, "empty window");
    if (average_freq < 1) return set_err(TRI_EINVAL, "average_freq must be >= 1");
    if (freq_chunks < 1) return set_err(TRI_EINVAL, "freq_chunks must be >= 1");
    if (chunk_cap < freq_chunks + 1) return set_err(TRI_EINVAL, "chunk_ends_buf too small");
    if (n_windows_time > TRI_MAX_WINDOWS || n_windows_freq > TRI_MAX_WINDOWS || n_windows_time < 0 || n_windows_freq < 0)
        return set_err(TRI_EINVAL, "at most %d windows per axis", TRI_MAX_WINDOWS);
    memset(out, 0, sizeof(*out));
    int64_t fa = (nchan + average_freq - 1) / average_freq;
    // flagging.py:1160-1162: float32 ceil, float32 division, truncation, unique
    std::vector<int64_t> wf;
    for (int64_t i = 0; i < n_windows_freq; i++) {
        float v = std::ceil((float)windows_freq[i]) / (float)average_freq;
        wf.push_back((int64_t)v);
    }
    std::sort(wf.begin(), wf.end());
    wf.erase(std::unique(wf.begin(), wf.end()), wf.end());
    // flagging.py:1172-1173: linspace(0, fa, freq_chunks + 1).astype(int)
    double step = (double)fa / (double)freq_chunks;
    for (int64_t i = 0; i <= freq_chunks; i++) chunk_ends_buf[i] = (int64_t)((double)i * step);
    chunk_ends_buf[freq_chunks] = fa;
    // flagging.py:1176-1179
    out->n_windows_time = 0;
    for (int64_t i = 0; i < n_windows_time; i++)
        if (windows_time[i] <= (double)ntime) out->windows_time[out->n_windows_time++] = (int64_t)windows_time[i];
    out->n_windows_freq = 0;
    for (size_t i = 0; i < wf.size(); i++)
        if (wf[i] <= fa) out->windows_freq[out->n_windows_freq++] = wf[i];
    for (int64_t i = 0; i < out->n_windows_freq; i++)
        if (out->windows_freq[i] <= 0)
            return set_err(TRI_EINVAL, "windows_freq / average_freq produced a window of size %lld; the reference fails here (operands could not be broadcast together, flagging.py:663)", (long long)out->windows_freq[i]);
    for (int64_t i = 0; i < out->n_windows_time; i++)
        if (out->windows_time[i] <= 0) return set_err(TRI_EINVAL, "windows_time must be positive");
    out->outlier_nsigma = outlier_nsigma;
    out->background_reject = background_reject;
    out->background_iterations = background_iterations;
    out->spike_width_time = spike_width_time;
    out->spike_width_freq = spike_width_freq;
    out->time_extend = time_extend;
    out->freq_extend = freq_extend;
    out->n_chunk_ends = freq_chunks + 1;
    out->chunk_ends = chunk_ends_buf;
    out->average_freq = average_freq;
    out->flag_all_time_frac = flag_all_time_frac;
    out->flag_all_freq_frac = flag_all_freq_frac;
    out->rho = rho;
    out->num_major_iterations = num_major_iterations;
    return TRI_OK;
}

namespace {

struct Debug {
    float* f32;     // [spec_resid Fa][background FT Fa*T][residual TF T*Fa]
    uint8_t* u8;    // [spec_flags Fa][time_flags TF][freq_flags TF]
};

// The side lane of a calling thread: two launches that share nothing but read-only inputs go to two streams of equal
// priority and run side by side.  That pays where two thin stream kernels meet (the write-bound k_boxw beside the read-heavier
// k_boxt); beside a stage pipeline the pair takes what it took in series.
struct SideLane {
    hipStream_t st = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    int device = -1;
};

// The route switches of the box-filter family (boxfilter_host.hpp) as one value.  The flagger runs with from_env();
// tri_bench_boxfilter builds its own for the variant it was asked for.  The picks are functions of it: nothing else steers them.
#ifndef BOXQF_B8_DEFAULT
#define BOXQF_B8_DEFAULT 1               // K4qf: blocks of 8 positions unless TRI_FILTER_PIPE_F_B8=0
#endif
enum class Want { Off, Auto, Forced };        // Auto: where the measured crossovers say so; Forced: wherever the shape allows
enum class SpecPipe { Off, B8, B16, Auto };     // B8 / B16: blocks of that length only
struct BoxRoutes {
    bool reg_rings = true, reg_rings_f = true;        // K4r: register delay lines (else the LDS-ring kernels); _f: in the fused frequency stage
    bool boxw = true;                                 // K4w: the time stage's weight image in integer arithmetic
    SpecPipe spec_pipe = SpecPipe::Auto;              // K4p: stage pipeline of the spectra
    Want pipe_t = Want::Auto, pipe_f = Want::Auto;    // K4q / K4qf: stage pipeline of the time stage / of the fused frequency stage ...
    bool pipe_t_b8 = true, pipe_f_b8 = BOXQF_B8_DEFAULT;         // ... with blocks of 8 positions where they exist
    Want exact = Want::Auto;                          // K4x: exact rows ...
    int exact_nti = 0;                                // ... only the instantiations with this many threads per image (128 / 256), 0 = any
    bool lane4 = true, multipass = false;             // K4c: lane per stage; the in-place multi-pass kernel (K4) for every radius
    bool t_in = true, fused_div = true;               // frequency stages that read the TF images directly; ... fused with the masked division
    bool unpadded = false;                            // the images are the caller's, n rows each, without the n + 4r rows K4 works in: it is refused

    // What the environment asks for, read once per process (A/B runs, tests)
    static const BoxRoutes& from_env() {
        static const BoxRoutes env = [] {
            BoxRoutes b;
            b.reg_rings = !is1(getenv("TRI_FILTER_NO_REGRING"));
            b.reg_rings_f = !is1(getenv("TRI_FILTER_NO_REGRING_F"));
            b.boxw = !is1(getenv("TRI_FILTER_NO_BOXW"));
            b.spec_pipe = is1(getenv("TRI_SPEC_NO_PIPE")) ? SpecPipe::Off : SpecPipe::Auto;
            b.pipe_t = is1(getenv("TRI_FILTER_NO_PIPE_T")) ? Want::Off : Want::Auto;
            // (both stages take their register slots from the time stage's pick: without it the frequency stage has no pipeline either)
            b.pipe_f = (is1(getenv("TRI_FILTER_NO_PIPE_F")) || b.pipe_t == Want::Off) ? Want::Off : Want::Auto;
            if (const char* e = getenv("TRI_FILTER_PIPE_T_B8")) b.pipe_t_b8 = atoi(e) != 0;
            if (const char* e = getenv("TRI_FILTER_PIPE_F_B8")) b.pipe_f_b8 = atoi(e) != 0;
            b.exact = is1(getenv("TRI_FILTER_NO_EXACT")) ? Want::Off : Want::Auto;
            if (const char* e = getenv("TRI_BOXX_NTI")) b.exact_nti = atoi(e);
            b.lane4 = !is1(getenv("TRI_FILTER_NO_LANE4"));
            b.multipass = is1(getenv("TRI_FILTER_MULTIPASS"));
            b.t_in = !is1(getenv("TRI_FILTER_NO_TIN"));
            b.fused_div = !is1(getenv("TRI_FILTER_NO_FUSED_DIV"));
            return b;
        }();
        return env;
    }
};

struct Run {
    BoxRoutes box = BoxRoutes::from_env();
    hipStream_t st;
    Plan pl;
    Ws ws;
    const tri_params* p;
    int64_t Wb;      // windows in this batch
    Debug* dbg;      // taps of window 0 (tests only), or NULL
    // true: ws.dataTF holds the batch's UNMASKED amplitudes, computed once (k_amplitude4,
    // NaNs folded into the running flags; the time-axis filter masks by its own flags),
    // ws.dataFT their transpose, masked in place every iteration (the flags only grow)
    bool ampl_cached = false;
    // the running flags (ws.iter: every iteration's input flags, in TF layout when nothing is averaged) while ws.dataTF is
    // unmasked (K4x masks its data row with them: data is zero where the iteration's _average_freq flagged it,
    // flagging.py:858-870), else NULL.  Set once per process_windows() call, beside ampl_cached.
    const uint8_t* data_mask = nullptr;
    size_t data_mask_ws = 0;
    // one extra stream for a launch that is independent of the next one on st (get_side_lane()), or NULL: single-stream order
    const SideLane* side = nullptr;
};

// Which sites fork (compile-time: the runtime switch is TRI_SUBSTREAMS=0, which takes the side lane away altogether)
#ifndef OVERLAP_TIME_STAGE
#define OVERLAP_TIME_STAGE 2             // weight image beside data image: 0 = never, 1 = beside k_boxq / k_boxq_deep, 2 = beside k_boxt too
#endif                                   // (1008-window step, profiles/overlap_ab.txt: 2 saves 15 - 19 ms, 1 nothing -- the gain is at the k_boxt radii)
#ifndef OVERLAP_RESID_MEDIANS
#define OVERLAP_RESID_MEDIANS 1          // time medians of the residual beside its transpose (9 - 11 ms; both sites together 23 - 26 ms)
#endif

// Everything queued on r.st so far happens before what is launched through the returned Run, whose st is the side stream.
// Without a side lane (or when an event call fails) the returned Run is r itself: the launches stay in order on r.st.
static Run fork(const Run& r) {
    Run f = r;
    f.side = nullptr;
    if (!r.side) return f;
    if (hipEventRecord(r.side->fork, r.st) != hipSuccess || hipStreamWaitEvent(r.side->st, r.side->fork, 0) != hipSuccess) {
        (void)hipGetLastError();
        return f;
    }
    f.st = r.side->st;
    return f;
}
// Everything queued on the side stream so far happens before what is launched on r.st from here on.  Called on every way
// out of a forked region: r.st never runs ahead of queued side work.
static void join(const Run& r) {
    if (!r.side) return;
    (void)hipEventRecord(r.side->join, r.side->st);
    (void)hipStreamWaitEvent(r.st, r.side->join, 0);
}

// The register cascade covers windows exactly (1,2,4,8) in that order; the
// environment variable TRI_ST_GENERIC=1 forces the generic kernel (tests).
bool st_use_fused(const StWin& sw) {
    static const bool force_generic = is1(getenv("TRI_ST_GENERIC"));
    if (force_generic) return false;
    return sw.nw == 4 && sw.w[0] == 1 && sw.w[1] == 2 && sw.w[2] == 4 && sw.w[3] == 8;
}

// The lane-mask cascade (K7c) addresses a window through signed 32-bit buffer
// offsets (windows below 2 GiB of float32); larger windows and TRI_ST_REGISTER=1 (tests) take the register
// cascade (K7b).
bool st_use_mask(int L, int C) {
    static const bool force_register = is1(getenv("TRI_ST_REGISTER"));
    return !force_register && (uint64_t)L * (uint64_t)C * 4u < (1ull << 31);   // signed 32-bit scalar offsets
}

// TRI_MEDIAN_NO_PREDICT=1: the two-pass medians read their segments twice, without the predicted-window candidates (A/B runs, tests)
static bool median_no_predict() { static const bool v = is1(getenv("TRI_MEDIAN_NO_PREDICT")); return v; }

// launch_median() can OR a second flag image and per-column flags into the flags it reads when the segments fit the wave kernels
static bool median_takes_extra_flags(int64_t max_len) { return max_len <= 64 * MW_K; }

// One segmented-median job: exact medians of |data| over the unflagged samples of each segment
// [seg_start[g], + seg_len[g]) of each of R rows, in each of W windows; med[w][row][g].
struct MedianJob {
    const float* data = nullptr; const uint8_t* flags = nullptr; double* med = nullptr;
    size_t WSd = 0, WSf = 0, RS = 0, ES = 1;    // window strides of data and flags, row stride, element stride
    const int64_t* seg_start = nullptr; const int64_t* seg_len = nullptr;
    int R = 0, G = 0;                           // rows, segments per row
    int64_t W = 0, max_len = 0;                 // windows, longest segment
    bool vec_ok = false;                        // segments contiguous, 16-byte aligned, a multiple of 4 long
    bool rows_aligned = false;                  // rows 4-aligned
    bool segs_aligned = false;                  // segment starts 4-aligned (no masked slots ahead of a segment)
    // wave kernels: a second flag image and per-column flags (WScol bytes per window) OR-ed in; data / flags2 as column panels
    const uint8_t* flags2 = nullptr; const uint8_t* colflags = nullptr; size_t WScol = 0; int panel_rows = 0;
    // two-pass kernel: candidate scratch, cand_ws keys per window, cand_cap per segment
    unsigned* gcand = nullptr; size_t cand_ws = 0; unsigned cand_cap = 0;
};

// The segmented-median kernels (kernels_median.hpp)
enum class MedianKernel {
    Wave8, Wave8Vec,            // k_median_wave<8, VEC>: segments of at most 512
    Wave16, Wave16Vec,          // k_median_wave<MW_K, VEC>: at most 1024
    Select, SelectVec,          // k_median<VEC>: three-pass select
    TwoPass, TwoPassVec,        // k_median2<VEC>: two-pass select (K3c)
    TwoPassVecLong,             // k_median2<true, false, 16>: sixteen 16-byte groups in flight per thread
};

template <int KS, bool VEC, int SPW>
static void median_wave(hipStream_t st, const MedianJob& j) {
    hipLaunchKernelGGL((k_median_wave<KS, VEC, SPW>), dim3((unsigned)cdiv((int64_t)cdiv((int64_t)j.R, SPW) * j.G, 4), (unsigned)j.W),
                       dim3(256), 0, st, j.data, j.flags, j.med, j.WSd, j.WSf, j.RS, j.ES, j.seg_start, j.seg_len, j.R, j.G,
                       j.flags2, j.colflags, j.WScol, j.panel_rows);
}
template <bool VEC>
static void median_select(hipStream_t st, const MedianJob& j) {
    hipLaunchKernelGGL(k_median<VEC>, dim3((unsigned)(j.R * j.G), (unsigned)j.W), dim3(256), 0, st,
                       j.data, j.flags, j.med, j.WSd, j.WSf, j.RS, j.ES, j.seg_start, j.seg_len, j.R, j.G);
}
template <bool VEC, int UNR = MED2_UNROLL>
static void median_two_pass(hipStream_t st, const MedianJob& j) {
    hipLaunchKernelGGL((k_median2<VEC, false, UNR>), dim3((unsigned)(j.R * j.G), (unsigned)j.W), dim3(256), 0, st,
                       j.data, j.flags, j.med, j.WSd, j.WSf, j.RS, j.ES, j.seg_start, j.seg_len, j.R, j.G, j.gcand, j.cand_ws, j.cand_cap);
}

// Launches kernel `k` on job `j` (the flagger's launch_median and the test hook tri_test_median); the caller checks the launch.
// The wave kernels take MW_SPW (8 slots) / MW_SPW16 (16 slots) rows of a segment per wave, one segment with seg_per_wave.
static void launch_median_kernel(hipStream_t st, MedianKernel k, bool seg_per_wave, const MedianJob& j) {
    switch (k) {
    case MedianKernel::Wave8: seg_per_wave ? median_wave<8, false, 1>(st, j) : median_wave<8, false, MW_SPW>(st, j); break;
    case MedianKernel::Wave8Vec: seg_per_wave ? median_wave<8, true, 1>(st, j) : median_wave<8, true, MW_SPW>(st, j); break;
    case MedianKernel::Wave16: seg_per_wave ? median_wave<MW_K, false, 1>(st, j) : median_wave<MW_K, false, MW_SPW16>(st, j); break;
    case MedianKernel::Wave16Vec: seg_per_wave ? median_wave<MW_K, true, 1>(st, j) : median_wave<MW_K, true, MW_SPW16>(st, j); break;
    case MedianKernel::Select: median_select<false>(st, j); break;
    case MedianKernel::SelectVec: median_select<true>(st, j); break;
    case MedianKernel::TwoPass: median_two_pass<false>(st, j); break;
    case MedianKernel::TwoPassVec: median_two_pass<true>(st, j); break;
    case MedianKernel::TwoPassVecLong: median_two_pass<true, 16>(st, j); break;
    }
}

// The flagger's segmented medians: the kernel that fits the job, launched on the run's stream.
int launch_median(const Run& r, MedianJob j) {
    const int R = j.R, G = j.G;
    const int64_t W = j.W, max_len = j.max_len;
    if ((int64_t)R * G <= 0 || W <= 0) return TRI_OK;
    // (data / flags2 as column panels: only the 16-byte wave kernels read them)
    if (j.panel_rows > 0 && !(j.ES == 1 && j.RS % 64 == 0 && j.rows_aligned && max_len + (j.segs_aligned ? 0 : 3) <= 64 * MW_K &&
                              j.WSd % 4 == 0 && j.WSf % 4 == 0 && ((uintptr_t)j.data % 16 == 0) && ((uintptr_t)j.flags % 4 == 0)))
        return set_err(TRI_EUNSUPPORTED, "panel images need wave-sized segments of 64-column aligned rows");
    // (extra flag sources: the wave kernels only -- see median_takes_extra_flags())
    if ((j.flags2 || j.colflags) && (max_len > 64 * MW_K || (j.colflags && j.ES != 1) || ((uintptr_t)j.flags2 % 4 != 0) ||
                                     ((uintptr_t)j.colflags % 4 != 0) || j.WScol % 4 != 0))
        return set_err(TRI_EUNSUPPORTED, "extra flag sources need wave-sized segments of contiguous, 4-byte aligned rows");
    if ((int64_t)R * G > 0x7FFFFFFF || W > 65535) return set_err(TRI_EUNSUPPORTED, "median grid too large");
    // segments of contiguous 4-aligned rows can be loaded 16 bytes at a time
    // (misaligned segment ends are masked, costing up to 3 extra slots)
    // (the 16-byte wave kernels address a window's image through 32-bit buffer offsets: below 4 GB)
    const bool row4 = j.ES == 1 && j.RS % 4 == 0 && j.WSd % 4 == 0 && j.WSf % 4 == 0 &&
                      ((uintptr_t)j.data % 16 == 0) && ((uintptr_t)j.flags % 4 == 0) && j.rows_aligned &&
                      (uint64_t)j.RS * (uint64_t)std::max(R, j.panel_rows) * 4u < (1ull << 32);
    if (j.panel_rows > 0 && !row4) return set_err(TRI_EUNSUPPORTED, "panel images of 4 GB or more per window");
    const int64_t slack = j.segs_aligned ? 0 : 3;   // misaligned segment starts cost up to 3 masked slots
    // wave medians: MW_SPW rows of a segment per wave, the next row's loads in flight (round 4; TRI_MEDIAN_WAVE_OLD=1: one segment per wave)
    static const bool wave_old = is1(getenv("TRI_MEDIAN_WAVE_OLD"));
    MedianKernel k;
    if (max_len + slack <= 64 * 8 && row4) k = MedianKernel::Wave8Vec;
    else if (max_len <= 64 * 8 && j.panel_rows == 0) k = MedianKernel::Wave8;     // (panel images: the 16-byte kernels only)
    else if (max_len + slack <= 64 * MW_K && row4) k = MedianKernel::Wave16Vec;
    else if (max_len <= 64 * MW_K) k = MedianKernel::Wave16;
    else {
        // long segments: two-pass select (K3c); TRI_MEDIAN_3PASS=1 keeps the three-pass kernel (A/B runs, tests)
        static const bool three = is1(getenv("TRI_MEDIAN_3PASS"));
        if (three) k = j.vec_ok ? MedianKernel::SelectVec : MedianKernel::Select;
        else {
            // scratch for the predicted-window candidates (K3c): one read of the segment instead of two
            if (median_no_predict() || j.cand_cap < max_len || j.cand_ws % 4 != 0 || j.cand_cap % 4 != 0 || ((uintptr_t)j.gcand % 16 != 0)) {
                j.gcand = nullptr; j.cand_ws = 0; j.cand_cap = 0;
            }
            // few, long segments (fewer workgroups than the machine holds at six per CU): sixteen 16-byte groups in flight per thread
            if ((j.vec_ok || row4) && (int64_t)R * G * W < 1536 && max_len >= (int64_t)1 << 20) k = MedianKernel::TwoPassVecLong;
            else k = (j.vec_ok || row4) ? MedianKernel::TwoPassVec : MedianKernel::TwoPass;
        }
    }
    launch_median_kernel(r.st, k, wave_old, j);
    LAUNCHCHK();
    return TRI_OK;
}

#include "boxfilter_host.hpp"

// K7p applies: up to eight windows whose flag-byte ring fits the CU's LDS (there are no prefix rings any more)
// (TRI_ST_NO_PIPE=1 keeps the global-scratch kernel)
bool st_use_pipe(const StWin& sw) {
    static const bool off = is1(getenv("TRI_ST_NO_PIPE"));
    return !off && sw.nw >= 1 && sw.nw <= 8 && stp_lds_bytes(sw) <= 160 * 1024;
}

// The SumThreshold kernels (kernels_sumthreshold.hpp): k_colst_dyn (any windows), k_colst_fused (register cascade),
// k_colst_mask (lane-mask cascade) on rows or on 64-column panels, k_colst_pipe (up to eight windows, K7p)
enum class StKernel { Dyn, Fused, Mask, MaskPanel, Pipe };

// Launches SumThreshold kernel `k` over the [L][C] images of W windows, G line groups each (the flagger's launch_colst and
// the measurement hook tri_bench_sumthreshold).  ring / acc: the scratch of k_colst_dyn.
int st_launch(hipStream_t st, StKernel k, const StWin& sw, const float* data, const double* med, uint8_t* out,
              const int64_t* d_chunk_ends, double thr_scale, int L, int C, int G, size_t ws_data, size_t ws_out, int64_t W,
              double* ring, uint8_t* acc) {
    int blk = C >= 256 ? 256 : (C >= 128 ? 128 : 64);
    if (const char* e = getenv("TRI_ST_BLK")) { int b = atoi(e); if (b >= 64 && b <= ST_MAXBLK && C >= b) blk = b; }
    const dim3 grid((unsigned)cdiv(C, blk), (unsigned)G, (unsigned)W);
    StFusedArgs fa;
    for (int j = 0; j < 4; j++) fa.tf[j] = sw.tf[j < sw.nw ? j : 0];
    if (k == StKernel::MaskPanel)
        hipLaunchKernelGGL((k_colst_mask<1, 2, 4, 8, true>), grid, dim3(blk), 0, st, data, med, out, d_chunk_ends, fa, thr_scale, L, C, G, ws_data, ws_out);
    else if (k == StKernel::Mask)
        hipLaunchKernelGGL((k_colst_mask<1, 2, 4, 8>), grid, dim3(blk), 0, st, data, med, out, d_chunk_ends, fa, thr_scale, L, C, G, ws_data, ws_out);
    else if (k == StKernel::Fused)
        hipLaunchKernelGGL((k_colst_fused<1, 2, 4, 8>), grid, dim3(blk), 0, st, data, med, out, d_chunk_ends, fa, thr_scale, L, C, G, ws_data, ws_out);
    else if (k == StKernel::Pipe) {
        HIPCHK(lds_optin_all(160 * 1024, &k_colst_pipe));
        hipLaunchKernelGGL(k_colst_pipe, dim3((unsigned)cdiv(C, 64), (unsigned)G, (unsigned)W), dim3(64 * sw.nw), stp_lds_bytes(sw), st,
                           data, med, out, d_chunk_ends, sw, stp_plan(sw), thr_scale, L, C, G, ws_data, ws_out);
    } else
        hipLaunchKernelGGL(k_colst_dyn, grid, dim3(blk), 0, st, data, med, out, ring, acc, d_chunk_ends, sw, thr_scale, L, C, G, ws_data, ws_out);
    LAUNCHCHK();
    return TRI_OK;
}

int launch_colst(const Run& r, const StWin& sw, const float* data, const double* med,
                 uint8_t* out, const int64_t* d_chunk_ends, int L, int C, int G, size_t ws_data,
                 size_t ws_out, int64_t W, bool panel = false) {
    StKernel k;
    if (st_use_fused(sw)) {
        if (panel && !(st_use_mask(L, C) && C % 64 == 0)) return set_err(TRI_EUNSUPPORTED, "panel images: lane-mask SumThreshold kernel on 64-column panels only");
        k = panel ? StKernel::MaskPanel : (st_use_mask(L, C) ? StKernel::Mask : StKernel::Fused);
    } else if (panel) {
        return set_err(TRI_EUNSUPPORTED, "panel images: windows (1, 2, 4, 8) only");
    } else {
        // any list of up to eight windows: one window per wave, lagging twin accumulators (K7p)
        k = st_use_pipe(sw) ? StKernel::Pipe : StKernel::Dyn;
    }
    const double thr_scale = r.p->outlier_nsigma * TRI_MAD_NORMAL;  // flagging.py:623
    return st_launch(r.st, k, sw, data, med, out, d_chunk_ends, thr_scale, L, C, G, ws_data, ws_out, W, r.ws.ring, r.ws.acc);
}

// _linearly_interpolate_nans1d along the line axis of [L][C] images (K6 / K6p)
int launch_interp(const Run& r, float* a, int L, int C, size_t ws, int64_t W, const uint8_t* nanflag,
                  const float* data, size_t ws_data, float* resid, float* panel = nullptr, size_t ws_panel = 0) {
    static const bool one_pass = is1(getenv("TRI_INTERP_ONE_PASS"));
    const int nseg = (int)cdiv(L, INTERP_SEG);
    if (one_pass || nseg < 2 || nseg > 65535) {
        hipLaunchKernelGGL(k_colinterp, dim3((unsigned)cdiv(C, 256), (unsigned)W), dim3(256), 0, r.st, a, L, C, ws, nanflag, data, ws_data, resid, panel, ws_panel);
    } else {
        dim3 grid((unsigned)cdiv(C, 64), (unsigned)nseg, (unsigned)W);
        hipLaunchKernelGGL(k_interp_scan, grid, dim3(64), 0, r.st, (const float*)a, L, C, ws, nanflag, r.ws.itab);
        hipLaunchKernelGGL(k_interp_fix, grid, dim3(64), 0, r.st, a, L, C, ws, (const int*)r.ws.itab, data, ws_data, resid, panel, ws_panel);
    }
    LAUNCHCHK();
    return TRI_OK;
}

template <typename T>
int launch_transpose(const Run& r, const T* src, T* dst, int R, int C, size_t sws, size_t dws,
                     int64_t W, float denom = 0.0f, bool panel = false) {
    dim3 grid((unsigned)cdiv(C, 64), (unsigned)cdiv(R, 64), (unsigned)W);
    if (panel) {
        if (R % 64 != 0) return set_err(TRI_EUNSUPPORTED, "panel output needs a multiple of 64 columns");
        hipLaunchKernelGGL((k_transpose<T, true>), grid, dim3(64, 4), 0, r.st, src, dst, R, C, sws, dws, denom);
        LAUNCHCHK();
        return TRI_OK;
    }
    if (sizeof(T) == 1 && R % 4 == 0 && C % 4 == 0 && sws % 4 == 0 && dws % 4 == 0 &&
        ((uintptr_t)src % 4 == 0) && ((uintptr_t)dst % 4 == 0)) {
        dim3 gridw((unsigned)cdiv(C, 64), (unsigned)cdiv(R, 128), (unsigned)W);
        hipLaunchKernelGGL((k_transpose_u8w<false, false>), gridw, dim3(256), 0, r.st, (const uint8_t*)src, (uint8_t*)dst,
                           (uint8_t*)nullptr, (float*)nullptr, R, C, sws, dws, (size_t)0, (size_t)0);
        LAUNCHCHK();
        return TRI_OK;
    }
    hipLaunchKernelGGL(k_transpose<T>, grid, dim3(64, 4), 0, r.st, src, dst, R, C, sws, dws, denom);
    LAUNCHCHK();
    return TRI_OK;
}


// ---- elementwise launch helpers (vector path when the plan allows) ----------
template <int OP>
int launch_u8(const Run& r, const uint8_t* a, uint8_t* b, size_t nper, size_t ws_a, size_t ws_b, int64_t W) {
    if (r.pl.vec && nper % 16 == 0 && ws_a % 16 == 0 && ws_b % 16 == 0) {
        hipLaunchKernelGGL(k_u8_op16<OP>, grid1(nper / 16, W), dim3(256), 0, r.st, a, b, nper / 16, ws_a, ws_b);
    } else if (OP == 0) {
        for (int64_t w = 0; w < W; w++)
            hipLaunchKernelGGL(k_copy_u8, dim3((unsigned)cdiv(nper, 256)), dim3(256), 0, r.st, a + w * ws_a, b + w * ws_b, nper);
    } else if (OP == 1) {
        hipLaunchKernelGGL(k_or, grid1(nper, W), dim3(256), 0, r.st, b, a, nper, ws_b, ws_a);
    } else {
        for (int64_t w = 0; w < W; w++)
            hipLaunchKernelGGL(k_normalise_flags, dim3((unsigned)cdiv(nper, 256)), dim3(256), 0, r.st, a + w * ws_a, b + w * ws_b, nper);
    }
    LAUNCHCHK();
    return TRI_OK;
}

template <int MODE>
int launch_masked_div(const Run& r, const float* w, float* o, const float* data, size_t nper, size_t ws_wo, size_t ws_data, int64_t W, float denom = 0.0f,
                      uint8_t* nanflag = nullptr, int C = 1) {
    if (nper % 4 == 0 && ws_wo % 4 == 0 && ws_data % 4 == 0 && (nanflag == nullptr || C % 4 == 0) && ((uintptr_t)w % 16 == 0) && ((uintptr_t)o % 16 == 0))
        hipLaunchKernelGGL(k_masked_div4<MODE>, grid1(nper / 4, W), dim3(256), 0, r.st, w, o, data, nper / 4, ws_wo, ws_data, denom, nanflag, C);
    else
        hipLaunchKernelGGL(k_masked_div<MODE>, grid1(nper, W), dim3(256), 0, r.st, w, o, data, nper, ws_wo, ws_data, denom, nanflag, C);
    LAUNCHCHK();
    return TRI_OK;
}

int launch_sub(const Run& r, const float* a, const float* b, float* out, size_t nper, size_t ws_a, size_t ws_b, size_t ws_o, int64_t W) {
    if (nper % 4 == 0 && ws_a % 4 == 0 && ws_b % 4 == 0 && ws_o % 4 == 0 && ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0) && ((uintptr_t)out % 16 == 0))
        hipLaunchKernelGGL(k_sub4, grid1(nper / 4, W), dim3(256), 0, r.st, a, b, out, nper / 4, ws_a, ws_b, ws_o);
    else
        hipLaunchKernelGGL(k_sub, grid1(nper, W), dim3(256), 0, r.st, a, b, out, nper, ws_a, ws_b, ws_o);
    LAUNCHCHK();
    return TRI_OK;
}

// _get_background2d (flagging.py:516-579) for the median spectra of the batch,
// held in spectrum layout [Fa][Wb] (line axis = channel, column = window).
// Result: rows [0,Fa) of ws.so hold the background.
// Per (window, chunk) medians of a spectrum-layout image [Fa][Wb]: the segments run along the slow axis there
// (stride Wb floats), so the image and its flags are first turned into rows [Wb][Fa] (a few MB) and the
// segments become contiguous.  Output smed[w][g].
int spectrum_medians(const Run& r, const float* img, const uint8_t* flg) {
    const Plan& pl = r.pl;
    const Ws& ws = r.ws;
    const int Fa = (int)pl.Fa, Wn = (int)r.Wb, G = (int)pl.G;
    int rc = launch_transpose<float>(r, img, ws.srowsf, Fa, Wn, 0, 0, 1);
    if (rc) return rc;
    rc = launch_transpose<uint8_t>(r, flg, ws.srowsu, Fa, Wn, 0, 0, 1);
    if (rc) return rc;
    bool seg4 = Fa % 4 == 0;
    for (int64_t g = 0; g < pl.G + 1 && seg4; g++) seg4 = r.p->chunk_ends[g] % 4 == 0;
    MedianJob j;
    j.data = ws.srowsf; j.flags = ws.srowsu; j.med = ws.smed; j.RS = (size_t)Fa;
    j.seg_start = ws.segC_start; j.seg_len = ws.segC_len; j.R = Wn; j.G = G; j.W = 1; j.max_len = pl.maxchunk;
    j.vec_ok = j.segs_aligned = seg4; j.rows_aligned = Fa % 4 == 0;
    return launch_median(r, j);
}

int spectrum_background(const Run& r) {
    const Plan& pl = r.pl;
    const Ws& ws = r.ws;
    int Fa = (int)pl.Fa, Wn = (int)r.Wb, G = (int)pl.G;
    size_t nS = (size_t)Fa * Wn;
    hipLaunchKernelGGL(k_copy_u8, dim3((unsigned)cdiv(nS, 256)), dim3(256), 0, r.st, ws.sflags, ws.sbgf, nS);
    LAUNCHCHK();
    double rej = TRI_MAD_NORMAL * r.p->background_reject;  // flagging.py:568
    // the exact row filter (K4x) is picked PER ITERATION (boxx_pick_l depends on the radius: a large first radius may not fit
    // its LDS line while a later, smaller one does), so the row copy of the spectra is made by the first iteration that
    // takes that route, whichever it is (it used to be made by the first iteration only)
    bool rowD_valid = false;
    for (int ext = pl.nit; ext >= 0; ext--) {
        bool final_pass = ext == 0;
        double sigma = (double)(final_pass ? 1 : ext) * r.p->spike_width_freq;  // flagging.py:554, 576
        int rad = (int)box_radius(sigma);
        // Radii beyond the stage pipeline (K4p): the spectra as ROWS through the exact row filter (K4x) -- the in-place
        // multi-pass kernel walks 4 x (Fa + 4 r) positions with one wave per 64 windows: 5.8 ms per launch whatever
        // the batch.  The 2-D time-stage scratch (ws.Aw ...) is idle here and holds the four row images.
        FreqPick rows;
        rows.xl = (rad > 0 && 2 * (size_t)pl.PT >= 4) ? boxx_pick_l(r.box, rad, Fa) : 0;
        if (rows.xl > 0) {
            float* rowW = ws.Aw;                       // [Wn][Fa] weight rows, then the signed residual (unused)
            float* rowO = ws.Aw + nS;                  // weight * data rows
            float* rowD = ws.Aw + 2 * nS;              // the spectra themselves
            float* rowR = ws.Aw + 3 * nS;              // result rows
            hipLaunchKernelGGL(k_build_wo, grid1(nS, 1), dim3(256), 0, r.st, ws.sdata, ws.sbgf, ws.sw, ws.so, nS, (size_t)0, (size_t)0);
            LAUNCHCHK();
            int rc = launch_transpose<float>(r, ws.sw, rowW, Fa, Wn, 0, 0, 1);
            if (!rc) rc = launch_transpose<float>(r, ws.so, rowO, Fa, Wn, 0, 0, 1);
            if (!rc && !rowD_valid) rc = launch_transpose<float>(r, ws.sdata, rowD, Fa, Wn, 0, 0, 1);
            if (rc) return rc;
            rowD_valid = true;
            FreqJob j;
            j.srcW = rowW; j.srcO = rowO; j.data = rowD; j.outA = rowR;
            j.n = Fa; j.C = Wn; j.ld = Fa; j.rad = rad;
            if (final_pass) { j.outB = rowW; j.nanflag = reinterpret_cast<uint8_t*>(ws.rowcnt); }
            rc = final_pass ? launch_boxx<2>(r, rows, j) : launch_boxx<1>(r, rows, j);
            if (!rc) rc = launch_transpose<float>(r, rowR, ws.so, Wn, Fa, 0, 0, 1);
            if (rc) return rc;
            if (!final_pass) {
                rc = spectrum_medians(r, ws.so, ws.sbgf);
                if (rc) return rc;
                hipLaunchKernelGGL(k_reject<false>, grid1(nS, 1), dim3(256), 0, r.st, ws.so, ws.sbgf, ws.smed, ws.d_chunk_of, rej, Fa, Wn, G, (size_t)0, (size_t)0);
                LAUNCHCHK();
            }
            continue;
        }
        if (rad > 0) {
            ColJob j;
            j.srcData = ws.sdata; j.srcFlags = ws.sbgf;
            j.bufW = j.dstW = ws.sw; j.bufO = j.dstO = ws.so;
            j.n = Fa; j.C = Wn; j.rad = rad;
            int rc = launch_colfilter(r, pick_col_filter(r.box, ColSrc::ByteFlags, COL_WEIGHTS_01, false, rad, Fa, Wn, 1, spectrum_aligned(j)), j);
            if (rc) return rc;
        } else {
            hipLaunchKernelGGL(k_build_wo, grid1(nS, 1), dim3(256), 0, r.st, ws.sdata, ws.sbgf, ws.sw, ws.so, nS, (size_t)0, (size_t)0);
            LAUNCHCHK();
        }
        if (final_pass) {
            { int rc2 = launch_masked_div<0>(r, ws.sw, ws.so, ws.sdata, nS, 0, 0, 1); if (rc2) return rc2; }
        } else {
            { int rc2 = launch_masked_div<1>(r, ws.sw, ws.so, ws.sdata, nS, 0, 0, 1); if (rc2) return rc2; }
            // per (window, chunk) median of the residual: element (f, w) at f*Wn + w
            // -> row = w (RS 1), element stride Wn
            int rc = spectrum_medians(r, ws.so, ws.sbgf);
            if (rc) return rc;
            hipLaunchKernelGGL(k_reject<false>, grid1(nS, 1), dim3(256), 0, r.st, ws.so, ws.sbgf, ws.smed, ws.d_chunk_of, rej, Fa, Wn, G, (size_t)0, (size_t)0);
            LAUNCHCHK();
        }
    }
    return launch_interp(r, ws.so, Fa, Wn, (size_t)0, 1, (const uint8_t*)nullptr, (const float*)nullptr, (size_t)0, (float*)nullptr);
}

// _get_background2d (flagging.py:516-579) for every window of the batch.
// In: dataTF / dataFT, flagsTF (spectral flags already OR-ed in).  Out: the
// background in FT layout in rows [0,Fa) of ws.Bo and the residual
// data - background in rows [0,Fa) of ws.Bw (window stride PF*T).
static bool bg_flags_packed(int T, size_t N) {
    static const bool no_pack = is1(getenv("TRI_NO_PACKED_FLAGS"));
    return !no_pack && (T % 4 == 0) && (N % 4 == 0);
}

// ---- the routes of one background iteration, picked once (pick_bg_step) and then only switched on -------------------------

enum class TimeStage {
    BuildOnly,        // r0 == 0: the weight / data images themselves
    PackedSweep,      // single sweep straight from (data, TF4 flag words): no image build
    Prebuilt,         // images built first, float images through the single sweep (faster than byte loads in its loop)
    PrebuiltDirectFT, // ... which writes the FT layout itself (TRI_FILTER_DIRECT_FT=1; measured no faster than two transposes)
    ByteFlags         // built on the fly from byte flags (multi-pass kernel of the large radii: 11.4 vs 16.8 ms per call with a build)
};
// (FreqStage / FreqPick, the frequency stage of one radius: boxfilter_host.hpp)
enum class Reject {
    None,             // final pass
    InRows,           // K4x iterations: block medians and rejection where the rows lie (TF4 flag words)
    Tile,             // K3t: median + rejection + TF4 re-pack, tile-parallel
    OnePass,          // K3r: the same, one workgroup per block
    MedianReject4T,   // block medians, then rejection + TF4 re-pack in one pass
    MedianReject4,    // block medians, then the vector rejection and a transpose of the flags
    MedianReject      // block medians, then the scalar rejection and a transpose of the flags
};

// K3t (tile-parallel median + rejection): scratch sizes and whether the rejection iterations take it
struct TileRoute { bool use; size_t ccap, ucap; int ytiles; };
static int medrej_force_fallback() { static const int v = [] { const char* e = getenv("TRI_MEDREJ_FORCE_FALLBACK"); return e ? atoi(e) : 0; }(); return v; }
static bool no_fused_reject() { static const bool v = is1(getenv("TRI_NO_FUSED_REJECT")); return v; }
// K3r is opt-in (TRI_FUSED_MEDREJ=1): one workgroup per block does not stream fast enough -- 3.7 against 3.0 ms per 252
// windows for the two kernels, scripts/ubench/medrej_dev.hip
static bool fused_medrej() { static const bool v = is1(getenv("TRI_FUSED_MEDREJ")); return v; }
static TileRoute pick_tile_route(const Run& r, bool packed) {
    const Plan& pl = r.pl;
    static const bool no_tile = is1(getenv("TRI_NO_TILE_MEDREJ"));
    const int T = (int)pl.T, G = (int)pl.G;
    const size_t wsA = 2 * (size_t)pl.PT * pl.Fa, wsB = (size_t)pl.PF * T;
    const size_t mr_nb = (size_t)pl.maxchunk * T;                  // samples of the largest block
    TileRoute t = {false, (mr_nb / 4) & ~(size_t)3, (mr_nb / 8) & ~(size_t)3, 0};
    for (int g = 0; g < G; g++) t.ytiles += (int)cdiv(r.p->chunk_ends[g + 1] - r.p->chunk_ends[g], 64);
    // (blocks too small to predict from -- fewer than 65536 samples -- would all take the redo path: the two-kernel route)
    t.use = pl.vec && wsB % 4 == 0 && wsA % 4 == 0 && packed && !no_fused_reject() && !no_tile && !fused_medrej() && G <= 65535 &&
            mrt_scratch_words(G, t.ccap, t.ucap) <= wsA && (medrej_force_fallback() || (pl.maxchunk - 1) * (int64_t)T >= 65536) &&
            t.ytiles > 0 && t.ytiles <= 65535;
    return t;
}
// K3r scratch per (window, chunk) block: the dead time-stage images, half for the window's keys, half for the undecided
// samples' indices
static unsigned medrej_capq(size_t wsA, int G) {
    const size_t per_block = (wsA / (size_t)G) & ~(size_t)7;
    return (unsigned)std::min<size_t>(per_block / 2, 0x3ffffffcu);
}

struct BgStep {
    int r0, r1;
    bool final_pass;
    TimeStage time;
    bool time_needs_bytes;   // the time stage reads a TF byte image of the flags, rebuilt into ws.comb while they are packed
    bool time_defers;        // it leaves its division by float32(d)**4 to the transposes (else it divides itself)
    ColPick tcol;            // r0 > 0: the filter of the time stage
    FreqPick freq;
    bool freq_transposes;    // Transposed: the FT images still have to be made (not after PrebuiltDirectFT)
    Reject reject;
    bool reads_ft_flags;     // the FT flag bytes are read: by the time stage's byte image, or by an FT-native median / rejection
};

// ext = background_iterations .. 1: rejection iterations; 0: the final pass.  packed: bg_flags_packed().
static BgStep pick_bg_step(const Run& r, bool packed, bool tile_route, int ext) {
    const Plan& pl = r.pl;
    const int T = (int)pl.T, Fa = (int)pl.Fa, G = (int)pl.G;
    const size_t wsA = 2 * (size_t)pl.PT * Fa, wsB = (size_t)pl.PF * T;
    BgStep s;
    s.final_pass = ext == 0;
    const double e = (double)(s.final_pass ? 1 : ext);
    s.r0 = (int)box_radius(e * r.p->spike_width_time);
    s.r1 = (int)box_radius(e * r.p->spike_width_freq);

    static const bool prebuild = [] { const char* e = getenv("TRI_TIME_PREBUILD"); return !(e && e[0] == '0'); }();
    const bool sweep = s.r0 > 0 && colfilter_lds_block(r.box, s.r0, Fa) > 0;
    if (s.r0 == 0) s.time = TimeStage::BuildOnly;
    else if (sweep && packed) s.time = TimeStage::PackedSweep;
    else if (sweep && prebuild) {
        static const bool want_direct = is1(getenv("TRI_FILTER_DIRECT_FT"));
        s.time = (want_direct && T % 4 == 0 && wsB % 4 == 0) ? TimeStage::PrebuiltDirectFT : TimeStage::Prebuilt;
    } else s.time = TimeStage::ByteFlags;
    s.time_needs_bytes = packed && (s.time == TimeStage::BuildOnly || s.time == TimeStage::ByteFlags);

    // (K4x masks the unmasked cached amplitudes with the iteration's input flags: it needs them)
    s.freq = s.time == TimeStage::PrebuiltDirectFT
                 ? pick_freq_unfused(r.box, s.r1, Fa, T, r.Wb)
                 : pick_freq_stage(r.box, s.final_pass ? 2 : 1, s.r1, Fa, T, r.Wb, r.ws.Aw, r.ws.Ao, wsA, !r.ampl_cached || r.data_mask);
    s.freq_transposes = s.time != TimeStage::PrebuiltDirectFT;
    s.time_defers = s.freq.route == FreqStage::Transposed;
    switch (s.time) {
        case TimeStage::BuildOnly: break;
        case TimeStage::PackedSweep: s.tcol = pick_col_filter(r.box, ColSrc::PackedFlags, COL_WEIGHTS_01, s.time_defers, s.r0, T, Fa, r.Wb, false); break;
        case TimeStage::Prebuilt: s.tcol = pick_col_filter(r.box, ColSrc::Images, COL_WEIGHTS_01, s.time_defers, s.r0, T, Fa, r.Wb, false); break;
        case TimeStage::PrebuiltDirectFT: s.tcol = pick_col_filter(r.box, ColSrc::Images, COL_TRANSPOSED_OUT, false, s.r0, T, Fa, r.Wb, false); break;
        case TimeStage::ByteFlags: s.tcol = pick_col_filter(r.box, ColSrc::ByteFlags, 0, false, s.r0, T, Fa, r.Wb, false); break;
    }

    // K4x iterations stay in the row layout altogether (TRI_FILTER_NO_TF_REJECT=1: transposes + FT kernels)
    static const bool no_tfr = is1(getenv("TRI_FILTER_NO_TF_REJECT"));
    const bool vec4 = pl.vec && wsB % 4 == 0;
    if (s.final_pass) s.reject = Reject::None;
    else if (s.freq.route == FreqStage::ExactRows && packed && !no_tfr && G <= 65535 && (uint64_t)T * Fa * 4u < (1ull << 31))
        s.reject = Reject::InRows;
    else if (tile_route) s.reject = Reject::Tile;
    else if (vec4 && wsA % 4 == 0 && packed && !no_fused_reject() && fused_medrej() && medrej_capq(wsA, G) >= 1024 && G <= 65535 &&
             (uint64_t)T * Fa * 4u < (1ull << 32))
        s.reject = Reject::OnePass;
    else if (vec4 && packed && !no_fused_reject()) s.reject = Reject::MedianReject4T;
    else s.reject = vec4 ? Reject::MedianReject4 : Reject::MedianReject;
    s.reads_ft_flags = s.time_needs_bytes || (!s.final_pass && s.reject != Reject::InRows);
    return s;
}

// The images the time and frequency stages work on: the flagger's workspace, or the arguments of tri_bench_boxfilter.
// TF images are [T][Fa], FT images [Fa][T]; every stride is per window, in elements.
struct BgImages {
    int T, Fa;
    int64_t W;
    const float *dataTF, *dataFT;   // amplitudes (stride T * Fa)
    const uint8_t* flagsTF;         // background flags of the time stage: bytes, or TF4 words when packed (stride T * Fa bytes)
    uint8_t* comb;                  // room for their byte image while they are packed
    float *Aw, *Ao; size_t wsA;     // TF weight / weight * data images: time stage out, frequency stage in
    float *Bw, *Bo; size_t wsB;     // FT images: frequency stage out
    float* rows; size_t ws_rows;    // ExactRows: where K4x leaves |data - background| / the background as rows
    const uint8_t* mask; size_t ws_mask;   // ExactRows: byte mask of the data rows, or NULL
    uint8_t* nanflag;               // final pass: per-line "background holds a NaN" markers, W * T ints
    float* residP;                  // final pass, optional: the residual a second time, as column panels (stride T * Fa)
    unsigned long long* xstats;     // ExactRows, optional: pass counters
};

// What survives from one iteration to the next
struct BgState {
    uint8_t *cur_ft, *alt_ft;   // FT flag bytes: current image, and the one K3t / K3r write (the two then swap)
    bool bgf_ft_stale;          // the FT flag bytes lag behind the TF4 words (rows-only rejection iterations)
    bool wrote_panel;           // the final frequency stage left the residual in residP as well
};

// --- time axis (TF layout: line = time, column = channel) ---
// *den_t: the division the stage left to the transposes, or 0
static int bg_time_stage(const Run& r, const BgStep& s, const BgImages& im, const BgState& st, float* den_t) {
    const int T = im.T, Fa = im.Fa;
    const size_t N = (size_t)T * Fa;
    const int64_t W = im.W;
    int rc = TRI_OK;
    *den_t = (s.r0 > 0 && s.tcol.defers) ? box_denominator(s.r0) : 0.0f;
    ColJob j;     // (the sweep's source: the float images in place, or data + flags)
    j.bufW = j.dstW = im.Aw; j.bufO = j.dstO = im.Ao;
    j.n = T; j.C = Fa; j.rad = s.r0;
    j.bws = j.dws = im.wsA; j.W = W;
    const uint8_t* fl = im.flagsTF;
    if (s.time_needs_bytes) {
        rc = launch_transpose<uint8_t>(r, st.cur_ft, im.comb, Fa, T, N, N, W);
        if (rc) return rc;
        fl = im.comb;
    }
    switch (s.time) {
        case TimeStage::BuildOnly:
            hipLaunchKernelGGL(k_build_wo, grid1(N, W), dim3(256), 0, r.st, im.dataTF, fl, im.Aw, im.Ao, N, N, im.wsA);
            LAUNCHCHK();
            return TRI_OK;
        case TimeStage::PackedSweep:
        case TimeStage::ByteFlags:
            j.srcData = im.dataTF; j.srcFlags = fl; j.sws = N;
            return launch_colfilter(r, s.tcol, j);
        case TimeStage::Prebuilt:
        case TimeStage::PrebuiltDirectFT:
            if (N % 4 == 0 && im.wsA % 4 == 0)
                hipLaunchKernelGGL(k_build_wo4, grid1(N / 4, W), dim3(256), 0, r.st, im.dataTF, fl, im.Aw, im.Ao, N / 4, N, im.wsA);
            else
                hipLaunchKernelGGL(k_build_wo, grid1(N, W), dim3(256), 0, r.st, im.dataTF, fl, im.Aw, im.Ao, N, N, im.wsA);
            LAUNCHCHK();
            if (s.time == TimeStage::PrebuiltDirectFT) { j.dstW = im.Bw + s.freq.off; j.dstO = im.Bo + s.freq.off; j.dws = im.wsB; }
            return launch_colfilter(r, s.tcol, j);
    }
    return set_err(TRI_EINVAL, "internal: no such time stage");
}

// --- frequency axis (FT layout: line = channel, column = time) + masked division ---
// Leaves |data - background| (final pass: the background) in im.Bo and, in the final pass, data - background in im.Bw;
// with Reject::InRows |data - background| stays in im.rows.
template <int MODE>
static int bg_freq_stage_mode(const Run& r, const BgStep& s, const BgImages& im, BgState& st, float den_t) {
    const int T = im.T, Fa = im.Fa, r1 = s.r1;
    const size_t N = (size_t)T * Fa, wsA = im.wsA, wsB = im.wsB;
    const int64_t W = im.W;
    uint8_t* const nan = MODE == 2 ? im.nanflag : nullptr;
    const float den_f = s.freq.defers ? box_denominator(r1) : 0.0f;   // division deferred to masked_div
    int rc = TRI_OK;
    FreqJob j;
    j.srcW = im.Aw; j.srcO = im.Ao; j.dstW = im.Bw; j.dstO = im.Bo; j.data = im.dataFT;
    j.n = Fa; j.C = T; j.ld = Fa; j.rad = r1;
    j.sws_img = wsA; j.dws = wsB; j.ws_data = N; j.W = W; j.nanflag = nan;
    // im.nanflag (W * T ints, idle until the end of the iteration) holds the per-line NaN markers
    if (MODE == 2) HIPCHK(hipMemsetAsync(im.nanflag, 0, (size_t)W * T, r.st));
    switch (s.freq.route) {
        case FreqStage::ExactRows:
            // (the flagger: im.rows == im.Ao, the rows are filtered in place; MODE 2: im.Aw <- data - background)
            j.data = im.dataTF; j.mask = im.mask; j.ws_mask = im.ws_mask; j.stats = im.xstats;
            j.outA = im.rows; j.ws_outA = im.ws_rows;
            if (MODE == 2) { j.outB = im.Aw; j.ws_outB = wsA; }
            rc = launch_boxx<MODE>(r, s.freq, j);
            if (!rc && MODE == 2) rc = launch_transpose<float>(r, im.Aw, im.Bw, T, Fa, wsA, wsB, W);
            if (rc || s.reject == Reject::InRows) return rc;
            return launch_transpose<float>(r, im.rows, im.Bo, T, Fa, im.ws_rows, wsB, W);
        case FreqStage::FusedRing:
            if (MODE == 2) { j.dstP = im.residP; j.pws = N; }
            j.wroteP = &st.wrote_panel;
            return launch_boxf<MODE>(r, s.freq, j);
        case FreqStage::FusedLds:
            return launch_colfilter_tf<MODE>(r, j);
        case FreqStage::LdsDiv:
        case FreqStage::Lane4Div:
            rc = launch_colfilter_t(r, s.freq, j);
            break;
        case FreqStage::Transposed:
            if (s.freq_transposes) {
                rc = launch_transpose<float>(r, im.Aw, im.Bw + s.freq.off, T, Fa, wsA, wsB, W, den_t);
                if (!rc) rc = launch_transpose<float>(r, im.Ao, im.Bo + s.freq.off, T, Fa, wsA, wsB, W, den_t);
            }
            if (!rc && r1 > 0) {
                ColJob c;
                c.bufW = c.dstW = im.Bw; c.bufO = c.dstO = im.Bo;
                c.n = Fa; c.C = T; c.rad = r1;
                c.bws = c.dws = wsB; c.W = W;
                rc = launch_colfilter(r, s.freq.col, c);
            }
            break;
    }
    if (rc) return rc;
    return launch_masked_div<MODE>(r, im.Bw, im.Bo, im.dataFT, N, wsB, N, W, den_f, nan, MODE == 2 ? T : 1);
}
static int bg_freq_stage(const Run& r, const BgStep& s, const BgImages& im, BgState& st, float den_t) {
    return s.final_pass ? bg_freq_stage_mode<2>(r, s, im, st, den_t) : bg_freq_stage_mode<1>(r, s, im, st, den_t);
}

// --- block medians of |data - background| and rejection of a non-final iteration; the flags end up in st.cur_ft (FT bytes,
//     unless Reject::InRows) and in ws.bgfTF (the time stage's form) ---
static int bg_reject_stage(const Run& r, const BgStep& s, const TileRoute& tile, bool packed, BgState& st) {
    const Plan& pl = r.pl;
    const Ws& ws = r.ws;
    const int T = (int)pl.T, Fa = (int)pl.Fa, G = (int)pl.G;
    const int64_t W = r.Wb;
    const size_t N = (size_t)T * Fa, wsA = 2 * (size_t)pl.PT * Fa, wsB = (size_t)pl.PF * T;
    const double rej = TRI_MAD_NORMAL * r.p->background_reject;
    if (s.reject == Reject::None) return TRI_OK;
    // (only K3t leaves the flags it reads alone: see flags_in_place in background2d)
    if (s.reject != Reject::Tile && st.cur_ft == ws.flagsFT)
        return set_err(TRI_EUNSUPPORTED, "internal: background flags read in place on a route that rewrites them");
    switch (s.reject) {
        case Reject::InRows: {
            // block medians over (all times) x (chunk channels) of the row image with the TF4 flag words, rejection straight
            // into those words -- no FT image of the residual or of the flags in this iteration (the FT flags are rebuilt
            // when an iteration that reads them follows)
            unsigned* gc = reinterpret_cast<unsigned*>(ws.Aw);          // the weight rows are dead: candidate scratch
            unsigned cap = (unsigned)(std::min<size_t>((wsA / 2) / (size_t)G, 0x7fffffffu) & ~(size_t)3);
            if (median_no_predict() || (int64_t)cap < pl.maxchunk * pl.T || wsA % 4 != 0) { gc = nullptr; cap = 0; }
            // (not through launch_median_kernel: a block of rows with TF4 flag words, not row segments)
            hipLaunchKernelGGL((k_median2<false, true>), dim3((unsigned)G, (unsigned)W), dim3(256), 0, r.st, (const float*)ws.Ao,
                               (const uint8_t*)ws.bgfTF, ws.med, wsA, N, (size_t)0, (size_t)1, ws.segC_start, ws.segC_len, 1, G,
                               gc, gc ? wsA : (size_t)0, cap, T / 4, Fa);
            hipLaunchKernelGGL(k_reject_tf, dim3((unsigned)cdiv(Fa, 256), (unsigned)(T / 4), (unsigned)W), dim3(256), 0, r.st,
                               (const float*)ws.Ao, reinterpret_cast<unsigned*>(ws.bgfTF), ws.med, ws.d_chunk_of, rej, T / 4, Fa, Fa, G,
                               wsA, N / 4);
            LAUNCHCHK();
            st.bgf_ft_stale = true;
            return TRI_OK;
        }
        case Reject::Tile: {
            // K3t (kernels_reject_tile.hpp): predict (per block) -> pass (per 64 x 64-word tile) -> finish (per block) -> redo of
            // the blocks that failed a check.  Scratch: the dead time-stage images of the window.  It never modifies the flags
            // it reads: cur_ft in, alt_ft out, then the two swap.
            unsigned* sc = reinterpret_cast<unsigned*>(ws.Aw);
            hipLaunchKernelGGL(k_mr_predict, dim3((unsigned)G, (unsigned)W), dim3(256), 0, r.st, (const float*)ws.Bo, (const uint8_t*)st.cur_ft,
                               ws.d_chunk_ends, rej, T / 4, G, wsB, N, sc, wsA, tile.ccap, tile.ucap, medrej_force_fallback());
            for (unsigned round = 1; round <= 2; round++) {        // (round 2: only the blocks whose median missed the predicted window)
                hipLaunchKernelGGL(k_mr_pass, dim3((unsigned)cdiv(T / 4, 64), (unsigned)tile.ytiles, (unsigned)W), dim3(256), 0, r.st, (const float*)ws.Bo,
                                   (const uint8_t*)st.cur_ft, st.alt_ft, ws.bgfTF, ws.d_chunk_ends, Fa, T / 4, G, wsB, N, sc, wsA, tile.ccap, tile.ucap, round);
                hipLaunchKernelGGL(k_mr_finish, dim3((unsigned)G, (unsigned)W), dim3(256), 0, r.st, (const float*)ws.Bo, (const uint8_t*)st.cur_ft, st.alt_ft,
                                   ws.bgfTF, ws.med, ws.d_chunk_ends, rej, Fa, T / 4, G, wsB, N, sc, wsA, tile.ccap, tile.ucap, round);
            }
            hipLaunchKernelGGL(k_median_reject, dim3((unsigned)G, (unsigned)W), dim3(256), 0, r.st, (const float*)ws.Bo, (const uint8_t*)st.cur_ft,
                               st.alt_ft, ws.bgfTF, ws.med, ws.d_chunk_ends, rej, Fa, T / 4, G, wsB, N, sc, wsA, 0u, 0u, 1,
                               (const unsigned*)sc, wsA, (int)MRT_PARW, 11);
            LAUNCHCHK();
            // (read in place, ws.flagsFT stays as it is -- the time medians of the residual read it: the first iteration
            //  writes ws.bgfFT, and from then on ws.bgfFT and ws.fflFT alternate)
            std::swap(st.cur_ft, st.alt_ft);
            if (st.alt_ft == ws.flagsFT) st.alt_ft = ws.fflFT;
            return TRI_OK;
        }
        case Reject::OnePass: {
            // K3r (kernels_reject.hpp) writes the updated FT flags to a SECOND image (its fallback redoes a block from the
            // input flags), so the FT flag image alternates between ws.bgfFT and ws.fflFT (free until the frequency-axis
            // SumThreshold writes it)
            const unsigned capq = medrej_capq(wsA, G);
            hipLaunchKernelGGL(k_median_reject, dim3((unsigned)G, (unsigned)W), dim3(256), 0, r.st, (const float*)ws.Bo, (const uint8_t*)st.cur_ft,
                               st.alt_ft, ws.bgfTF, ws.med, ws.d_chunk_ends, rej, Fa, T / 4, G, wsB, N,
                               reinterpret_cast<unsigned*>(ws.Aw), wsA, capq, capq, medrej_force_fallback());
            LAUNCHCHK();
            std::swap(st.cur_ft, st.alt_ft);
            return TRI_OK;
        }
        default:   // the three median-then-reject routes: below
            break;
    }
    // block medians over (all times) x (chunk channels): contiguous in FT
    // (the time stage's images in ws.Aw / ws.Ao are dead here: candidate scratch, wsA / G keys per block)
    MedianJob j;
    j.data = ws.Bo; j.flags = st.cur_ft; j.med = ws.med; j.WSd = wsB; j.WSf = N;
    j.seg_start = ws.segB_start; j.seg_len = ws.segB_len; j.R = 1; j.G = G; j.W = W; j.max_len = pl.maxchunk * pl.T;
    j.vec_ok = T % 4 == 0 && wsB % 4 == 0 && N % 4 == 0;
    j.gcand = reinterpret_cast<unsigned*>(ws.Aw); j.cand_ws = wsA;
    j.cand_cap = (unsigned)(std::min<size_t>(wsA / (size_t)G, 0x7fffffffu) & ~(size_t)3);
    const int rc = launch_median(r, j);
    if (rc) return rc;
    if (s.reject == Reject::MedianReject4T) {
        hipLaunchKernelGGL(k_reject4_t, dim3((unsigned)cdiv(T / 4, 64), (unsigned)cdiv(Fa, 64), (unsigned)W), dim3(64, 4), 0, r.st,
                           ws.Bo, st.cur_ft, ws.bgfTF, ws.med, ws.d_chunk_of, rej, Fa, T / 4, G, wsB, N);
        LAUNCHCHK();
        return TRI_OK;
    }
    if (s.reject == Reject::MedianReject4)
        hipLaunchKernelGGL(k_reject4, grid1(N / 4, W), dim3(256), 0, r.st, ws.Bo, st.cur_ft, ws.med, ws.d_chunk_of, rej, T / 4, G, N / 4, wsB, N);
    else
        hipLaunchKernelGGL(k_reject<true>, grid1(N, W), dim3(256), 0, r.st, ws.Bo, st.cur_ft, ws.med, ws.d_chunk_of, rej, Fa, T, G, wsB, N);
    LAUNCHCHK();
    if (packed) return launch_transpose<float>(r, reinterpret_cast<const float*>(st.cur_ft), reinterpret_cast<float*>(ws.bgfTF), Fa, T / 4, N / 4, N / 4, W);
    return launch_transpose<uint8_t>(r, st.cur_ft, ws.bgfTF, Fa, T, N, N, W);
}

// residP (optional): where the final frequency stage may leave the residual a second time, as column panels
// [Fa / 64][T][64] with window stride N; *wroteP tells whether it did (only the register-ring kernel K4r can).
int background2d(const Run& r, bool flagsFT_current, float* residP = nullptr, bool* wroteP = nullptr) {
    const Plan& pl = r.pl;
    const Ws& ws = r.ws;
    const int T = (int)pl.T, Fa = (int)pl.Fa;
    const int64_t W = r.Wb;
    const size_t N = (size_t)T * Fa;
    // Background flags live in FT layout (ws.bgfFT).  For the time-axis stage
    // they are needed per (time, channel) column thread: either as a TF byte
    // image (general case) or, when T % 4 == 0, packed four times per word
    // ("TF4": [T/4][Fa] uint32) -- which is exactly the 32-bit transpose of the
    // FT byte image viewed as [Fa][T/4] words.
    const bool packed = bg_flags_packed(T, N);
    const TileRoute tile = pick_tile_route(r, packed);
    // K3t never modifies the flags it reads, so its first iteration can read ws.flagsFT where it lies and the copy into
    // ws.bgfFT is not needed.  Only when every rejection iteration is sure to take that route: the FT-native rejections
    // (k_reject4_t, k_reject4, k_reject) and the rebuild after rows-only iterations (bgf_ft_stale, K4x) write into cur_ft.
    // TRI_BG_COPY_FLAGS=1 restores the copy (A/B runs).
    static const bool copy_flags = is1(getenv("TRI_BG_COPY_FLAGS"));
    bool flags_in_place = flagsFT_current && !copy_flags && packed && tile.use;
    for (int ext = pl.nit; ext >= 1 && flags_in_place; ext--)
        if (pick_bg_step(r, packed, tile.use, ext).freq.route == FreqStage::ExactRows) flags_in_place = false;
    int rc = TRI_OK;
    if (!flags_in_place)
        rc = flagsFT_current ? launch_u8<0>(r, ws.flagsFT, ws.bgfFT, N, N, N, W)
                             : launch_transpose<uint8_t>(r, ws.flagsTF, ws.bgfFT, T, Fa, N, N, W);
    if (rc) return rc;
    if (packed)
        rc = launch_transpose<float>(r, reinterpret_cast<const float*>(flags_in_place ? ws.flagsFT : ws.bgfFT), reinterpret_cast<float*>(ws.bgfTF), Fa, T / 4, N / 4, N / 4, W);
    else
        rc = launch_u8<0>(r, ws.flagsTF, ws.bgfTF, N, N, N, W);
    if (rc) return rc;

    BgImages im;
    im.T = T; im.Fa = Fa; im.W = W;
    im.dataTF = ws.dataTF; im.dataFT = ws.dataFT;
    im.flagsTF = ws.bgfTF; im.comb = ws.comb;
    im.Aw = ws.Aw; im.Ao = ws.Ao; im.wsA = 2 * (size_t)pl.PT * Fa;   // Aw / Ao interleaved per window (carve)
    im.Bw = ws.Bw; im.Bo = ws.Bo; im.wsB = (size_t)pl.PF * T;
    im.rows = ws.Ao; im.ws_rows = im.wsA;
    im.mask = r.ampl_cached ? r.data_mask : nullptr; im.ws_mask = r.data_mask_ws;
    im.nanflag = reinterpret_cast<uint8_t*>(ws.rowcnt);
    im.residP = residP; im.xstats = nullptr;
    BgState st = {flags_in_place ? ws.flagsFT : ws.bgfFT, flags_in_place ? ws.bgfFT : ws.fflFT, false, false};
    for (int ext = pl.nit; ext >= 0; ext--) {
        const BgStep s = pick_bg_step(r, packed, tile.use, ext);
        if (st.bgf_ft_stale && s.reads_ft_flags) {
            // an iteration that reads the FT flag bytes follows rows-only ones: they are the 32-bit transpose of the TF4 words
            rc = launch_transpose<float>(r, reinterpret_cast<const float*>(ws.bgfTF), reinterpret_cast<float*>(st.cur_ft), T / 4, Fa, N / 4, N / 4, W);
            if (rc) return rc;
            st.bgf_ft_stale = false;
        }
        float den_t = 0.0f;
        rc = bg_time_stage(r, s, im, st, &den_t);
        if (!rc) rc = bg_freq_stage(r, s, im, st, den_t);
        if (!rc) rc = bg_reject_stage(r, s, tile, packed, st);
        if (rc) return rc;
    }
    if (wroteP) *wroteP = st.wrote_panel;
    // (a repaired line's residual is redone: in the panel image too)
    return launch_interp(r, ws.Bo, Fa, T, im.wsB, W, reinterpret_cast<const uint8_t*>(ws.rowcnt), (const float*)ws.dataFT, N, ws.Bw,
                         st.wrote_panel ? residP : nullptr, N);
}

// ---- the routes of one major iteration, picked once per process_windows() call (pick_iteration) and then only switched on -------------

enum class Begin {
    FusedCached,      // cached amplitudes: flagsTF, flagsFT and the masked FT amplitudes in one pass over the running flags
    Cached,           // cached amplitudes: the running flags copied, transposed, then k_zero_flagged4 on the FT amplitudes
    Prepare4,         // k_prepare4 (16-byte loads) every iteration, then both transposes
    Prepare           // k_prepare (any shape, channel averaging), then both transposes
};
enum class SpecOr {
    Scalar,           // k_or_spec into the TF flags; the FT flags are transposed again before the time medians of the residual
    Rows16,           // k_or_spec16 into the TF flags; the FT flags are transposed again
    FtInPlace,        // ... and k_or_spec_ft16 updates the FT flags where they lie (rows of flagged channels): no second transpose
    FtInPlaceDeferTf  // FT in place only: with packed background flags nobody reads the TF flags before the time flags are OR-ed in too
};
enum class ChunkFlags {
    ExtraSources,     // the wave medians take flagsTF, the time flags and the spectral rows as they are: no pass writes the union
    OrMore16,         // k_or_spec_more16: the deferred spectral rows and the time flags into flagsTF in one pass
    OrBytes           // launch_u8<1>: the time flags into flagsTF
};
enum class Finish {
    FusedDilate,      // k_combine_dilate16: both smearings in one pass, no intermediate image
    Combine16Dilate,  // k_combine16, then k_unaverage16<-1, 3>
    Combine16,        // k_combine16, then k_unaverage (any frequency extents)
    Combine           // k_combine, then k_unaverage (any shape, channel averaging)
};
enum class FinalKernel {
    NanMask16,        // k_final16, isnan(|vis|) from the cached amplitudes' bit mask: half the bytes of the complex visibilities
    Vis16,            // k_final16 on the visibilities
    Scalar            // k_final
};
struct IterStep {
    Begin begin; SpecOr spec_or; ChunkFlags chunk_flags; Finish finish; FinalKernel final_kernel;
    // Column panels for the time-axis SumThreshold (round 4): the TF residual and the time flags as [Fa / 64][T][64], so the
    // column kernel's row walk is one linear stream.  Who else touches the two images reads panels too: the frequency-axis MAD
    // (ChunkFlags::ExtraSources; an aligned group of four channels is contiguous either way) and Finish::FusedDilate.
    bool panel;
    bool fused_resid;       // panel, and the background's final frequency stage is asked to write the panel residual itself
    int lo, hi, flo, fhi;   // smearing extents along time / frequency
    bool ft_current() const { return spec_or == SpecOr::FtInPlace || spec_or == SpecOr::FtInPlaceDeferTf; }
};

// smearing by e samples reaches [-(e // 2), e - e // 2), where // is Python's floor division
static void smear_extents(int64_t e, int* lo, int* hi) {
    const int64_t half = e >= 0 ? e / 2 : -((-e + 1) / 2);
    *lo = (int)-half; *hi = (int)(-half + e);
}
// TRI_ST_NO_PANEL=1: the time-axis SumThreshold and whoever shares its images read plain rows, never column panels (A/B runs)
static bool st_no_panel() { static const bool off = is1(getenv("TRI_ST_NO_PANEL")); return off; }

// Launches nothing.  Reads the plan, the parameters, r.ampl_cached and the alignment of the running flags (r.ws.iter): all
// constant over the batches and major iterations of a process_windows() call.
static IterStep pick_iteration(const Run& r) {
    const Plan& pl = r.pl;
    const int T = (int)pl.T, F = (int)pl.F, Fa = (int)pl.Fa;
    const size_t N = (size_t)T * Fa;
    static const bool no_fused_begin = is1(getenv("TRI_NO_FUSED_BEGIN"));
    static const bool no_ft_or = is1(getenv("TRI_NO_FT_SPEC_OR"));
    static const bool no_fused_or = is1(getenv("TRI_NO_FUSED_OR"));
    static const bool no_fused_dilate = is1(getenv("TRI_NO_FUSED_DILATE"));
    // Where the background's final frequency stage is the register-ring kernel (K4r) it can write the panel residual itself,
    // over byte images that are dead by then (ws.residP, see carve()).  Measured on the 252-baseline slab the third store
    // stream costs that kernel as much as the transpose it saves, so the transpose stays the default:
    // TRI_NO_FUSED_RESID_TF=0 switches the fused write on, unset or 1 keeps the transpose (A/B runs, tests).
    static const bool no_fused_resid = [] { const char* e = getenv("TRI_NO_FUSED_RESID_TF"); return !(e && e[0] == '0'); }();
    IterStep s;
    smear_extents(r.p->time_extend, &s.lo, &s.hi);
    smear_extents(r.p->freq_extend, &s.flo, &s.fhi);
    if (!r.ampl_cached) s.begin = pl.vec ? Begin::Prepare4 : Begin::Prepare;
    else s.begin = (!no_fused_begin && T % 4 == 0 && Fa % 4 == 0 && N % 4 == 0 && (uintptr_t)r.ws.iter % 4 == 0) ? Begin::FusedCached : Begin::Cached;
    // (in place: whole 16-byte groups along time)
    if (!pl.vec) s.spec_or = SpecOr::Scalar;
    else if (no_ft_or || T % 16 != 0) s.spec_or = SpecOr::Rows16;
    else s.spec_or = bg_flags_packed(T, N) ? SpecOr::FtInPlaceDeferTf : SpecOr::FtInPlace;
    // (the union is read by the chunk medians only: the next major iteration rebuilds the TF flags)
    const bool defer_tf = s.spec_or == SpecOr::FtInPlaceDeferTf;
    if (defer_tf && !no_fused_or && median_takes_extra_flags(pl.maxchunk) && Fa % 4 == 0) s.chunk_flags = ChunkFlags::ExtraSources;
    else s.chunk_flags = defer_tf ? ChunkFlags::OrMore16 : ChunkFlags::OrBytes;
    if (!pl.vec) s.finish = Finish::Combine;
    else if (s.flo != -1 || s.fhi != 2) s.finish = Finish::Combine16;
    else s.finish = no_fused_dilate ? Finish::Combine16Dilate : Finish::FusedDilate;
    s.final_kernel = !pl.vec ? FinalKernel::Scalar : r.ampl_cached ? FinalKernel::NanMask16 : FinalKernel::Vis16;
    // only where exactly the panel-reading kernels run (TRI_ST_NO_PANEL=1: plain rows everywhere), so that no route that reads
    // rows can meet a panel image
    s.panel = !st_no_panel() && s.chunk_flags == ChunkFlags::ExtraSources && s.finish == Finish::FusedDilate && Fa % 64 == 0 && Fa == F &&
              median_takes_extra_flags(pl.maxchunk + 3) && st_use_fused(pl.swT) && st_use_mask(T, Fa);
    s.fused_resid = s.panel && !no_fused_resid;
    return s;
}

// The two launches of an iteration that read the visibilities: the only ones whose kernels depend on the dtype VD.
template <int VD>
static int launch_prepare(const Run& r, const IterStep& s, const void* vis) {
    const Plan& pl = r.pl;
    const Ws& ws = r.ws;
    const size_t N = (size_t)pl.T * pl.Fa, W = (size_t)r.Wb;
    if (s.begin == Begin::Prepare4)
        hipLaunchKernelGGL(k_prepare4<VD>, dim3((unsigned)cdiv(N * W / 4, 256)), dim3(256), 0, r.st, vis, ws.iter, ws.dataTF, ws.flagsTF, N * W / 4);
    else
        hipLaunchKernelGGL(k_prepare<VD>, grid1(N, W), dim3(256), 0, r.st, vis, ws.iter, ws.dataTF, ws.flagsTF, (int)pl.T, (int)pl.F, (int)pl.Fa, (int)pl.avg);
    LAUNCHCHK();
    return TRI_OK;
}
// flagging.py:910-918 whole-row / whole-column rules; :777-781 NaN OR; :1193
template <int VD>
static int launch_final(const Run& r, const IterStep& s, const void* vis, uint8_t* out_flags, bool update_iter) {
    const Ws& ws = r.ws;
    const int T = (int)r.pl.T, F = (int)r.pl.F, upd = update_iter ? 1 : 0;
    const size_t NF = (size_t)T * F, W = (size_t)r.Wb;
    const double row_limit = r.p->flag_all_freq_frac * (double)F, col_limit = (double)T * r.p->flag_all_time_frac;
    if (s.final_kernel == FinalKernel::NanMask16)
        hipLaunchKernelGGL(k_final16<TRI_VIS_NANMASK>, grid1(NF / 16, W), dim3(256), 0, r.st, ws.dil, ws.rowcnt, ws.colcnt, (const void*)ws.nanmask, out_flags, ws.iter, T, F / 16, row_limit, col_limit, upd);
    else if (s.final_kernel == FinalKernel::Vis16)
        hipLaunchKernelGGL(k_final16<VD>, grid1(NF / 16, W), dim3(256), 0, r.st, ws.dil, ws.rowcnt, ws.colcnt, vis, out_flags, ws.iter, T, F / 16, row_limit, col_limit, upd);
    else
        hipLaunchKernelGGL(k_final<VD>, grid1(NF, W), dim3(256), 0, r.st, ws.dil, ws.rowcnt, ws.colcnt, vis, out_flags, ws.iter, T, F, row_limit, col_limit, upd);
    LAUNCHCHK();
    return TRI_OK;
}
// (float32 amplitudes unless the dtype is one of the other two)
#define BY_VIS_DTYPE(FN, ...) \
    (vis_dtype == TRI_VIS_C64 ? FN<TRI_VIS_C64>(__VA_ARGS__) : vis_dtype == TRI_VIS_F64 ? FN<TRI_VIS_F64>(__VA_ARGS__) : FN<TRI_VIS_F32>(__VA_ARGS__))

// flagging.py:756  _average_freq: the amplitudes and the iteration's flags, each in the TF and in the FT layout
static int iter_begin(const Run& r, const IterStep& s, const void* vis, int vis_dtype) {
    const Ws& ws = r.ws;
    const int T = (int)r.pl.T, Fa = (int)r.pl.Fa;
    const size_t N = (size_t)T * Fa;
    const int64_t W = r.Wb;
    int rc = TRI_OK;
    switch (s.begin) {
        case Begin::FusedCached:
            hipLaunchKernelGGL((k_transpose_u8w<true, true>), dim3((unsigned)cdiv(Fa, 64), (unsigned)cdiv(T, 128), (unsigned)W), dim3(256), 0, r.st,
                               ws.iter, ws.flagsFT, ws.flagsTF, ws.dataFT, T, Fa, N, N, N, N);
            break;
        case Begin::Cached:
            // amplitudes (both layouts) were made once for the batch; this iteration's flags = running flags (NaNs already folded in)
            rc = launch_u8<0>(r, ws.iter, ws.flagsTF, N, N, N, W);
            if (!rc) rc = launch_transpose<uint8_t>(r, ws.flagsTF, ws.flagsFT, T, Fa, N, N, W);
            if (rc) return rc;
            hipLaunchKernelGGL(k_zero_flagged4, grid1(N / 4, W), dim3(256), 0, r.st, ws.flagsFT, ws.dataFT, N / 4, N, N);
            break;
        case Begin::Prepare4:
        case Begin::Prepare:
            rc = BY_VIS_DTYPE(launch_prepare, r, s, vis);
            if (!rc) rc = launch_transpose<float>(r, ws.dataTF, ws.dataFT, T, Fa, N, N, W);
            if (!rc) rc = launch_transpose<uint8_t>(r, ws.flagsTF, ws.flagsFT, T, Fa, N, N, W);
            return rc;
    }
    LAUNCHCHK();
    return TRI_OK;
}

// flagging.py:944  _time_median: rows of the FT layout are contiguous in time
static int time_medians(const Run& r, const float* dataFT, size_t ws_data) {
    const Ws& ws = r.ws;
    const int T = (int)r.pl.T, Fa = (int)r.pl.Fa;
    MedianJob j;
    j.data = dataFT; j.flags = ws.flagsFT; j.med = ws.med; j.WSd = ws_data; j.WSf = (size_t)T * Fa; j.RS = (size_t)T;
    j.seg_start = ws.segT_start; j.seg_len = ws.segT_len; j.R = Fa; j.G = 1; j.W = r.Wb; j.max_len = r.pl.T;
    j.rows_aligned = T % 4 == 0; j.segs_aligned = true;
    return launch_median(r, j);
}

// flagging.py:944-954  the spectrum of time medians, its background, SumThreshold on the residual, flags |= spec_flags
static int iter_spectrum(const Run& r, const IterStep& s) {
    const Ws& ws = r.ws;
    const int T = (int)r.pl.T, Fa = (int)r.pl.Fa, Wn = (int)r.Wb;
    const size_t N = (size_t)T * Fa, nS = (size_t)Fa * Wn;
    const int64_t W = r.Wb;
    int rc = time_medians(r, ws.dataFT, N);
    if (rc) return rc;
    hipLaunchKernelGGL(k_spec_from_med, dim3((unsigned)cdiv(nS, 256)), dim3(256), 0, r.st, ws.med, ws.sdata, ws.sflags, Fa, Wn);
    LAUNCHCHK();
    rc = spectrum_background(r);
    if (!rc) rc = launch_sub(r, ws.sdata, ws.so, ws.sres, nS, 0, 0, 0, 1);
    if (!rc) rc = spectrum_medians(r, ws.sres, ws.sflags);
    if (!rc) rc = launch_colst(r, r.pl.swF, ws.sres, ws.smed, ws.sout, ws.d_chunk_ends, Fa, Wn, (int)r.pl.G, 0, 0, 1);
    if (rc) return rc;
    if (s.spec_or != SpecOr::Scalar)
        hipLaunchKernelGGL(k_spec_rows, dim3((unsigned)cdiv(nS, 256)), dim3(256), 0, r.st, ws.sout, ws.srows, Fa, Wn);
    switch (s.spec_or) {
        case SpecOr::Scalar:
            hipLaunchKernelGGL(k_or_spec, grid1(N, W), dim3(256), 0, r.st, ws.flagsTF, ws.sout, T, Fa, Wn);
            break;
        case SpecOr::Rows16:
            hipLaunchKernelGGL(k_or_spec16, grid1(N / 16, W), dim3(256), 0, r.st, ws.flagsTF, ws.srows, T, Fa / 16);
            break;
        case SpecOr::FtInPlace:
            hipLaunchKernelGGL(k_or_spec16, grid1(N / 16, W), dim3(256), 0, r.st, ws.flagsTF, ws.srows, T, Fa / 16);
            hipLaunchKernelGGL(k_or_spec_ft16, grid1(N / 16, W), dim3(256), 0, r.st, ws.flagsFT, ws.srows, T / 16, Fa);
            break;
        case SpecOr::FtInPlaceDeferTf:
            hipLaunchKernelGGL(k_or_spec_ft16, grid1(N / 16, W), dim3(256), 0, r.st, ws.flagsFT, ws.srows, T / 16, Fa);
            break;
    }
    LAUNCHCHK();
    return TRI_OK;
}

// flagging.py:957-962  2-D background (FT layout, ws.Bo); the residual data - background was written by its final masked
// division (and redone by the interpolation pass on repaired lines) into ws.Bw, window stride PF * T.  *residTF: the same
// in the TF layout, window stride N: ws.residP where the final frequency stage wrote the panels itself, else ws.Aw (the
// time-axis scratch is free again), which iter_time_inputs() still has to fill (*transpose_pending).
static int iter_residual(const Run& r, const IterStep& s, const float** residTF, bool* transpose_pending) {
    const Ws& ws = r.ws;
    bool wrote_panel = false;
    const int rc = background2d(r, s.ft_current(), s.fused_resid ? ws.residP : nullptr, &wrote_panel);
    *residTF = wrote_panel ? ws.residP : ws.Aw;
    *transpose_pending = !wrote_panel;
    return rc;
}

// What SumThreshold along time reads besides the flags: the residual in the TF layout, and its MAD per channel over time =
// contiguous rows of the FT layout (flags = input | spectral flags, so the FT flag image is brought up to date first).
// Transpose and medians only read ws.Bw: where both run, the medians (and the flag transpose ahead of them) take the side lane.
// Nothing on r.st touches ws.med or ws.flagsFT before the join.
static int iter_time_inputs(const Run& r, const IterStep& s, bool transpose_pending) {
    const Ws& ws = r.ws;
    const int T = (int)r.pl.T, Fa = (int)r.pl.Fa;
    const size_t N = (size_t)T * Fa, wsB = (size_t)r.pl.PF * T;
    const bool overlap = OVERLAP_RESID_MEDIANS && transpose_pending;
    const Run side = overlap ? fork(r) : r;
    int rc = transpose_pending ? launch_transpose<float>(r, ws.Bw, ws.Aw, Fa, T, wsB, N, r.Wb, 0.0f, s.panel) : TRI_OK;
    if (!rc && !s.ft_current()) rc = launch_transpose<uint8_t>(side, ws.flagsTF, ws.flagsFT, T, Fa, N, N, r.Wb);
    if (!rc) rc = time_medians(side, ws.Bw, wsB);
    if (overlap) join(r);
    return rc;
}

// flagging.py:964-969  SumThreshold along time, flags |= time_flags, SumThreshold along frequency
static int iter_sumthreshold(const Run& r, const IterStep& s, const float* residTF) {
    const Plan& pl = r.pl;
    const Ws& ws = r.ws;
    const int T = (int)pl.T, Fa = (int)pl.Fa, G = (int)pl.G;
    const size_t N = (size_t)T * Fa, wsB = (size_t)pl.PF * T;
    const int64_t W = r.Wb;
    int rc = launch_colst(r, pl.swT, residTF, ws.med, ws.tflTF, ws.d_tends, T, Fa, 1, N, N, W, s.panel);
    if (rc) return rc;
    // MAD per (time, chunk) = contiguous row segments of the TF layout; flags = input | spectral | time flags
    MedianJob cj;
    cj.data = residTF; cj.flags = ws.flagsTF; cj.med = ws.med; cj.WSd = cj.WSf = N; cj.RS = (size_t)Fa;
    cj.seg_start = ws.segC_start; cj.seg_len = ws.segC_len; cj.R = T; cj.G = G; cj.W = W; cj.max_len = pl.maxchunk;
    cj.rows_aligned = Fa % 4 == 0;
    switch (s.chunk_flags) {
        case ChunkFlags::ExtraSources:
            cj.flags2 = ws.tflTF; cj.colflags = ws.srows; cj.WScol = (size_t)Fa; cj.panel_rows = s.panel ? T : 0;
            break;
        case ChunkFlags::OrMore16:
            hipLaunchKernelGGL(k_or_spec_more16, grid1(N / 16, W), dim3(256), 0, r.st, ws.flagsTF, ws.srows, ws.tflTF, T, Fa / 16);
            LAUNCHCHK();
            break;
        case ChunkFlags::OrBytes:
            rc = launch_u8<1>(r, ws.tflTF, ws.flagsTF, N, N, N, W);
            break;
    }
    if (!rc) rc = launch_median(r, cj);
    if (!rc) rc = launch_colst(r, pl.swF, ws.Bw, ws.med, ws.fflFT, ws.d_chunk_ends, Fa, T, G, wsB, N, W);
    if (!rc) rc = launch_transpose<uint8_t>(r, ws.fflFT, ws.fflTF, Fa, T, N, N, W);
    return rc;
}

// the six intermediates of window 0 (tests), laid out as Debug says
static int iter_taps(const Run& r, const IterStep& s, const float* residTF) {
    const Ws& ws = r.ws;
    const int T = (int)r.pl.T, Fa = (int)r.pl.Fa, Wn = (int)r.Wb;
    const size_t N = (size_t)T * Fa;
    const Debug& d = *r.dbg;
    hipLaunchKernelGGL(k_gather_col_f32, dim3((unsigned)cdiv(Fa, 256)), dim3(256), 0, r.st, ws.sres, d.f32, Fa, Wn, 0);
    hipLaunchKernelGGL(k_gather_col_u8, dim3((unsigned)cdiv(Fa, 256)), dim3(256), 0, r.st, ws.sout, d.u8, Fa, Wn, 0);
    if (s.panel) {
        hipLaunchKernelGGL(k_unpanel<float>, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, r.st, residTF, d.f32 + Fa + N, T, Fa);
        hipLaunchKernelGGL(k_unpanel<uint8_t>, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, r.st, (const uint8_t*)ws.tflTF, d.u8 + Fa, T, Fa);
    } else {
        HIPCHK(hipMemcpyAsync(d.f32 + Fa + N, residTF, N * sizeof(float), hipMemcpyDeviceToDevice, r.st));
        HIPCHK(hipMemcpyAsync(d.u8 + Fa, ws.tflTF, N, hipMemcpyDeviceToDevice, r.st));
    }
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(d.f32 + Fa, ws.Bo, N * sizeof(float), hipMemcpyDeviceToDevice, r.st));
    HIPCHK(hipMemcpyAsync(d.u8 + Fa + N, ws.fflTF, N, hipMemcpyDeviceToDevice, r.st));
    return TRI_OK;
}

// flagging.py:973  _combine_flags (time smearing), flagging.py:975  _unaverage_freq (replication, frequency smearing,
// counts), then the final kernel
static int iter_finish(const Run& r, const IterStep& s, const void* vis, int vis_dtype, uint8_t* out_flags, bool update_iter) {
    const Ws& ws = r.ws;
    const int T = (int)r.pl.T, F = (int)r.pl.F, Fa = (int)r.pl.Fa, Wn = (int)r.Wb;
    const size_t N = (size_t)T * Fa;
    const int64_t W = r.Wb;
    const dim3 grid16((unsigned)cdiv(F / 16, 64), (unsigned)T, (unsigned)W);
    HIPCHK(hipMemsetAsync(ws.rowcnt, 0, (size_t)W * T * sizeof(int), r.st));
    switch (s.finish) {
        case Finish::FusedDilate:
            if (s.panel) hipLaunchKernelGGL(k_combine_dilate16<true>, grid16, dim3(64), 0, r.st, ws.srows, ws.tflTF, ws.fflTF, ws.dil, ws.rowcnt, T, F / 16, s.lo, s.hi);
            else hipLaunchKernelGGL(k_combine_dilate16<false>, grid16, dim3(64), 0, r.st, ws.srows, ws.tflTF, ws.fflTF, ws.dil, ws.rowcnt, T, F / 16, s.lo, s.hi);
            hipLaunchKernelGGL(k_colcount, grid1(F / 4, W), dim3(256), 0, r.st, ws.dil, ws.colcnt, T, F / 4);
            break;
        case Finish::Combine16Dilate:
            hipLaunchKernelGGL(k_combine16, grid1(N / 16, W), dim3(256), 0, r.st, ws.srows, ws.tflTF, ws.fflTF, ws.comb, T, Fa / 16, s.lo, s.hi);
            hipLaunchKernelGGL((k_unaverage16<-1, 3>), grid16, dim3(64), 0, r.st, ws.comb, ws.dil, ws.rowcnt, T, F / 16);
            hipLaunchKernelGGL(k_colcount, grid1(F / 4, W), dim3(256), 0, r.st, ws.dil, ws.colcnt, T, F / 4);
            break;
        case Finish::Combine16:
        case Finish::Combine:
            if (s.finish == Finish::Combine16)
                hipLaunchKernelGGL(k_combine16, grid1(N / 16, W), dim3(256), 0, r.st, ws.srows, ws.tflTF, ws.fflTF, ws.comb, T, Fa / 16, s.lo, s.hi);
            else
                hipLaunchKernelGGL(k_combine, grid1(N, W), dim3(256), 0, r.st, ws.sout, ws.tflTF, ws.fflTF, ws.comb, T, Fa, Wn, s.lo, s.hi);
            LAUNCHCHK();
            HIPCHK(hipMemsetAsync(ws.colcnt, 0, (size_t)W * F * sizeof(int), r.st));
            hipLaunchKernelGGL(k_unaverage, dim3((unsigned)cdiv(F, 256), (unsigned)T, (unsigned)W), dim3(256), 0, r.st, ws.comb, ws.dil, ws.rowcnt, ws.colcnt,
                               T, Fa, F, (int)r.pl.avg, s.flo, s.fhi);
            break;
    }
    LAUNCHCHK();
    return BY_VIS_DTYPE(launch_final, r, s, vis, out_flags, update_iter);
}
#undef BY_VIS_DTYPE

// One major iteration (_get_flags_impl, flagging.py:745-781) for a batch: the stages in the order of flagging.py:921-976.
int run_iteration(const Run& r, const IterStep& s, const void* vis, int vis_dtype, uint8_t* out_flags, bool update_iter, bool tap) {
    const float* residTF = nullptr;
    bool transpose_pending = false;
    int rc = iter_begin(r, s, vis, vis_dtype);
    if (!rc) rc = iter_spectrum(r, s);
    if (!rc) rc = iter_residual(r, s, &residTF, &transpose_pending);
    if (!rc) rc = iter_time_inputs(r, s, transpose_pending);
    if (!rc) rc = iter_sumthreshold(r, s, residTF);
    if (!rc && tap && r.dbg) rc = iter_taps(r, s, residTF);
    if (!rc) rc = iter_finish(r, s, vis, vis_dtype, out_flags, update_iter);
    return rc;
}

// All batches of the windows [w_begin, w_end) on r.st with the workspace [wsp, wsp + ws_bytes).
int process_windows(Run& r, const void* vis, int vis_dtype, const uint8_t* flags, uint8_t* out_flags,
                    int64_t w_begin, int64_t w_end, int64_t T, int64_t F, void* wsp, size_t ws_bytes, bool tap_first) {
    const tri_params* p = r.p;
    Ws probe;
    carve(r.pl, 1, nullptr, 0, true, &probe);
    if (probe.total > ws_bytes)
        return set_err(TRI_EWORKSPACE, "workspace of %zu bytes is smaller than the %zu needed for one window", ws_bytes, probe.total);
    // largest batch the workspace admits (the carve-up is monotone in Wb)
    int64_t lo = 1, hi = std::min<int64_t>(w_end - w_begin, 16384);
    while (lo < hi) {
        int64_t mid = (lo + hi + 1) / 2;
        carve(r.pl, mid, nullptr, 0, true, &probe);
        if (probe.total <= ws_bytes) lo = mid; else hi = mid - 1;
    }
    const int64_t Wb = lo;
    carve(r.pl, Wb, wsp, ws_bytes, false, &r.ws);

    // device tables
    ChunkTab ct;
    ct.n = (int)p->n_chunk_ends;
    for (int i = 0; i < ct.n; i++) ct.ends[i] = p->chunk_ends[i];
    {
        int nthr = (int)std::max<int64_t>(r.pl.Fa, ct.n);
        hipLaunchKernelGGL(k_tables, dim3((unsigned)cdiv(nthr, 256)), dim3(256), 0, r.st, ct, (int)T, (int)r.pl.Fa,
                           r.ws.d_chunk_ends, r.ws.d_tends, r.ws.segC_start, r.ws.segC_len, r.ws.segB_start,
                           r.ws.segB_len, r.ws.segT_start, r.ws.segT_len, r.ws.d_chunk_of);
        LAUNCHCHK();
    }
    const size_t NF = (size_t)T * F;
    const size_t esz = (vis_dtype == TRI_VIS_C64 || vis_dtype == TRI_VIS_F64) ? 8 : 4;
    // without channel averaging |vis| is the same in every major iteration:
    // compute it once per batch, in both layouts (TRI_NO_AMPL_CACHE=1 recomputes it per iteration)
    static const bool no_cache = is1(getenv("TRI_NO_AMPL_CACHE"));
    r.ampl_cached = r.pl.vec && !no_cache && p->num_major_iterations > 0;
    r.data_mask = (r.ampl_cached && r.pl.Fa == F) ? r.ws.iter : nullptr;
    r.data_mask_ws = (size_t)T * r.pl.Fa;
    const IterStep step = pick_iteration(r);
    int rc = TRI_OK;
    for (int64_t w0 = w_begin; w0 < w_end; w0 += Wb) {
        r.Wb = std::min(Wb, w_end - w0);
        const char* vis_b = (const char*)vis + (size_t)w0 * NF * esz;
        uint8_t* out_b = out_flags + (size_t)w0 * NF;
        // flagging.py:1182  iter_flags = flags.copy()  (non-zero = flagged)
        rc = launch_u8<2>(r, flags + (size_t)w0 * NF, r.ws.iter, NF, NF, NF, r.Wb);
        if (rc) return rc;
        if (r.ampl_cached) {
            const size_t n4 = (size_t)r.Wb * NF / 4;
            if (vis_dtype == TRI_VIS_C64)
                hipLaunchKernelGGL(k_amplitude4<TRI_VIS_C64>, dim3((unsigned)cdiv(n4, 256)), dim3(256), 0, r.st, (const void*)vis_b, r.ws.dataTF, r.ws.iter, r.ws.nanmask, n4);
            else
                hipLaunchKernelGGL(k_amplitude4<TRI_VIS_F32>, dim3((unsigned)cdiv(n4, 256)), dim3(256), 0, r.st, (const void*)vis_b, r.ws.dataTF, r.ws.iter, r.ws.nanmask, n4);
            LAUNCHCHK();
            rc = launch_transpose<float>(r, r.ws.dataTF, r.ws.dataFT, (int)T, (int)r.pl.Fa, NF, NF, r.Wb);
            if (rc) return rc;
        }
        for (int64_t it = 0; it < p->num_major_iterations; it++) {
            bool last = it == p->num_major_iterations - 1;
            bool tap = last && tap_first && w0 == w_begin;
            rc = run_iteration(r, step, vis_b, vis_dtype, out_b, !last, tap);
            if (rc) return rc;
        }
    }
    return TRI_OK;
}

// Optional schedule (TRI_SUBSTREAMS=1): two internal streams per calling thread (created once).  A window set
// whose 1-D spectrum path is a long sequential recurrence on a handful of lanes (SKA-sized windows:
// 65536-channel lines, one lane per window) is split in two halves that run concurrently -- the high-priority
// half at full speed, the other one in the gaps its spectrum kernels leave on the device.
struct SubStreams {
    hipStream_t st[2] = {nullptr, nullptr};
    hipEvent_t fork = nullptr, join[2] = {nullptr, nullptr};
    int device = -1;
};
thread_local SubStreams g_sub;

int get_substreams(SubStreams** out) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (g_sub.device != dev) {
        if (g_sub.device >= 0) return set_err(TRI_EUNSUPPORTED, "a calling thread must stay on one device");
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));    // lo = least, hi = greatest priority (numerically lower)
        // (made in owning locals and kept only once all five exist: a failed create leaks nothing)
        HipStream st0, st1;
        HipEvent fork, join0, join1;
        HIPCHK(hipStreamCreateWithPriority(st0.out(), hipStreamNonBlocking, hi));
        HIPCHK(hipStreamCreateWithPriority(st1.out(), hipStreamNonBlocking, lo));
        HIPCHK(hipEventCreateWithFlags(fork.out(), hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(join0.out(), hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(join1.out(), hipEventDisableTiming));
        g_sub.st[0] = st0.release();
        g_sub.st[1] = st1.release();
        g_sub.fork = fork.release();
        g_sub.join[0] = join0.release();
        g_sub.join[1] = join1.release();
        g_sub.device = dev;
    }
    *out = &g_sub;
    return TRI_OK;
}

// TRI_SUBSTREAMS=0 / 1 forces the single-stream / two-stream schedule; -1 when unset.  Read per call: tests toggle it
static int substreams_forced() {
    const char* fe = getenv("TRI_SUBSTREAMS");
    return fe ? atoi(fe) : -1;
}

// The side lane of the calling thread on the current device (created once, owned like the SubStreams), or NULL: under
// TRI_SUBSTREAMS=0, and when a stream or an event cannot be made -- the caller then keeps the single-stream order.
thread_local SideLane g_side;
const SideLane* get_side_lane() {
    if (substreams_forced() == 0) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (g_side.device == dev) return &g_side;
    if (g_side.device >= 0) return nullptr;              // (a calling thread stays on one device)
    HipStream st;
    HipEvent fork, join;
    // (a plain stream: the priority a caller's stream has unless it asked for another -- neither kernel of a pair is preferred)
    const bool ok = hipStreamCreateWithFlags(st.out(), hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(fork.out(), hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(join.out(), hipEventDisableTiming) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); return nullptr; }
    g_side.st = st.release();
    g_side.fork = fork.release();
    g_side.join = join.release();
    g_side.device = dev;
    return &g_side;
}

int flagger_impl(const void* vis, int vis_dtype, const uint8_t* flags, uint8_t* out_flags,
                 int64_t n_cp, int64_t T, int64_t F, const tri_params* p, void* workspace,
                 size_t workspace_bytes, void* stream, Debug* dbg) {
    if (!vis || !flags || !out_flags || !p) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_cp < 0) return set_err(TRI_EINVAL, "negative window count");
    if (vis_dtype != TRI_VIS_C64 && vis_dtype != TRI_VIS_F32 && vis_dtype != TRI_VIS_F64)
        return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64, float32 or float64 amplitudes");
    Run r;
    r.st = (hipStream_t)stream;
    r.p = p;
    r.dbg = dbg;
    int rc = make_plan(T, F, p, &r.pl);
    if (rc) return rc;
    if (r.pl.G > TRI_MAX_CHUNKS) return set_err(TRI_EUNSUPPORTED, "at most %d frequency chunks", TRI_MAX_CHUNKS);
    // the 16-byte kernels need 16-byte aligned user buffers (torch allocations are)
    if ((((uintptr_t)vis) | ((uintptr_t)flags) | ((uintptr_t)out_flags)) & 15) r.pl.vec = false;
    if (vis_dtype == TRI_VIS_F64) r.pl.vec = false;       // float64 amplitudes: the scalar preparation / final kernels (rare input type)
    if (n_cp == 0) return TRI_OK;
    if (!workspace) return set_err(TRI_EWORKSPACE, "NULL workspace");
    if (((uintptr_t)workspace & 255) != 0) return set_err(TRI_EINVAL, "workspace must be 256-byte aligned");
    if (p->num_major_iterations == 0)
        HIPCHK(hipMemsetAsync(out_flags, 0, (size_t)n_cp * (size_t)T * F, r.st));

    const int force = substreams_forced();
    Ws probe;
    carve(r.pl, 1, nullptr, 0, true, &probe);
    const size_t half = (workspace_bytes / 2) & ~(size_t)255;
    const bool can_split = n_cp >= 2 && half >= probe.total && dbg == nullptr;
    // (off by default: on slabs of 64 SKA-sized windows the halves lose more parallelism in the 2-D kernels --
    //  512 lines per window on the frequency axis -- than the overlap of the spectrum kernels returns:
    //  1.5 against 2.5 Gvis/s, profiles/r02_bench_ska.log)
    const bool want_split = force == 1;
    if (!(can_split && want_split)) {
        // one stream for the windows, the side lane for the independent launch pairs inside a major iteration (the halves
        // of the split below are on internal streams already and get none)
        r.side = get_side_lane();
        return process_windows(r, vis, vis_dtype, flags, out_flags, 0, n_cp, T, F, workspace, workspace_bytes, true);
    }

    SubStreams* ss = nullptr;
    rc = get_substreams(&ss);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ss->fork, r.st));
    const int64_t mid = (n_cp + 1) / 2;
    for (int k = 0; k < 2 && rc == TRI_OK; k++) {
        Run rk;
        rk.st = ss->st[k];
        rk.p = p;
        rk.dbg = nullptr;
        rk.pl = r.pl;
        HIPCHK(hipStreamWaitEvent(rk.st, ss->fork, 0));
        rc = process_windows(rk, vis, vis_dtype, flags, out_flags, k == 0 ? 0 : mid, k == 0 ? mid : n_cp, T, F,
                             (char*)workspace + (size_t)k * half, half, false);
        // join even after an error: the caller's stream must not run ahead of work already queued
        (void)hipEventRecord(ss->join[k], rk.st);
        (void)hipStreamWaitEvent(r.st, ss->join[k], 0);
    }
    return rc;
}

}  // namespace

extern "C" int tri_sum_threshold_flagger(const void* vis, int vis_dtype, const uint8_t* flags,
                                         uint8_t* out_flags, int64_t n_cp, int64_t ntime,
                                         int64_t nchan, const tri_params* p, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    return flagger_impl(vis, vis_dtype, flags, out_flags, n_cp, ntime, nchan, p, workspace,
                        workspace_bytes, stream, nullptr);
}

// Test hook: as above, additionally taps the last major iteration's
// intermediates of window 0 into caller-provided device buffers:
//   dbg_f32: [spec_resid (Fa)][background, FT layout (Fa*T)][residual, TF layout (T*Fa)]
//   dbg_u8 : [spec_flags (Fa)][time_flags TF (T*Fa)][freq_flags TF (T*Fa)]
extern "C" int tri_sum_threshold_flagger_debug(const void* vis, int vis_dtype, const uint8_t* flags,
                                               uint8_t* out_flags, int64_t n_cp, int64_t ntime,
                                               int64_t nchan, const tri_params* p, void* workspace,
                                               size_t workspace_bytes, void* stream,
                                               float* dbg_f32, uint8_t* dbg_u8) {
    Debug d{dbg_f32, dbg_u8};
    return flagger_impl(vis, vis_dtype, flags, out_flags, n_cp, ntime, nchan, p, workspace,
                        workspace_bytes, stream, (dbg_f32 && dbg_u8) ? &d : nullptr);
}

extern "C" int tri_abs_c64(const void* z, float* out, int64_t n, void* stream) {
    if (!z || !out || n < 0) return set_err(TRI_EINVAL, "bad argument");
    if (n == 0) return TRI_OK;
    hipLaunchKernelGGL(k_abs_c64, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const float2*)z, out, (size_t)n);
    LAUNCHCHK();
    return TRI_OK;
}

extern "C" int tri_fill_windows(void* vis_windows_c64, uint8_t* flag_windows, int64_t n, void* stream) {
    if (!vis_windows_c64 || !flag_windows || n < 0) return set_err(TRI_EINVAL, "bad argument");
    if (n == 0) return TRI_OK;
    hipLaunchKernelGGL(k_fill_windows, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (float2*)vis_windows_c64, flag_windows, (size_t)n);
    LAUNCHCHK();
    return TRI_OK;
}

// Rows of the pack / unpack entry points: launch(r0, nr) for each slab [r0, r0 + nr) of [0, rows), at most 65535 rows
// (gridDim.y) each.  The kernels index with int: a dimension above 2^31 - 1 is refused.
template <class Launch>
static int for_row_slabs(int64_t rows, int64_t nchan, int64_t ncorr, int64_t nbl, int64_t ntime, Launch&& launch) {
    if (rows == 0) return TRI_OK;
    if (rows > 0x7FFFFFFF || nchan > 0x7FFFFFFF || ncorr > 0x7FFFFFFF || nbl > 0x7FFFFFFF || ntime > 0x7FFFFFFF)
        return set_err(TRI_EUNSUPPORTED, "dimension too large for one call");
    for (int64_t r0 = 0; r0 < rows; r0 += 65535) {
        launch(r0, (unsigned)std::min<int64_t>(65535, rows - r0));
        LAUNCHCHK();
    }
    return TRI_OK;
}

extern "C" int tri_pack_data(const void* data_c64, const uint8_t* flag, const int32_t* row_bl,
                             const int32_t* row_time, int64_t rows, int64_t nchan, int64_t ncorr,
                             int64_t nbl, int64_t ntime, void* vis_windows_c64,
                             uint8_t* flag_windows, void* stream) {
    if (!data_c64 || !flag || !row_bl || !row_time || !vis_windows_c64 || !flag_windows)
        return set_err(TRI_EINVAL, "NULL pointer argument");
    if (rows < 0 || nchan <= 0 || ncorr <= 0 || nbl < 0 || ntime < 0) return set_err(TRI_EINVAL, "bad shape");
    // 1 / 2 / 4 correlations with 16-byte aligned rows: vector loads of a thread's (chan, corr) piece
    const bool al = ((uintptr_t)data_c64 % 16 == 0) && ((uintptr_t)flag % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    return for_row_slabs(rows, nchan, ncorr, nbl, ntime, [&](int64_t r0, unsigned nr) {
        const dim3 grid((unsigned)cdiv(nchan, 256), nr, 1);
        const float2* dsl = (const float2*)data_c64 + (size_t)r0 * nchan * ncorr;
        const uint8_t* fsl = flag + (size_t)r0 * nchan * ncorr;
        if (ncorr == 4 && al)
            hipLaunchKernelGGL(k_pack_v<4>, grid, dim3(256), 0, st, dsl, fsl, row_bl + r0, row_time + r0,
                               (int)nchan, (int)nbl, (int)ntime, (float2*)vis_windows_c64, flag_windows);
        else if (ncorr == 2 && al)
            hipLaunchKernelGGL(k_pack_v<2>, grid, dim3(256), 0, st, dsl, fsl, row_bl + r0, row_time + r0,
                               (int)nchan, (int)nbl, (int)ntime, (float2*)vis_windows_c64, flag_windows);
        else if (ncorr == 1)
            hipLaunchKernelGGL(k_pack_v<1>, grid, dim3(256), 0, st, dsl, fsl, row_bl + r0, row_time + r0,
                               (int)nchan, (int)nbl, (int)ntime, (float2*)vis_windows_c64, flag_windows);
        else
            hipLaunchKernelGGL(k_pack, grid, dim3(256), 0, st, dsl, fsl,
                               row_bl + r0, row_time + r0, (int)nchan, (int)ncorr, (int)nbl, (int)ntime,
                               (float2*)vis_windows_c64, flag_windows);
    });
}

extern "C" int tri_unpack_data(const uint8_t* flag_windows, const int32_t* row_bl,
                               const int32_t* row_time, int64_t rows, int64_t nchan, int64_t ncorr,
                               int64_t nbl, int64_t ntime, uint8_t* out_flags, int any_corr,
                               void* stream) {
    if (!flag_windows || !row_bl || !row_time || !out_flags) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (rows < 0 || nchan <= 0 || ncorr <= 0 || nbl < 0 || ntime < 0) return set_err(TRI_EINVAL, "bad shape");
    const bool al = (uintptr_t)out_flags % 4 == 0;
    hipStream_t st = (hipStream_t)stream;
    return for_row_slabs(rows, nchan, ncorr, nbl, ntime, [&](int64_t r0, unsigned nr) {
        const dim3 grid((unsigned)cdiv(nchan, 256), nr, 1);
        uint8_t* osl = out_flags + (size_t)r0 * nchan * ncorr;
        if (ncorr == 4 && al)
            hipLaunchKernelGGL(k_unpack_v<4>, grid, dim3(256), 0, st, flag_windows, row_bl + r0, row_time + r0,
                               (int)nchan, (int)nbl, (int)ntime, osl, any_corr);
        else if (ncorr == 2 && al)
            hipLaunchKernelGGL(k_unpack_v<2>, grid, dim3(256), 0, st, flag_windows, row_bl + r0, row_time + r0,
                               (int)nchan, (int)nbl, (int)ntime, osl, any_corr);
        else if (ncorr == 1)
            hipLaunchKernelGGL(k_unpack_v<1>, grid, dim3(256), 0, st, flag_windows, row_bl + r0, row_time + r0,
                               (int)nchan, (int)nbl, (int)ntime, osl, any_corr);
        else
            hipLaunchKernelGGL(k_unpack, grid, dim3(256), 0, st, flag_windows, row_bl + r0, row_time + r0,
                               (int)nchan, (int)ncorr, (int)nbl, (int)ntime, osl, any_corr);
    });
}

// host term tables (idx = (c1, c2, s1, s2), alpha = (re, im) per term) -> StokesTerm; false if a
// correlation index is outside [0, ncorr)
static bool fill_stokes_terms(StokesTerm* dst, const int32_t* idx, const double* alpha, int64_t cnt, int64_t ncorr) {
    for (int64_t k = 0; k < cnt; k++) {
        dst[k].c1 = idx[4 * k];
        dst[k].c2 = idx[4 * k + 1];
        dst[k].s1 = idx[4 * k + 2];
        dst[k].s2 = idx[4 * k + 3];
        dst[k].ar = alpha[2 * k];
        dst[k].ai = alpha[2 * k + 1];
        if (dst[k].c1 < 0 || dst[k].c1 >= ncorr || dst[k].c2 < 0 || dst[k].c2 >= ncorr) return false;
    }
    return true;
}

// mode and term tables of the scan pack entry points -> terms (none in mode 0)
static int scan_stokes_terms(int mode, const int32_t* pol_idx, const double* pol_alpha, int64_t n_pol, int64_t ncorr,
                             StokesTerms& terms) {
    if (mode < 0 || mode > 2) return set_err(TRI_EINVAL, "mode must be 0 (standard), 1 (polarisation) or 2 (total_power)");
    terms.n_pol = 0;
    terms.n_unpol = 0;
    if (mode != 0) {
        if (n_pol <= 0) return set_err(TRI_EINVAL, "modes 1 and 2 need at least one stokes term");
        if (n_pol > TRI_MAX_STOKES_TERMS) return set_err(TRI_EUNSUPPORTED, "at most 4 stokes terms");
        if (!pol_idx || !pol_alpha) return set_err(TRI_EINVAL, "NULL pointer argument");
        terms.n_pol = (int)n_pol;
        if (!fill_stokes_terms(terms.pol, pol_idx, pol_alpha, n_pol, ncorr))
            return set_err(TRI_EINVAL, "correlation index out of range");
    }
    return TRI_OK;
}

extern "C" int tri_pack_scan(const void* data_c64, const void* model_c64, const uint8_t* flag,
                             const int32_t* row_bl, const int32_t* row_time, int64_t rows, int64_t nchan,
                             int64_t ncorr, int64_t nbl, int64_t ntime, int mode, const int32_t* pol_idx,
                             const double* pol_alpha, int64_t n_pol, void* vis_windows_c64,
                             uint8_t* flag_windows, void* stream) {
    if (!data_c64 || !row_bl || !row_time || !vis_windows_c64 || !flag_windows)
        return set_err(TRI_EINVAL, "NULL pointer argument");
    if (rows < 0 || nchan <= 0 || ncorr <= 0 || nbl < 0 || ntime < 0) return set_err(TRI_EINVAL, "bad shape");
    StokesTerms terms;
    if (const int rc = scan_stokes_terms(mode, pol_idx, pol_alpha, n_pol, ncorr, terms)) return rc;
    const bool stokes = mode != 0;
    // 1 / 2 / 4 correlations with 16-byte aligned rows: vector loads of a thread's (chan, corr) piece
    const bool al = (uintptr_t)data_c64 % 16 == 0 && (uintptr_t)model_c64 % 16 == 0 && (uintptr_t)flag % 4 == 0;
    const bool vec = al && (ncorr == 4 || ncorr == 2 || ncorr == 1);
    hipStream_t st = (hipStream_t)stream;
    float2* vw = (float2*)vis_windows_c64;
    return for_row_slabs(rows, nchan, ncorr, nbl, ntime, [&](int64_t r0, unsigned nr) {
        const dim3 grid((unsigned)cdiv(nchan, 256), nr, 1);
        const size_t off = (size_t)r0 * nchan * ncorr;
        const float2* d = (const float2*)data_c64 + off;
        const float2* m = model_c64 ? (const float2*)model_c64 + off : nullptr;
        const uint8_t* fl = flag ? flag + off : nullptr;
        const int32_t* rb = row_bl + r0;
        const int32_t* rt = row_time + r0;
#define TRI_PACK_SCAN_V(NC, S)                                                                                      \
        do {                                                                                                         \
            if (m && fl)  hipLaunchKernelGGL((k_pack_scan_v<NC, S, true, true>), grid, dim3(256), 0, st, d, m, fl,   \
                                             rb, rt, (int)nchan, (int)nbl, (int)ntime, terms, vw, flag_windows);     \
            else if (m)   hipLaunchKernelGGL((k_pack_scan_v<NC, S, true, false>), grid, dim3(256), 0, st, d, m, fl,  \
                                             rb, rt, (int)nchan, (int)nbl, (int)ntime, terms, vw, flag_windows);     \
            else if (fl)  hipLaunchKernelGGL((k_pack_scan_v<NC, S, false, true>), grid, dim3(256), 0, st, d, m, fl,  \
                                             rb, rt, (int)nchan, (int)nbl, (int)ntime, terms, vw, flag_windows);     \
            else          hipLaunchKernelGGL((k_pack_scan_v<NC, S, false, false>), grid, dim3(256), 0, st, d, m, fl, \
                                             rb, rt, (int)nchan, (int)nbl, (int)ntime, terms, vw, flag_windows);     \
        } while (0)
        if (vec && ncorr == 4 && stokes) TRI_PACK_SCAN_V(4, true);
        else if (vec && ncorr == 4) TRI_PACK_SCAN_V(4, false);
        else if (vec && ncorr == 2 && stokes) TRI_PACK_SCAN_V(2, true);
        else if (vec && ncorr == 2) TRI_PACK_SCAN_V(2, false);
        else if (vec && ncorr == 1 && stokes) TRI_PACK_SCAN_V(1, true);
        else if (vec && ncorr == 1) TRI_PACK_SCAN_V(1, false);
        else
            hipLaunchKernelGGL(k_pack_scan, grid, dim3(256), 0, st, d, m, fl, rb, rt, (int)nchan, (int)ncorr,
                               (int)nbl, (int)ntime, stokes ? 1 : 0, terms, vw, flag_windows);
#undef TRI_PACK_SCAN_V
    });
}

extern "C" int tri_unpack_scan(const uint8_t* flag_windows, const int32_t* row_bl, const int32_t* row_time,
                               int64_t rows, int64_t nchan, int64_t wcorr, int64_t out_ncorr, int64_t nbl,
                               int64_t ntime, uint8_t* out_flags, void* stream) {
    if (!flag_windows || !row_bl || !row_time || !out_flags) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (rows < 0 || nchan <= 0 || out_ncorr <= 0 || nbl < 0 || ntime < 0) return set_err(TRI_EINVAL, "bad shape");
    if (wcorr != 1 && wcorr != out_ncorr) return set_err(TRI_EINVAL, "wcorr must be 1 or out_ncorr");
    hipStream_t st = (hipStream_t)stream;
    return for_row_slabs(rows, nchan, out_ncorr, nbl, ntime, [&](int64_t r0, unsigned nr) {
        const dim3 grid((unsigned)cdiv(nchan, 256), nr, 1);
        uint8_t* osl = out_flags + (size_t)r0 * nchan * out_ncorr;
        if (out_ncorr == 4 && (uintptr_t)out_flags % 4 == 0)
            hipLaunchKernelGGL(k_unpack_scan<4>, grid, dim3(256), 0, st, flag_windows, row_bl + r0,
                               row_time + r0, (int)nchan, (int)wcorr, 4, (int)nbl, (int)ntime, osl);
        else
            hipLaunchKernelGGL(k_unpack_scan<0>, grid, dim3(256), 0, st, flag_windows, row_bl + r0,
                               row_time + r0, (int)nchan, (int)wcorr, (int)out_ncorr, (int)nbl, (int)ntime, osl);
    });
}

extern "C" int tri_pack_scan_rows(const void* data_c64, const void* model_c64, const uint8_t* flag,
                                  const int64_t* src_row, int64_t src_rows, const int32_t* row_bl,
                                  const int32_t* row_time, int64_t n, int64_t nchan, int64_t ncorr, int64_t nbl,
                                  int64_t ntime, int mode, const int32_t* pol_idx, const double* pol_alpha,
                                  int64_t n_pol, void* vis_windows_c64, uint8_t* flag_windows, void* stream) {
    if (!data_c64 || !row_bl || !row_time || !vis_windows_c64 || !flag_windows)
        return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n < 0 || src_rows < 0 || nchan <= 0 || ncorr <= 0 || nbl < 0 || ntime < 0) return set_err(TRI_EINVAL, "bad shape");
    if (!src_row && n > src_rows) return set_err(TRI_EINVAL, "a list without src_row reads rows [0, n): n > src_rows");
    StokesTerms terms;
    if (const int rc = scan_stokes_terms(mode, pol_idx, pol_alpha, n_pol, ncorr, terms)) return rc;
    const bool stokes = mode != 0;
    // the vector path of tri_pack_scan: 1 / 2 / 4 correlations with 16-byte aligned rows
    const bool al = (uintptr_t)data_c64 % 16 == 0 && (uintptr_t)model_c64 % 16 == 0 && (uintptr_t)flag % 4 == 0;
    const bool vec = al && (ncorr == 4 || ncorr == 2 || ncorr == 1);
    hipStream_t st = (hipStream_t)stream;
    const float2* d = (const float2*)data_c64;
    const float2* m = (const float2*)model_c64;
    const uint8_t* fl = flag;
    float2* vw = (float2*)vis_windows_c64;
    return for_row_slabs(n, nchan, ncorr, nbl, ntime, [&](int64_t e0, unsigned nr) {
        const dim3 grid((unsigned)cdiv(nchan, 256), nr, 1);
#define TRI_PACK_SCAN_ROWS_V(NC, S)                                                                                 \
        do {                                                                                                         \
            if (m && fl)  hipLaunchKernelGGL((k_pack_scan_rows_v<NC, S, true, true>), grid, dim3(256), 0, st, d, m,  \
                                             fl, src_row, src_rows, row_bl, row_time, e0, (int)nchan, (int)nbl,      \
                                             (int)ntime, terms, vw, flag_windows);                                   \
            else if (m)   hipLaunchKernelGGL((k_pack_scan_rows_v<NC, S, true, false>), grid, dim3(256), 0, st, d, m, \
                                             fl, src_row, src_rows, row_bl, row_time, e0, (int)nchan, (int)nbl,      \
                                             (int)ntime, terms, vw, flag_windows);                                   \
            else if (fl)  hipLaunchKernelGGL((k_pack_scan_rows_v<NC, S, false, true>), grid, dim3(256), 0, st, d, m, \
                                             fl, src_row, src_rows, row_bl, row_time, e0, (int)nchan, (int)nbl,      \
                                             (int)ntime, terms, vw, flag_windows);                                   \
            else          hipLaunchKernelGGL((k_pack_scan_rows_v<NC, S, false, false>), grid, dim3(256), 0, st, d,   \
                                             m, fl, src_row, src_rows, row_bl, row_time, e0, (int)nchan, (int)nbl,   \
                                             (int)ntime, terms, vw, flag_windows);                                   \
        } while (0)
        if (vec && ncorr == 4 && stokes) TRI_PACK_SCAN_ROWS_V(4, true);
        else if (vec && ncorr == 4) TRI_PACK_SCAN_ROWS_V(4, false);
        else if (vec && ncorr == 2 && stokes) TRI_PACK_SCAN_ROWS_V(2, true);
        else if (vec && ncorr == 2) TRI_PACK_SCAN_ROWS_V(2, false);
        else if (vec && ncorr == 1 && stokes) TRI_PACK_SCAN_ROWS_V(1, true);
        else if (vec && ncorr == 1) TRI_PACK_SCAN_ROWS_V(1, false);
        else
            hipLaunchKernelGGL(k_pack_scan_rows, grid, dim3(256), 0, st, d, m, fl, src_row, src_rows, row_bl, row_time,
                               e0, (int)nchan, (int)ncorr, (int)nbl, (int)ntime, stokes ? 1 : 0, terms, vw,
                               flag_windows);
#undef TRI_PACK_SCAN_ROWS_V
    });
}

extern "C" int tri_unpack_scan_rows(const uint8_t* flag_windows, const int64_t* dst_row, int64_t out_rows,
                                    const int32_t* row_bl, const int32_t* row_time, int64_t n, int64_t nchan,
                                    int64_t wcorr, int64_t out_ncorr, int64_t nbl, int64_t ntime, uint8_t* out_flags,
                                    void* stream) {
    if (!flag_windows || !row_bl || !row_time || !out_flags) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n < 0 || out_rows < 0 || nchan <= 0 || out_ncorr <= 0 || nbl < 0 || ntime < 0)
        return set_err(TRI_EINVAL, "bad shape");
    if (wcorr != 1 && wcorr != out_ncorr) return set_err(TRI_EINVAL, "wcorr must be 1 or out_ncorr");
    if (!dst_row && n > out_rows) return set_err(TRI_EINVAL, "a list without dst_row writes rows [0, n): n > out_rows");
    hipStream_t st = (hipStream_t)stream;
    return for_row_slabs(n, nchan, out_ncorr, nbl, ntime, [&](int64_t e0, unsigned nr) {
        const dim3 grid((unsigned)cdiv(nchan, 256), nr, 1);
        if (out_ncorr == 4 && (uintptr_t)out_flags % 4 == 0)
            hipLaunchKernelGGL(k_unpack_scan_rows<4>, grid, dim3(256), 0, st, flag_windows, dst_row, out_rows, row_bl,
                               row_time, e0, (int)nchan, (int)wcorr, 4, (int)nbl, (int)ntime, out_flags);
        else
            hipLaunchKernelGGL(k_unpack_scan_rows<0>, grid, dim3(256), 0, st, flag_windows, dst_row, out_rows, row_bl,
                               row_time, e0, (int)nchan, (int)wcorr, (int)out_ncorr, (int)nbl, (int)ntime, out_flags);
    });
}

// Measurement / test hook: ONE rejection step of the background loop (flagging.py:553-574) as the flagger runs it for blocks
// of >= 65536 samples: k_mr_predict, two rounds of k_mr_pass + k_mr_finish, the redo kernel (K3t).  resid: (n_win, n_chan, n_time)
// float32 = |data - background| in the FT layout, flags_in: (n_win, n_chan, n_time) bytes; flags_out (FT bytes), flags_t4 (TF4 words,
// (n_win, n_time / 4, n_chan) x 4 bytes) and med (n_win, n_chunks) float64 receive the results.
extern "C" int tri_bench_reject(const float* resid, const uint8_t* flags_in, uint8_t* flags_out, uint8_t* flags_t4, double* med,
                                int64_t n_win, int64_t n_chan, int64_t n_time, const int64_t* chunk_ends, int64_t n_chunk_ends,
                                double reject, int repeats, float* ms_per_step, void* stream) {
    if (!resid || !flags_in || !flags_out || !flags_t4 || !med || !chunk_ends || !ms_per_step) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win <= 0 || n_win > 65535 || n_chan <= 0 || n_time <= 0 || n_time % 4 != 0 || n_chunk_ends < 2 || n_chunk_ends > 256 || repeats <= 0)
        return set_err(TRI_EINVAL, "bad shape");
    if ((uint64_t)n_chan * (uint64_t)n_time * 4u >= (1ull << 31)) return set_err(TRI_EUNSUPPORTED, "a window of 2^31 bytes or more");
    const int G = (int)n_chunk_ends - 1, T = (int)n_time, Fa = (int)n_chan;
    int64_t maxchunk = 0, minchunk = n_chan;
    int ytiles = 0;
    for (int g = 0; g < G; g++) {
        const int64_t c = chunk_ends[g + 1] - chunk_ends[g];
        if (c <= 0 || chunk_ends[g] < 0 || chunk_ends[g + 1] > n_chan) return set_err(TRI_EINVAL, "bad chunk");
        maxchunk = std::max(maxchunk, c); minchunk = std::min(minchunk, c);
        ytiles += (int)cdiv(c, 64);
    }
    if (chunk_ends[0] != 0 || chunk_ends[G] != n_chan) return set_err(TRI_EINVAL, "chunks must cover the channels");
    if (minchunk * (int64_t)T < 65536 || ytiles > 65535) return set_err(TRI_EUNSUPPORTED, "blocks below 65536 samples take the two-kernel route");
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)Fa * T;
    const size_t nb = (size_t)maxchunk * T, ccap = (nb / 4) & ~(size_t)3, ucap = (nb / 8) & ~(size_t)3;
    const size_t wsS = mrt_scratch_words(G, ccap, ucap);
    DevBuf<unsigned> scb;
    DevBuf<int64_t> endsb;
    HIPCHK(scb.alloc((size_t)n_win * wsS));
    HIPCHK(endsb.alloc((size_t)n_chunk_ends));
    unsigned* sc = scb.get();
    int64_t* d_ends = endsb.get();
    HIPCHK(hipMemcpyAsync(d_ends, chunk_ends, (size_t)n_chunk_ends * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    const double rej = TRI_MAD_NORMAL * reject;
    HipEvent e0, e1;
    HIPCHK(hipEventCreate(e0.out()));
    HIPCHK(hipEventCreate(e1.out()));
    const unsigned W = (unsigned)n_win;
    HIPCHK(hipEventRecord(e0.get(), st));
    for (int i = 0; i < repeats; i++) {
        hipLaunchKernelGGL(k_mr_predict, dim3((unsigned)G, W), dim3(256), 0, st, resid, flags_in, d_ends, rej, T / 4, G, N, N, sc, wsS, ccap, ucap, 0);
        for (unsigned round = 1; round <= 2; round++) {
            hipLaunchKernelGGL(k_mr_pass, dim3((unsigned)cdiv(T / 4, 64), (unsigned)ytiles, W), dim3(256), 0, st, resid, flags_in, flags_out, flags_t4,
                               d_ends, Fa, T / 4, G, N, N, sc, wsS, ccap, ucap, round);
            hipLaunchKernelGGL(k_mr_finish, dim3((unsigned)G, W), dim3(256), 0, st, resid, flags_in, flags_out, flags_t4, med, d_ends, rej, Fa, T / 4, G,
                               N, N, sc, wsS, ccap, ucap, round);
        }
        hipLaunchKernelGGL(k_median_reject, dim3((unsigned)G, W), dim3(256), 0, st, resid, flags_in, flags_out, flags_t4, med, d_ends, rej, Fa, T / 4, G,
                           N, N, sc, wsS, 0u, 0u, 1, (const unsigned*)sc, wsS, (int)MRT_PARW, 11);
    }
    HIPCHK(hipEventRecord(e1.get(), st));
    hipError_t le = hipGetLastError();
    hipError_t se = hipEventSynchronize(e1.get());
    float ms = 0.f;
    if (le == hipSuccess && se == hipSuccess) (void)hipEventElapsedTime(&ms, e0.get(), e1.get());
    if (le != hipSuccess) return set_err(TRI_EHIP, "launch: %s", hipGetErrorString(le));
    if (se != hipSuccess) return set_err(TRI_EHIP, "sync: %s", hipGetErrorString(se));
    *ms_per_step = ms / (float)repeats;
    return TRI_OK;
}

// The body of tri_bench_sumthreshold ({0, n_line}, the measurement hook's own pick for variant 0) and of
// tri_test_sumthreshold (the caller's chunks, launch_colst's pick): G = n_chunk_ends - 1 line groups per column.
static int st_hook(const float* data, const double* mad, uint8_t* out, int64_t n_win, int64_t n_line, int64_t n_col,
                   const int64_t* windows, int64_t n_windows, double outlier_nsigma, double rho, int variant, int repeats,
                   float* ms_per_launch, void* stream, const int64_t* chunk_ends, int64_t n_chunk_ends, bool flagger_pick) {
    if (!data || !mad || !out || !windows || !ms_per_launch || !chunk_ends) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win <= 0 || n_line <= 0 || n_col <= 0 || repeats <= 0 || n_win > 65535) return set_err(TRI_EINVAL, "bad shape");
    if (n_chunk_ends < 2 || n_chunk_ends > 256) return set_err(TRI_EINVAL, "2 .. 256 chunk ends");
    for (int64_t g = 0; g < n_chunk_ends; g++)
        if (chunk_ends[g] < 0 || chunk_ends[g] > n_line || (g > 0 && chunk_ends[g] < chunk_ends[g - 1]))
            return set_err(TRI_EINVAL, "chunk ends must not decrease and must lie in [0, n_line]");
    const int G = (int)n_chunk_ends - 1;
    const int64_t o0 = chunk_ends[0], o1 = chunk_ends[G];     // the lines the kernels write
    hipStream_t st = (hipStream_t)stream;
    StWin sw;
    int rc = make_stwin(windows, n_windows, rho, &sw);
    if (rc) return rc;
    double thr_scale = outlier_nsigma * TRI_MAD_NORMAL;
    size_t nthreads = (size_t)n_win * n_col * G;             // (k_colst_dyn: one ring per (window, chunk, column))
    int C = (int)n_col, L = (int)n_line;
    bool can_fuse = sw.nw == 4 && sw.w[0] == 1 && sw.w[1] == 2 && sw.w[2] == 4 && sw.w[3] == 8;
    if ((variant == 2 || variant == 3) && !can_fuse) return set_err(TRI_EUNSUPPORTED, "register cascade needs windows (1,2,4,8)");
    if (variant == 3 && !((uint64_t)L * (uint64_t)C * 4u < (1ull << 31)))
        return set_err(TRI_EUNSUPPORTED, "lane-mask cascade needs a window below 2^31 bytes");
    // variant 5 (round 4): the lane-mask cascade on COLUMN PANELS, as the flagger's time-axis pass runs it -- the row images
    // handed in are re-laid out before the timed region and the flags taken back to rows after it
    if (variant == 5 && !(can_fuse && C % 64 == 0 && (uint64_t)L * (uint64_t)C * 4u < (1ull << 31)))
        return set_err(TRI_EUNSUPPORTED, "panel SumThreshold: windows (1,2,4,8), a multiple of 64 columns, a window below 2^31 bytes");
    if (variant == 5 && G > 1) return set_err(TRI_EUNSUPPORTED, "panel SumThreshold: one chunk only (launch_colst never pairs a panel with chunks)");
    if (variant == 0 && can_fuse) variant = st_use_mask(L, C) ? ((G == 1 && C % 64 == 0 && !st_no_panel()) ? 5 : 3) : 2;
    if (variant == 0 && flagger_pick && st_use_pipe(sw)) variant = 4;
    if (variant == 4) {
        if (sw.nw > 8 || stp_lds_bytes(sw) > 160 * 1024) return set_err(TRI_EUNSUPPORTED, "stage pipeline: more than eight windows, or the flag ring does not fit LDS");
        HIPCHK(lds_optin_all(160 * 1024, &k_colst_pipe));
    }
    DevBuf<double> ring;
    DevBuf<uint8_t> acc;
    DevBuf<int64_t> d_ends;
    HIPCHK(ring.alloc(nthreads * sw.ringtot));
    HIPCHK(acc.alloc(nthreads * sw.acccap));
    HIPCHK(d_ends.alloc((size_t)n_chunk_ends));
    HIPCHK(hipMemcpyAsync(d_ends.get(), chunk_ends, (size_t)n_chunk_ends * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    HipEvent e0, e1;
    HIPCHK(hipEventCreate(e0.out()));
    HIPCHK(hipEventCreate(e1.out()));
    size_t ws = (size_t)n_line * n_col;
    DevBuf<float> pdata;
    DevBuf<uint8_t> pout;
    if (variant == 5) {
        HIPCHK(pdata.alloc((size_t)n_win * ws));
        HIPCHK(pout.alloc((size_t)n_win * ws));
        {
            ScopedSet<bool> pause(g_klog_on, false);         // (re-layout helpers are not part of what is measured)
            hipLaunchKernelGGL(k_panelize<float>, dim3((unsigned)cdiv((int64_t)ws, 256), (unsigned)n_win), dim3(256), 0, st, data, pdata.get(), L, C, ws);
        }
        LAUNCHCHK();
    }
    const StKernel k = variant == 5 ? StKernel::MaskPanel : variant == 3 ? StKernel::Mask : variant == 2 ? StKernel::Fused :
                       variant == 4 ? StKernel::Pipe : StKernel::Dyn;
    const float* kdata = variant == 5 ? (const float*)pdata.get() : data;
    uint8_t* kout = variant == 5 ? pout.get() : out;
    HIPCHK(hipEventRecord(e0.get(), st));
    for (int i = 0; i < repeats; i++) {
        rc = st_launch(st, k, sw, kdata, mad, kout, d_ends.get(), thr_scale, L, C, G, ws, ws, n_win, ring.get(), acc.get());
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(e1.get(), st));
    HIPCHK(hipEventSynchronize(e1.get()));
    LAUNCHCHK();
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0.get(), e1.get()));
    *ms_per_launch = ms / repeats;
    if (variant == 5) {
        // (a chunk short of the line: the rows outside it are not the kernel's to write -- back through a row image, the
        // chunk's rows alone copied out)
        const bool whole = o0 == 0 && o1 == n_line;
        DevBuf<uint8_t> rows;
        if (!whole) HIPCHK(rows.alloc((size_t)n_win * ws));
        uint8_t* dst = whole ? out : rows.get();
        {
            ScopedSet<bool> pause(g_klog_on, false);
            hipLaunchKernelGGL(k_unpanel_w<uint8_t>, dim3((unsigned)cdiv((int64_t)ws, 256), (unsigned)n_win), dim3(256), 0, st, (const uint8_t*)pout.get(), dst, L, C, ws);
        }
        LAUNCHCHK();
        if (!whole && o1 > o0)
            for (int64_t w = 0; w < n_win; w++)
                HIPCHK(hipMemcpyAsync(out + (size_t)w * ws + (size_t)o0 * C, dst + (size_t)w * ws + (size_t)o0 * C, (size_t)(o1 - o0) * C,
                                      hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return TRI_OK;
}

extern "C" int tri_bench_sumthreshold(const float* data, const double* mad, uint8_t* out,
                                      int64_t n_win, int64_t n_line, int64_t n_col,
                                      const int64_t* windows, int64_t n_windows,
                                      double outlier_nsigma, double rho, int variant, int repeats,
                                      float* ms_per_launch, void* stream) {
    const int64_t ends[2] = {0, n_line};
    return st_hook(data, mad, out, n_win, n_line, n_col, windows, n_windows, outlier_nsigma, rho, variant, repeats, ms_per_launch,
                   stream, ends, 2, false);
}

extern "C" int tri_test_sumthreshold(const float* data, const double* mad, uint8_t* out,
                                     int64_t n_win, int64_t n_line, int64_t n_col,
                                     const int64_t* windows, int64_t n_windows,
                                     double outlier_nsigma, double rho, int variant, int repeats,
                                     float* ms_per_launch, void* stream, const int64_t* chunk_ends, int64_t n_chunk_ends) {
    return st_hook(data, mad, out, n_win, n_line, n_col, windows, n_windows, outlier_nsigma, rho, variant, repeats, ms_per_launch,
                   stream, chunk_ends, n_chunk_ends, true);
}

// what tri_boxx_last_stats() reports: the K4x pass counters of this thread's last tri_bench_boxfilter(stage 1, variant 4)
static thread_local unsigned long long g_boxx_last_stats[2] = {0, 0};

// Measurement / test hook: one axis stage of the masked box filter in the launch geometry of
// the step (see include/tricolour_amd.h).
extern "C" int tri_bench_boxfilter(const float* data, const uint8_t* flags4, float* out_w, float* out_o,
                                   int64_t n_win, int64_t n_line, int64_t n_col, int64_t radius,
                                   int stage, int variant, int repeats, float* ms_per_launch, void* stream) {
    if (!data || !flags4 || !out_w || !out_o || !ms_per_launch) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_win <= 0 || n_line <= 0 || n_col <= 0 || repeats <= 0 || n_win > 65535 || radius <= 0 || (stage != 2 && n_line % 4 != 0))
        return set_err(TRI_EINVAL, "bad shape");
    if (stage < 0 || stage > 2) return set_err(TRI_EUNSUPPORTED, "stage must be 0, 1 or 2");
    if (variant < 0 || variant > 5 || (variant == 4 && stage != 1) || (variant == 5 && stage == 2))
        return set_err(TRI_EINVAL, "variant must be 0 .. 3 (4: exact row filter, stage 1 only; 5: stage pipeline with blocks of 16, stages 0 and 1)");
    if (stage == 2 && n_win != 1) return set_err(TRI_EINVAL, "the spectrum stage takes one window");
    Run r;
    r.st = (hipStream_t)stream;
    r.p = nullptr;
    r.dbg = nullptr;
    r.side = get_side_lane();       // as in the flagger: the time-axis legs time the weight image beside the data image
    HipEvent e0, e1;
    HIPCHK(hipEventCreate(e0.out()));
    HIPCHK(hipEventCreate(e1.out()));
    const size_t N = (size_t)n_line * n_col;
    // The routes of this call: the flagger's (variant 0), or the variant's own.  They live in this call's Run alone.
    BoxRoutes& b = r.box;
    b.unpadded = true;
    const bool pipe = variant == 3 || variant == 5;
    if (variant != 0) b.boxw = false;                   // the named variants run BOTH images through their own kernels
    if (stage == 2) {
        // stage 2: 0 = the flagger's route, 1 = register rings, 2 / 3 = stage pipeline with blocks of 16 / 8
        if (variant != 0) b.spec_pipe = variant == 1 ? SpecPipe::Off : (variant == 2 ? SpecPipe::B16 : SpecPipe::B8);
    } else {
        // stage 0: 0 = the flagger's route, 1 = LDS delay lines, 2 = register delay lines (K4r), 3 = stage pipeline (K4q)
        // (5 = the stage pipeline with blocks of 16 positions wherever 3 takes blocks of 8)
        if (variant != 0) b.pipe_t = b.pipe_f = pipe ? Want::Forced : Want::Off;
        if (variant != 0 && !pipe) b.reg_rings = variant != 1;
        if (variant == 5) b.pipe_t_b8 = b.pipe_f_b8 = false;
        if (variant == 4) b.exact = Want::Forced;       // (at any radius, not only where the flagger takes it)
    }
    int rc = TRI_OK;
    // The stage as one step of the background loop on the hook's images: stage 0 the single sweep from packed flags into
    // (out_w, out_o), stage 1 the frequency stage of a non-final iteration from the TF images in flags4 (n_win, 2, n_line,
    // n_col: weight, weight * data) into (out_w, out_o)
    BgStep s = {};
    s.r0 = s.r1 = (int)radius;
    s.time = TimeStage::PackedSweep;
    BgImages im = {};
    im.T = (int)n_line; im.Fa = (int)n_col; im.W = n_win;
    BgState bst = {};
    if (stage == 0) {
        im.dataTF = data; im.flagsTF = flags4;
        im.Aw = out_w; im.Ao = out_o; im.wsA = N;
        s.tcol = pick_col_filter(b, ColSrc::PackedFlags, COL_WEIGHTS_01, false, (int)radius, (int)n_line, (int)n_col, n_win, false);
    } else if (stage == 1) {
        im.Aw = const_cast<float*>(reinterpret_cast<const float*>(flags4));   // (read only in a non-final iteration)
        im.Ao = im.Aw + N; im.wsA = 2 * N;
        im.Bw = out_w; im.Bo = out_o; im.wsB = N;
        im.dataFT = data;
        s.freq = pick_freq_stage(b, 1, (int)radius, (int)n_col, (int)n_line, n_win, im.Aw, im.Ao, im.wsA, false);
    }
    // stage 1, variant 4: K4x works on rows -- the amplitudes are taken to the TF layout once (untimed), the rows it
    // writes go back to FT inside the timed loop (as in the flagger); out_w doubles as the row buffer.
    // ms_per_launch then covers kernel + transpose; the counters in stats[] are printed with TRI_BOXX_STATS=1
    DevBuf<float> x_data_tf;
    DevBuf<unsigned long long> x_stats;
    int xl = 0;
    if (stage == 1 && variant == 4) {
        xl = boxx_pick_l(b, (int)radius, (int)n_col);
        if (!xl) return set_err(TRI_EUNSUPPORTED, "no exact row filter for radius %d on lines of %d", (int)radius, (int)n_col);
        HIPCHK(x_data_tf.alloc((size_t)n_win * N));
        HIPCHK(x_stats.alloc(2));
        HIPCHK(hipMemsetAsync(x_stats.get(), 0, 2 * sizeof(unsigned long long), r.st));
        rc = launch_transpose<float>(r, data, x_data_tf.get(), (int)n_col, (int)n_line, N, N, n_win);
        if (rc) return rc;
        s.freq = FreqPick();
        s.freq.route = FreqStage::ExactRows; s.freq.xl = xl;
        im.dataTF = x_data_tf.get(); im.rows = out_w; im.ws_rows = N; im.xstats = x_stats.get();
    }
    if (stage == 1 && s.freq.route == FreqStage::Transposed)
        return set_err(TRI_EUNSUPPORTED, "no single-sweep frequency stage for radius %d", (int)radius);
    HIPCHK(hipEventRecord(e0.get(), r.st));
    for (int i = 0; i < repeats && rc == TRI_OK; i++) {
        if (stage == 2) {
            // spectrum path: byte flags [n_line][n_col] + data -> filtered weight and data images
            ColJob j;
            j.srcData = data; j.srcFlags = flags4;
            j.bufW = j.dstW = out_w; j.bufO = j.dstO = out_o;
            j.n = (int)n_line; j.C = (int)n_col; j.rad = (int)radius;
            if (variant >= 2 && boxp_pick_block(b, j.rad, j.C) == 0) rc = set_err(TRI_EUNSUPPORTED, "no stage pipeline for this shape");
            else rc = launch_colfilter(r, pick_col_filter(b, ColSrc::ByteFlags, COL_WEIGHTS_01, false, j.rad, j.n, j.C, 1, spectrum_aligned(j)), j);
        } else if (stage == 0) {
            float den_t;
            rc = bg_time_stage(r, s, im, bst, &den_t);
        } else {
            rc = bg_freq_stage(r, s, im, bst, 0.0f);
        }
    }
    if (rc) return rc;
    HIPCHK(hipEventRecord(e1.get(), r.st));
    HIPCHK(hipEventSynchronize(e1.get()));
    LAUNCHCHK();
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0.get(), e1.get()));
    *ms_per_launch = ms / repeats;
    if (xl) {
        unsigned long long h[2] = {0, 0};
        HIPCHK(hipMemcpy(h, x_stats.get(), sizeof(h), hipMemcpyDeviceToHost));
        g_boxx_last_stats[0] = h[0];
        g_boxx_last_stats[1] = h[1];
        if (const char* e = getenv("TRI_BOXX_STATS")) if (e[0] == '1')
            fprintf(stderr, "k_boxx r=%d L=%d x %d threads: %llu line passes, %llu redone sequentially\n", (int)radius, xl & 255, xl >> 8, h[0], h[1]);
    }
    return TRI_OK;
}

// Kernel log of the calling thread: op 0 = clear and switch on, op 1 = write "name=count;name=count;..." (demangled
// kernel symbols, launches since op 0) into buf and switch off, op 2 = switch off.  Returns the number of distinct kernels.
#include <cxxabi.h>
extern "C" int tri_kernel_log(int op, char* buf, int64_t cap) {
    if (op == 0) {
        if (g_klog) g_klog->clear();
        g_klog_on = true;
        return 0;
    }
    g_klog_on = false;
    if (op != 1) return 0;
    if (!buf || cap <= 0) return set_err(TRI_EINVAL, "kernel log: no buffer");
    buf[0] = 0;
    if (!g_klog) return 0;
    std::vector<std::pair<std::string, long long>> rows;
    for (const auto& kv : *g_klog) {
        const char* m = hipKernelNameRefByPtr(kv.first, nullptr);
        std::string name = m ? m : "?";
        int st = 0;
        char* d = m ? abi::__cxa_demangle(m, nullptr, nullptr, &st) : nullptr;
        if (d && st == 0) { name = d; }
        if (d) free(d);
        const size_t par = name.find('(');                      // drop the argument list and a leading "void "
        if (par != std::string::npos) name.erase(par);
        if (name.compare(0, 5, "void ") == 0) name.erase(0, 5);
        rows.emplace_back(name, kv.second);
    }
    std::sort(rows.begin(), rows.end());
    size_t off = 0;
    for (const auto& r : rows) {
        const int n = snprintf(buf + off, (size_t)cap - off, "%s=%lld;", r.first.c_str(), r.second);
        if (n < 0 || off + (size_t)n >= (size_t)cap) break;
        off += (size_t)n;
    }
    return (int)rows.size();
}

// Test hook: statistics of the fused median + rejection kernel (K3r) since the last reset: blocks run, fallbacks before the
// pass, after it, at the bracket verification.
extern "C" int tri_medrej_stats(uint64_t* out20, int reset) {
    unsigned long long h[20] = {0};
    HIPCHK(hipDeviceSynchronize());
    if (out20) {
        HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_medrej_stats), sizeof(h)));
        for (int k = 0; k < 20; k++) out20[k] = h[k];
    }
    if (reset) {
        unsigned long long z[20] = {0};
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_medrej_stats), z, sizeof(z)));
    }
    return TRI_OK;
}

// Test hook: line passes run / redone sequentially by the last tri_bench_boxfilter(stage 1, variant 4) of this thread
extern "C" int tri_boxx_last_stats(uint64_t* passes, uint64_t* sequential) {
    if (!passes || !sequential) return set_err(TRI_EINVAL, "NULL pointer argument");
    *passes = g_boxx_last_stats[0];
    *sequential = g_boxx_last_stats[1];
    return TRI_OK;
}

// Test hook: exhaustive check of box_divide() for one radius (see include/tricolour_amd.h)
__global__ void k_check_box_divide(BoxDenom dn, unsigned long long* out) {
    unsigned long long bad = 0;
    const unsigned stride = gridDim.x * blockDim.x;
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned long long it = 0; it < (1ull << 32) / stride; it++, i += stride) {
        const float a = __uint_as_float(i);
        const float q = box_divide_checked(a, dn);
        const float e = a / dn.b;
        if (!((__float_as_uint(q) == __float_as_uint(e)) || (isnan(q) && isnan(e)))) bad++;
    }
    if (bad) atomicAdd(out, bad);
}
extern "C" int tri_test_box_divide(int64_t radius, uint64_t* mismatches, void* stream) {
    if (!mismatches || radius < 0 || radius > (1 << 20)) return set_err(TRI_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    DevBuf<unsigned long long> d;
    HIPCHK(d.alloc(1));
    HIPCHK(hipMemsetAsync(d.get(), 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_check_box_divide, dim3(4096), dim3(256), 0, st, box_reciprocal(box_denominator(radius)), d.get());
    LAUNCHCHK();
    unsigned long long h = 0;
    HIPCHK(hipMemcpyAsync(&h, d.get(), sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *mismatches = h;
    return TRI_OK;
}

static int launch_median_big(hipStream_t st, const float* data, const uint8_t* flags, size_t N, int64_t B, const double* centre,
                             double* med, MedBigPar* par, unsigned* ghist, unsigned* gcand, bool vec);

// Test hook: exact segmented medians of |x| over unflagged samples of a
// [n_win][rows][row_len] array; segments [ends[g], ends[g+1]) along each row.
// variant: 0 = automatic choice, 1 = wave kernel (segments <= 1024),
// 2 = workgroup kernel with scalar loads, 3 = workgroup kernel with vector
// loads (needs row_len, segment bounds % 4 == 0).  med: [n_win][rows][G].
extern "C" int tri_test_median(const float* data, const uint8_t* flags, double* med,
                               int64_t n_win, int64_t rows, int64_t row_len,
                               const int64_t* seg_ends, int64_t n_seg_ends, int variant,
                               void* stream) {
    if (!data || !flags || !med || !seg_ends || n_seg_ends < 2 || n_win <= 0 || rows <= 0)
        return set_err(TRI_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    int G = (int)n_seg_ends - 1;
    std::vector<int64_t> start(G), len(G);
    int64_t maxlen = 0;
    bool al4 = row_len % 4 == 0;
    for (int g = 0; g < G; g++) {
        start[g] = seg_ends[g];
        len[g] = seg_ends[g + 1] - seg_ends[g];
        if (len[g] < 0 || seg_ends[g] < 0 || seg_ends[g + 1] > row_len) return set_err(TRI_EINVAL, "bad segment");
        maxlen = std::max(maxlen, len[g]);
        al4 = al4 && start[g] % 4 == 0 && len[g] % 4 == 0;
    }
    DevBuf<int64_t> d_start_b, d_len_b;
    HIPCHK(d_start_b.alloc(G));
    HIPCHK(d_len_b.alloc(G));
    HIPCHK(hipMemcpy(d_start_b.get(), start.data(), G * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_len_b.get(), len.data(), G * sizeof(int64_t), hipMemcpyHostToDevice));
    size_t WS = (size_t)rows * row_len, RS = (size_t)row_len;
    int R = (int)rows;
    if (variant == 8) {
        // multi-workgroup two-pass select (K3d): one segment spanning each whole row
        if (G != 1 || seg_ends[0] != 0 || seg_ends[1] != row_len) return set_err(TRI_EINVAL, "variant 8 takes one segment covering the row");
        const int64_t B = n_win * rows;
        DevBuf<MedBigPar> par;
        DevBuf<unsigned> ghist, gcand;
        HIPCHK(par.alloc(B));
        HIPCHK(ghist.alloc(B * SEL_BINS));
        HIPCHK(gcand.alloc(B * (size_t)MEDBIG_CAND));
        int rcb = launch_median_big(st, data, flags, (size_t)row_len, B, nullptr, med, par.get(), ghist.get(), gcand.get(),
                                    row_len % 4 == 0 && ((uintptr_t)data % 16 == 0) && ((uintptr_t)flags % 4 == 0));
        HIPCHK(hipStreamSynchronize(st));
        return rcb;
    }
    if (variant == 0) variant = maxlen <= 64 * MW_K ? 1 : (al4 ? 3 : 2);
    // variants 11 / 14: variants 1 / 4 with one segment per wave (the round-3 launch shape; TRI_MEDIAN_WAVE_OLD=1 in the pipeline)
    const bool wave_old = variant == 11 || variant == 14;
    if (wave_old) variant -= 10;
    if ((variant == 1 || variant == 4) && maxlen > 64 * MW_K) return set_err(TRI_EINVAL, "wave kernel handles segments <= 1024");
    if (variant == 4 && (row_len % 4 != 0 || maxlen + 3 > 64 * MW_K)) return set_err(TRI_EINVAL, "masked vector variant needs row_len % 4 == 0 and segments <= 1021");
    if ((uint64_t)rows * (uint64_t)row_len * 4u >= (1ull << 32) && (variant == 4 || variant == 1)) return set_err(TRI_EUNSUPPORTED, "wave kernels: a window below 4 GB");
    if ((variant == 3 || variant == 5) && !al4) return set_err(TRI_EINVAL, "vector loads need 4-aligned segments");
    MedianJob j;
    j.data = data; j.flags = flags; j.med = med; j.WSd = j.WSf = WS; j.RS = RS;
    j.seg_start = d_start_b.get(); j.seg_len = d_len_b.get(); j.R = R; j.G = G; j.W = n_win; j.max_len = maxlen;
    const bool full_row = G == 1 && al4 && seg_ends[0] == 0 && seg_ends[1] == row_len;
    MedianKernel k = MedianKernel::Select;
    DevBuf<unsigned> gc;
    if (variant == 1 && maxlen <= 64 * 8) k = MedianKernel::Wave8;
    else if (variant == 4 && row_len % 4 == 0 && maxlen + 3 <= 64 * 8) k = MedianKernel::Wave8Vec;
    else if ((variant == 4 && row_len % 4 == 0 && maxlen + 3 <= 64 * MW_K) || (variant == 1 && full_row)) k = MedianKernel::Wave16Vec;
    else if (variant == 1) k = MedianKernel::Wave16;
    else if (variant == 3) k = MedianKernel::SelectVec;
    else if (variant == 5) k = MedianKernel::TwoPassVec;
    else if (variant == 9 || variant == 10) {
        // K3c with the predicted-window candidates in global scratch (9: vector loads, 10: scalar)
        if (variant == 9 && row_len % 4 != 0) return set_err(TRI_EINVAL, "variant 9 needs row_len % 4 == 0");
        const size_t cap = ((size_t)maxlen + 3) & ~(size_t)3, per_win = cap * (size_t)R * G;
        HIPCHK(gc.alloc(per_win * (size_t)n_win));
        j.gcand = gc.get(); j.cand_ws = per_win; j.cand_cap = (unsigned)cap;
        k = variant == 9 ? MedianKernel::TwoPassVec : MedianKernel::TwoPass;
    } else if (variant == 7) {
        if (row_len % 4 != 0) return set_err(TRI_EINVAL, "variant 7 needs row_len % 4 == 0");
        k = MedianKernel::TwoPassVec;
    } else if (variant == 6) k = MedianKernel::TwoPass;
    launch_median_kernel(st, k, wave_old, j);
    if (variant == 9 || variant == 10) {
        hipError_t le = hipGetLastError();
        hipError_t se = hipStreamSynchronize(st);
        if (le != hipSuccess || se != hipSuccess) return set_err(TRI_EHIP, "median variant %d failed", variant);
        return TRI_OK;
    }
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(st));
    return TRI_OK;
}

extern "C" int tri_flag_nans_and_zeros(const void* vis, int vis_dtype, const uint8_t* flags,
                                       uint8_t* out_flags, int64_t n, void* stream) {
    if (!vis || !flags || !out_flags || n < 0) return set_err(TRI_EINVAL, "bad argument");
    if (vis_dtype != TRI_VIS_C64 && vis_dtype != TRI_VIS_F32) return set_err(TRI_EUNSUPPORTED, "vis dtype must be complex64 or float32");
    if (n == 0) return TRI_OK;
    dim3 grid((unsigned)cdiv(n, 256));
    if (vis_dtype == TRI_VIS_C64)
        hipLaunchKernelGGL(k_flag_nans_zeros<TRI_VIS_C64>, grid, dim3(256), 0, (hipStream_t)stream, vis, flags, out_flags, (size_t)n);
    else
        hipLaunchKernelGGL(k_flag_nans_zeros<TRI_VIS_F32>, grid, dim3(256), 0, (hipStream_t)stream, vis, flags, out_flags, (size_t)n);
    LAUNCHCHK();
    return TRI_OK;
}

extern "C" int tri_stokes_intensity(const void* vis, int vis_dtype, int64_t n, int64_t ncorr,
                                    const int32_t* pol_idx, const double* pol_alpha, int64_t n_pol,
                                    const int32_t* unpol_idx, const double* unpol_alpha, int64_t n_unpol,
                                    int mode, void* out, void* stream) {
    if (n < 0 || ncorr <= 0 || n_pol < 0 || n_unpol < 0) return set_err(TRI_EINVAL, "bad shape");
    if (mode != 0 && mode != 1) return set_err(TRI_EINVAL, "mode must be 0 (polarised) or 1 (unpolarised)");
    if (vis_dtype != TRI_VIS_C64 && vis_dtype != TRI_VIS_C128) return set_err(TRI_EUNSUPPORTED, "visibilities must be complex64 or complex128");
    if (n_pol > TRI_MAX_STOKES_TERMS || n_unpol > TRI_MAX_STOKES_TERMS) return set_err(TRI_EUNSUPPORTED, "at most 4 stokes terms per kind");
    if ((n_pol > 0 && (!pol_idx || !pol_alpha)) || (n_unpol > 0 && (!unpol_idx || !unpol_alpha))) return set_err(TRI_EINVAL, "NULL pointer argument");
    StokesTerms terms;
    terms.n_pol = (int)n_pol;
    terms.n_unpol = (int)n_unpol;
    if (!fill_stokes_terms(terms.pol, pol_idx, pol_alpha, n_pol, ncorr) ||
        !fill_stokes_terms(terms.unpol, unpol_idx, unpol_alpha, n_unpol, ncorr))
        return set_err(TRI_EINVAL, "correlation index out of range");
    if (n == 0) return TRI_OK;
    if (!vis || !out) return set_err(TRI_EINVAL, "NULL pointer argument");
    dim3 grid((unsigned)cdiv(n, 256));
    if (vis_dtype == TRI_VIS_C64)
        hipLaunchKernelGGL(k_stokes_intensity<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)vis, (float*)out, (size_t)n, (int)ncorr, terms, mode);
    else
        hipLaunchKernelGGL(k_stokes_intensity<double>, grid, dim3(256), 0, (hipStream_t)stream, (const double*)vis, (double*)out, (size_t)n, (int)ncorr, terms, mode);
    LAUNCHCHK();
    return TRI_OK;
}

extern "C" int tri_window_counts(const uint8_t* flags, int64_t nbl, int64_t ncorr, int64_t ntime,
                                 int64_t nchan, uint64_t* per_bl, uint64_t* per_chan, void* stream) {
    if (!per_bl || !per_chan) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (nbl < 0 || ncorr < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    hipStream_t st = (hipStream_t)stream;
    if (nbl > 0) HIPCHK(hipMemsetAsync(per_bl, 0, (size_t)nbl * sizeof(uint64_t), st));
    if (nchan > 0) HIPCHK(hipMemsetAsync(per_chan, 0, (size_t)nchan * sizeof(uint64_t), st));
    const int64_t rows = ncorr * ntime;
    if (nbl == 0 || rows == 0 || nchan == 0) return TRI_OK;
    if (!flags) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (nbl > 65535 || rows >= (1ll << 31) || nchan >= (1ll << 31)) return set_err(TRI_EUNSUPPORTED, "window too large for one call");
    // enough row chunks per baseline to fill the device, at most 65535
    int rows_per_block = 256;
    while (cdiv(rows, rows_per_block) > 65535) rows_per_block *= 2;
    const bool vec = nchan % 4 == 0 && ((uintptr_t)flags % 4 == 0);
    dim3 grid((unsigned)cdiv(nchan, vec ? 1024 : 256), (unsigned)cdiv(rows, rows_per_block), (unsigned)nbl);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit counters");
    if (vec)
        hipLaunchKernelGGL(k_window_counts<true>, grid, dim3(256), 0, st, flags, (unsigned long long*)per_bl,
                           (unsigned long long*)per_chan, (int)rows, (int)nchan, rows_per_block);
    else
        hipLaunchKernelGGL(k_window_counts<false>, grid, dim3(256), 0, st, flags, (unsigned long long*)per_bl,
                           (unsigned long long*)per_chan, (int)rows, (int)nchan, rows_per_block);
    LAUNCHCHK();
    return TRI_OK;
}

extern "C" int tri_apply_baseline_channel_mask(const uint8_t* flags, uint8_t* out_flags,
                                               const uint8_t* bl_sel, const uint8_t* chan_mask,
                                               int mode, int64_t nbl, int64_t ncorr, int64_t ntime,
                                               int64_t nchan, void* stream) {
    if (!flags || !out_flags || !bl_sel || !chan_mask) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (mode != 0 && mode != 1) return set_err(TRI_EINVAL, "mode must be 0 (or) or 1 (override)");
    if (nbl < 0 || ncorr < 0 || ntime < 0 || nchan < 0) return set_err(TRI_EINVAL, "bad shape");
    if (nbl == 0 || ncorr * ntime == 0 || nchan == 0) return TRI_OK;
    if (nchan > 0x7FFFFFFF) return set_err(TRI_EUNSUPPORTED, "dimension too large for one call");
    // slabs of at most 65535 rows (gridDim.y) of at most 65535 baselines (gridDim.z), as for_row_slabs cuts rows
    const int64_t rows = ncorr * ntime;
    for (int64_t b0 = 0; b0 < nbl; b0 += 65535) {
        for (int64_t r0 = 0; r0 < rows; r0 += 65535) {
            dim3 grid((unsigned)cdiv(nchan, 256), (unsigned)std::min<int64_t>(65535, rows - r0),
                      (unsigned)std::min<int64_t>(65535, nbl - b0));
            hipLaunchKernelGGL(k_apply_bl_chan_mask, grid, dim3(256), 0, (hipStream_t)stream, flags, out_flags, bl_sel,
                               chan_mask, mode, (int)nchan, (size_t)rows, (size_t)r0, (size_t)b0);
            LAUNCHCHK();
        }
    }
    return TRI_OK;
}


// ---------------------------------------------------------------------------
// uvcontsub_flagger (flagging.py:989-1073), SURVEY.md 8f-2
// ---------------------------------------------------------------------------
extern "C" size_t tri_uvcontsub_workspace_bytes(int64_t batch, int64_t ntime, int64_t nchan) {
    if (batch <= 0 || ntime <= 0 || nchan <= 0) return 0;
    size_t N = (size_t)ntime * nchan, B = (size_t)batch;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // |residual| image, median flags, mean / smooth spectra, two medians, flag counts, and the global histogram /
    // candidate list / parameters of the multi-workgroup median (K3d)
    return al(B * N * 4) + al(B * N) + al(B * nchan * 8) * 2 + al(B * 8) * 2 + al(B * 4) +
           al(B * SEL_BINS * 4) + al(B * MEDBIG_CAND * 4) + al(B * sizeof(MedBigPar)) + 4 * 256;
}

// Exact median of | |x| - centre | (centre == nullptr: of |x|) over the unflagged samples of each of B windows of N
// contiguous samples, many workgroups per window (K3d).
static int launch_median_big(hipStream_t st, const float* data, const uint8_t* flags, size_t N, int64_t B, const double* centre,
                             double* med, MedBigPar* par, unsigned* ghist, unsigned* gcand, bool vec) {
    const unsigned slices = (unsigned)cdiv((int64_t)N, MEDBIG_SLICE);
    if (B > 65535) return set_err(TRI_EUNSUPPORTED, "too many windows in one median batch");
    hipLaunchKernelGGL(k_medbig_range, dim3((unsigned)B), dim3(256), 0, st, data, flags, N, centre, par, ghist);
    if (vec) hipLaunchKernelGGL(k_medbig_hist<true>, dim3(slices, (unsigned)B), dim3(256), 0, st, data, flags, N, centre, par, ghist);
    else hipLaunchKernelGGL(k_medbig_hist<false>, dim3(slices, (unsigned)B), dim3(256), 0, st, data, flags, N, centre, par, ghist);
    hipLaunchKernelGGL(k_medbig_pick, dim3((unsigned)B), dim3(256), 0, st, ghist, par);
    if (vec) {
        hipLaunchKernelGGL(k_medbig_compact<true>, dim3(slices, (unsigned)B), dim3(256), 0, st, data, flags, N, centre, par, gcand);
        hipLaunchKernelGGL(k_medbig_select<true>, dim3((unsigned)B), dim3(256), 0, st, data, flags, N, centre, par, gcand, med);
    } else {
        hipLaunchKernelGGL(k_medbig_compact<false>, dim3(slices, (unsigned)B), dim3(256), 0, st, data, flags, N, centre, par, gcand);
        hipLaunchKernelGGL(k_medbig_select<false>, dim3((unsigned)B), dim3(256), 0, st, data, flags, N, centre, par, gcand, med);
    }
    LAUNCHCHK();
    return TRI_OK;
}

// Caller-provided device buffers of tri_uvcontsub_flagger_debug (any may be NULL), indexed by the GLOBAL product number:
// avg / smooth (n_cp, F), absres / mflags (n_cp, T, F), med (n_cp, 2) = {first median, MAD}, cnt (n_cp)
struct UvTaps { float2* avg; float2* smooth; float* absres; uint8_t* mflags; double* med; unsigned* cnt; };

static int uvcontsub_impl(const void* vis_c64, const uint8_t* flags, uint8_t* out_flags,
                          int64_t n_cp, int64_t ntime, int64_t nchan,
                          int64_t major_cycles, int64_t or_original_from_cycle,
                          int64_t taylor_degrees, double sigma, void* workspace,
                          size_t workspace_bytes, void* stream, const UvTaps* taps) {
    if (!vis_c64 || !flags || !out_flags) return set_err(TRI_EINVAL, "NULL pointer argument");
    if (n_cp < 0 || ntime <= 0 || nchan <= 0) return set_err(TRI_EINVAL, "bad shape");
    if (taylor_degrees < 0 || taylor_degrees > 64) return set_err(TRI_EUNSUPPORTED, "taylor_degrees must be in [0, 64]");
    if ((int64_t)ntime * nchan >= ((int64_t)1 << 31)) return set_err(TRI_EUNSUPPORTED, "window too large");
    if (n_cp == 0) return TRI_OK;
    hipStream_t st = (hipStream_t)stream;
    int T = (int)ntime, F = (int)nchan;
    size_t N = (size_t)T * F;
    size_t one = tri_uvcontsub_workspace_bytes(1, ntime, nchan);
    if (!workspace || workspace_bytes < one) return set_err(TRI_EWORKSPACE, "workspace of %zu bytes is smaller than the %zu needed for one window", workspace_bytes, one);
    int64_t Bmax = std::min<int64_t>(n_cp, 16384);
    while (Bmax > 1 && tri_uvcontsub_workspace_bytes(Bmax, ntime, nchan) > workspace_bytes) Bmax = (Bmax + 1) / 2;
    while (tri_uvcontsub_workspace_bytes(Bmax, ntime, nchan) > workspace_bytes) Bmax--;
    Bump b(workspace, workspace_bytes, false);
    float* absres = b.get<float>((size_t)Bmax * N);
    uint8_t* mflags = b.get<uint8_t>((size_t)Bmax * N);
    float2* avg = b.get<float2>((size_t)Bmax * F);
    float2* smooth = b.get<float2>((size_t)Bmax * F);
    double* med1 = b.get<double>((size_t)Bmax);
    double* mad = b.get<double>((size_t)Bmax);
    unsigned* cnt = b.get<unsigned>((size_t)Bmax);
    unsigned* ghist = b.get<unsigned>((size_t)Bmax * SEL_BINS);
    unsigned* gcand = b.get<unsigned>((size_t)Bmax * MEDBIG_CAND);
    MedBigPar* mpar = b.get<MedBigPar>((size_t)Bmax);
    int K = (int)std::min<int64_t>(taylor_degrees, F);
    bool vec = N % 4 == 0 && (((uintptr_t)workspace) % 16 == 0);
    for (int64_t c0 = 0; c0 < n_cp; c0 += Bmax) {
        int64_t B = std::min(Bmax, n_cp - c0);
        const float2* v = (const float2*)vis_c64 + (size_t)c0 * N;
        uint8_t* rf = out_flags + (size_t)c0 * N;
        // result_flags = flags.copy()  (:1028), normalised to 0/1
        hipLaunchKernelGGL(k_normalise_flags, dim3((unsigned)cdiv((int64_t)(B * N), 256)), dim3(256), 0, st, flags + (size_t)c0 * N, rf, (size_t)B * N);
        LAUNCHCHK();
        for (int64_t mi = 0; mi < major_cycles; mi++) {
            HIPCHK(hipMemsetAsync(cnt, 0, (size_t)B * sizeof(unsigned), st));
            hipLaunchKernelGGL(k_uv_mean, dim3((unsigned)cdiv(F, 256), (unsigned)B), dim3(256), 0, st, v, rf, avg, T, F);
            hipLaunchKernelGGL(k_uv_lowpass, dim3((unsigned)B), dim3(256), 0, st, avg, smooth, F, K);
            // |vis - smooth|, the median flags and (in the same pass) the number of flagged samples per product
            static const bool uv_scalar = is1(getenv("TRI_UV_SCALAR"));   // (A/B, tests)
            if (!uv_scalar && F % 4 == 0 && ((uintptr_t)v % 16 == 0) && ((uintptr_t)rf % 4 == 0) && ((uintptr_t)smooth % 16 == 0) &&
                ((uintptr_t)absres % 16 == 0) && ((uintptr_t)mflags % 4 == 0))
                hipLaunchKernelGGL(k_uv_resid4, dim3((unsigned)cdiv((int64_t)N, 2048), (unsigned)B), dim3(256), 0, st, v, rf, smooth, absres, mflags, cnt, T, F);
            else
                hipLaunchKernelGGL(k_uv_resid, dim3((unsigned)cdiv((int64_t)N, 2048), (unsigned)B), dim3(256), 0, st, v, rf, smooth, absres, mflags, cnt, T, F);
            LAUNCHCHK();
            // nanmedian over the unflagged, non-NaN residuals of each product (:1061), then the median of
            // | |residual| - median | (:1064-1066) straight from the residual image
            int rcm = launch_median_big(st, absres, mflags, N, B, nullptr, med1, mpar, ghist, gcand, vec);
            if (rcm) return rcm;
            rcm = launch_median_big(st, absres, mflags, N, B, med1, mad, mpar, ghist, gcand, vec);
            if (rcm) return rcm;
            if (!uv_scalar && N % 4 == 0 && ((uintptr_t)absres % 16 == 0) && ((uintptr_t)rf % 4 == 0))
                hipLaunchKernelGGL(k_uv_apply4, dim3((unsigned)cdiv((int64_t)(N / 4), 256), (unsigned)B), dim3(256), 0, st, absres, mad, cnt, rf, (float)sigma, mi >= or_original_from_cycle ? 1 : 0, N / 4);
            else
                hipLaunchKernelGGL(k_uv_apply, dim3((unsigned)cdiv((int64_t)N, 256), (unsigned)B), dim3(256), 0, st, absres, mad, cnt, rf, (float)sigma, mi >= or_original_from_cycle ? 1 : 0, N);
            LAUNCHCHK();
            if (taps && mi == major_cycles - 1) {
                // the last cycle's state of this batch, device to device on the call's stream, to the products' global places
                const size_t g = (size_t)c0, nb = (size_t)B;
                if (taps->avg) HIPCHK(hipMemcpyAsync(taps->avg + g * F, avg, nb * F * sizeof(float2), hipMemcpyDeviceToDevice, st));
                if (taps->smooth) HIPCHK(hipMemcpyAsync(taps->smooth + g * F, smooth, nb * F * sizeof(float2), hipMemcpyDeviceToDevice, st));
                if (taps->absres) HIPCHK(hipMemcpyAsync(taps->absres + g * N, absres, nb * N * sizeof(float), hipMemcpyDeviceToDevice, st));
                if (taps->mflags) HIPCHK(hipMemcpyAsync(taps->mflags + g * N, mflags, nb * N, hipMemcpyDeviceToDevice, st));
                if (taps->med) {
                    HIPCHK(hipMemcpy2DAsync(taps->med + 2 * g, 2 * sizeof(double), med1, sizeof(double), sizeof(double), nb, hipMemcpyDeviceToDevice, st));
                    HIPCHK(hipMemcpy2DAsync(taps->med + 2 * g + 1, 2 * sizeof(double), mad, sizeof(double), sizeof(double), nb, hipMemcpyDeviceToDevice, st));
                }
                if (taps->cnt) HIPCHK(hipMemcpyAsync(taps->cnt + g, cnt, nb * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
            }
        }
    }
    return TRI_OK;
}

extern "C" int tri_uvcontsub_flagger(const void* vis_c64, const uint8_t* flags, uint8_t* out_flags,
                                     int64_t n_cp, int64_t ntime, int64_t nchan,
                                     int64_t major_cycles, int64_t or_original_from_cycle,
                                     int64_t taylor_degrees, double sigma, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return uvcontsub_impl(vis_c64, flags, out_flags, n_cp, ntime, nchan, major_cycles, or_original_from_cycle, taylor_degrees,
                          sigma, workspace, workspace_bytes, stream, nullptr);
}

// Test hook: as above, additionally taps the LAST major cycle's intermediates of every product (see UvTaps)
extern "C" int tri_uvcontsub_flagger_debug(const void* vis_c64, const uint8_t* flags, uint8_t* out_flags,
                                           int64_t n_cp, int64_t ntime, int64_t nchan,
                                           int64_t major_cycles, int64_t or_original_from_cycle,
                                           int64_t taylor_degrees, double sigma, void* workspace,
                                           size_t workspace_bytes, void* stream, void* dbg_avg, void* dbg_smooth,
                                           float* dbg_absres, uint8_t* dbg_mflags, double* dbg_med, uint32_t* dbg_cnt) {
    UvTaps t{(float2*)dbg_avg, (float2*)dbg_smooth, dbg_absres, dbg_mflags, dbg_med, dbg_cnt};
    return uvcontsub_impl(vis_c64, flags, out_flags, n_cp, ntime, nchan, major_cycles, or_original_from_cycle, taylor_degrees,
                          sigma, workspace, workspace_bytes, stream, &t);
}

// ---------------------------------------------------------------------------
// The stand-alone device steps: workspace, checks, launches and extern "C" entry points of each in a host file of its
// own, beside its kernels where the step has a folder (still this one translation unit).  step_host.hpp holds the
// checks they share.
// ---------------------------------------------------------------------------
#include "steps/step_host.hpp"
#include "steps/sir/sir_host.hpp"
#include "steps/linerms/linerms_host.hpp"
#include "steps/blint_host.hpp"
#include "steps/ldev/ldev_host.hpp"
#include "steps/ins/ins_host.hpp"
#include "steps/hyst/hyst_host.hpp"
#include "steps/quality/quality_host.hpp"
#include "steps/hist/hist_host.hpp"
#include "steps/medz/medz_host.hpp"
#include "steps/antint/antint_host.hpp"
#include "steps/sk/sk_host.hpp"
#include "steps/polyfit/polyfit_host.hpp"
