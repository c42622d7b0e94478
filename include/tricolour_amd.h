/*
 * tricolour_amd.h -- C ABI of the MI355X-native SumThreshold flagger.
 *
 * This is the drop-in boundary for ONE path of ratt-ru/tricolour: the
 * per-block callable behind tricolour.dask_wrappers.sum_threshold_flagger
 * (reference tricolour/dask_wrappers.py:23-46), i.e.
 * tricolour.flagging.sum_threshold_flagger (reference
 * tricolour/flagging.py:1076-1196) and the window pack / unpack transposes
 * either side of it (reference tricolour/packing.py:243-278, 369-415).
 *
 * Plain pointers and sizes only; no torch / Python types.  All data pointers
 * are DEVICE pointers (HBM resident); `stream` is a hipStream_t (NULL = the
 * null stream).  Functions enqueue work on `stream` and return without
 * synchronising (tri_sum_threshold_flagger and tri_bench_boxfilter also use
 * one internal stream per calling thread for launches that are independent of
 * their neighbours; it is ordered behind `stream` and `stream` behind it by
 * events, so the caller sees the order of a single stream; TRI_SUBSTREAMS=0
 * keeps everything on `stream`); inputs are never written; outputs and the workspace are
 * caller-allocated.  Every function returns 0 on success or a TRI_E* code, in
 * which case tri_last_error() (thread-local) describes the failure.  The
 * library is re-entrant: it keeps no mutable global state, so concurrent calls
 * from several host threads (the reference's dask ThreadPool,
 * apps/tricolour/app.py:266-271) are safe when each uses its own stream and
 * workspace.
 */
#ifndef TRICOLOUR_AMD_H
#define TRICOLOUR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRI_MAX_WINDOWS 16
#define TRI_MAX_HIST_BINS 2048   /* bins of an amplitude histogram (tri_amplitude_histogram) */

enum tri_status {
    TRI_OK = 0,
    TRI_EINVAL = 1,      /* bad shape / NULL pointer -> Python ValueError       */
    TRI_EUNSUPPORTED = 2,/* parameter combination the reference itself rejects
                            or that this build does not implement               */
    TRI_EWORKSPACE = 3,  /* workspace smaller than tri_workspace_bytes(.., 1)   */
    TRI_EHIP = 4         /* a HIP runtime call failed                           */
};

enum tri_vis_dtype {
    TRI_VIS_C64 = 0,     /* interleaved (re, im) float32 -- MS DATA columns     */
    TRI_VIS_F32 = 1,     /* real float32 amplitudes (flagging.py:830-832)       */
    TRI_VIS_C128 = 2,    /* interleaved float64: tri_stokes_intensity only       */
    TRI_VIS_F64 = 3      /* real float64 AMPLITUDES: what float64 / complex128 visibilities are to
                            _average_freq (np.abs in float64, flagging.py:856), added to the float32
                            accumulator in float64 and rounded at every step (:858-859).  The caller forms
                            them (|x|, hypot(re, im)); a visibility with a NaN part must arrive as NaN
                            (the final isnan(in_data), :777-781).  tri_sum_threshold_flagger only.      */
};

/*
 * Prepared parameters of one sum_threshold_flagger call: the keyword
 * arguments of flagging.py:1076-1083 after the plain-Python preparation of
 * flagging.py:1156-1179 (window de-duplication / clipping, frequency chunk
 * ends).  Build it with tri_prepare_params().
 */
typedef struct tri_params {
    double  outlier_nsigma;
    int64_t n_windows_time;
    int64_t windows_time[TRI_MAX_WINDOWS];
    int64_t n_windows_freq;
    int64_t windows_freq[TRI_MAX_WINDOWS];
    double  background_reject;
    int64_t background_iterations;
    double  spike_width_time;
    double  spike_width_freq;
    int64_t time_extend;
    int64_t freq_extend;
    int64_t n_chunk_ends;          /* freq_chunks + 1                          */
    const int64_t *chunk_ends;     /* HOST pointer, averaged-channel units     */
    int64_t average_freq;
    double  flag_all_time_frac;
    double  flag_all_freq_frac;
    double  rho;
    int64_t num_major_iterations;
} tri_params;

/*
 * Restates flagging.py:1156-1179: windows_freq = unique(int(ceil(f32(w)) /
 * average_freq)); freq_chunk_ends = linspace(0, averaged_channels,
 * freq_chunks + 1).astype(int); windows clipped to <= ntime / <=
 * averaged_channels.  `chunk_ends_buf` (HOST, capacity `chunk_cap` >=
 * freq_chunks + 1) receives the chunk ends and is referenced by `out`.
 * A zero-sized frequency window (possible with average_freq > 1, where the
 * reference fails with a broadcasting ValueError at flagging.py:663) returns
 * TRI_EINVAL.
 */
int tri_prepare_params(int64_t ntime, int64_t nchan,
                       double outlier_nsigma,
                       const double *windows_time, int64_t n_windows_time,
                       const double *windows_freq, int64_t n_windows_freq,
                       double background_reject, int64_t background_iterations,
                       double spike_width_time, double spike_width_freq,
                       int64_t time_extend, int64_t freq_extend,
                       int64_t freq_chunks, int64_t average_freq,
                       double flag_all_time_frac, double flag_all_freq_frac,
                       double rho, int64_t num_major_iterations,
                       int64_t *chunk_ends_buf, int64_t chunk_cap,
                       tri_params *out);

/*
 * Device workspace needed to process `batch_windows` correlation products
 * (bl x corr windows) of shape (ntime, nchan) at a time.  The flagger accepts
 * any workspace >= tri_workspace_bytes(.., 1) and sizes its internal batch to
 * what it is given; larger batches fill the GPU better.
 */
size_t tri_workspace_bytes(int64_t batch_windows, int64_t ntime, int64_t nchan,
                           const tri_params *p);

/*
 * Replaces tricolour.flagging.sum_threshold_flagger (flagging.py:1076-1196)
 * for one window block.
 *   vis        (n_cp, ntime, nchan) visibilities, C order, dtype `vis_dtype`
 *              [n_cp = bl * corr after the reshape of flagging.py:1156-1158]
 *   flags      (n_cp, ntime, nchan) uint8 / bool, non-zero = flagged
 *   out_flags  (n_cp, ntime, nchan) uint8, receives 0/1: the LAST major
 *              iteration's flags (flagging.py:1181-1196), not OR-ed with the
 *              input flags
 * Bit-exact with the reference executed under its numba JIT.
 */
int tri_sum_threshold_flagger(const void *vis, int vis_dtype,
                              const uint8_t *flags, uint8_t *out_flags,
                              int64_t n_cp, int64_t ntime, int64_t nchan,
                              const tri_params *p,
                              void *workspace, size_t workspace_bytes,
                              void *stream);

/*
 * Replaces packing._numba_pack_data (packing.py:243-278): scatter MS rows
 * (row, chan, corr) into windows (bl, corr, time, chan).  `row_bl` / `row_time`
 * (int32, length `rows`) give each row's window baseline index and time index
 * (row_bl < 0: row belongs to no baseline of this block and is skipped); they
 * replace the reference's O(nbl * rows) antenna matching with a precomputed
 * row -> (bl, t) map (see tri_row_map in the Python mirror).  Cells no row
 * maps to keep their prior contents: initialise the windows with
 * tri_fill_windows (NaN+NaNj / 1, packing.py:97,117).
 */
int tri_pack_data(const void *data_c64, const uint8_t *flag,
                  const int32_t *row_bl, const int32_t *row_time,
                  int64_t rows, int64_t nchan, int64_t ncorr,
                  int64_t nbl, int64_t ntime,
                  void *vis_windows_c64, uint8_t *flag_windows, void *stream);

int tri_fill_windows(void *vis_windows_c64, uint8_t *flag_windows,
                     int64_t n_elements, void *stream);

/*
 * Replaces packing._unpack_data / _numpy_unpack_transpose
 * (packing.py:369-415): gather flag windows (bl, corr, time, chan) back to MS
 * row order (row, chan, corr); rows with row_bl < 0 are set to 0.  With
 * any_corr != 0 every correlation of a (row, chan) cell receives the OR over
 * its correlations -- the equalisation the application applies right after
 * unpacking (apps/tricolour/app.py:479-480).
 */
int tri_unpack_data(const uint8_t *flag_windows,
                    const int32_t *row_bl, const int32_t *row_time,
                    int64_t rows, int64_t nchan, int64_t ncorr,
                    int64_t nbl, int64_t ntime,
                    uint8_t *out_flags, int any_corr, void *stream);

/*
 * The per-scan input steps of apps/tricolour/app.py:389-457 fused into one
 * pass over the MS rows (row, chan, ncorr), complex64:
 *   vis = data - model            (:389-395; model == NULL: vis = data)
 *   flags = 0 if flag == NULL     (--ignore-flags, :403-410)
 *   mode 0 (standard):    windows of wcorr = ncorr correlations, vis and flags
 *                         per correlation
 *   mode 1 (polarisation), 2 (total_power): windows of wcorr = 1 correlation,
 *                         vis = polarised_intensity(vis, terms) as in
 *                         tri_stokes_intensity mode 0 (same device arithmetic,
 *                         same bits), flags = any over corr (:415-439)
 * then the scatter of tri_pack_data (packing.py:243-278) into windows
 * (bl, wcorr, time, chan): row_bl / row_time as there, rows with row_bl < 0
 * skipped.  Term tables are HOST arrays as in tri_stokes_intensity (idx =
 * (c1, c2, s1, s2), alpha = (re, im) per term): the non-I terms of
 * stokes_corr_map for mode 1, all of them for mode 2; ignored in mode 0.
 * Cells no row maps to keep their prior contents: initialise the windows
 * with tri_fill_windows.
 */
int tri_pack_scan(const void *data_c64, const void *model_c64, const uint8_t *flag,
                  const int32_t *row_bl, const int32_t *row_time,
                  int64_t rows, int64_t nchan, int64_t ncorr,
                  int64_t nbl, int64_t ntime, int mode,
                  const int32_t *pol_idx, const double *pol_alpha, int64_t n_pol,
                  void *vis_windows_c64, uint8_t *flag_windows, void *stream);

/*
 * Flags of the MS after a scan (apps/tricolour/app.py:475-480): gathers the
 * (bl, wcorr, time, chan) flag windows back to MS row order as
 *   out_flags[row, chan, :] = any(flag_windows[bl, :, time, chan])
 * broadcast to all out_ncorr correlations (unpack_data, then
 * sum(axis=corr) > 0 and broadcast_to(..., ncorr)).  wcorr is 1 (Stokes
 * modes) or out_ncorr (standard); rows with row_bl < 0 are set to 0.
 */
int tri_unpack_scan(const uint8_t *flag_windows,
                    const int32_t *row_bl, const int32_t *row_time,
                    int64_t rows, int64_t nchan, int64_t wcorr, int64_t out_ncorr,
                    int64_t nbl, int64_t ntime, uint8_t *out_flags, void *stream);

/*
 * tri_pack_scan for a list of n rows, one baseline chunk of a scan at a time:
 * entry i reads source row src_row[i] (NULL: row i, a compact slab) of the
 * (src_rows, nchan, ncorr) data, model (optional) and flags (optional) and
 * scatters it to cell (row_bl[i], row_time[i]) of the (nbl, wcorr, ntime,
 * nchan) windows with tri_pack_scan's arithmetic.  Entries whose source row
 * is outside [0, src_rows) or whose cell is outside the windows are skipped.
 * Only the list is launched.  Initialise the windows with tri_fill_windows.
 */
int tri_pack_scan_rows(const void *data_c64, const void *model_c64, const uint8_t *flag,
                       const int64_t *src_row, int64_t src_rows,
                       const int32_t *row_bl, const int32_t *row_time,
                       int64_t n, int64_t nchan, int64_t ncorr,
                       int64_t nbl, int64_t ntime, int mode,
                       const int32_t *pol_idx, const double *pol_alpha, int64_t n_pol,
                       void *vis_windows_c64, uint8_t *flag_windows, void *stream);

/*
 * tri_unpack_scan for a list of n rows: entry i writes destination row
 * dst_row[i] (NULL: row i) of the (out_rows, nchan, out_ncorr) flags from
 * cell (row_bl[i], row_time[i]) of the flag windows (0 if the cell is
 * outside them).  Entries whose destination is outside [0, out_rows) are
 * skipped; rows not in the list are never written.
 */
int tri_unpack_scan_rows(const uint8_t *flag_windows,
                         const int64_t *dst_row, int64_t out_rows,
                         const int32_t *row_bl, const int32_t *row_time,
                         int64_t n, int64_t nchan, int64_t wcorr, int64_t out_ncorr,
                         int64_t nbl, int64_t ntime, uint8_t *out_flags, void *stream);

/*
 * Replaces tricolour.stokes.polarised_intensity (stokes.py:157-209, mode 0)
 * and unpolarised_intensity (stokes.py:79-153, mode 1) on (row, chan, corr)
 * visibilities, n = row * chan samples:
 *   value_k = a_k * (s1_k * vis[c1_k] + s2_k * vis[c2_k])     in complex128
 *   mode 0: out = sqrt(sum_pol |value|^2)
 *   mode 1: out = sum_unpol |value| - sqrt(sum_pol |value|^2)
 * written as one correlation of the visibility dtype (imaginary part 0).
 * Term tables are HOST arrays: idx = (c1, c2, s1, s2) per term, alpha =
 * (re, im) per term (the (c1, c2, a, s1, s2) tuples of stokes_corr_map).
 * vis_dtype: TRI_VIS_C64 or TRI_VIS_C128.
 */
int tri_stokes_intensity(const void *vis, int vis_dtype, int64_t n, int64_t ncorr,
                         const int32_t *pol_idx, const double *pol_alpha, int64_t n_pol,
                         const int32_t *unpol_idx, const double *unpol_alpha, int64_t n_unpol,
                         int mode, void *out, void *stream);

/*
 * Flag counts behind tricolour.window_statistics._window_stats
 * (window_statistics.py:12-66): one pass over a (bl, corr, time, chan) uint8
 * flag window gives
 *   per_bl[bl]     number of set flags of baseline bl     (per-antenna,
 *                  per-baseline, per-scan and per-field sums, :27-53)
 *   per_chan[chan] number of set flags of channel chan    (per-ddid frequency
 *                  bins, :55-66)
 * Both outputs are device arrays of uint64 and are zeroed by the call.
 */
int tri_window_counts(const uint8_t *flags, int64_t nbl, int64_t ncorr,
                      int64_t ntime, int64_t nchan, uint64_t *per_bl,
                      uint64_t *per_chan, void *stream);

/*
 * Replaces tricolour.flagging.flag_nans_and_zeros (flagging.py:29-62):
 * out = (vis == 0) | isnan(vis) | (flags != 0), elementwise over n samples.
 */
int tri_flag_nans_and_zeros(const void *vis, int vis_dtype, const uint8_t *flags,
                            uint8_t *out_flags, int64_t n, void *stream);

/*
 * Device half of tricolour.flagging.apply_static_mask (flagging.py:151-172,
 * one call per mask) and flag_autos (flagging.py:90-93): out = flags, then on
 * every baseline with bl_sel[bl] != 0 either out |= chan_mask (mode 0, "or")
 * or out = chan_mask (mode 1, "override"), broadcast over corr and time.
 * flags / out: (nbl, ncorr, ntime, nchan) uint8; may alias.  Any nbl and
 * ncorr * ntime: the call launches slabs of 65535 x 65535.  The channel mask
 * and the baseline selection (uv-range test on antenna positions) are
 * computed on the host exactly as flagging.py:131-160 does.
 */
int tri_apply_baseline_channel_mask(const uint8_t *flags, uint8_t *out_flags,
                                    const uint8_t *bl_sel, const uint8_t *chan_mask,
                                    int mode, int64_t nbl, int64_t ncorr, int64_t ntime,
                                    int64_t nchan, void *stream);

/*
 * Replaces tricolour.flagging.uvcontsub_flagger (flagging.py:989-1073): per
 * correlation product and major cycle, the time-mean spectrum of the unflagged
 * visibilities is low-passed (first `taylor_degrees` Fourier bins), samples
 * whose |vis - smooth| exceeds sigma x the MAD-of-MAD of the unflagged
 * residuals are flagged; cycles below `or_original_from_cycle` REPLACE the
 * flags, later ones OR them in.  vis complex64 (n_cp, ntime, nchan); out_flags
 * receives 0/1.  The reference is plain NumPy whose FFT / residual precision
 * depends on the NumPy version (float32 under NumPy >= 2, followed here), so
 * parity is by flag-agreement rate, not bit for bit.
 */
size_t tri_uvcontsub_workspace_bytes(int64_t batch_windows, int64_t ntime, int64_t nchan);
int tri_uvcontsub_flagger(const void *vis_c64, const uint8_t *flags, uint8_t *out_flags,
                          int64_t n_cp, int64_t ntime, int64_t nchan,
                          int64_t major_cycles, int64_t or_original_from_cycle,
                          int64_t taylor_degrees, double sigma,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Scale-invariant rank (SIR) operator (Offringa, van de Gronde & Roerdink
 * 2012, A&A 539, A95) over (n_win, ntime, nchan) uint8 flag windows
 * (nonzero = flagged).  For one line f[0..n) and 0 <= eta < 1:
 *   U(i)   = number of unflagged samples in [0, i), i = 0..n
 *   W(i)   = eta * (double)i - (double)U(i)     (IEEE multiply, then subtract)
 *   out[x] = max_{x < j <= n} W(j) >= min_{0 <= k <= x} W(k)
 * i.e. x is flagged iff some interval [k, j) containing it has at most
 * eta * (j - k) unflagged samples.  Per window
 *   out_flags = f | SIR_time(f, eta_time) | SIR_freq(f, eta_freq)
 * where both axes read the INPUT mask (not chained; the result does not
 * depend on the order), and eta = 0 skips an axis.  out_flags receives 0/1
 * and must not overlap flags.  TRI_EINVAL for NULL pointers, negative shapes,
 * eta NaN or outside [0, 1) and overlapping buffers; TRI_EWORKSPACE when
 * workspace_bytes < tri_sir_workspace_bytes() (0 unless a line is longer
 * than one workgroup's span: ntime > 1024 or nchan > 65536).  Empty shapes
 * return TRI_OK without a launch.
 */
size_t tri_sir_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan);
int tri_scale_invariant_rank(const uint8_t *flags, uint8_t *out_flags,
                             int64_t n_win, int64_t ntime, int64_t nchan,
                             double eta_time, double eta_freq,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * The SIR operator with a mask of missing samples and a penalty (after
 * AOFlagger's masked SIR operator; the definition is this project's own).
 * `missing` has the shape of `flags` (nonzero = missing: absent cells of the
 * window grid, dead samples, statically masked bands -- flags that are no
 * detections).  For one line f[0..n), m[0..n), 0 <= eta < 1 and a finite
 * penalty >= 0, with integer prefix counts for i = 0..n
 *   M(i)   = number of missing samples in [0, i),  P(i) = i - M(i)
 *   U(i)   = number of present and unflagged samples in [0, i)
 *   W(i)   = (eta * (double)P(i) - (double)U(i)) - penalty * (double)M(i)
 *            (four IEEE operations in that order, no FMA)
 *   out[x] = max_{x < j <= n} W(j) >= min_{0 <= k <= x} W(k)   for a present x
 *   out[x] = f[x] != 0                                         for a missing x
 * i.e. a present x is flagged iff some interval containing it holds at most
 * eta * (its present samples) - penalty * (its missing samples) present and
 * unflagged samples: a missing sample counts neither as RFI nor as clean
 * data, crossing it costs `penalty`, and it is never flagged or unflagged.
 * Per window
 *   out_flags = f | SIRm_time(f, m, eta_time) | SIRm_freq(f, m, eta_freq)
 * where both axes read the INPUT masks and eta = 0 skips an axis.  With m all
 * zero the result is tri_scale_invariant_rank's bit for bit; with penalty = 0
 * it is, on the present samples, that of the line with the missing samples
 * deleted; it shrinks as the penalty grows and always contains f.
 * out_flags receives 0/1 and must overlap neither flags nor missing.
 * TRI_EINVAL for NULL pointers, negative shapes, eta NaN or outside [0, 1), a
 * penalty that is NaN, infinite or negative, and overlapping buffers;
 * TRI_EWORKSPACE when workspace_bytes < tri_sir_masked_workspace_bytes() (0
 * unless ntime > 1024 or nchan > 65536; larger than the unmasked workspace:
 * two counts per line segment).  Empty shapes return TRI_OK without a launch.
 */
size_t tri_sir_masked_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan);
int tri_scale_invariant_rank_masked(const uint8_t *flags, const uint8_t *missing,
                                    uint8_t *out_flags,
                                    int64_t n_win, int64_t ntime, int64_t nchan,
                                    double eta_time, double eta_freq, double penalty,
                                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Line-RMS statistics of (n_win, ntime, nchan) windows and the thresholding
 * of whole timesteps and whole channels on them (beyond the reference; the
 * model is AOFlagger's threshold_timestep_rms / threshold_channel_rms, the
 * definition is this library's own).  Per window, visibilities v (complex64,
 * or float32 amplitudes) and uint8 flags f (nonzero = flagged):
 *   p    = (double)re * (double)re + (double)im * (double)im   (a * a for
 *          amplitudes); a sample counts if f == 0 and p is not NaN
 *   rms  = sqrt(sum p / n) in float64 over the n counting samples of a time
 *          row (over channels) or of a channel (over times); NaN when n == 0.
 *          The order of the sum is fixed by the shape alone: no atomics, the
 *          same bits on every run and for every split of the windows.
 *   per axis: usable lines are those with a finite rms; med = their median
 *          (even count: (a + b) / 2), sigma = 1.4826 * median(|rms - med|).
 *          A usable line is bad if |rms - med| > nsigma * sigma (flag_low
 *          nonzero) or rms - med > nsigma * sigma (flag_low zero) -- unless
 *          the axis is inert: nsigma == 0, fewer than 3 usable lines, or
 *          sigma > 1e-9 * med does not hold.  A non-empty line whose rms is
 *          not finite is bad whenever nsigma > 0.
 *   out_flags = f | bad_time[t] | bad_chan[c]   (0/1; both axes read f)
 * tri_line_rms writes the statistics only: rms_time (n_win, ntime) and
 * rms_chan (n_win, nchan) float64, and the counts n as int32 where count_time
 * / count_chan are not NULL.  TRI_EINVAL for NULL pointers (other than the
 * counts), negative shapes, nsigma negative or NaN, out_flags overlapping
 * flags; TRI_EUNSUPPORTED for other dtypes and for more lines than one launch
 * holds (pass fewer windows per call); TRI_EWORKSPACE when workspace_bytes <
 * tri_line_rms_workspace_bytes().  Empty shapes return TRI_OK without a
 * launch.
 */
size_t tri_line_rms_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan);
int tri_line_rms(const void *vis, int vis_dtype, const uint8_t *flags,
                 int64_t n_win, int64_t ntime, int64_t nchan,
                 double *rms_time, double *rms_chan,
                 int32_t *count_time, int32_t *count_chan,
                 void *workspace, size_t workspace_bytes, void *stream);
int tri_line_rms_threshold(const void *vis, int vis_dtype, const uint8_t *flags,
                           uint8_t *out_flags, int64_t n_win, int64_t ntime,
                           int64_t nchan, double nsigma_time, double nsigma_freq,
                           int flag_low, void *workspace, size_t workspace_bytes,
                           void *stream);

/*
 * Baseline integration (beyond the reference; the model is AOFlagger's
 * baseline-integrated flagging, the definition is this library's own): the
 * amplitudes of all baselines averaged into one image of n = ncorr * ntime *
 * nchan positions, which the ordinary flagger flags, and the detections given
 * back to every baseline.  vis (nbl, n) complex64 or float32 amplitudes, flags
 * (nbl, n) uint8 (nonzero = flagged), select[nbl] uint8 on the device
 * (nonzero = the baseline takes part) or NULL for all:
 *   a        = +inf if re or im is infinite, else (float)sqrt((double)re * re
 *              + (double)im * im)   (fabsf(v) for amplitudes); a sample counts
 *              if its baseline is selected, its flag is 0 and a is not NaN
 *   tri_baseline_accumulate: for b = 0 .. nbl - 1 in that order and every
 *              counting sample sum[i] += (double)a, count[i] += 1.  One thread
 *              per position, no atomics, no re-association: the order over
 *              baselines is the order in memory.  The call ADDS to sum and
 *              count (the caller zeroes them first), so the baselines fed in
 *              several calls in ascending order give the bits of one call.
 *   tri_baseline_mean: flag[i] = count[i] < min_count;  amp[i] = (float)(sum[i]
 *              / (double)count[i]) where flag[i] is 0, else 0.  The caller
 *              computes min_count = max(1, ceil(min_baseline_frac * selected)).
 *   (the flagger: tri_sum_threshold_flagger on amp / flag as one float32
 *   block of ncorr windows gives line[n])
 *   tri_broadcast_or: out[b, i] = (flags[b, i] != 0) | (line[i] != 0) for every
 *              baseline, the unselected ones included; out may be flags itself.
 * TRI_EINVAL for NULL pointers (other than select), negative sizes, min_count
 * < 1, out overlapping line (or overlapping flags without being flags);
 * TRI_EUNSUPPORTED for dtypes other than complex64 and float32.  No
 * workspace.  Empty shapes return TRI_OK without a launch.
 */
int tri_baseline_accumulate(const void *vis, int vis_dtype, const uint8_t *flags,
                            const uint8_t *select /* may be NULL */,
                            int64_t nbl, int64_t n, double *sum, int32_t *count,
                            void *stream);
int tri_baseline_mean(const double *sum, const int32_t *count, int64_t n,
                      int64_t min_count, float *amp, uint8_t *flag, void *stream);
int tri_broadcast_or(const uint8_t *flags, const uint8_t *line, uint8_t *out,
                     int64_t nbl, int64_t n, void *stream);

/*
 * Sliding-window complex deviation of (n_win, ntime, nchan) windows and the
 * thresholding of single samples on it (beyond the reference; the model is
 * CASA's rflag, the definition is this library's own and identity with rflag
 * is not claimed).  Every other detector of the library sees the amplitude
 * alone; this one sees the complex value.  Per window, visibilities v
 * (complex64, or float32 amplitudes taken as re = a, im = 0) and uint8 flags f
 * (nonzero = flagged); a sample counts if f == 0 and neither part is NaN.
 * Time axis, window_time odd in [3, 31], h = (window_time - 1) / 2: for sample
 * (t, c) walk t' ascending over [max(0, t - h), min(ntime - 1, t + h)], the
 * counting samples only, all arithmetic in float64 from +0.0 without FMA:
 *   n  = their number;  sr += (double)re, si += (double)im;
 *   mr = sr / (double)n, mi = si / (double)n;
 *   a second walk in the same order: dr = re - mr, di = im - mi,
 *        acc = acc + dr * dr, then acc = acc + di * di;
 *   d  = (float)sqrt(acc / (double)n).
 *   The sample is usable iff it counts itself and n >= 2; an unusable sample
 *   has d = NaN and is never flagged by the step.  If any counting sample of
 *   the window has an infinite part, d = +inf.
 *   A line is one (window, channel); its level med is the median of the finite
 *   d of its usable samples, m values in all: the middle one for odd m,
 *   float32(a + b) / 2 of the two middle ones for even m (the sum rounded to
 *   float32).  The line is live iff m >= 3 and med > 0.
 *   hit_t = usable && (d == +inf || (live && (double)d > (double)med *
 *           scale_time)).
 * Frequency axis: the same with the window sliding along channels
 * (window_freq, scale_freq) and one level per (window, time row, frequency
 * chunk k = channels [chunk_ends[k], chunk_ends[k + 1])); chunk_ends is a HOST
 * array of n_chunk_ends non-decreasing entries from 0 to nchan, read before
 * the call returns.  The sliding window does not stop at chunk ends, only the
 * level does; an empty chunk is a no-op.
 *   out_flags = (f != 0) | hit_t | hit_f   (0/1)
 * Both axes read the inputs and are not chained; a scale of 0 switches an
 * axis off; with both off out_flags = (f != 0).  Input buffers are never
 * written.  No floating-point atomics: the same bits on every run, for every
 * alignment and for every split of the windows over calls.
 * tri_local_deviation writes the statistics only: d_time and d_freq,
 * (n_win, ntime, nchan) float32 images (NaN is 0x7FC00000); either may be
 * NULL; it needs no workspace.  TRI_EINVAL for NULL pointers (other than
 * those), negative shapes, a window that is even or outside [3, 31], a scale
 * that is negative or NaN, chunk ends that do not run from 0 to nchan, and
 * out_flags overlapping flags; TRI_EUNSUPPORTED for other dtypes and for more
 * lines than one launch holds (pass fewer windows per call); TRI_EWORKSPACE
 * when workspace_bytes < tri_local_deviation_workspace_bytes().  Empty shapes
 * return TRI_OK without a launch.
 */
size_t tri_local_deviation_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan,
                                           int64_t n_chunk_ends);
int tri_local_deviation(const void *vis, int vis_dtype, const uint8_t *flags,
                        int64_t n_win, int64_t ntime, int64_t nchan,
                        int64_t window_time, int64_t window_freq,
                        float *d_time /* may be NULL */, float *d_freq /* may be NULL */,
                        void *stream);
int tri_local_deviation_threshold(const void *vis, int vis_dtype, const uint8_t *flags,
                                  uint8_t *out_flags, int64_t n_win, int64_t ntime,
                                  int64_t nchan, int64_t window_time, int64_t window_freq,
                                  double scale_time, double scale_freq,
                                  const int64_t *chunk_ends, int64_t n_chunk_ends,
                                  void *workspace, size_t workspace_bytes, void *stream);

/*
 * Sky-subtracted incoherent noise spectrum (beyond the reference; the model is
 * SSINS, Wilensky et al. 2019; the definition below is this library's own and
 * identity with SSINS is not claimed: the level of a channel is the median
 * over time, not the mean, so every time row is judged in the same round, and
 * matched sums are taken on fixed-point z-scores in integer arithmetic, so
 * the result has the same bits for every reduction order).  Every baseline's
 * visibilities are differenced along time: sky and fringe vary slowly and
 * cancel, noise and whatever changed between two dumps remain.  The amplitudes
 * of the differences are averaged over baselines; their distribution is a
 * Rayleigh mixture whose sigma is tied to its mean, so a z-score needs no
 * background fit.
 *
 * Inputs.  vis (nbl, ncorr, ntime, nchan) complex64, or float32 amplitudes
 * taken as re = a, im = 0; flags uint8 of the same shape, nonzero = flagged;
 * select[nbl] uint8 on the device (nonzero = the baseline takes part) or NULL
 * for all.  nd = ntime - 1 difference rows; the image has ncorr * nd * nchan
 * positions i = (k, t, c).
 *
 * 1. Accumulate (tri_ins_accumulate), for the pair (t, t + 1), t in [0, nd):
 *    dr = re[t+1] - re[t], di = im[t+1] - im[t] in float32;
 *    d  = the flagger's amplitude of (dr, di): +inf if either part is
 *         infinite, otherwise (float)sqrt((double)dr * dr + (double)di * di);
 *    the pair counts if its baseline is selected, both flags are 0 and d is
 *    not NaN; for b = 0 .. nbl - 1 in that order sum[i] += (double)d,
 *    count[i] += 1.  The call ADDS to sum (float64) and count (int32), which
 *    the caller zeroes first: baselines fed over several calls in ascending
 *    order give the bits of one call.  No atomics; one order per position,
 *    whatever the grid.
 * 2. z-score image, given a mask image (ncorr, nd, nchan) uint8 of earlier
 *    detections (all 0 in the first round):
 *    usable = count >= min_count (the caller computes min_count = max(1,
 *             ceil(min_baseline_frac * selected)), as for baseline integration);
 *    x      = (float)(sum / (double)count);
 *    the level med of line (k, c) is the median of the finite x over its
 *    usable, unmasked rows, m values in all: the middle one for odd m,
 *    float32(a + b) / 2 of the two middle ones for even m (the sum rounded to
 *    float32).  The line is live iff m >= 3 and med > 0.
 *    valid  = usable && !mask && live;
 *    z      = ((double)x / (double)med - 1.0) * sqrt((double)count / C),
 *             C = 0.2732395447351628 (4 / pi - 1);
 *    q      = 2^30 if x == +inf, otherwise (int32)rint(clamp(z, -16384, 16384)
 *             * 65536), ties to even; an invalid position has q = 0 and is
 *             never summed.
 *    tri_ins_zscore writes one round's level (ncorr, nchan) float32 (NaN
 *    0x7FC00000 for a line with m == 0), q int32 and valid uint8 (0/1).
 *    (sum is a sum of amplitudes and so never negative or NaN.)
 * 3. Match, per row (k, t), all comparisons strict: for shape i in index order
 *    with channels [lo_i, hi_i), m = the valid positions in the range; a shape
 *    with m == 0 is skipped; S = sum of q in int64, r_i = ((double)S / 65536.0)
 *    / sqrt((double)m) / nsigma_i.  After the shapes, if nsigma_narrow > 0, the
 *    valid position with the largest q, lowest channel on ties, gives
 *    r = ((double)q / 65536.0) / nsigma_narrow.  The row's pick is the first
 *    candidate with the largest r, and only if r > 1; its whole channel range
 *    (for narrow: the one position) is set in the mask.  One-sided: RFI adds
 *    power.
 * 4. Rounds.  tri_ins_match zeroes mask and runs steps 2 and 3 `rounds` times,
 *    each round on the mask the previous rounds left.  The number is fixed and
 *    nothing is read back to the host; a round that finds nothing changes
 *    nothing.  shape_lo / shape_hi / shape_nsigma are HOST arrays of n_shapes
 *    entries, read before the call returns.
 * 5. Apply (tri_ins_apply): out[b,k,t,c] = (flags[b,k,t,c] != 0) |
 *    (mask[k,t-1,c] != 0) | (mask[k,t,c] != 0), rows outside [0, nd) counting
 *    as 0, for every baseline, the unselected ones included; out may be flags
 *    itself.  ntime < 2: out = (flags != 0), with no other launch.
 *
 * At most 32 shapes, 0 <= lo < hi <= nchan, nsigma_i > 0, nsigma_narrow >= 0
 * (0 = no narrow candidate), rounds in [1, 16], min_count >= 1.  TRI_EINVAL
 * for violations, NULL pointers (other than select, and the shape arrays when
 * n_shapes == 0), negative sizes or overlapping outputs; TRI_EUNSUPPORTED for
 * dtypes other than complex64 and float32; TRI_EWORKSPACE when
 * workspace_bytes < tri_ins_workspace_bytes().  Empty shapes (for all but
 * tri_ins_apply that includes ntime < 2) return TRI_OK without a launch.
 * Input buffers are never written.  No floating-point atomics.
 */
int tri_ins_accumulate(const void *vis, int vis_dtype, const uint8_t *flags,
                       const uint8_t *select /* may be NULL */, int64_t nbl,
                       int64_t ncorr, int64_t ntime, int64_t nchan, double *sum,
                       int32_t *count, void *stream);
size_t tri_ins_workspace_bytes(int64_t ncorr, int64_t ntime, int64_t nchan);
int tri_ins_zscore(const double *sum, const int32_t *count, const uint8_t *mask,
                   int64_t ncorr, int64_t ntime, int64_t nchan, int64_t min_count,
                   float *level, int32_t *q, uint8_t *valid, void *workspace,
                   size_t workspace_bytes, void *stream);
int tri_ins_match(const double *sum, const int32_t *count, int64_t ncorr,
                  int64_t ntime, int64_t nchan, int64_t min_count,
                  const int64_t *shape_lo, const int64_t *shape_hi,
                  const double *shape_nsigma, int64_t n_shapes, double nsigma_narrow,
                  int64_t rounds, uint8_t *mask, void *workspace,
                  size_t workspace_bytes, void *stream);
int tri_ins_apply(const uint8_t *flags, const uint8_t *mask, uint8_t *out,
                  int64_t nbl, int64_t ncorr, int64_t ntime, int64_t nchan,
                  void *stream);

/*
 * Value-driven hysteresis growth of the flags of (n_win, ntime, nchan) windows
 * (beyond the reference; the model is the watershed of HERA's xrfi, the same
 * idea as Canny's edge linking; the definition below is this library's own
 * and identity with xrfi is not claimed).  What is flagged is a seed; an
 * unflagged neighbour joins it if it clears a threshold much lower than a
 * detection needs.  Per window, visibilities v[t, c] (complex64, or float32)
 * and uint8 flags f[t, c] (nonzero = flagged).
 *
 * 1. Amplitude, the flagger's own.  complex64: a = +inf if either part is
 *    infinite, otherwise (float)sqrt((double)re * re + (double)im * im);
 *    float32: a = fabsf(v).  A sample counts iff f == 0 and a is not NaN.
 * 2. Levels.  A time line is one (window, channel) over all rows; a frequency
 *    line is one (window, time row, frequency chunk k = channels
 *    [chunk_ends[k], chunk_ends[k + 1])); chunk_ends is a HOST array of
 *    n_chunk_ends non-decreasing entries from 0 to nchan, read before the call
 *    returns; an empty chunk is a no-op.  Over the m counting samples of a
 *    line with finite a: med is their median (the middle one for odd m,
 *    float32(x + y) / 2 of the two middle ones for even m, the sum rounded to
 *    float32); dev_i = fabsf(a_i - med), one float32 subtraction; mad is the
 *    median of the dev_i by the same rule.  The line is live iff m >= 3, med
 *    and mad are finite and mad > 0.
 * 3. Eligibility, per axis, with thr = (double)med + (nsigma_axis * 1.4826) *
 *    (double)mad in float64 without FMA (the product is rounded before the
 *    sum):
 *      e_axis = counts && (a == +inf || (live && (double)a > thr));
 *    nsigma_axis == 0 switches the axis off: e_axis = 0 everywhere.  The test
 *    is one-sided: RFI adds power.
 * 4. Seeds.  G_0 = (f != 0) & ~(missing != 0); missing is a uint8 image of the
 *    shape of f or NULL (nothing is missing).  A flagged sample that is no
 *    seed does not count: it is never eligible, blocks growth and starts none.
 * 5. Growth, `reach` synchronous rounds, neighbours outside the window are 0:
 *      G_{k+1}[t,c] = G_k[t,c] | (e_time[t,c] & (G_k[t-1,c] | G_k[t+1,c]))
 *                              | (e_freq[t,c] & (G_k[t,c-1] | G_k[t,c+1]))
 *    Growth along frequency does not stop at chunk ends; only the levels do.
 *      out_flags = (f != 0) | G_reach   (0/1)
 * A sample joins iff a path of at most `reach` steps leads to it from a seed
 * through cells that are each eligible on the axis of the step taken.  Every
 * round reads only the previous one: the result does not depend on tile shape,
 * batch size or schedule.  No floating-point atomics; input buffers are never
 * written.
 *
 * tri_hyst_levels writes the four level arrays, float32: med_time / mad_time
 * (n_win, nchan), med_freq / mad_freq (n_win, ntime, n_chunk_ends - 1); both
 * values of a line that is not live are NaN (0x7FC00000).  tri_hyst_eligible
 * writes e_time and e_freq as (n_win, ntime, nchan) uint8 0/1 images.
 * tri_hyst_grow is stage 5 alone on any three uint8 images (nonzero = set):
 * out = G_reach with G_0 = (seeds != 0).  tri_hysteresis_growth is the whole
 * step.
 *
 * Workspace (tri_hyst_workspace_bytes; the same size serves all four calls;
 * tri_hyst_grow needs that of n_chunk_ends = 2): three bit planes of 32-channel
 * words, rows padded to whole words, and the level arrays -- 3 / 8 byte per
 * sample, plus 8 bytes per time line and per frequency line, each array
 * rounded up to 256 bytes: 0.40 byte per sample at 1024 x 4096 and 10 chunks.
 *
 * TRI_EINVAL for NULL pointers (other than missing), negative shapes, an
 * nsigma that is negative or NaN, a reach outside [1, 32], chunk ends that do
 * not run from 0 to nchan, and outputs overlapping inputs; TRI_EUNSUPPORTED
 * for dtypes other than complex64 and float32 and for more lines than one
 * launch holds (pass fewer windows per call); TRI_EWORKSPACE when
 * workspace_bytes < tri_hyst_workspace_bytes().  Empty shapes return TRI_OK
 * without a launch.
 */
size_t tri_hyst_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan,
                                int64_t n_chunk_ends);
int tri_hyst_levels(const void *vis, int vis_dtype, const uint8_t *flags,
                    int64_t n_win, int64_t ntime, int64_t nchan,
                    const int64_t *chunk_ends, int64_t n_chunk_ends,
                    float *med_time, float *mad_time, float *med_freq, float *mad_freq,
                    void *workspace, size_t workspace_bytes, void *stream);
int tri_hyst_eligible(const void *vis, int vis_dtype, const uint8_t *flags,
                      int64_t n_win, int64_t ntime, int64_t nchan,
                      double nsigma_time, double nsigma_freq,
                      const int64_t *chunk_ends, int64_t n_chunk_ends,
                      uint8_t *e_time, uint8_t *e_freq,
                      void *workspace, size_t workspace_bytes, void *stream);
int tri_hyst_grow(const uint8_t *seeds, const uint8_t *e_time, const uint8_t *e_freq,
                  uint8_t *out, int64_t n_win, int64_t ntime, int64_t nchan,
                  int64_t reach, void *workspace, size_t workspace_bytes, void *stream);
int tri_hysteresis_growth(const void *vis, int vis_dtype, const uint8_t *flags,
                          const uint8_t *missing /* may be NULL */, uint8_t *out_flags,
                          int64_t n_win, int64_t ntime, int64_t nchan,
                          double nsigma_time, double nsigma_freq, int64_t reach,
                          const int64_t *chunk_ends, int64_t n_chunk_ends,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Quality statistics of the unflagged samples: a measurement beside the
 * strategy chain, not a strategy step (after AOFlagger's quality statistics;
 * the definition is this library's own).
 *
 * vis (n_bl, n_corr, ntime, nchan) complex64, or float32 amplitudes whose
 * imaginary part is 0; flags of the same shape, uint8, nonzero = flagged.
 * A sample is valid iff it is unflagged and both parts are finite; in float64,
 * with the parts converted exactly, p = re * re + im * im.  A pair (t, c),
 * 0 <= c < nchan - 1, is valid iff samples (t, c) and (t, c + 1) are:
 * dre = re[c + 1] - re[c], dim likewise, dp = dre * dre + dim * dim (every
 * operation rounded on its own, no FMA).  The pair belongs to channel c.
 *
 * Six numbers per cell -- n (valid samples), sum_re, sum_im, sum_p, dn (valid
 * pairs), dsum_p -- for the cells of three groupings:
 *   bl    (n_bl, n_corr)   over time and chan
 *   time  (n_corr, ntime)  over bl and chan
 *   chan  (n_corr, nchan)  over bl and time
 * With N the grouping's cell count in that order, counts_* is int64 [2][N] =
 * (n, dn) and sums_* is float64 [4][N] = (sum_re, sum_im, sum_p, dsum_p).
 * All accumulation is in float64 and int64.
 *
 * Order contract.  A window's contribution to each of its cells is reduced in
 * an order that depends on (ntime, nchan) alone, never on the number of
 * windows of the call or the window's place in it.  The time and chan cells
 * add the windows' contributions sequentially in ascending baseline order,
 * acc = acc + contribution[b], from 0 -- or, with accumulate != 0, from the
 * values the arrays hold.  So one call over all baselines, one call per
 * baseline and any split into consecutive baseline ranges continued with
 * accumulate give the same bits, and so does every run.  bl cells are always
 * written, never accumulated.  No floating-point atomics; the inputs are never
 * written.
 *
 * Workspace (tri_quality_workspace_bytes; 0 for an empty shape or one beyond
 * the launch geometry): 40 bytes per (window, strip of 256 channels, time row)
 * and 48 bytes per (window, channel) and per (window, time row), each array
 * rounded up to 256 bytes -- 2.7 % of a complex64 window at 1024 x 4096.
 *
 * TRI_EINVAL for NULL pointers, negative sizes, a dtype other than complex64
 * and float32, and outputs that overlap the inputs or each other;
 * TRI_EWORKSPACE for a missing or short workspace; TRI_EUNSUPPORTED for more
 * windows, rows or channels than one launch holds (pass fewer baselines per
 * call).  A shape with a zero extent writes zeros (time and chan cells stay
 * as they are under accumulate) and returns TRI_OK without a launch.
 */
size_t tri_quality_workspace_bytes(int64_t n_bl, int64_t n_corr, int64_t ntime, int64_t nchan);
int tri_window_quality(const void *vis, int vis_dtype, const uint8_t *flags,
                       int64_t n_bl, int64_t n_corr, int64_t ntime, int64_t nchan,
                       int64_t *counts_bl, double *sums_bl,
                       int64_t *counts_time, double *sums_time,
                       int64_t *counts_chan, double *sums_chan, int accumulate,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * Log-binned amplitude histograms of the kept and of the flagged samples: a
 * measurement beside the strategy chain, not a strategy step (after the
 * "log N - log S" histogram AOFlagger keeps beside its quality statistics; the
 * definition is this library's own).
 *
 * vis (n_bl, n_corr, ntime, nchan) complex64, or float32 amplitudes; flags of
 * the same shape, uint8, nonzero = flagged.  Every sample is counted exactly
 * once, in one population (0 = kept: its flag is 0; 1 = flagged) and one slot.
 *
 * Bins are three integers: emin and emax, -126 <= emin < emax <= 128, and
 * sub_bits, 0 <= sub_bits <= 5; nb = (emax - emin) << sub_bits bins, at most
 * TRI_MAX_HIST_BINS.  There are nb + 3 slots (tri_histogram_slots; 0 for bins
 * that are not allowed): 0 underflow (zero included), 1 .. nb the bins, nb + 1
 * overflow, nb + 2 non-finite.  The slot of a sample:
 *   1. either part NaN or +-Inf (a float32 input has one part): nb + 2;
 *   2. otherwise a = (float)sqrt((double)re * re + (double)im * im) for
 *      complex64, |x| for float32;
 *   3. u = the bit pattern of a, and
 *      k = (u >> (23 - sub_bits)) - ((emin + 127) << sub_bits);
 *   4. k < 0: slot 0; k >= nb: slot nb + 1 (finite parts whose amplitude
 *      rounds to +Inf land here); otherwise slot k + 1.
 * No logarithm and no floating-point comparison.  With s = sub_bits, bin k
 * covers [2^(emin + (k >> s)) * (1 + (k mod 2^s) / 2^s), next edge).
 *
 * Two groupings, filled in the same pass:
 *   hist_bl     (n_bl, n_corr, 2, nb + 3) int64: one cell per window;
 *   hist_chunk  (n_corr, n_chunk_ends - 1, 2, nb + 3) int64: over baselines and
 *               times, per frequency chunk [chunk_ends[g], chunk_ends[g + 1]).
 * chunk_ends is a host array that runs from 0 to nchan and never decreases; a
 * repeated end is an empty chunk whose cells get nothing.  hist_bl is always
 * written fresh (zeroed on `stream` first); hist_chunk is zeroed first when
 * accumulate is 0 and continued from its contents otherwise.  Counts are
 * integers added with integer atomics: the same bits for every order, every
 * split into baseline ranges continued with accumulate, and every run.  No
 * workspace; both outputs are the caller's; the inputs are never written.
 *
 * TRI_EINVAL for NULL pointers, negative sizes, a dtype other than complex64
 * and float32, bins that are not allowed, chunk ends that do not run from 0 to
 * nchan in non-decreasing order, and outputs that overlap an input or each
 * other.  TRI_EUNSUPPORTED beyond the launch geometry: an extent above
 * 2^31 - 1, more than 2^24 - 1 (window, band of 64 time rows) pairs in one
 * call (pass fewer baselines per call), a chunk wider than 65535 * 1024
 * channels, more than 2^30 chunk ends.  A shape with a zero extent zeroes what
 * it would have zeroed and returns TRI_OK without a launch.
 */
int64_t tri_histogram_slots(int emin, int emax, int sub_bits);
int tri_amplitude_histogram(const void *vis, int vis_dtype, const uint8_t *flags,
                            int64_t n_bl, int64_t n_corr, int64_t ntime, int64_t nchan,
                            const int64_t *chunk_ends, int64_t n_chunk_ends,
                            int emin, int emax, int sub_bits,
                            int64_t *hist_bl, int64_t *hist_chunk, int accumulate, void *stream);

/*
 * Sliding 2-D median background of (n_win, ntime, nchan) windows and the
 * thresholding of single samples on the robust z-score against it (beyond the
 * reference; the model is detrend_medfilt of HERA's xrfi, the definition is
 * this library's own and identity with xrfi is not claimed: the neighbourhood
 * is cut at the edges, not reflected, and flagged samples are left out of both
 * medians).  Every window is treated on its own.  Per window, visibilities v
 * (complex64, or float32 amplitudes), uint8 flags f (nonzero = flagged), radii
 * Kt = radius_time, Kf = radius_freq and min_samples:
 *   a      = the flagger's amplitude: hypotf for complex64, fabsf for float32.
 *   valid  = f == 0 and a is finite (its bit pattern lies below 0x7F800000).
 *   W(t,f) = every (t', f') of the window's image with |t' - t| <= Kt and
 *            |f' - f| <= Kf: cut at the edges, never reflected, never another
 *            window's sample.
 *   median of n values x_0 <= ... <= x_{n-1}: x_{(n-1)/2} for odd n,
 *            (float)(((double)x_{n/2-1} + (double)x_{n/2}) / 2.0) for even n,
 *            NaN for n < min_samples.
 *   b(t,f) = the median of the valid a over W(t,f): defined at every sample,
 *            whether or not the centre is valid.
 *   r      = a - b, one float32 subtraction without contraction, where the
 *            centre is valid and b is not NaN; NaN otherwise.
 *   m(t,f) = the median, by the same rule and min_samples, of fabsf(r) over the
 *            non-NaN r of W(t,f).
 *   z      = (float)((double)r / ((double)m * 1.4826)) where r and m are not
 *            NaN, NaN otherwise; IEEE from there: m == 0 gives NaN for r == 0
 *            and +-inf otherwise.
 *   hit    = (double)fabsf(z) > nsigma: a NaN never hits, an infinite z does.
 *   rounds: g_0 = (f != 0); for k = 1 ... rounds the hits of (v, g_{k-1}) give
 *            g_k = g_{k-1} | hit_k;  out_flags = g_rounds  (0/1).
 * Every NaN written is 0x7FC00000.  The medians are exact selections: the same
 * bits on every run, for every alignment and for every split of the windows
 * over calls.  Input buffers are never written.
 * Limits: Kt and Kf in [0, 32], not both 0; area = (2 Kt + 1)(2 Kf + 1) <= 625;
 * min_samples in [1, area]; nsigma > 0 and not NaN; rounds in [1, 4].
 * tri_medfilt_background writes b (background) and, unless NULL, r (residual).
 * tri_medfilt_zscore takes any float32 residual image (every non-NaN value
 * counts, an infinite one too) and writes z (zscore) and, unless NULL, m
 * (scale); its outputs must not overlap residual.
 * tri_median_zscore_threshold runs the rounds.  There is no workspace: residual
 * and zscore are required (n_win, ntime, nchan) float32 images of the caller's
 * and are OUTPUTS: on return they hold the last round's r and z, every element
 * written, whatever they held before.  out_flags doubles as the running flags
 * g_k.  No output may overlap an input or another output.
 * TRI_EINVAL for NULL pointers (other than those marked), negative shapes, bad
 * radii, min_samples, nsigma, rounds and overlaps; TRI_EUNSUPPORTED for vis
 * dtypes other than complex64 and float32 and for more tiles than one launch
 * holds (pass fewer windows per call).  Empty shapes return TRI_OK without a
 * launch.
 */
int tri_medfilt_background(const void *vis, int vis_dtype, const uint8_t *flags,
                           int64_t n_win, int64_t ntime, int64_t nchan,
                           int64_t radius_time, int64_t radius_freq, int64_t min_samples,
                           float *background, float *residual /* may be NULL */,
                           void *stream);
int tri_medfilt_zscore(const float *residual, int64_t n_win, int64_t ntime, int64_t nchan,
                       int64_t radius_time, int64_t radius_freq, int64_t min_samples,
                       float *scale /* may be NULL */, float *zscore, void *stream);
int tri_median_zscore_threshold(const void *vis, int vis_dtype, const uint8_t *flags,
                                uint8_t *out_flags, int64_t n_win, int64_t ntime,
                                int64_t nchan, int64_t radius_time, int64_t radius_freq,
                                int64_t min_samples, double nsigma, int64_t rounds,
                                float *residual, float *zscore, void *stream);

/*
 * Antenna integration (beyond the reference; the models are CASA's antint mode
 * and AOFlagger's antenna selection, the definition is this library's own):
 * baseline integration with one image per antenna instead of one for all
 * baselines, and a flags-only variant that extends the flags of an antenna
 * whose baselines are mostly flagged.  vis (nbl, n) complex64 or float32
 * amplitudes, flags (nbl, n) uint8 (nonzero = flagged), n = ncorr * ntime *
 * nchan, i a position in [0, n).  Baseline b has the antennas ant1[b], ant2[b].
 *   membership: baseline b is a member of antenna a if it is selected, is not an
 *              auto-correlation where those are excluded, and ant1[b] == a or
 *              ant2[b] == a; an auto-correlation that takes part is a member of
 *              its antenna once.  members[a] is their number and list[a] the
 *              members in ascending b.  The caller builds the lists on the host
 *              in CSR form: list[a] = baselines[offsets[a] .. offsets[a + 1]),
 *              offsets[nant + 1] and baselines[] int32 on the device, offsets
 *              never decreasing and inside baselines[].
 *   a        = +inf if re or im is infinite, else (float)sqrt((double)re * re
 *              + (double)im * im)   (fabsf(v) for amplitudes), exactly as in
 *              baseline integration; a sample counts if its flag is 0 and a is
 *              not NaN
 *   tri_antenna_accumulate: for every antenna a, b over list[a] in list order
 *              and every counting sample sum[a, i] += (double)a, count[a, i]
 *              += 1; sum float64 and count int32 of shape (nant, n).  One
 *              thread per (a, i), no atomics, no re-association.  A list entry
 *              outside [0, nbl) is skipped.  The call ADDS to sum and count
 *              (the caller zeroes them first), so the baselines fed in several
 *              calls in ascending order, each call with the lists of its own
 *              baselines, give the bits of one call.  vis == NULL is the
 *              flags-only form: a sample counts if its flag is 0, vis_dtype is
 *              not read, sum is not touched and may be NULL.
 *   tri_antenna_mean: flag[a, i] = count[a, i] < min_count[a];  amp[a, i] =
 *              (float)(sum[a, i] / (double)count[a, i]) where flag is 0, else 0.
 *              min_count[nant] int32 on the device; the caller computes
 *              min_count[a] = max(1, ceil(min_baseline_frac * members[a])), and
 *              a value below 1 counts as 1, so an antenna without members is
 *              flagged throughout.
 *   (the flagger: tri_sum_threshold_flagger on amp / flag as one float32 block
 *   of nant * ncorr windows gives det[nant, n])
 *   tri_antenna_flag_excess: det[a, i] = members[a] > 0 && members[a] -
 *              count[a, i] > max_flagged[a], with count of the flags-only
 *              form; members[nant], max_flagged[nant] int32 on the device; the
 *              caller computes max_flagged[a] = floor(min_flagged_frac *
 *              members[a]).  Integers only.
 *   tri_antenna_broadcast_or: out[b, i] = (flags[b, i] != 0) | (det[ant1[b], i]
 *              != 0) | (det[ant2[b], i] != 0) for EVERY baseline, whether it is
 *              a member of anything or not; ant1[nbl], ant2[nbl] int32 on the
 *              device; an antenna number outside [0, nant) contributes
 *              nothing.  out may be flags itself.
 * TRI_EINVAL for NULL pointers (other than those named), negative sizes, det
 * overlapping count, out overlapping det (or overlapping flags without being
 * flags); TRI_EUNSUPPORTED for dtypes other than complex64 and float32, more
 * than 65535 antennas and images beyond the index range.  No workspace.  Empty
 * shapes return TRI_OK without a launch.
 */
int tri_antenna_accumulate(const void *vis /* may be NULL */, int vis_dtype,
                           const uint8_t *flags, const int32_t *offsets,
                           const int32_t *baselines, int64_t nbl, int64_t nant,
                           int64_t n, double *sum /* may be NULL without vis */,
                           int32_t *count, void *stream);
int tri_antenna_mean(const double *sum, const int32_t *count, const int32_t *min_count,
                     int64_t nant, int64_t n, float *amp, uint8_t *flag, void *stream);
int tri_antenna_flag_excess(const int32_t *count, const int32_t *members,
                            const int32_t *max_flagged, int64_t nant, int64_t n,
                            uint8_t *det, void *stream);
int tri_antenna_broadcast_or(const uint8_t *flags, const uint8_t *det,
                             const int32_t *ant1, const int32_t *ant2, uint8_t *out,
                             int64_t nbl, int64_t nant, int64_t n, void *stream);

/*
 * Spectral kurtosis along time (beyond the reference; the estimator is Nita &
 * Gary 2010, the definition with its operation order is this library's own).
 * It asks whether the statistics of a channel over a stretch of time are those
 * of noise, and flags whole (block of rows, channel) cells where they are not:
 * pulsed interference pushes the estimator well above 1, a steady carrier
 * towards 0.  It needs no background, no noise estimate and no bandpass.
 * vis (n_win, ntime, nchan) complex64 or float32, flags of the same shape,
 * any non-zero byte is flagged; windows are independent.
 *   power:   arithmetic is float64, the operation order below is the
 *            definition, nothing is fused.  complex64: p = (double)re *
 *            (double)re + (double)im * (double)im (both products exact, one
 *            rounding).  float32: p = (double)x * (double)x.  A sample is valid
 *            when its flag is 0 and p is finite; a NaN or infinite part makes
 *            it invalid.
 *   blocks:  block_time = M is an integer in [2, 65536].  Block b holds the rows
 *            [b*M, min(T, (b+1)*M)), so there are nb = ceil(T / M) blocks.
 *   sums:    for every window, block and channel, walk the block's rows in
 *            ascending time order, starting from n = 0, S1 = +0.0, S2 = +0.0.
 *            For each valid sample: n += 1; S1 = S1 + p; S2 = S2 + (p * p), the
 *            product rounded before the add.  The order is sequential.  A tree
 *            or pairwise sum is a different result and is wrong.
 *   estimator: with d = shape (a finite double greater than 0; it is 1 for raw
 *            correlator dumps and N for data that is already an average of N):
 *              q  = ((double)n * S2) / (S1 * S1)
 *              k  = (((double)n * d + 1.0) / ((double)n - 1.0)) * (q - 1.0)
 *              sk = (float)k
 *            sk is the NaN 0x7FC00000 in two cases: n < min_samples
 *            (min_samples is an integer in [2, M]; a last block with fewer
 *            than min_samples rows never reaches it and is never hit), and
 *            S1 * S1 not greater than 0 (all-zero data, underflow).  Any other
 *            NaN is also written as 0x7FC00000.  Under a gamma law of shape d,
 *            which exponential power is with d = 1, the expectation of k is 1.
 *   outputs of the statistics pass: sk float32 (n_win, nb, nchan); count int32
 *            of the same shape, holding n.  Every element of both is written.
 *   decision: two tables of M + 1 doubles, lower[n] and upper[n], indexed by
 *            the valid count.  hit = (double)sk < lower[n] || (double)sk >
 *            upper[n].  A NaN sk never hits.  A NaN table entry never hits:
 *            that is how a side is switched off.  A count outside [0, M]
 *            (tri_sk_apply takes any) never hits.
 *            out[w, t, f] = (flags[w, t, f] != 0) | hit[w, t / M, f], 0 or 1.
 *            The inputs are never written.  A second round cannot change
 *            anything, because a hit block has no valid sample left: there is
 *            no rounds argument.
 * tri_sk_statistics writes sk and, unless NULL, count.  tri_sk_apply takes the
 * statistics back in.  tri_sk_threshold runs both; sk and count are required
 * and are OUTPUTS.  lower and upper are device pointers to block_time + 1
 * doubles each; they belong to the caller and are read only.  There is no
 * workspace: all buffers are the caller's.  The sums run in the order above
 * whatever the alignment and however the windows are split over calls: the
 * same bits on every run.
 * TRI_EINVAL for NULL pointers (other than count of tri_sk_statistics),
 * negative shapes, block_time, shape or min_samples out of range or NaN, and
 * any output overlapping an input or another output; TRI_EUNSUPPORTED for vis
 * dtypes other than complex64 and float32 and for more cells than one launch
 * holds (pass fewer windows per call).  Empty shapes return TRI_OK without a
 * launch.
 */
int tri_sk_statistics(const void *vis, int vis_dtype, const uint8_t *flags,
                      int64_t n_win, int64_t ntime, int64_t nchan,
                      int64_t block_time, double shape, int64_t min_samples,
                      float *sk, int32_t *count /* may be NULL */,
                      void *stream);
int tri_sk_apply(const float *sk, const int32_t *count, const uint8_t *flags,
                 uint8_t *out_flags,
                 int64_t n_win, int64_t ntime, int64_t nchan, int64_t block_time,
                 const double *lower, const double *upper,
                 void *stream);
int tri_sk_threshold(const void *vis, int vis_dtype, const uint8_t *flags,
                     uint8_t *out_flags,
                     int64_t n_win, int64_t ntime, int64_t nchan,
                     int64_t block_time, double shape, int64_t min_samples,
                     const double *lower, const double *upper,
                     float *sk, int32_t *count,
                     void *stream);

/*
 * Piecewise-polynomial fit along the lines of a window and flagging of what
 * stands off it (beyond the reference; after CASA's tfcrop, the definition
 * with its operation order is this library's own).  Every line is normalised
 * by itself: the fit absorbs a bandpass shape, a fringe or a gain drift, and
 * the threshold is the scatter about the fit on the same line.
 * vis (n_win, ntime, nchan) complex64 or float32, flags of the same shape,
 * any non-zero byte is flagged; windows are independent.
 *   a      = the float32 amplitude: complex64 (float)sqrt((double)re *
 *            (double)re + (double)im * (double)im), +inf when a part is
 *            infinite; float32 fabsf(x).
 *   valid  = flag == 0 and a is finite.
 * All arithmetic below is float64, one correctly rounded operation at a time
 * in the order written; nothing is fused; division and sqrt are IEEE.
 *   fit of one line a[0..n) under a mask m, P pieces, degree D in 0..3:
 *            piece p covers [e_p, e_{p+1}) with e_p = (p * n) / P (integer
 *            division); a piece may be empty.  In a piece of length L the
 *            sample j = i - e_p has x = (double)(2 * j + 1 - L) / (double)L.
 *     moments: two-level sums with cells of 32 consecutive samples counted
 *            from the piece start.  Within a cell, from +0.0, in ascending j
 *            over the masked samples, with pw_0 = 1.0 and pw_k = pw_{k-1} * x:
 *            s_k = s_k + pw_k (k = 0..2D), b_k = b_k + pw_k * (double)a
 *            (k = 0..D).  S_k and B_k are the cell sums added from +0.0 in
 *            ascending cell order; n_p is the masked count of the piece.  The
 *            two-level order is part of the definition; a sequential, tree or
 *            pairwise sum over the piece is a different result and is wrong.
 *     solve: n_p == 0: the fit is NaN over the piece.  Otherwise d = min(D,
 *            n_p - 1) and A[i][j] = S_{i+j} (i, j <= d) is factored by
 *            Cholesky, column j = 0..d:  v = A[j][j], then v = v - l[j][k] *
 *            l[j][k] for k = 0..j-1 one term at a time.  If !(v > 0x1p-20 *
 *            S_0): d = j - 1, the leading factor is kept and the factoring
 *            ends (samples clustered in a corner of a piece get a lower
 *            degree, down to the mean).  Else l[j][j] = sqrt(v) and for i > j:
 *            t = A[i][j], t = t - l[i][k] * l[j][k] for k = 0..j-1 one term at
 *            a time, l[i][j] = t / l[j][j].  Forward: for i = 0..d, t = B_i,
 *            t = t - l[i][k] * y_k for k = 0..i-1, y_i = t / l[i][i].  Back:
 *            for i = d..0, t = y_i, t = t - l[k][i] * c_k for k = i+1..d in
 *            ascending k, c_i = t / l[i][i].
 *     value: Horner from c_d down: f = c_d, then f = f * x + c_k for
 *            k = d-1..0.  Residual r = (double)a - f.
 *   rounds on one line with the starting mask m0, max_pieces, degree, cutoff,
 *            rounds, min_samples: hit = 0; for r = 0..rounds-1: m = m0 & ~hit;
 *            P = min(2r + 1, max_pieces); the degree is min(1, degree) in round
 *            0 and degree after it; n_m = the masked count of the line; if n_m
 *            < min_samples the rounds end.  Fit.  Q: the cell sums of r * r
 *            (the cells of the fit, chains in ascending j over the masked
 *            samples, from +0.0) added from +0.0 in ascending cell order
 *            within a piece, pieces ascending -- one chain over all cells of
 *            the line.  sigma = sqrt(Q / (double)n_m).  A masked sample is hit
 *            when fabs(r) > cutoff * sigma and fabs(r) > fabs(f) * 0x1p-20;
 *            the second condition keeps noise-free data from being flagged on
 *            rounding residue.
 *   step:    order 0 = freqtime (along frequency: every time row is a line;
 *            then along time: every channel is a line), 1 = timefreq, 2 = freq
 *            only, 3 = time only.  The first pass has m0 = valid, the second
 *            m0 = valid & ~hits_first.  out = (flags != 0) | hits_time |
 *            hits_freq, 0 or 1.  The inputs are never written.
 *   ranges:  cutoffs finite and > 0, degrees in 0..3, pieces in 1..32, rounds
 *            in 1..16, min_samples >= 2.  tfcrop's defaults: time cutoff 4.0,
 *            degree 1, 1 piece; frequency cutoff 3.0, degree 3, 7 pieces;
 *            5 rounds, min_samples 8.
 * tri_polyfit_background does one fit per line of `axis` (0 = time, 1 =
 * frequency) with m = valid, `pieces` pieces and `degree`, no rounds:
 * background (n_win, ntime, nchan) float32 is (float)f at EVERY sample, flagged
 * ones included, and the NaN 0x7FC00000 where a piece has no valid sample (and
 * for any other NaN).  Called with the flags of tri_polyfit_threshold it is the
 * robust bandpass or time trend.
 * A fitted line holds at most 16384 samples: a longer ntime (when the time axis
 * is fitted) or nchan (when the frequency axis is) is TRI_EUNSUPPORTED before
 * any launch; the axis that is not fitted has no such limit.
 * scratch: a device buffer of tri_polyfit_workspace_bytes(n_win, ntime, nchan,
 * time_pieces) bytes, with time_pieces the pieces of the fit along time (0
 * when no fit runs along time; 0..32, anything else gives 0).  It holds the
 * amplitudes, one state byte per sample and the fits of the time pass; its
 * prior contents do not matter (tests/test_polyfit.py fills it with 0xFF and
 * with zeros before every call of the C entry points).  The
 * sums run in the order above whatever the alignment and however the windows
 * are split over calls: the same bits on every run.
 * TRI_EINVAL for NULL pointers, negative shapes, an order, axis, cutoff,
 * degree, pieces, rounds or min_samples out of range or NaN, and an output or
 * the scratch buffer overlapping an input or each other; TRI_EUNSUPPORTED for vis
 * dtypes other than complex64 and float32, for a fitted line of more than 16384
 * samples and for more lines than one launch holds (pass fewer windows per
 * call); TRI_EWORKSPACE for a NULL or short scratch buffer.  Empty shapes return
 * TRI_OK without a launch.
 */
size_t tri_polyfit_workspace_bytes(int64_t n_win, int64_t ntime, int64_t nchan,
                                   int64_t time_pieces);
int tri_polyfit_background(const void *vis, int vis_dtype, const uint8_t *flags,
                           int64_t n_win, int64_t ntime, int64_t nchan,
                           int axis, int64_t pieces, int64_t degree,
                           float *background,
                           void *scratch, size_t scratch_bytes, void *stream);
int tri_polyfit_threshold(const void *vis, int vis_dtype, const uint8_t *flags,
                          uint8_t *out_flags,
                          int64_t n_win, int64_t ntime, int64_t nchan, int order,
                          double time_cutoff, int64_t time_degree,
                          int64_t time_pieces,
                          double freq_cutoff, int64_t freq_degree,
                          int64_t freq_pieces,
                          int64_t rounds, int64_t min_samples,
                          void *scratch, size_t scratch_bytes, void *stream);

/* Thread-local description of the last failure in the calling thread. */
const char *tri_last_error(void);

/* Library / ABI version (major * 100 + minor). */
int tri_version(void);

/*
 * Measurement hooks (used by bench.py and tests only; not part of the
 * reference's interface).
 *
 * tri_bench_sumthreshold runs ONLY the fused SumThreshold column kernel
 * (clamp + float64 prefix + multi-scale thresholds + flag dilation, all
 * windows in one pass; flagging.py:582-681) `repeats` times on `stream`,
 * bracketed by HIP events recorded on that stream, and returns the mean kernel
 * time in milliseconds through `ms_per_launch`.
 *   data (n_win, n_line, n_col) float32 residuals; the sequential axis is
 *        n_line, columns are coalesced
 *   mad  (n_win, n_col) float64 medians of |data| (NaN = nothing unflagged)
 *   out  (n_win, n_line, n_col) uint8
 * `variant`: 0 = best available for these windows, 1 = generic (dynamic
 * windows, global rings), 2 = register cascade (windows 1,2,4,8 only),
 * 3 = lane-mask cascade (windows 1,2,4,8, window below 2^31 bytes; what 0
 * selects for those), 4 = stage pipeline across the waves of a workgroup with
 * the prefix rings in LDS (K7p; any list of up to eight windows whose rings
 * fit 160 KB, e.g. 32, 48, 64, 128 -- the flagger's route for such lists),
 * 5 = the lane-mask cascade on COLUMN PANELS [n_col / 64][n_line][64] (what the
 * flagger's time-axis pass runs, and what 0 selects when n_col % 64 == 0): the
 * row images are re-laid out before the timed region, the flags taken back to
 * rows after it.
 */
int tri_bench_sumthreshold(const float *data, const double *mad, uint8_t *out,
                           int64_t n_win, int64_t n_line, int64_t n_col,
                           const int64_t *windows, int64_t n_windows,
                           double outlier_nsigma, double rho, int variant,
                           int repeats, float *ms_per_launch, void *stream);

/*
 * tri_test_sumthreshold: the same launch (one body with
 * tri_bench_sumthreshold) over CHUNKED lines, as the flagger's frequency-axis
 * pass runs it: chunk g of every column is the lines
 * [chunk_ends[g], chunk_ends[g + 1]) with a threshold of its own, thresholded
 * on its line padded by max(windows) - 1 positions on either side
 * (flagging.py:610-681).  2 <= n_chunk_ends <= 256; the ends must not decrease
 * and lie in [0, n_line] (TRI_EINVAL otherwise); empty chunks are legal.
 *   mad  (n_win, n_col, n_chunk_ends - 1) float64
 *   out  written inside [chunk_ends[0], chunk_ends[n_chunk_ends - 1]) only
 * `variant` as above, except that 0 picks what the flagger would for these
 * windows and chunks (the stage pipeline for a list it takes; the panel form
 * of the lane-mask cascade with one chunk only), and that variant 5 with more
 * than one chunk is TRI_EUNSUPPORTED: the flagger never pairs column panels
 * with chunks.  Windows wider than n_line are not supported (the flagger's
 * parameter preparation drops them before any kernel sees them).
 */
int tri_test_sumthreshold(const float *data, const double *mad, uint8_t *out,
                          int64_t n_win, int64_t n_line, int64_t n_col,
                          const int64_t *windows, int64_t n_windows,
                          double outlier_nsigma, double rho, int variant,
                          int repeats, float *ms_per_launch, void *stream,
                          const int64_t *chunk_ends, int64_t n_chunk_ends);

/*
 * tri_bench_boxfilter runs ONE axis stage of masked_gaussian_filter's two box
 * filters (flagging.py:362-419, 469-513) `repeats` times on `stream` in the
 * launch geometry the flagger itself uses, bracketed by HIP events on that
 * stream; mean time per stage in `ms_per_launch`.
 *   stage 0: time-axis stage.  data (n_win, n_line, n_col) float32, line axis
 *            = time, columns coalesced; flags4 the same window's flags packed
 *            four line positions per 32-bit word, (n_win, n_line / 4, n_col)
 *            words; out_w / out_o (n_win, n_line, n_col) receive the filtered
 *            weight (!flag) and weight * data images, already divided by
 *            float32(2 r + 1) ** 4.
 *   stage 1: frequency-axis stage fused with the masked division of the
 *            rejection loop (flagging.py:506-513, 563-566).  `flags4` is a float32
 *            array (n_win, 2, n_line, n_col): per window the time-filtered weight
 *            image followed by the weight * data image, lines contiguous (n_col
 *            positions each); `data` the amplitudes (n_win, n_col, n_line);
 *            out_o (n_win, n_col, n_line) receives |data - background|, out_w
 *            is scratch of the same size.
 *   stage 2: the 1-D filter of the spectrum path (flagging.py:945-947 via
 *            :516-579): n_win = 1, data (n_line, n_col) float32 with the line
 *            axis = channel and one column per window of a batch, flags4 one
 *            BYTE per sample (n_line, n_col); out_w / out_o (n_line, n_col)
 *            receive the filtered weight and weight * data images, divided by
 *            float32(2 r + 1) ** 4.
 * `variant`: 0 = the flagger's default route for this radius, 1 = LDS delay
 * lines only (K4b / K4c), 2 = register delay lines (K4r).  Stages 0 and 2:
 * TRI_EUNSUPPORTED where the route would be the in-place multi-pass filter
 * (K4), which needs images padded to n_line + 4 r rows -- stage 0 beyond
 * LANE4_R_MAX, stage 2 beyond the register rings and the stage pipeline.
 * (Stage 1, radius >= 56: the flagger takes the exact row filter, variant 0 the stage pipeline; variant 4 is K4x.)
 * For stage 2: 0 = default route, 1 = register delay lines (K4r), 2 / 3 = the
 * stage pipeline across four waves (K4p) with blocks of 16 / 8 positions
 * (TRI_EUNSUPPORTED when that block length does not apply to the shape).
 * For stage 1 also: 3 = the eight-wave stage pipeline (K4qf), 4 = the exact
 * row filter (K4x: one line pair resident in LDS, lanes = positions, any
 * radius; the time covers the kernel and the transpose of its rows to out_o).
 * Stages 0 and 1: 3 = the stage pipeline (K4q / K4qf) with the block length the
 * flagger would take (8 positions while the delay line fits 128 registers,
 * else 16), 5 = the same with blocks of 16 positions throughout.
 */
int tri_bench_boxfilter(const float *data, const uint8_t *flags4, float *out_w,
                        float *out_o, int64_t n_win, int64_t n_line, int64_t n_col,
                        int64_t radius, int stage, int variant, int repeats,
                        float *ms_per_launch, void *stream);

/*
 * Test hook: how many line passes the last tri_bench_boxfilter(stage 1,
 * variant 4) call of this thread ran, and how many of them failed the exactness
 * check and were redone in the reference's sequential order
 * (kernels_boxexact.hpp; flagging.py:398-416).
 */
int tri_boxx_last_stats(uint64_t *passes, uint64_t *sequential);

/*
 * Test hook: counters of the one-pass block-median + rejection kernels of the background loop (kernels_reject.hpp,
 * kernels_reject_tile.hpp) since the last reset -- out20[0..2] = blocks the one-workgroup form (K3r) ran, fell back
 * before / after its pass; [3] = second rounds of the tile-parallel form (K3t: median outside the predicted window or
 * the decision bracket); [4 + r] = blocks K3t handed to the one-workgroup redo for reason r (1 nothing to predict
 * from, 2 / 10 a wave's window-key / undecided list overflowed, 3 empty, 4 median in an end bin, 5 a block list
 * overflowed, 6 / 7 window / bracket miss in round 2).  Synchronises the device.  No reference counterpart.
 */
int tri_medrej_stats(uint64_t *out20, int reset);

/*
 * Measurement hook: per-thread kernel log.  op 0 clears the log and switches it on; op 1 writes
 * "kernel=launches;kernel=launches;..." (demangled device kernel symbols launched by this thread since op 0)
 * into buf[cap] and switches the log off; op 2 switches it off.  bench.py names the kernels of its roofline
 * legs with it and derives the step's dominant kernel family from the launch counts.  Returns the number of
 * distinct kernels (op 1).  No reference counterpart.
 */
int tri_kernel_log(int op, char *buf, int64_t cap);

/*
 * Test hook: tri_sum_threshold_flagger that additionally taps the LAST major
 * iteration's intermediates of window 0 into caller-provided device buffers
 * (Fa = averaged channels, N = ntime * Fa):
 *   dbg_f32: [spec_resid (Fa)][background, FT layout (Fa x ntime)][residual, TF layout (ntime x Fa)]
 *   dbg_u8 : [spec_flags (Fa)][time_flags TF (N)][freq_flags TF (N)]
 */
int tri_sum_threshold_flagger_debug(const void *vis, int vis_dtype,
                                    const uint8_t *flags, uint8_t *out_flags,
                                    int64_t n_cp, int64_t ntime, int64_t nchan,
                                    const tri_params *p,
                                    void *workspace, size_t workspace_bytes,
                                    void *stream, float *dbg_f32, uint8_t *dbg_u8);

/*
 * Test hook: tri_uvcontsub_flagger (same arguments, launches and flags) that additionally taps the LAST major
 * cycle's intermediates of ALL n_cp products into caller-provided device buffers, indexed by the global product
 * number also when the call runs in several workspace batches.  Any buffer may be NULL; with major_cycles == 0
 * they are left untouched.
 *   dbg_avg    (n_cp, nchan) complex64         time-mean spectrum (k_uv_mean)
 *   dbg_smooth (n_cp, nchan) complex64         its low-passed form (k_uv_lowpass)
 *   dbg_absres (n_cp, ntime, nchan) float32    |vis - smooth|
 *   dbg_mflags (n_cp, ntime, nchan) uint8      samples the MAD ignores: flagged at the cycle's start, or NaN residual
 *   dbg_med    (n_cp, 2) float64               median of the residual and median of | residual - median | (NaN: nothing to take it of)
 *   dbg_cnt    (n_cp) uint32                   flagged samples at the cycle's start
 * No reference counterpart.
 */
int tri_uvcontsub_flagger_debug(const void *vis_c64, const uint8_t *flags, uint8_t *out_flags,
                                int64_t n_cp, int64_t ntime, int64_t nchan,
                                int64_t major_cycles, int64_t or_original_from_cycle,
                                int64_t taylor_degrees, double sigma,
                                void *workspace, size_t workspace_bytes, void *stream,
                                void *dbg_avg, void *dbg_smooth, float *dbg_absres,
                                uint8_t *dbg_mflags, double *dbg_med, uint32_t *dbg_cnt);

/*
 * Measurement / test hook: ONE rejection step of the background loop,
 *     flags |= resid > median_abs(resid[~flags]) * 1.4826 * reject     per (window, chunk) block
 * (flagging.py:553-574 with _median_abs :267), by the one-pass route the flagger
 * takes for blocks of at least 65536 samples (k_mr_predict / k_mr_pass /
 * k_mr_finish + the redo kernel; TRI_EUNSUPPORTED for smaller blocks).
 * resid (n_win, n_chan, n_time) float32 and flags_in (same shape, bytes) are the
 * channel-major images of the loop; flags_out (same shape) receives the new
 * flags, flags_t4 (n_win, n_time / 4, n_chan, 4) the same flags with four
 * consecutive times of a channel per 32-bit word (the time-axis filter's input),
 * med (n_win, n_chunk_ends - 1) float64 the block medians (NaN: nothing
 * unflagged).  chunk_ends is a HOST array of channel boundaries, 0 ... n_chan.
 * ms_per_step: mean time of the whole step over `repeats`, HIP events on `stream`.
 */
int tri_bench_reject(const float *resid, const uint8_t *flags_in, uint8_t *flags_out,
                     uint8_t *flags_t4, double *med, int64_t n_win, int64_t n_chan,
                     int64_t n_time, const int64_t *chunk_ends, int64_t n_chunk_ends,
                     double reject, int repeats, float *ms_per_step, void *stream);

/*
 * Test hook: exact segmented medians of |x| over the unflagged samples of a
 * (n_win, rows, row_len) float32 array; segments [seg_ends[g], seg_ends[g+1])
 * (HOST array) along each row; med is (n_win, rows, n_seg_ends - 1) float64,
 * NaN where a segment has no unflagged sample.  variant 0 = automatic,
 * 1 = wave kernel (4: its 16-byte-load form over masked groups), 2 / 3 = three-pass workgroup kernel with scalar / vector loads,
 * 5 / 6 = two-pass workgroup kernel with vector / scalar loads, 7 = two-pass
 * kernel, vector loads over segments that need not be 4-aligned (row_len % 4 == 0),
 * 8 = multi-workgroup two-pass select (one segment spanning the row),
 * 9 / 10 = the two-pass select with the predicted-bin candidate window in
 * global scratch (one read of the segment when the prediction holds;
 * 9 vector loads, 10 scalar).  1 / 4 run the wave kernels with several rows of a
 * segment per wave (the flagger's launch shape), 11 / 14 with one segment per
 * wave (TRI_MEDIAN_WAVE_OLD=1 in the flagger).
 * Restates _median_abs / _median_abs_axis0 (flagging.py:267-304).
 */
int tri_test_median(const float *data, const uint8_t *flags, double *med,
                    int64_t n_win, int64_t rows, int64_t row_len,
                    const int64_t *seg_ends, int64_t n_seg_ends, int variant,
                    void *stream);

/*
 * Test hook: the register-ring box-filter kernels divide by the launch constant
 * float32(2 r + 1) ** 4 (flagging.py:419) through its reciprocal with exact
 * remainder corrections.  Runs that division on ALL 2^32 float32 bit patterns
 * for one radius and counts the inputs whose result differs from the correctly
 * rounded IEEE quotient (NaN results compare equal); must be 0.
 */
int tri_test_box_divide(int64_t radius, uint64_t *mismatches, void *stream);

/* Device amplitude of complex64 samples, the |z| used at flagging.py:856
 * (libm hypotf semantics); exposed so the tests can pin it (golden G0). */
int tri_abs_c64(const void *z_c64, float *out, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRICOLOUR_AMD_H */
