#!/usr/bin/env python3
"""Generates the seeded random fixtures tests/golden/GR*_random_sumthreshold.npz and
GR_random_uvcontsub.npz by running the reference UN-JITTED (refshim.py), under the harness
rules of make_golden.py's docstring: every float kwarg wrapped in np.float64 (D3), float32
amplitudes as input (D6; the complex64 cases have one zero component per sample, whose
magnitude is exact under any hypot).  Build-container only; only the .npz files travel.

Run:  cd tests/golden && PYTHONDONTWRITEBYTECODE=1 python3 make_golden_random.py [--workers N]

The kwarg space is the one tests/test_gpu_parity.py::_random_case draws from (the value sets
are restated below; the test module is not imported), with the shapes capped so that the
un-jitted reference stays affordable.  A case is a pure function of its seed (`make_case`,
`make_uv_case`): running the script again regenerates byte-identical inputs.

Selection (reference and kwargs only -- never the oracle or the product):
  1. seeds COVER_BASE, COVER_BASE + 1, ... are walked in order; a seed is picked while it
     serves a coverage condition of COVERAGE that fewer than two picks serve so far (whether
     the reference will refuse it is predicted from shape and kwargs, and verified by the
     run); seeds whose window lists the reference refuses are picked until each of the two
     refusal kinds has REJECTED_PER_KIND cases;
  2. seeds FILL_BASE, ... fill the accepted set up to N_ACCEPTED plain random draws;
  3. the reference runs on every pick; a case is a D-site case (`d_site`) if the run touched
     D1 (a box filter of width d = 2 r + 1 whose float32 powf value float32(d) ** passes
     differs from float32 square-and-multiply) or D2 (_linearly_interpolate_nans1d called
     with a NaN in its input);
  4. while more than a third of the accepted cases are D-site cases, further seeds are run
     and those that are accepted and no D-site case are appended;
  5. the coverage conditions and the cap are asserted, then the files are written.
"""
import argparse
import io
import json
import multiprocessing
import os
import sys
import time
import warnings

import numpy as np

from make_golden import run_reference
from refshim import load_reference_flagging

# ---- the value sets of _random_case(), shapes capped (n_bl * n_corr <= 2, T * F <= 6000) ----
T_SET = [1, 2, 5, 16, 31, 48, 64, 100]
F_SET = [1, 3, 16, 33, 64, 97, 128, 200]
CP_SHAPES = [(1, 1), (1, 2), (2, 1)]
MAX_SAMPLES = 6000
AVERAGE_FREQ = [1, 1, 1, 2, 3]
OUTLIER_NSIGMA = [3.0, 4.5, 10.0]
WINDOWS_TIME = [[1, 2, 4, 8], [1, 2, 4, 8], [1, 3], [2, 8, 16]]
WINDOWS_FREQ = [[1, 2, 4, 8], [1, 2, 4, 8], [1, 5, 9], [4]]
BACKGROUND_REJECT = [2.0, 3.5]
BACKGROUND_ITERATIONS = [0, 1, 1, 2, 3]
SPIKE_WIDTH_TIME = [0.3, 3.0, 6.5, 12.5, 20.0, 40.0]
SPIKE_WIDTH_FREQ = [0.3, 2.0, 10.0, 18.0, 30.0]
EXTEND = [0, 1, 2, 3, 4]
FREQ_CHUNKS = [1, 2, 5, 10]
FLAG_ALL_TIME_FRAC = [0.3, 0.6, 1.0]
FLAG_ALL_FREQ_FRAC = [0.4, 0.8, 1.0]
RHO = [1.3, 1.5]
NUM_MAJOR_ITERATIONS = [1, 2, 3]
CHANNEL_SCALE = [4.0, 9.0, 30.0]
TIME_OFFSET = [3.0, 7.0]
FLAG_DENSITY = [0.0, 0.02, 0.3]
P_COMPLEX = 0.2

COVER_BASE, FILL_BASE, EXTRA_BASE = 100000, 200000, 300000
N_ACCEPTED = 56
N_COMPLEX = 8
REJECTED_PER_KIND = 3
MAX_FILE_BYTES = 900 * 1000
INTERMEDIATES = ("spec_resid", "spec_flags", "background", "residual", "time_flags", "freq_flags")


def make_case(seed):
    """(vis, flags, kw, meta) of one SumThreshold case; a pure function of the seed."""
    rs = np.random.RandomState(seed)
    while True:
        T, F = int(rs.choice(T_SET)), int(rs.choice(F_SET))
        if T * F <= MAX_SAMPLES:
            break
    n_bl, n_corr = CP_SHAPES[int(rs.randint(0, len(CP_SHAPES)))]
    shape = (n_bl, n_corr, T, F)
    kw = dict(
        outlier_nsigma=float(rs.choice(OUTLIER_NSIGMA)),
        windows_time=WINDOWS_TIME[int(rs.randint(0, 4))],
        windows_freq=WINDOWS_FREQ[int(rs.randint(0, 4))],
        background_reject=float(rs.choice(BACKGROUND_REJECT)),
        background_iterations=int(rs.choice(BACKGROUND_ITERATIONS)),
        spike_width_time=float(rs.choice(SPIKE_WIDTH_TIME)),
        spike_width_freq=float(rs.choice(SPIKE_WIDTH_FREQ)),
        time_extend=int(rs.choice(EXTEND)), freq_extend=int(rs.choice(EXTEND)),
        freq_chunks=int(rs.choice(FREQ_CHUNKS)), average_freq=int(rs.choice(AVERAGE_FREQ)),
        flag_all_time_frac=float(rs.choice(FLAG_ALL_TIME_FRAC)),
        flag_all_freq_frac=float(rs.choice(FLAG_ALL_FREQ_FRAC)),
        rho=float(rs.choice(RHO)), num_major_iterations=int(rs.choice(NUM_MAJOR_ITERATIONS)))
    z = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    deco = dict(scaled_channel=False, offset_timestep=False, zeros=False, flagged_third=False)
    if rs.uniform() < 0.7 and F > 4:
        z[..., int(rs.randint(0, F))] *= rs.choice(CHANNEL_SCALE)
        deco["scaled_channel"] = True
    if rs.uniform() < 0.7 and T > 4:
        z[:, :, int(rs.randint(0, T)), :] += rs.choice(TIME_OFFSET)
        deco["offset_timestep"] = True
    if rs.uniform() < 0.3:
        z[rs.uniform(size=shape) < 0.01] = np.nan
    if rs.uniform() < 0.3:
        z[rs.uniform(size=shape) < 0.01] = 0
        deco["zeros"] = True
    density = float(rs.choice(FLAG_DENSITY))
    flags = rs.uniform(size=shape) < density
    if rs.uniform() < 0.2:
        flags[:, :, :, : max(1, F // 3)] = True
        deco["flagged_third"] = True
    re, im = z.real.astype(np.float64), z.imag.astype(np.float64)
    amp = np.sqrt(re * re + im * im).astype(np.float32)
    is_complex = bool(rs.uniform() < P_COMPLEX)
    if is_complex:
        # one component exactly zero per sample; NaN and infinite components ride along
        pick = rs.uniform(size=shape) < 0.5
        sign = np.where(rs.uniform(size=shape) < 0.5, -1.0, 1.0).astype(np.float32)
        vis = np.empty(shape, np.complex64)
        vis.real = np.where(pick, amp * sign, np.float32(0))
        vis.imag = np.where(pick, np.float32(0), amp * sign)
        flat_v, flat_f = vis.reshape(-1), flags.reshape(-1)
        spots = rs.choice(flat_v.size, size=min(4, flat_v.size), replace=False)
        special = [complex(np.nan, 1.0), complex(1.0, np.nan), complex(np.nan, np.nan), complex(np.inf, np.nan)]
        for k, at in enumerate(spots):
            flat_v[at] = special[k]
            if k == 3:
                flat_f[at] = True     # |inf + nan j| is inf, not NaN: kept under a flag (unflagged infinities are out of contract)
    else:
        vis = amp
    meta = dict(seed=int(seed), shape=[int(s) for s in shape], dtype=str(vis.dtype), kw=kw, flag_density=density,
                nans=bool(np.isnan(vis).any()), **deco)
    return vis, flags, kw, meta


def prepared_windows(meta):
    """The window lists after the reference's preparation (shape and kwargs only; what the run does with them is
    recorded from the run): time windows clipped to T; frequency windows divided by average_freq, truncated,
    made unique, clipped to the averaged channel count."""
    kw = meta["kw"]
    T, F = meta["shape"][2:]
    avg = kw["average_freq"]
    fa = (F + avg - 1) // avg
    wt = [w for w in kw["windows_time"] if w <= T]
    wf = sorted(set(int(np.float32(w) / np.float32(avg)) for w in kw["windows_freq"]))
    wf = [w for w in wf if w <= fa]
    return wt, wf


def predicted_refusal(meta):
    wt, wf = prepared_windows(meta)
    if not wt or not wf:
        return "no_window_fits"
    if 0 in wf:
        return "window_averaged_to_zero"
    return None


def _count_conditions():
    c = {
        "background_iterations=0": lambda m: m["kw"]["background_iterations"] == 0,
        "freq_chunks=1": lambda m: m["kw"]["freq_chunks"] == 1,
        "radius0_axis": lambda m: m["kw"]["spike_width_time"] == 0.3 or m["kw"]["spike_width_freq"] == 0.3,
    }
    for w in ([1, 2, 4, 8], [1, 3], [2, 8, 16]):
        c["windows_time=%s" % w] = lambda m, w=w: m["kw"]["windows_time"] == w
    for w in ([1, 2, 4, 8], [1, 5, 9], [4]):
        c["windows_freq=%s" % w] = lambda m, w=w: m["kw"]["windows_freq"] == w
    for t in (1, 2, 5):
        c["T=%d" % t] = lambda m, t=t: m["shape"][2] == t
    for f in (1, 3):
        c["F=%d" % f] = lambda m, f=f: m["shape"][3] == f
    for a in (2, 3):
        c["average_freq=%d+nans" % a] = lambda m, a=a: m["kw"]["average_freq"] == a and m["nans"]
        c["average_freq=%d+flagged_third" % a] = lambda m, a=a: m["kw"]["average_freq"] == a and m["flagged_third"]
    for key, values in (("background_reject", BACKGROUND_REJECT), ("rho", RHO), ("flag_all_time_frac", FLAG_ALL_TIME_FRAC),
                        ("flag_all_freq_frac", FLAG_ALL_FREQ_FRAC), ("time_extend", EXTEND), ("freq_extend", EXTEND)):
        for v in values:
            c["%s=%s" % (key, v)] = lambda m, key=key, v=v: m["kw"][key] == v
    return c


COVERAGE = _count_conditions()          # each: at least two accepted cases
COMPLEX_ONE_ZERO = lambda m: m["dtype"] == "complex64"      # noqa: E731   at least N_COMPLEX accepted cases


def coverage_report(metas):
    """{condition: count} over accepted cases, and the list of unmet conditions."""
    acc = [m for m in metas if m["accepted"]]
    counts = {name: sum(1 for m in acc if cond(m)) for name, cond in COVERAGE.items()}
    counts["complex64"] = sum(1 for m in acc if COMPLEX_ONE_ZERO(m))
    unmet = [n for n, k in counts.items() if k < (N_COMPLEX if n == "complex64" else 2)]
    return counts, unmet


def pick_seeds():
    counts = {name: 0 for name in COVERAGE}
    n_complex = 0
    refused = {"no_window_fits": [], "window_averaged_to_zero": []}
    picks = []
    seed = COVER_BASE
    while (min(counts.values()) < 2 or n_complex < N_COMPLEX
           or min(len(v) for v in refused.values()) < REJECTED_PER_KIND):
        meta = make_case(seed)[3]
        why = predicted_refusal(meta)
        if why is not None:
            if len(refused[why]) < REJECTED_PER_KIND:
                refused[why].append(seed)
        else:
            serves = [n for n, cond in COVERAGE.items() if counts[n] < 2 and cond(meta)]
            if serves or (n_complex < N_COMPLEX and COMPLEX_ONE_ZERO(meta)):
                picks.append(seed)
                for n, cond in COVERAGE.items():
                    counts[n] += bool(cond(meta))
                n_complex += bool(COMPLEX_ONE_ZERO(meta))
        seed += 1
        assert seed < COVER_BASE + 50000, "coverage walk does not end"
    seed = FILL_BASE
    while len(picks) < N_ACCEPTED:
        if predicted_refusal(make_case(seed)[3]) is None:
            picks.append(seed)
        seed += 1
    return picks, sorted(refused["no_window_fits"] + refused["window_averaged_to_zero"])


# ---- the reference run (worker processes) -------------------------------------------------------------------

_FL = None


def is_d1(r, passes):
    d = np.float32(2 * r + 1)
    powf = d ** passes                  # float32 scalar ** int: NumPy's float32 power, as flagging.py:419 evaluates un-jitted
    res, a, e = np.float32(1), d, int(passes)
    with np.errstate(over="ignore"):
        while e:
            if e & 1:
                res = np.float32(res * a)
            e >>= 1
            a = np.float32(a * a)
    return bool(powf != res)


def run_case(seed):
    global _FL
    if _FL is None:
        _FL = load_reference_flagging()
    fl = _FL
    vis, flags, kw, meta = make_case(seed)
    radii, interp_nan = set(), [False]
    orig_box, orig_interp = fl._box_gaussian_filter1d, fl._linearly_interpolate_nans1d

    def rec_box(data, r, out, passes):
        radii.add((int(r), int(passes)))
        return orig_box(data, r, out, passes)

    def rec_interp(data):
        if np.isnan(data).any():
            interp_nan[0] = True
        return orig_interp(data)

    fl._box_gaussian_filter1d, fl._linearly_interpolate_nans1d = rec_box, rec_interp
    t0 = time.time()
    out = inter = exc = None
    try:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            try:
                out, inter = run_reference(fl, vis.copy(), flags.copy(), **kw)
            except Exception:
                # the flagger itself refused the input, or run_reference's indexing of the recorded calls did not hold
                try:
                    kw64 = {k: (np.float64(v) if isinstance(v, float) else v) for k, v in kw.items()}
                    out = fl.sum_threshold_flagger(vis.copy(), flags.copy(), **kw64)
                except Exception as e:
                    exc = type(e).__name__
    finally:
        fl._box_gaussian_filter1d, fl._linearly_interpolate_nans1d = orig_box, orig_interp
    meta["seconds"] = time.time() - t0
    meta["accepted"] = exc is None
    arrays = dict(vis=vis, flags=flags)
    if exc is not None:
        meta["exception"] = exc
        meta["refusal"] = predicted_refusal(meta)
        return meta, arrays
    T, F = meta["shape"][2:]
    fa = (F + kw["average_freq"] - 1) // kw["average_freq"]
    if inter is not None:
        ok = (inter["spec_resid"].size == fa and inter["spec_flags"].size == fa
              and all(inter[k].shape == (T, fa) for k in ("background", "residual", "time_flags", "freq_flags")))
        if not ok:
            inter = None
    meta["intermediates"] = inter is not None
    meta["radii"] = sorted(set(r for r, _ in radii))
    meta["passes"] = sorted(set(p for _, p in radii))
    meta["d1"] = any(is_d1(r, p) for r, p in radii)
    meta["d2"] = bool(interp_nan[0])
    meta["d_site"] = meta["d1"] or meta["d2"]
    arrays["out"] = np.asarray(out, np.bool_)
    if inter is not None:
        for k in INTERMEDIATES:
            arrays["i_" + k] = np.ascontiguousarray(inter[k])
    return meta, arrays


def run_all(pool, seeds, done):
    for meta, arrays in pool.imap(run_case, seeds):
        if meta["accepted"]:
            print("seed %d shape %s %s: %.1f s, d_site %s (D1 %s, D2 %s, radii %s), flagged %d/%d%s" % (
                meta["seed"], meta["shape"], meta["dtype"], meta["seconds"], meta["d_site"], meta["d1"], meta["d2"],
                meta["radii"], arrays["out"].sum(), arrays["out"].size, "" if meta["intermediates"] else ", flags only"))
        else:
            print("seed %d shape %s: refused with %s (%s), %.1f s" % (meta["seed"], meta["shape"], meta["exception"],
                                                                      meta["refusal"], meta["seconds"]))
        sys.stdout.flush()
        done.append((meta, arrays))


def _npz_bytes(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getbuffer().nbytes


def write_sumthreshold_files(done):
    """Cases in pick order, packed into GR<k>_random_sumthreshold.npz of less than MAX_FILE_BYTES each."""
    for name in os.listdir("."):
        if name.startswith("GR") and name.endswith("_random_sumthreshold.npz"):
            os.remove(name)
    files, cur, cur_meta, cur_bytes = [], {}, [], 0

    def flush():
        if cur_meta:
            name = "GR%d_random_sumthreshold.npz" % (len(files) + 1)
            np.savez_compressed(name, cases=np.asarray(json.dumps(cur_meta)), **cur)
            assert os.path.getsize(name) < 1000 * 1000, name
            files.append(name)
            print("%s: %d cases, %d bytes" % (name, len(cur_meta), os.path.getsize(name)))

    for idx, (meta, arrays) in enumerate(done):
        meta = dict(meta, id="c%03d" % idx)
        meta.pop("seconds")
        named = {"%s_%s" % (meta["id"], k): v for k, v in arrays.items()}
        size = _npz_bytes(named)
        if cur_meta and cur_bytes + size > MAX_FILE_BYTES:
            flush()
            cur, cur_meta, cur_bytes = {}, [], 0
        cur.update(named)
        cur_meta.append(meta)
        cur_bytes += size
    flush()
    return files


# ---- uvcontsub ------------------------------------------------------------------------------------------------

UV_KWARGS = [dict(major_cycles=7, or_original_from_cycle=1, taylor_degrees=20, sigma=15.0),    # residual_flag_initial
             dict(major_cycles=10, or_original_from_cycle=0, taylor_degrees=25, sigma=13.0),   # residual_flag_final
             dict(major_cycles=3, or_original_from_cycle=0, taylor_degrees=25, sigma=5.0),
             dict(major_cycles=4, or_original_from_cycle=1, taylor_degrees=20, sigma=6.0)]
# (n_bl <= 3, n_corr <= 2, T in {8, 33, 64}, F in {64, 130, 257}): every (T, F) pair once, the large ones with few products
UV_SHAPES = [(3, 2, 8, 64), (2, 2, 8, 130), (2, 1, 8, 257), (3, 1, 33, 64), (1, 2, 33, 130), (1, 1, 33, 257), (2, 1, 64, 64),
             (1, 2, 64, 130), (1, 1, 64, 257), (3, 2, 8, 130), (1, 2, 8, 257), (2, 2, 33, 64), (1, 1, 8, 64), (2, 1, 8, 64)]
UV_FEATURES = ("unflagged_inf", "unflagged_nan", "flagged_channel", "flagged_timestep", "flagged_product")
UV_SEED_BASE = 500000


def make_uv_case(idx):
    """(vis, flags, kw, meta) of uvcontsub case `idx`: smooth band + noise + lines, as tests/test_uvcontsub.py builds them."""
    rs = np.random.RandomState(UV_SEED_BASE + idx)
    shape = UV_SHAPES[idx]
    n_bl, n_corr, T, F = shape
    kw = dict(UV_KWARGS[idx % len(UV_KWARGS)])
    x = np.linspace(0, 1, F)
    band = 2 + np.cos(7 * x) + 0.5 * np.sin(23 * x)
    vis = (band[None, None, None, :] + 0.3 * rs.standard_normal(shape)
           + 1j * (0.2 * x[None, None, None, :] + 0.3 * rs.standard_normal(shape))).astype(np.complex64)
    vis[..., F // 5] += 5                                   # a strong line
    vis[..., (3 * F) // 5: (3 * F) // 5 + 4] += 1.0         # a faint one: near the threshold in later cycles
    vis[n_bl - 1, 0, T // 3] += 3                           # a bad timestep
    flags = rs.uniform(size=shape) < 0.02
    feats = [f for k, f in enumerate(UV_FEATURES) if (idx + k) % 3 != 2]
    if n_bl * n_corr == 1 and "flagged_product" in feats:
        feats.remove("flagged_product")
    if "flagged_channel" in feats:
        flags[..., F // 2] = True
    if "flagged_timestep" in feats:
        flags[:, :, T // 2, :] = True
    if "unflagged_inf" in feats:
        at = (0, 0, 1, F // 4)
        vis[at] = [complex(np.inf, 0.0), complex(1.0, -np.inf), complex(np.inf, np.inf)][idx % 3]
        flags[at] = False
    if "unflagged_nan" in feats:
        for at, v in (((0, 0, 2, F // 3), complex(np.nan, 1.0)), ((0, 0, T - 1, 3), complex(np.nan, np.nan))):
            vis[at] = v
            flags[at] = False
    if "flagged_product" in feats:
        flags[n_bl - 1, n_corr - 1] = True
    meta = dict(id="u%02d" % idx, seed=UV_SEED_BASE + idx, shape=list(shape), kw=kw, features=feats)
    return vis, flags, kw, meta


def write_uvcontsub_file(fl):
    arrays, metas = {}, []
    for idx in range(len(UV_SHAPES)):
        vis, flags, kw, meta = make_uv_case(idx)
        t0 = time.time()
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            out = fl.uvcontsub_flagger(vis.copy(), flags.copy(), **kw)
        print("%s shape %s %s %s: %.2f s, flagged %d/%d" % (meta["id"], meta["shape"], kw, meta["features"], time.time() - t0,
                                                            out.sum(), out.size))
        for k, v in (("vis", vis), ("flags", flags), ("out", out)):
            arrays["%s_%s" % (meta["id"], k)] = v
        metas.append(meta)
    for f in UV_FEATURES:
        assert sum(1 for m in metas if f in m["features"]) >= 2, f
    assert {m["kw"]["or_original_from_cycle"] for m in metas} == {0, 1}
    assert len(metas) >= 12
    name = "GR_random_uvcontsub.npz"
    np.savez_compressed(name, cases=np.asarray(json.dumps(metas)), numpy_version=np.asarray(np.__version__), **arrays)
    assert os.path.getsize(name) < 1000 * 1000, name
    print("%s: %d cases, %d bytes" % (name, len(metas), os.path.getsize(name)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    assert 1 <= args.workers <= 16
    os.chdir(os.path.dirname(os.path.abspath(__file__)))      # the fixtures live next to this script
    t_start = time.time()
    picks, refused = pick_seeds()
    print("%d picks (coverage walk + fill), %d predicted refusals" % (len(picks), len(refused)))
    done = []
    with multiprocessing.get_context("fork").Pool(args.workers) as pool:
        run_all(pool, picks + refused, done)
        for seed in picks:
            assert [m for m, _ in done if m["seed"] == seed][0]["accepted"], "seed %d was predicted to be accepted" % seed
        for seed in refused:
            assert not [m for m, _ in done if m["seed"] == seed][0]["accepted"], "seed %d was predicted to be refused" % seed
        seed = EXTRA_BASE
        while True:
            acc = [m for m, _ in done if m["accepted"]]
            n_d = sum(1 for m in acc if m["d_site"])
            if 3 * n_d <= len(acc):
                break
            batch = []
            while len(batch) < args.workers:
                if predicted_refusal(make_case(seed)[3]) is None:
                    batch.append(seed)
                seed += 1
            more = []
            run_all(pool, batch, more)
            done.extend(x for x in more if x[0]["accepted"] and not x[0]["d_site"])
            assert seed < EXTRA_BASE + 2000, "the D-site cap cannot be met"
    metas = [m for m, _ in done]
    acc = [m for m in metas if m["accepted"]]
    rej = [m for m in metas if not m["accepted"]]
    counts, unmet = coverage_report(metas)
    assert not unmet, "coverage conditions not met: %s" % unmet
    assert len(acc) >= 48 and len(rej) >= 4
    assert {m["refusal"] for m in rej} == {"no_window_fits", "window_averaged_to_zero"}
    n_d = sum(1 for m in acc if m["d_site"])
    assert 3 * n_d <= len(acc)
    done.sort(key=lambda x: not x[0]["accepted"])        # accepted cases first, each group in pick order
    write_sumthreshold_files(done)
    write_uvcontsub_file(load_reference_flagging())
    print("accepted %d (D-site %d: D1 %d, D2 %d; flags only %d), refused %d, reference time %.0f s, wall %.0f s" % (
        len(acc), n_d, sum(m["d1"] for m in acc), sum(m["d2"] for m in acc), sum(not m["intermediates"] for m in acc),
        len(rej), sum(m["seconds"] for m in metas), time.time() - t_start))
    print("coverage:", json.dumps(counts, sort_keys=True))


if __name__ == "__main__":
    main()
