"""Pins the oracle -- and through it the HIP path -- to the reference across the kwarg space the GPU sweep
(test_gpu_parity.py::_random_case) draws from.  tests/golden/make_golden_random.py ran the un-jitted reference on seeded
random cases from that space (shapes capped so that the un-jitted run stays affordable) and on uvcontsub blocks with
unflagged non-finite samples and fully flagged channels / timesteps / products; only the .npz files are read here.

CPU: the oracle in (POW_POWF, INTERP_F32) mode -- the arithmetic of un-jitted NumPy 2 -- reproduces every case bit for bit,
flags and float32 intermediates; in its canonical (numba) mode it reproduces the flags of every case whose reference run
touched neither D1 nor D2 (`d_site` false, classified from the reference run alone); inputs the reference refuses raise
ValueError; the index of the fixtures still covers what it was generated to cover.
GPU: the product equals the canonical oracle on every case and the reference's own output wherever `d_site` is false."""
import functools
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

ST_FILES = ["GR1_random_sumthreshold.npz", "GR2_random_sumthreshold.npz"]
UV_FILE = "GR_random_uvcontsub.npz"
INTERMEDIATES_F32 = ("spec_resid", "background", "residual")
INTERMEDIATES_FLAGS = ("spec_flags", "time_flags", "freq_flags")


def _index(name):
    with np.load(os.path.join(GOLDEN, name)) as d:
        return json.loads(str(d["cases"]))


ST_INDEX = {m["id"]: dict(m, file=name) for name in ST_FILES for m in _index(name)}
UV_INDEX = {m["id"]: m for m in _index(UV_FILE)}
ACCEPTED = sorted(i for i, m in ST_INDEX.items() if m["accepted"])
REFUSED = sorted(i for i, m in ST_INDEX.items() if not m["accepted"])


@functools.lru_cache(maxsize=None)
def _file(name):
    with np.load(os.path.join(GOLDEN, name)) as d:
        return {k: d[k] for k in d.files}


def _st_case(cid):
    m = ST_INDEX[cid]
    d = _file(m["file"])
    arrays = {k[len(cid) + 1:]: v for k, v in d.items() if k.startswith(cid + "_")}
    for v in arrays.values():
        v.setflags(write=False)          # shared between the tests: left unchanged
    return m, arrays


def _uv_case(cid):
    d = _file(UV_FILE)
    arrays = {k[len(cid) + 1:]: v for k, v in d.items() if k.startswith(cid + "_")}
    for v in arrays.values():
        v.setflags(write=False)
    return UV_INDEX[cid], arrays, str(d["numpy_version"])


def _same_f32(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32).reshape(a.shape)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@functools.lru_cache(maxsize=None)
def _canonical(cid):
    """The oracle's flags in its canonical (numba) mode: computed once per case, shared by the CPU and GPU tests."""
    from oracle import oracle
    oracle.set_modes(oracle.POW_SQMUL, oracle.INTERP_F64)
    m, a = _st_case(cid)
    out = oracle.sum_threshold_flagger(a["vis"], a["flags"], **m["kw"])
    out.setflags(write=False)
    return out


# ---- the index still covers what it was generated to cover -------------------------------------------------------

def _coverage_problems(index):
    """Every condition the generator asserts before it writes, re-evaluated on an index of cases."""
    acc = [m for m in index if m["accepted"]]
    rej = [m for m in index if not m["accepted"]]
    kw = lambda key, v: (lambda m: m["kw"][key] == v)                 # noqa: E731
    twice = {
        "background_iterations=0": kw("background_iterations", 0),
        "freq_chunks=1": kw("freq_chunks", 1),
        "radius-0 axis": lambda m: 0.3 in (m["kw"]["spike_width_time"], m["kw"]["spike_width_freq"]),
    }
    for w in ([1, 2, 4, 8], [1, 3], [2, 8, 16]):
        twice["windows_time=%s" % w] = kw("windows_time", w)
    for w in ([1, 2, 4, 8], [1, 5, 9], [4]):
        twice["windows_freq=%s" % w] = kw("windows_freq", w)
    for t in (1, 2, 5):
        twice["T=%d" % t] = lambda m, t=t: m["shape"][2] == t
    for f in (1, 3):
        twice["F=%d" % f] = lambda m, f=f: m["shape"][3] == f
    for a in (2, 3):
        twice["average_freq=%d with NaNs" % a] = lambda m, a=a: m["kw"]["average_freq"] == a and m["nans"]
        twice["average_freq=%d with the flagged third" % a] = lambda m, a=a: m["kw"]["average_freq"] == a and m["flagged_third"]
    for key, values in (("background_reject", (2.0, 3.5)), ("rho", (1.3, 1.5)), ("flag_all_time_frac", (0.3, 0.6, 1.0)),
                        ("flag_all_freq_frac", (0.4, 0.8, 1.0)), ("time_extend", range(5)), ("freq_extend", range(5))):
        for v in values:
            twice["%s=%s" % (key, v)] = kw(key, v)
    problems = ["%s: %d accepted cases" % (name, sum(1 for m in acc if cond(m)))
                for name, cond in twice.items() if sum(1 for m in acc if cond(m)) < 2]
    if len(acc) < 48:
        problems.append("%d accepted cases" % len(acc))
    if len(rej) < 4:
        problems.append("%d refused cases" % len(rej))
    if {m["refusal"] for m in rej} != {"no_window_fits", "window_averaged_to_zero"}:
        problems.append("refusal kinds %s" % sorted({m["refusal"] for m in rej}))
    if sum(1 for m in acc if m["dtype"] == "complex64") < 8:
        problems.append("fewer than 8 complex64 cases")
    if 3 * sum(1 for m in acc if m["d_site"]) > len(acc):
        problems.append("more than a third of the accepted cases are D-site cases")
    for m in acc:
        n_bl, n_corr, T, F = m["shape"]
        if n_bl * n_corr > 2 or T * F > 6000:
            problems.append("%s: shape %s beyond the caps" % (m["id"], m["shape"]))
    return problems


def test_index_covers_the_sweep_space():
    assert _coverage_problems(list(ST_INDEX.values())) == []


@pytest.mark.parametrize("drop", [lambda m: m["kw"]["background_iterations"] == 0, lambda m: m["shape"][2] == 1,
                                  lambda m: m["kw"]["average_freq"] == 3, lambda m: not m["accepted"],
                                  lambda m: m["accepted"] and not m["d_site"] and m["shape"][2] > 5 and m["shape"][3] > 3])
def test_coverage_check_notices_a_thinner_index(drop):
    assert _coverage_problems([m for m in ST_INDEX.values() if not drop(m)])


def test_uvcontsub_index_covers_the_edges():
    metas = list(UV_INDEX.values())
    assert len(metas) >= 12
    for feature in ("unflagged_inf", "unflagged_nan", "flagged_channel", "flagged_timestep", "flagged_product"):
        assert sum(1 for m in metas if feature in m["features"]) >= 2, feature
    assert {m["kw"]["or_original_from_cycle"] for m in metas} == {0, 1}
    for shipped in (dict(major_cycles=7, or_original_from_cycle=1, taylor_degrees=20, sigma=15.0),
                    dict(major_cycles=10, or_original_from_cycle=0, taylor_degrees=25, sigma=13.0)):
        assert any(m["kw"] == shipped for m in metas)
    for m in metas:
        _, a, _ = _uv_case(m["id"])
        vis, flags = a["vis"], a["flags"]
        n_bl, n_corr, T, F = vis.shape
        assert n_bl <= 3 and n_corr <= 2 and T in (8, 33, 64) and F in (64, 130, 257)
        have = {"unflagged_inf": (np.isinf(vis.real) | np.isinf(vis.imag)) & ~flags,
                "unflagged_nan": np.isnan(vis) & ~(np.isinf(vis.real) | np.isinf(vis.imag)) & ~flags,
                "flagged_channel": np.broadcast_to(flags.all(axis=2, keepdims=True), flags.shape),
                "flagged_timestep": np.broadcast_to(flags.all(axis=3, keepdims=True), flags.shape),
                "flagged_product": np.broadcast_to(flags.all(axis=(2, 3), keepdims=True), flags.shape)}
        for feature in m["features"]:
            assert have[feature].any(), (m["id"], feature)


def test_inputs_are_what_the_seeds_give():
    """The committed inputs are a pure function of the recorded seeds (the generator's own functions, which need no
    reference to build a case)."""
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden_random as gen
    finally:
        sys.path.remove(GOLDEN)
    for cid, m in ST_INDEX.items():
        vis, flags, kw, meta = gen.make_case(m["seed"])
        _, a = _st_case(cid)
        assert vis.dtype == a["vis"].dtype and vis.tobytes() == a["vis"].tobytes(), cid
        assert np.array_equal(flags, a["flags"]) and kw == m["kw"], cid
        assert all(meta[k] == m[k] for k in meta), cid
        assert (gen.predicted_refusal(meta) is None) == m["accepted"], cid
    for cid, m in UV_INDEX.items():
        vis, flags, kw, meta = gen.make_uv_case(int(cid[1:]))
        _, a, _ = _uv_case(cid)
        assert vis.tobytes() == a["vis"].tobytes() and np.array_equal(flags, a["flags"]) and meta == m, cid


def test_complex_cases_have_one_zero_component():
    n = 0
    for cid in ACCEPTED:
        m, a = _st_case(cid)
        assert a["vis"].dtype == np.dtype(m["dtype"]) and a["vis"].dtype in (np.float32, np.complex64)
        if a["vis"].dtype == np.complex64:
            v = a["vis"]
            odd = np.isnan(v.real) | np.isnan(v.imag) | np.isinf(v.real) | np.isinf(v.imag)
            assert (((v.real == 0) | (v.imag == 0)) | odd).all(), cid
            assert not (np.isinf(np.abs(v)) & ~a["flags"]).any(), cid          # no unflagged infinity
            n += 1
    assert n >= 8


# ---- the oracle against the reference's output --------------------------------------------------------------------

@pytest.mark.parametrize("cid", ACCEPTED)
def test_oracle_equals_reference_bitwise(oracle, cid):
    m, a = _st_case(cid)
    oracle.set_modes(oracle.POW_POWF, oracle.INTERP_F32)
    try:
        out, inter = oracle.sum_threshold_flagger(a["vis"], a["flags"], dump=True, **m["kw"])
    finally:
        oracle.set_modes(oracle.POW_SQMUL, oracle.INTERP_F64)
    bad = int((out != a["out"]).sum())
    assert bad == 0, "%s shape %s kw %s: %d of %d flags differ" % (cid, m["shape"], m["kw"], bad, out.size)
    assert m["intermediates"] == all("i_" + k in a for k in INTERMEDIATES_F32 + INTERMEDIATES_FLAGS)
    if m["intermediates"]:
        for k in INTERMEDIATES_F32:
            assert _same_f32(inter[k], a["i_" + k]).all(), (cid, k)
        for k in INTERMEDIATES_FLAGS:
            assert np.array_equal(inter[k].astype(bool), a["i_" + k].reshape(inter[k].shape)), (cid, k)


@pytest.mark.parametrize("cid", ACCEPTED)
def test_canonical_mode_flags_equal(oracle, cid):
    m, a = _st_case(cid)
    out = _canonical(cid)
    bad = int((out != a["out"]).sum())
    if m["d_site"]:
        print("%s (D1 %s, D2 %s): %d of %d flags differ between the canonical oracle and the un-jitted reference"
              % (cid, m["d1"], m["d2"], bad, out.size))
    else:
        assert bad == 0, "%s shape %s kw %s: %d of %d flags differ" % (cid, m["shape"], m["kw"], bad, out.size)


@pytest.mark.parametrize("cid", REFUSED)
def test_oracle_refuses_what_the_reference_refuses(oracle, cid):
    m, a = _st_case(cid)
    assert m["exception"] == "ValueError"
    with pytest.raises(ValueError):
        oracle.sum_threshold_flagger(a["vis"], a["flags"], **m["kw"])


@pytest.mark.parametrize("cid", sorted(UV_INDEX))
def test_oracle_uvcontsub_equals_reference(oracle, cid):
    m, a, npver = _uv_case(cid)
    if npver.split(".")[0] != np.__version__.split(".")[0]:
        pytest.skip("fixture generated with NumPy %s" % npver)
    got = oracle.uvcontsub_flagger(a["vis"], a["flags"], **m["kw"])
    assert np.array_equal(got, a["out"])
    if "flagged_product" in m["features"]:
        assert got[-1, -1].all()


# ---- the HIP path ------------------------------------------------------------------------------------------------

def _product_both_ways(gpu, vis, flags, kw):
    import torch
    yield "numpy input", gpu.sum_threshold_flagger(vis.copy(), flags.copy(), **kw)
    out = gpu.sum_threshold_flagger(torch.from_numpy(vis.copy()).cuda(), torch.from_numpy(flags.copy()).cuda(), **kw)
    assert out.is_cuda
    yield "device input", out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ACCEPTED)
def test_gpu_equals_oracle_and_reference(gpu, oracle, cid):
    m, a = _st_case(cid)
    exp = _canonical(cid)
    for how, out in _product_both_ways(gpu, a["vis"], a["flags"], m["kw"]):
        bad = int((out != exp).sum())
        assert bad == 0, "%s, %s: %d of %d flags differ from the canonical oracle (shape %s kw %s)" % (
            cid, how, bad, out.size, m["shape"], m["kw"])
        if not m["d_site"]:
            assert np.array_equal(out, a["out"]), "%s, %s: differs from the reference's output" % (cid, how)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", REFUSED)
def test_gpu_refuses_what_the_reference_refuses(gpu, cid):
    import torch
    m, a = _st_case(cid)
    with pytest.raises(ValueError):
        gpu.sum_threshold_flagger(a["vis"].copy(), a["flags"].copy(), **m["kw"])
    with pytest.raises(ValueError):
        gpu.sum_threshold_flagger(torch.from_numpy(a["vis"].copy()).cuda(), torch.from_numpy(a["flags"].copy()).cuda(), **m["kw"])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(UV_INDEX))
def test_gpu_uvcontsub_mismatches_are_borderline(gpu, oracle, cid):
    """Lock step, one major cycle at a time from the fixture's flags (the criterion of
    test_uvcontsub.py::test_gpu_uvcontsub_shipped_kwargs_mismatches_are_borderline): every flag that differs from the
    oracle's sits within 1e-5 (relative) of the threshold sigma * mad; a fully flagged product stays untouched."""
    from tricolour_amd import flagging
    m, a, npver = _uv_case(cid)
    vis, kw, shape = a["vis"].copy(), m["kw"], a["vis"].shape
    cur = a["flags"].copy()
    total_bad = 0
    for mi in range(kw["major_cycles"]):
        one = dict(kw, major_cycles=1, or_original_from_cycle=0 if mi >= kw["or_original_from_cycle"] else 1)
        exp, d = oracle.uvcontsub_flagger(vis, cur, dump=True, **one)
        got = flagging.uvcontsub_flagger(vis, cur, **one)
        assert got.shape == exp.shape and got.dtype == np.bool_
        bad = got != exp
        if bad.any():
            thr = np.broadcast_to(d["thr"].reshape(shape[0], shape[1], 1, 1), shape)
            with np.errstate(all="ignore"):
                rel = np.abs(d["absres"].reshape(shape) - thr)[bad] / thr[bad]
            assert rel.max() < 1e-5, "%s cycle %d: %d flags differ, farthest %.3g of the threshold away" % (
                cid, mi, bad.sum(), rel.max())
        if "flagged_product" in m["features"]:
            assert got[-1, -1].all()
        total_bad += int(bad.sum())
        cur = exp
    print("%s: %d borderline flags over %d lock-step cycles" % (cid, total_bad, kw["major_cycles"]))
    if npver.split(".")[0] == np.__version__.split(".")[0]:
        assert np.array_equal(cur, a["out"])          # the lock-step chain of the oracle is the reference's own run
