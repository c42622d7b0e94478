"""The host-side scaffolding shared by the strategy steps: the window-batch arithmetic and the pointer offsets of
``tricolour_amd.flagging`` and the step table of ``tricolour_amd.strategies``.  The expected batches and messages
below were recorded from the code as it stood before the steps shared this scaffolding (one batch picker per step
family, one if/elif per task), run on these same tables with these same fake workspace sizes."""
import numpy as np
import pytest

from test_sir import sir_windows
from test_sir_masked import sirm_windows

# ---------------------------------------------------------------------------
# _window_batch against the batch pickers it replaced
# ---------------------------------------------------------------------------
BIG = 1 << 60
# (n_win, ntime, nchan, n_ends, max_windows, budget)
LINE_RMS_ROWS = [
    (1, 7, 1, None, None, BIG),
    (64, 100, 1025, None, None, BIG),
    (64, 100, 1025, None, 5, BIG),
    (64, 100, 1025, None, 0, BIG),                        # max_windows 0: no cap
    (64, 100, 1025, None, 100, BIG),                      # max_windows beyond n_win
    (64, 100, 1025, None, None, 100),                     # less than one window's workspace
    (64, 100, 1025, None, None, 256 + 16 * 10 * 1125),    # room for 10 windows: 64 -> 32 -> 16 -> 8
    (7, 10, 10, None, None, 256 + 16 * 2 * 20),           # odd halving: 7 -> 4 -> 2
    (7, 10, 10, None, 6, 256 + 16 * 2 * 20),              # max_windows, then halving: 6 -> 3 -> 2
    (16383, 1024, 1, None, None, BIG),                    # n_win * ntime = 2^24 - 1024: fits one launch
    (16385, 1024, 1, None, None, BIG),                    # n_win * ntime = 2^24 + 1024: capped
    (20000, 1024, 4096, None, None, BIG),
    (10000, 1, 1 << 21, None, None, BIG),                 # ntime + nchan binds (1023), before the power pass's tiles (8191)
    (3, 1 << 24, 1, None, None, BIG),                     # one window's rows overflow a launch: floor of 1
    (40, 1, 1 << 30, None, None, BIG),
    (40, (1 << 30) - 1, 1 << 30, None, None, BIG),        # ntime + nchan = 2^31 - 1
]
LDEV_ROWS = [
    (1, 5, 1, 2, None, BIG),
    (12, 9, 1025, 11, None, BIG),
    (12, 9, 1025, 11, 5, BIG),
    (12, 9, 1025, 11, 0, BIG),
    (12, 9, 1025, 11, None, 10),
    (9, 16, 64, 2, None, 256 + 4 * 3 * (64 + 16)),        # local_deviation's n_ends = 2: 9 -> 5 -> 3
    (9, 16, 64, 2, 4, 256 + 4 * 3 * (64 + 16)),           # 4 -> 2
    (5000, 1 << 20, 1, 2, None, BIG),                     # ntime * strips = 2^20
    (5000, 1 << 20, 1025, 2, None, BIG),                  # two strips; the scalar apply pass binds
    (100, 1 << 20, 1, 33, None, BIG),                     # ntime * (n_ends - 1) = 2^25
    (3, (1 << 31) - 1, 1, 2, None, BIG),                  # ntime * strips = 2^31 - 1: one window per launch
    (3, 1 << 31, 1, 2, None, BIG),                        # beyond a launch: floor of 1
    (3, 1 << 30, 1025, 2, None, BIG),                     # ntime * strips = 2^31
    (3, 1 << 26, 1, 33, None, BIG),                       # ntime * (n_ends - 1) = 2^31
    (70, 1, (1 << 31) - 1, 2, None, BIG),                 # nchan / 32 binds
]
HYST_ROWS = [
    (1, 5, 1, 2, None, BIG),
    (12, 9, 1025, 11, None, BIG),
    (12, 9, 1025, 11, 5, BIG),
    (12, 9, 1025, 11, 0, BIG),
    (12, 9, 1025, 11, None, 10),
    (9, 16, 64, 2, None, 256 + 8 * 3 * (64 + 16) + 2 * 3 * 16 * 64),   # grow_flags' n_ends = 2: 9 -> 5 -> 3
    (9, 16, 64, 2, 4, 256 + 8 * 3 * (64 + 16) + 2 * 3 * 16 * 64),      # 4 -> 2
    (1000, 1 << 20, 1, 33, None, BIG),                    # ntime * (n_ends - 1) = 2^25
    (1000, 1 << 24, 1025, 2, None, BIG),                  # the eligibility pass binds
    (10, (1 << 31) - 1, 1, 2, None, BIG),                 # ntime * (n_ends - 1) = 2^31 - 1
    (10, 1 << 31, 1, 2, None, BIG),
    (10, 1 << 33, 1, 2, None, BIG),                       # (4 lim) // (ntime * (n_ends - 1)) - 1 = -1: floor of 1
    (10, 1 << 26, 1, 33, None, BIG),                      # ntime * (n_ends - 1) = 2^31
    (70, 1, (1 << 31) - 1, 2, None, BIG),                 # nchan / 8 binds
]
SIR_ROWS = [
    (3, 4, 2100, None, None, BIG),
    (3, 4, 2100, None, None, 256 + 12 * 2 * 4 * 2),       # room for 2 windows: 3 -> 2
    (3, 4, 2100, None, None, 10),                         # less than one window's workspace: 3 -> 2 -> 1
    (3, 4, 1025, None, None, 10),                         # no workspace: the budget is never asked for
    (1, 1, 1, None, None, 10),
    (1, 4, 2100, None, None, 10),
    (1000, 4, 5000, None, None, 256 + 12 * 100 * 4 * 3),  # 1000 -> 500 -> 250 -> 125 -> 63
    (1 << 26, 64, 4096, None, None, BIG),                 # no launch cap
]

# recorded (batch, nbytes); for SIR (batch, nbytes, times the budget was asked for)
LINE_RMS_EXPECTED = [
    (1, 384),
    (64, 1152256),
    (5, 90256),
    (64, 1152256),
    (64, 1152256),
    (1, 18256),
    (8, 144256),
    (2, 896),
    (2, 896),
    (16383, 268681456),
    (16383, 268681456),
    (16383, 1342095616),
    (1023, 34326200560),
    (1, 268435728),
    (1, 17179869456),
    (1, 34359738608),
]
LDEV_EXPECTED = [
    (1, 280),
    (12, 53776),
    (5, 22556),
    (12, 53776),
    (1, 4716),
    (3, 1216),
    (2, 896),
    (2047, 8585748732),
    (511, 2145384700),
    (63, 8455717372),
    (1, 8589934848),
    (1, 8589934852),
    (1, 4294971652),
    (1, 8589934852),
    (31, 266287972608),
]
HYST_EXPECTED = [
    (1, 314),
    (12, 328696),
    (5, 137106),
    (12, 328696),
    (1, 27626),
    (3, 8320),
    (2, 5632),
    (254, 68715284720),
    (204, 7043613820768),
    (3, 64424509690),
    (2, 42949673232),
    (1, 85899346184),
    (2, 34628174096),
    (7, 150323855602),
]
SIR_EXPECTED = [
    (3, 544, 1),
    (2, 448, 1),
    (1, 352, 1),
    (3, 0, 0),
    (1, 0, 0),
    (1, 352, 1),
    (63, 9328, 1),
    (67108864, 103079215360, 1),
]


# the fake workspace sizes the expectations were recorded with (linear in the batch, like the library's)
def _ws_line_rms(b, t, c, e):
    return 256 + 16 * b * (t + c)


def _ws_ldev(b, t, c, e):
    return 256 + 4 * b * (c + t * (e - 1))


def _ws_hyst(b, t, c, e):
    return 256 + 8 * b * (c + t * (e - 1)) + 2 * b * t * c


def _ws_sir(b, t, c, e):
    return 0 if c <= 2048 else 256 + 12 * b * t * -(-c // 2048)


def _families():
    from tricolour_amd import flagging
    return {"line_rms": (LINE_RMS_ROWS, LINE_RMS_EXPECTED, _ws_line_rms, lambda t, c, e: flagging._line_rms_cap(t, c)),
            "ldev": (LDEV_ROWS, LDEV_EXPECTED, _ws_ldev, flagging._ldev_cap),
            "hyst": (HYST_ROWS, HYST_EXPECTED, _ws_hyst, flagging._hyst_cap)}


@pytest.mark.parametrize("family", ["line_rms", "ldev", "hyst"])
def test_window_batch_gives_the_batches_of_the_family_pickers(family):
    from tricolour_amd import flagging
    rows, expected, ws, cap = _families()[family]
    assert len(rows) == len(expected)
    for (n_win, ntime, nchan, n_ends, max_windows, budget), want in zip(rows, expected):
        got = flagging._window_batch(n_win, lambda b: ws(b, ntime, nchan, n_ends), budget, cap(ntime, nchan, n_ends),
                                     max_windows)
        assert tuple(got) == want, (family, n_win, ntime, nchan, n_ends, max_windows, budget)
        lazy = flagging._window_batch(n_win, lambda b: ws(b, ntime, nchan, n_ends), lambda: budget,
                                      cap(ntime, nchan, n_ends), max_windows)
        assert tuple(lazy) == want


def test_window_batch_gives_the_batches_of_the_sir_loop():
    """No launch cap, and the budget is asked for only when the windows need a workspace at all."""
    from tricolour_amd import flagging
    assert len(SIR_ROWS) == len(SIR_EXPECTED)
    for (n_win, ntime, nchan, _, _, budget), (batch, nbytes, asked) in zip(SIR_ROWS, SIR_EXPECTED):
        calls = []

        def ask():
            calls.append(1)
            return budget
        got = flagging._window_batch(n_win, lambda b: _ws_sir(b, ntime, nchan, None), ask)
        assert tuple(got) == (batch, nbytes) and len(calls) == asked, (n_win, ntime, nchan, budget)


# ---------------------------------------------------------------------------
# batches and pointer offsets
# ---------------------------------------------------------------------------
def test_batches_cover_the_windows_in_order():
    from tricolour_amd import flagging
    assert list(flagging._batches(5, 2)) == [(0, 2), (2, 2), (4, 1)]
    assert list(flagging._batches(5, 5)) == [(0, 5)]
    assert list(flagging._batches(5, 7)) == [(0, 5)]
    assert list(flagging._batches(4, 1)) == [(0, 1), (1, 1), (2, 1), (3, 1)]


@pytest.mark.parametrize("dtype,itemsize", [("uint8", 1), ("float32", 4), ("float64", 8), ("complex64", 8), ("int32", 4)])
@pytest.mark.parametrize("per_window", [(3, 7), (1,), (4, 2, 3)])
def test_offsets_take_the_element_size_from_the_tensor(dtype, itemsize, per_window):
    import torch
    from tricolour_amd import flagging
    n_win, per = 5, int(np.prod(per_window))
    for lead in ((5,), (5, 1), (1, 5)):                       # (bl, corr) in any split
        t = torch.zeros(lead + per_window, dtype=getattr(torch, dtype))
        offsets = [flagging._at(t, n_win, w0) - t.data_ptr() for w0, _ in flagging._batches(n_win, 2)]
        assert offsets == [w0 * per * itemsize for w0 in (0, 2, 4)]
    assert flagging._at(None, n_win, 2) is None              # an optional array stays NULL


# ---------------------------------------------------------------------------
# the step table
# ---------------------------------------------------------------------------
TASKS = ("sum_threshold", "uvcontsub_flagger", "flag_autos", "combine_with_input_flags", "unflag", "flag_nans_zeros",
         "apply_static_mask", "scale_invariant_rank_operator", "threshold_line_rms", "mark_missing",
         "baseline_integrated_sum_threshold", "threshold_local_deviation", "threshold_incoherent_noise_spectrum",
         "hysteresis_growth")


def test_step_table_is_the_task_list():
    from tricolour_amd import scan, strategies
    assert tuple(strategies.STEPS) == scan.VALID_TASKS == TASKS
    assert scan.WHOLE_SCAN_TASKS == ("baseline_integrated_sum_threshold", "threshold_incoherent_noise_spectrum")
    for task, step in strategies.STEPS.items():
        assert callable(step.run), task
        assert step.check is None or callable(step.check), task
        assert step.whole_scan == (task in scan.WHOLE_SCAN_TASKS)
    with_rules = {t for t, s in strategies.STEPS.items() if s.check is not None}
    assert with_rules == {SIR, BLI, LDEV, INS, HYST}
    assert [t for t, s in strategies.STEPS.items() if s.marks] == ["mark_missing"]


def test_scan_imports_without_torch():
    import subprocess
    import sys
    from conftest import ROOT
    code = "import sys; import tricolour_amd.scan as s; s.check_strategies([]); assert 'torch' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ---------------------------------------------------------------------------
# messages
# ---------------------------------------------------------------------------
SIR, BLI, LDEV, INS, HYST = ("scale_invariant_rank_operator", "baseline_integrated_sum_threshold", "threshold_local_deviation",
                             "threshold_incoherent_noise_spectrum", "hysteresis_growth")


def step(task, **kwargs):
    return {"task": task, "kwargs": kwargs}


# (id, which function, strategies, keyword arguments of apply_strategies)
CASES = [
    ("check-no-task", "check", [{"kwargs": {"eta_time": 0.2}}], {}),
    ("check-unknown-task", "check", [step("flag_everything")], {}),
    ("check-unknown-task-after-valid", "check", [step("unflag"), {"task": "sumthreshold"}], {}),
    ("check-sir-unknown-missing", "check", [step(SIR, missing="sometimes")], {}),
    ("check-sir-marked-unmarked", "check", [step(SIR, missing="marked")], {}),
    ("check-sir-marked-too-late", "check", [step(SIR, missing="marked"), step("mark_missing")], {}),
    ("check-hyst-unknown-missing", "check", [step(HYST, missing="sometimes")], {}),
    ("check-hyst-missing-not-a-string", "check", [step(HYST, missing=["input"])], {}),
    ("check-hyst-marked-unmarked", "check", [step("unflag"), step(HYST, missing="marked")], {}),
    ("check-hyst-unknown-kwargs", "check", [step(HYST, reach=4, zeta=1, alpha=2)], {}),
    ("check-hyst-reach", "check", [step(HYST, reach=33)], {}),
    ("check-hyst-range-before-marked", "check", [step(HYST, missing="marked", nsigma_time=-1.0)], {}),
    ("check-ldev-unknown-kwargs", "check", [step(LDEV, window=3)], {}),
    ("check-ldev-even-window", "check", [step(LDEV, window_time=4)], {}),
    ("check-ldev-freq-chunks", "check", [step(LDEV, freq_chunks=0)], {}),
    ("check-ins-unknown-kwargs", "check", [step(INS, nsigma=5.0, sigma=3.0)], {}),
    ("check-ins-exclude-autos", "check", [step(INS, exclude_autos="yes")], {}),
    ("check-ins-bands", "check", [step(INS, bands_hz=[[2.0e9, 1.0e9]])], {}),
    ("check-ins-rounds", "check", [step(INS, rounds=17)], {}),
    ("check-ins-too-many-shapes", "check", [step(INS, shapes=[(0, 1)] * 20, bands_hz=[[1.0e9, 2.0e9]] * 12)], {}),
    ("check-bli-frac-high", "check", [step(BLI, min_baseline_frac=1.5)], {}),
    ("check-bli-frac-nan", "check", [step(BLI, min_baseline_frac=float("nan"))], {}),
    ("check-bli-frac-text", "check", [step(BLI, min_baseline_frac="half")], {}),
    ("apply-no-task", "apply", [{"kwargs": {}}], {}),
    ("apply-unknown-task", "apply", [step("flag_everything")], {}),
    ("apply-sir-unknown-missing", "apply", [step(SIR, missing="sometimes")], {}),
    ("apply-sir-marked-unmarked", "apply", [step(SIR, missing="marked", missing_penalty=0.5)], {}),
    ("apply-hyst-unknown-missing", "apply", [step(HYST, missing="sometimes")], {}),
    ("apply-hyst-marked-unmarked", "apply", [step(HYST, missing="marked")], {}),
    ("apply-hyst-unknown-kwargs", "apply", [step(HYST, zeta=1)], {}),
    ("apply-ldev-unknown-kwargs", "apply", [step(LDEV, window=3)], {}),
    ("apply-ins-unknown-kwargs", "apply", [step(INS, exclude_autos=False, sigma=3.0)], {}),
    ("apply-bli-autos-without-ubl", "apply", [step(BLI)], {}),
    ("apply-ins-autos-without-ubl", "apply", [step(INS, nsigma=4.0)], {}),
    ("apply-ins-bands-without-chan-freq", "apply", [step(INS, exclude_autos=False, bands_hz=[[1.0e9, 2.0e9]])], {}),
    ("apply-ins-bands-without-chan-freq-ubl-given", "apply", [step(INS, bands_hz=[[1.0e9, 2.0e9]])], {"ubl": "UBL"}),
    ("apply-bli-frac-high", "apply", [step(BLI, exclude_autos=False, min_baseline_frac=1.5)], {}),
]

# recorded (exception type, its args)
EXPECTED = {
    'check-no-task': (ValueError, ("strategy has no 'task': {'kwargs': {'eta_time': 0.2}}",)),
    'check-unknown-task': (ValueError, ("Task '%s' does not name a valid task", 'flag_everything')),
    'check-unknown-task-after-valid': (ValueError, ("Task '%s' does not name a valid task", 'sumthreshold')),
    'check-sir-unknown-missing': (ValueError, ("scale_invariant_rank_operator: missing must be 'none', 'input' or 'marked', got 'sometimes'",)),
    'check-sir-marked-unmarked': (ValueError, ("scale_invariant_rank_operator: missing 'marked' needs an earlier mark_missing",)),
    'check-sir-marked-too-late': (ValueError, ("scale_invariant_rank_operator: missing 'marked' needs an earlier mark_missing",)),
    'check-hyst-unknown-missing': (ValueError, ("hysteresis_growth: missing must be 'none', 'input' or 'marked', got 'sometimes'",)),
    'check-hyst-missing-not-a-string': (ValueError, ("hysteresis_growth: missing must be 'none', 'input' or 'marked', got ['input']",)),
    'check-hyst-marked-unmarked': (ValueError, ("hysteresis_growth: missing 'marked' needs an earlier mark_missing",)),
    'check-hyst-unknown-kwargs': (ValueError, ("hysteresis_growth: unknown kwargs ['alpha', 'zeta']",)),
    'check-hyst-reach': (ValueError, ('hysteresis_growth: reach must be an integer in [1, 32], got 33',)),
    'check-hyst-range-before-marked': (ValueError, ('hysteresis_growth: nsigma_time must be >= 0, got -1.0',)),
    'check-ldev-unknown-kwargs': (ValueError, ("threshold_local_deviation: unknown kwargs ['window']",)),
    'check-ldev-even-window': (ValueError, ('threshold_local_deviation: window_time must be an odd integer in [3, 31], got 4',)),
    'check-ldev-freq-chunks': (ValueError, ('threshold_local_deviation: freq_chunks must be an integer >= 1, got 0',)),
    'check-ins-unknown-kwargs': (ValueError, ("threshold_incoherent_noise_spectrum: unknown kwargs ['sigma']",)),
    'check-ins-exclude-autos': (ValueError, ("threshold_incoherent_noise_spectrum: exclude_autos must be True or False, got 'yes'",)),
    'check-ins-bands': (ValueError, ('threshold_incoherent_noise_spectrum: bands_hz must be a list of [f_lo, f_hi] pairs of finite numbers with f_lo <= f_hi, got [[2000000000.0, 1000000000.0]]',)),
    'check-ins-rounds': (ValueError, ('threshold_incoherent_noise_spectrum: rounds must be an integer in [1, 16], got 17',)),
    'check-ins-too-many-shapes': (ValueError, ('threshold_incoherent_noise_spectrum: at most 32 shapes (bands and the streak included)',)),
    'check-bli-frac-high': (ValueError, ('baseline_integrated_sum_threshold: min_baseline_frac must lie in [0, 1], got 1.5',)),
    'check-bli-frac-nan': (ValueError, ('baseline_integrated_sum_threshold: min_baseline_frac must lie in [0, 1], got nan',)),
    'check-bli-frac-text': (ValueError, ("baseline_integrated_sum_threshold: min_baseline_frac must lie in [0, 1], got 'half'",)),
    'apply-no-task': (ValueError, ("strategy has no 'task': {'kwargs': {}}",)),
    'apply-unknown-task': (ValueError, ("Task '%s' does not name a valid task", 'flag_everything')),
    'apply-sir-unknown-missing': (ValueError, ("scale_invariant_rank_operator: missing must be 'none', 'input' or 'marked', got 'sometimes'",)),
    'apply-sir-marked-unmarked': (ValueError, ("scale_invariant_rank_operator: missing 'marked' needs an earlier mark_missing",)),
    'apply-hyst-unknown-missing': (ValueError, ("hysteresis_growth: missing must be 'none', 'input' or 'marked', got 'sometimes'",)),
    'apply-hyst-marked-unmarked': (ValueError, ("hysteresis_growth: missing 'marked' needs an earlier mark_missing",)),
    'apply-hyst-unknown-kwargs': (TypeError, ("hysteresis_growth() got an unexpected keyword argument 'zeta'",)),
    'apply-ldev-unknown-kwargs': (TypeError, ("threshold_local_deviation() got an unexpected keyword argument 'window'",)),
    'apply-ins-unknown-kwargs': (TypeError, ("threshold_incoherent_noise_spectrum() got an unexpected keyword argument 'sigma'",)),
    'apply-bli-autos-without-ubl': (ValueError, ('baseline_integrated_sum_threshold: exclude_autos needs ubl',)),
    'apply-ins-autos-without-ubl': (ValueError, ('threshold_incoherent_noise_spectrum: exclude_autos needs ubl',)),
    'apply-ins-bands-without-chan-freq': (ValueError, ('threshold_incoherent_noise_spectrum: bands_hz needs chan_freq',)),
    'apply-ins-bands-without-chan-freq-ubl-given': (ValueError, ('threshold_incoherent_noise_spectrum: bands_hz needs chan_freq',)),
    'apply-bli-frac-high': (ValueError, ('min_baseline_frac must lie in [0, 1], got 1.5',)),
}


@pytest.mark.parametrize("cid,which,strats,kw", CASES, ids=[c[0] for c in CASES])
def test_rejections_keep_their_type_and_message(cid, which, strats, kw):
    """Every case fires before any device work: no GPU needed."""
    from tricolour_amd import scan, strategies
    kind, args = EXPECTED[cid]
    kw = {k: (np.array([[0, 0, 1], [1, 1, 1]]) if isinstance(v, str) and v == "UBL" else v) for k, v in kw.items()}
    with pytest.raises(kind) as err:
        if which == "check":
            scan.check_strategies(strats)
        else:
            strategies.apply_strategies(strats, np.zeros((2, 1, 4, 8), bool), np.ones((2, 1, 4, 8), np.complex64), **kw)
    assert type(err.value) is kind and err.value.args == args


# ---------------------------------------------------------------------------
# GPU: the SIR loop with more than one batch
# ---------------------------------------------------------------------------
# (shape, workspace budget in bytes, windows per batch).  A frequency line beyond 65536 channels needs the workspace
# (per-segment aggregates); 4 time rows round to the same 768 bytes for 1, 2 and 3 windows, so a budget below that
# halves down to single windows; 16 rows need 768 / 1280 / 2048 bytes, so 1500 bytes hold 2 windows: batches of 2 and 1.
SIR_BATCHED = [((3, 1, 4, 65537), 100, 1), ((3, 1, 16, 65537), 1500, 2)]


@pytest.mark.parametrize("shape,budget,batch", SIR_BATCHED)
def test_sir_budgets_force_the_batches(shape, budget, batch):
    from tricolour_amd import _lib, flagging
    lib = _lib.lib()
    n_win, ntime, nchan = shape[0] * shape[1], shape[2], shape[3]
    for ws_bytes in (lib.tri_sir_workspace_bytes, lib.tri_sir_masked_workspace_bytes):
        assert ws_bytes(n_win, ntime, nchan) > 0
        assert flagging._window_batch(n_win, lambda b: ws_bytes(b, ntime, nchan), 1 << 40)[0] == n_win
    assert flagging._window_batch(n_win, lambda b: lib.tri_sir_workspace_bytes(b, ntime, nchan), budget)[0] == batch


@pytest.mark.gpu
@pytest.mark.parametrize("shape,budget,batch", SIR_BATCHED)
def test_gpu_sir_batching_gives_the_same_result(gpu, monkeypatch, shape, budget, batch):
    import torch
    from tricolour_amd import flagging
    rng = np.random.RandomState(shape[2])
    f = rng.uniform(size=shape) < 0.3
    m = rng.uniform(size=shape) < 0.1
    ft, mt = torch.from_numpy(f).cuda(), torch.from_numpy(m).cuda()
    seen = []
    batches = flagging._batches

    def recording(n_win, b):
        seen.append((n_win, b))
        return batches(n_win, b)
    monkeypatch.setattr(flagging, "_batches", recording)
    monkeypatch.delenv("TRICOLOUR_AMD_WORKSPACE_GB", raising=False)
    whole = flagging.scale_invariant_rank_operator(ft, 0.2, 0.25).cpu().numpy()
    whole_m = flagging.scale_invariant_rank_operator_masked(ft, mt, 0.2, 0.25, 0.1).cpu().numpy()
    assert seen == [(3, 3), (3, 3)]
    del seen[:]
    monkeypatch.setenv("TRICOLOUR_AMD_WORKSPACE_GB", repr(budget / float(1 << 30)))
    parts = flagging.scale_invariant_rank_operator(ft, 0.2, 0.25).cpu().numpy()
    if batch == 2:
        # the masked aggregates are wider: the same budget holds one window at a time
        assert seen == [(3, 2)]
    parts_m = flagging.scale_invariant_rank_operator_masked(ft, mt, 0.2, 0.25, 0.1).cpu().numpy()
    assert len(seen) == 2 and all(n == 3 and b < 3 for n, b in seen), seen
    assert np.array_equal(parts, whole) and np.array_equal(parts_m, whole_m)
    assert np.array_equal(parts, sir_windows(f, 0.2, 0.25))
    assert np.array_equal(parts_m, sirm_windows(f, m, 0.2, 0.25, 0.1))
