"""Device-resident strategy chain: the combination rules of
``StrategyExecutor.apply_strategies`` (reference
``tricolour/apps/tricolour/strat_executor.py:29-83``) applied to torch tensors
that stay in HBM between steps.  Every task is described once, by its row of
:data:`STEPS`: how it runs and combines with the running flags, what
``scan.check_strategies`` rejects before any work, whether it needs the whole
scan.  Importing this module needs neither torch nor a GPU."""
import collections
import functools

import numpy as np

from tricolour_amd import flagging


def _copy(flags):
    return flags.clone() if hasattr(flags, "clone") else flags.copy()


class Chain:
    """The state of a running chain: the current ``flags``, the ``original`` ones, the last ``mark_missing`` snapshot
    ``marked`` (or None) and what the chain was called with."""

    def __init__(self, flags, vis, **arrays):
        self.flags, self.vis, self.original, self.marked = flags, vis, _copy(flags), None
        self.__dict__.update(arrays)          # ubl, ant_pos, chan_freq, chan_width, masked_channels

    def ored(self, new_flags):
        """``new_flags | flags``: how most steps combine with the running flags (strat_executor.py:43, 54)."""
        import torch
        return torch.logical_or(new_flags, self.flags) if torch.is_tensor(self.flags) else new_flags | self.flags


# --- rules that several steps share, for check and run alike ---
def _check_missing(task, which, marked_seen):
    """The ``missing`` kwarg names the mask of samples that are flagged without being detections: ``none``, ``input``
    (the flags the chain started from) or ``marked`` (the last ``mark_missing`` snapshot, which must exist)."""
    if which not in flagging.HYST_MISSING:
        raise ValueError("%s: missing must be 'none', 'input' or 'marked', got %r" % (task, which))
    if which == "marked" and not marked_seen:
        raise ValueError("%s: missing 'marked' needs an earlier mark_missing" % task)


def _missing_mask(task, chain, which):
    _check_missing(task, which, chain.marked is not None)
    return {"none": None, "input": chain.original, "marked": chain.marked}[which]


def _pop_select(task, kw, ubl):
    """``exclude_autos`` (default True) -> the baseline selection ``select`` of the steps that integrate over baselines
    (every baseline receives their detections, the unselected ones included)."""
    if not kw.pop("exclude_autos", True):
        return None
    if ubl is None:
        raise ValueError("%s: exclude_autos needs ubl" % task)
    u = np.asarray(ubl)
    return u[:, 1] != u[:, 2]


def _check_known(task, kw, names):
    unknown = sorted(set(kw) - set(names))
    if unknown:
        raise ValueError("%s: unknown kwargs %s" % (task, unknown))


# --- run: (task, chain, kwargs) -> the new flags; the kwargs are the step's own copy ---
def _ored(detector):
    """The run of a ``detector(vis, flags, **kwargs)`` whose result is ORed into the running flags."""
    return lambda task, chain, kw: chain.ored(detector(chain.vis, chain.flags, **kw))


def _run_unflag(task, chain, kw):
    import torch
    return torch.zeros_like(chain.flags) if torch.is_tensor(chain.flags) else chain.flags * 0


def _run_apply_static_mask(task, chain, kw):
    new_flags = flagging.apply_static_mask(chain.flags, chain.ubl, chain.ant_pos, chain.masked_channels,
                                           chain.chan_freq, chain.chan_width, **kw)
    return chain.ored(new_flags) if kw["accumulation_mode"].strip() == "or" else new_flags   # strat_executor.py:75-78


def _run_sir(task, chain, kw):
    mask = _missing_mask(task, chain, kw.pop("missing", "none"))
    penalty = kw.pop("missing_penalty", 0.1)
    if mask is None:
        return chain.ored(flagging.scale_invariant_rank_operator(chain.flags, **kw))
    return chain.ored(flagging.scale_invariant_rank_operator_masked(chain.flags, mask, penalty=penalty, **kw))


def _run_hysteresis_growth(task, chain, kw):
    mask = _missing_mask(task, chain, kw.pop("missing", "none"))
    return chain.ored(flagging.hysteresis_growth(chain.vis, chain.flags, missing=mask, **kw))


def _run_baseline_integrated(task, chain, kw):
    select = _pop_select(task, kw, chain.ubl)
    return chain.ored(flagging.baseline_integrated_flagger(chain.vis, chain.flags, select=select, **kw))


def _run_incoherent_noise(task, chain, kw):
    select = _pop_select(task, kw, chain.ubl)
    bands = kw.pop("bands_hz", None)
    if bands is not None:
        if chain.chan_freq is None:
            raise ValueError("%s: bands_hz needs chan_freq" % task)
        # on the host: a channel belongs to a band if its centre lies in it; an empty band is dropped
        kw["shapes"] = list(kw.get("shapes", ())) + flagging.incoherent_noise_bands(
            flagging.check_incoherent_noise_bands(bands), chain.chan_freq)
    return chain.ored(flagging.threshold_incoherent_noise_spectrum(chain.vis, chain.flags, select=select, **kw))


# --- check: (task, kwargs, marked_seen) -> None, or a ValueError that names the task; the kwargs are its own copy ---
def _check_sir(task, kw, marked_seen):
    """``missing`` must be ``none`` / ``input`` / ``marked``, and ``marked`` needs a ``mark_missing`` step before it."""
    _check_missing(task, kw.get("missing", "none"), marked_seen)


def _check_baseline_integrated(task, kw, marked_seen):
    """``min_baseline_frac`` must lie in [0, 1]."""
    frac = kw.get("min_baseline_frac", 0.25)
    try:
        ok = 0.0 <= float(frac) <= 1.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: min_baseline_frac must lie in [0, 1], got %r" % (task, frac))


def _check_local_deviation(task, kw, marked_seen):
    """No unknown kwarg; a window must be odd and in [3, 31], a scale >= 0 and not NaN, ``freq_chunks >= 1``
    (``flagging.check_local_deviation_kwargs``)."""
    _check_known(task, kw, ("window_time", "window_freq", "scale_time", "scale_freq", "freq_chunks"))
    try:
        flagging.check_local_deviation_kwargs(**kw)
    except ValueError as e:
        raise ValueError("%s: %s" % (task, e))


def _check_hysteresis_growth(task, kw, marked_seen):
    """No unknown kwarg, none out of range (``flagging.check_hysteresis_kwargs``), and ``missing: marked`` needs a
    ``mark_missing`` step before it."""
    _check_known(task, kw, ("nsigma_time", "nsigma_freq", "reach", "freq_chunks", "missing"))
    try:
        which = flagging.check_hysteresis_kwargs(**kw)[4]
    except ValueError as e:
        raise ValueError("%s: %s" % (task, e))
    _check_missing(task, which, marked_seen)


def _check_incoherent_noise(task, kw, marked_seen):
    """No unknown kwarg, none out of range (``flagging.check_incoherent_noise_kwargs``), ``exclude_autos`` a boolean,
    ``bands_hz`` well-formed (``flagging.check_incoherent_noise_bands``), and at most ``flagging.INS_MAX_SHAPES``
    shapes, bands and the streak included."""
    _check_known(task, kw, ("min_baseline_frac", "nsigma", "shapes", "streak", "narrow", "rounds", "exclude_autos", "bands_hz"))
    try:
        autos = kw.pop("exclude_autos", True)
        if not isinstance(autos, (bool, np.bool_)):
            raise ValueError("exclude_autos must be True or False, got %r" % (autos,))
        bands = kw.pop("bands_hz", None)
        if bands is not None:
            bands = flagging.check_incoherent_noise_bands(bands)
        checked = flagging.check_incoherent_noise_kwargs(**kw)
        if len(checked[2]) + (1 if checked[3] else 0) + len(bands or ()) > flagging.INS_MAX_SHAPES:
            raise ValueError("at most %d shapes (bands and the streak included)" % flagging.INS_MAX_SHAPES)
    except ValueError as e:
        raise ValueError("%s: %s" % (task, e))


# --- the table ---
# run(chain, kwargs) -> the new flags; check(kwargs, marked_seen), or None: no pre-flight rules; whole_scan: needs every
# baseline of the scan at once, so cannot run per baseline chunk; marks: its flags are what `missing: marked` refers to
Step = collections.namedtuple("Step", "run check whole_scan marks", defaults=(None, False, False))


def _named(table):
    """The table with every task's name bound into its functions (they put it in front of their messages)."""
    return {task: step._replace(run=functools.partial(step.run, task),
                                check=step.check and functools.partial(step.check, task))
            for task, step in table.items()}


STEPS = _named({
    # strat_executor.py:36-83
    "sum_threshold": Step(_ored(flagging.sum_threshold_flagger)),
    # discards the previous flags by design (strat_executor.py:44-51)
    "uvcontsub_flagger": Step(lambda task, chain, kw: flagging.uvcontsub_flagger(chain.vis, chain.flags, **kw)),
    "flag_autos": Step(lambda task, chain, kw: chain.ored(flagging.flag_autos(chain.flags, [chain.ubl]))),
    "combine_with_input_flags": Step(lambda task, chain, kw: chain.ored(chain.original)),
    "unflag": Step(_run_unflag),
    "flag_nans_zeros": Step(lambda task, chain, kw: flagging.flag_nans_and_zeros(chain.vis, chain.flags)),
    "apply_static_mask": Step(_run_apply_static_mask),
    # beyond the reference: the steps of tricolour_amd.flagging
    "scale_invariant_rank_operator": Step(_run_sir, _check_sir),
    "threshold_line_rms": Step(_ored(flagging.threshold_line_rms)),
    "mark_missing": Step(lambda task, chain, kw: chain.flags, marks=True),
    "baseline_integrated_sum_threshold": Step(_run_baseline_integrated, _check_baseline_integrated, whole_scan=True),
    "threshold_local_deviation": Step(_ored(flagging.threshold_local_deviation), _check_local_deviation),
    "threshold_incoherent_noise_spectrum": Step(_run_incoherent_noise, _check_incoherent_noise, whole_scan=True),
    "hysteresis_growth": Step(_run_hysteresis_growth, _check_hysteresis_growth),
})
TASKS = tuple(STEPS)


def strategy_task(strategy):
    """The task of one strategy dict, or the reference's error for none or an unknown one (strat_executor.py:33-36, 82-83)."""
    try:
        task = strategy['task']
    except KeyError:
        raise ValueError("strategy has no 'task': %s" % strategy)
    if task not in TASKS:
        raise ValueError("Task '%s' does not name a valid task", task)
    return task


def apply_strategies(strategies, flag_windows, vis_windows, ubl=None, ant_pos=None,
                     chan_freq=None, chan_width=None, masked_channels=None):
    """Runs the ordered ``strategies`` (dicts with ``task`` and ``kwargs``, as
    parsed from the YAML) on (bl, corr, time, chan) tensors and returns the
    final flags."""
    chain = Chain(flag_windows, vis_windows, ubl=ubl, ant_pos=ant_pos, chan_freq=chan_freq, chan_width=chan_width,
                  masked_channels=masked_channels)
    for strategy in strategies:
        step = STEPS[strategy_task(strategy)]
        chain.flags = step.run(chain, dict(strategy.get('kwargs') or {}))
        if step.marks:
            # what is flagged by now is missing data, not a detection: the mask of later steps with `missing: marked`
            chain.marked = _copy(chain.flags)
    return chain.flags
