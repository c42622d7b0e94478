"""Device-resident strategy chain: the combination rules of
``StrategyExecutor.apply_strategies`` (reference
``tricolour/apps/tricolour/strat_executor.py:29-83``) applied to torch tensors
that stay in HBM between steps."""
import numpy as np

from tricolour_amd import flagging


def apply_strategies(strategies, flag_windows, vis_windows, ubl=None, ant_pos=None,
                     chan_freq=None, chan_width=None, masked_channels=None):
    """Runs the ordered ``strategies`` (dicts with ``task`` and ``kwargs``, as
    parsed from the YAML) on (bl, corr, time, chan) tensors and returns the
    final flags."""
    import torch
    original = flag_windows.clone() if torch.is_tensor(flag_windows) else flag_windows.copy()
    lor = torch.logical_or if torch.is_tensor(flag_windows) else (lambda a, b: a | b)
    marked = None                 # the last mark_missing snapshot
    for strategy in strategies:
        try:
            task = strategy['task']
        except KeyError:
            raise ValueError("strategy has no 'task': %s" % strategy)
        kw = strategy.get('kwargs') or {}
        if task == "sum_threshold":
            new_flags = flagging.sum_threshold_flagger(vis_windows, flag_windows, **kw)
            flag_windows = lor(new_flags, flag_windows)          # strat_executor.py:43
        elif task == "uvcontsub_flagger":
            # discards the previous flags by design (strat_executor.py:44-51)
            flag_windows = flagging.uvcontsub_flagger(vis_windows, flag_windows, **kw)
        elif task == "flag_autos":
            new_flags = flagging.flag_autos(flag_windows, [ubl])
            flag_windows = lor(new_flags, flag_windows)          # :54
        elif task == "combine_with_input_flags":
            flag_windows = lor(flag_windows, original)           # :59
        elif task == "unflag":
            flag_windows = flag_windows * 0 if not torch.is_tensor(flag_windows) else torch.zeros_like(flag_windows)
        elif task == "flag_nans_zeros":
            flag_windows = flagging.flag_nans_and_zeros(vis_windows, flag_windows)   # :63
        elif task == "mark_missing":
            # what is flagged by now is missing data, not a detection: the mask of later masked SIR steps
            marked = flag_windows.clone() if torch.is_tensor(flag_windows) else flag_windows.copy()
        elif task == "scale_invariant_rank_operator":
            kw = dict(kw)
            which = kw.pop("missing", "none")
            penalty = kw.pop("missing_penalty", 0.1)
            if which == "none":
                new_flags = flagging.scale_invariant_rank_operator(flag_windows, **kw)
            elif which in ("input", "marked"):
                if which == "marked" and marked is None:
                    raise ValueError("scale_invariant_rank_operator: missing 'marked' needs an earlier mark_missing")
                new_flags = flagging.scale_invariant_rank_operator_masked(
                    flag_windows, original if which == "input" else marked, penalty=penalty, **kw)
            else:
                raise ValueError("scale_invariant_rank_operator: missing must be 'none', 'input' or 'marked', got %r" % (which,))
            flag_windows = lor(new_flags, flag_windows)
        elif task == "threshold_line_rms":
            new_flags = flagging.threshold_line_rms(vis_windows, flag_windows, **kw)
            flag_windows = lor(new_flags, flag_windows)
        elif task == "threshold_local_deviation":
            new_flags = flagging.threshold_local_deviation(vis_windows, flag_windows, **kw)
            flag_windows = lor(new_flags, flag_windows)
        elif task == "hysteresis_growth":
            kw = dict(kw)
            which = kw.pop("missing", "none")
            if which not in flagging.HYST_MISSING:
                raise ValueError("hysteresis_growth: missing must be 'none', 'input' or 'marked', got %r" % (which,))
            if which == "marked" and marked is None:
                raise ValueError("hysteresis_growth: missing 'marked' needs an earlier mark_missing")
            mask = {"none": None, "input": original, "marked": marked}[which]
            new_flags = flagging.hysteresis_growth(vis_windows, flag_windows, missing=mask, **kw)
            flag_windows = lor(new_flags, flag_windows)
        elif task == "baseline_integrated_sum_threshold":
            kw = dict(kw)
            select = None
            if kw.pop("exclude_autos", True):
                if ubl is None:
                    raise ValueError("baseline_integrated_sum_threshold: exclude_autos needs ubl")
                u = np.asarray(ubl)
                select = u[:, 1] != u[:, 2]
            # every baseline receives the detections of the integrated image, the unselected ones included
            new_flags = flagging.baseline_integrated_flagger(vis_windows, flag_windows, select=select, **kw)
            flag_windows = lor(new_flags, flag_windows)
        elif task == "threshold_incoherent_noise_spectrum":
            kw = dict(kw)
            select = None
            if kw.pop("exclude_autos", True):
                if ubl is None:
                    raise ValueError("threshold_incoherent_noise_spectrum: exclude_autos needs ubl")
                u = np.asarray(ubl)
                select = u[:, 1] != u[:, 2]
            bands = kw.pop("bands_hz", None)
            if bands is not None:
                if chan_freq is None:
                    raise ValueError("threshold_incoherent_noise_spectrum: bands_hz needs chan_freq")
                # on the host: a channel belongs to a band if its centre lies in it; an empty band is dropped
                kw["shapes"] = list(kw.get("shapes", ())) + flagging.incoherent_noise_bands(
                    flagging.check_incoherent_noise_bands(bands), chan_freq)
            # every baseline receives the detections, the unselected ones included
            new_flags = flagging.threshold_incoherent_noise_spectrum(vis_windows, flag_windows, select=select, **kw)
            flag_windows = lor(new_flags, flag_windows)
        elif task == "apply_static_mask":
            new_flags = flagging.apply_static_mask(flag_windows, ubl, ant_pos, masked_channels,
                                                   chan_freq, chan_width, **kw)
            if kw["accumulation_mode"].strip() == "or":          # :75-78
                flag_windows = lor(new_flags, flag_windows)
            else:
                flag_windows = new_flags
        else:
            raise ValueError("Task '%s' does not name a valid task", task)
    return flag_windows
