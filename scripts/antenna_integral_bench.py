"""Times the antenna-integration calls with HIP events on one slab (headline: 23 antennas without autos, 253 bl x 4
corr x 1024 x 4096 complex64, 2 % flagged), next to baseline integration on the same input, which is the yardstick:

  baseline_accumulate / antenna_accumulate   the two C entry points on preallocated accumulators, in two alternating
                                             rounds; antenna_accumulate also in its flags-only form
  baseline_integral / antenna_integral       the Python calls (they allocate and zero their accumulators)
  antenna_integrated_flagger_stage1          the whole call with the stage-1 kwargs of default.yaml
  extend_flags_by_antenna                    the whole flags-only call

Bytes are counted under the two-read model: the antenna accumulate reads every sample once per antenna it belongs
to, so 2 x (8 + 1) B per complex64 visibility, and reads and writes 12 B of accumulator per (antenna, position);
baseline integration reads 8 + 1 B once.  `time_over_baseline` is the accumulate's median time over the baseline
accumulate's of the same round and `bytes_over_baseline` the ratio of the two byte counts: a time ratio near the byte
ratio says the second read of each sample is HBM traffic, a ratio near 1 that a cache absorbs it.  Rates are at these
algorithmic bytes; `frac_of_copy` is the rate over scripts/hbm_peak.py's copy_rate().  The first positions of the
sum of two antennas are checked against the same sequential float64 adds done in torch.

The last line is a demonstration, recorded and not asserted: 16 antennas, (120, 1, 128, 256), unit noise, a constant
signal on times 40-71 of channels 100-107 of the 15 baselines of antenna 5; what the per-baseline flagger and
antenna_integrated_flagger, with the same kwargs, newly flag in the burst on that antenna's baselines and on the
others, and outside the burst.  One JSON line per leg; --out also writes them to a file.

    python scripts/antenna_integral_bench.py [--shape headline] [--repeats 20] [--out profiles/antenna_integral_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from baseline_integral_bench import STAGE1, sequential_sum, synth, timed  # noqa: E402
from hbm_peak import copy_rate  # noqa: E402
from tricolour_amd import _lib, flagging  # noqa: E402

# (antennas, (corr, time, chan)); no autos: antennas * (antennas - 1) / 2 baselines
SHAPES = {"headline": (23, (4, 1024, 4096)), "short": (64, (1, 64, 1024)), "small": (16, (2, 256, 1024)),
          "tiny": (4, (1, 8, 64))}
DEMO_KW = dict(outlier_nsigma=6.0, freq_chunks=4, num_major_iterations=5)
DEMO_AMPLITUDE = 1.5


def triangle(nant):
    a1, a2 = np.triu_indices(nant, 1)
    return np.stack([np.arange(a1.size), a1, a2], axis=1)


def demonstration(dev):
    nant, bad = 16, 5
    ubl = triangle(nant)
    shape = (len(ubl), 1, 128, 256)
    g = torch.Generator(device=dev).manual_seed(77)
    vis = torch.view_as_complex(torch.randn(shape + (2,), generator=g, device=dev))
    on = torch.from_numpy((ubl[:, 1] == bad) | (ubl[:, 2] == bad)).to(dev)
    phase = torch.polar(torch.ones(len(ubl), device=dev), 2 * np.pi * torch.rand(len(ubl), generator=g, device=dev))
    burst = torch.zeros(shape[1:], dtype=torch.bool, device=dev)
    burst[0, 40:72, 100:108] = True
    vis = vis + DEMO_AMPLITUDE * (phase * on)[:, None, None, None] * burst[None]
    flags = torch.rand(shape, generator=g, device=dev) < 0.02

    def shares(out):
        new = out & ~flags
        return dict(burst_on_the_antenna=round(new[on][:, burst].float().mean().item(), 4),
                    burst_on_the_others=round(new[~on][:, burst].float().mean().item(), 4),
                    outside_the_burst=round(new[:, ~burst].float().mean().item(), 4))
    return dict(leg="demonstration", antennas=nant, antenna=bad, dims=list(shape), amplitude=DEMO_AMPLITUDE, kwargs=DEMO_KW,
                newly_flagged_per_baseline=shares(flagging.sum_threshold_flagger(vis, flags, **DEMO_KW)),
                newly_flagged_antenna_integrated=shares(flagging.antenna_integrated_flagger(vis, flags, ubl, **DEMO_KW)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="headline", choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--check-positions", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nant, img = SHAPES[a.shape]
    ubl = triangle(nant)
    nbl, n = len(ubl), img[0] * img[1] * img[2]
    shape = (nbl,) + img
    offsets, baselines, members, ant1, ant2 = flagging.antenna_baselines(ubl)
    copy_bps = copy_rate(dev)
    torch.cuda.empty_cache()
    vis, flags = synth(shape, dev, 1234, "c64")
    stream = torch.cuda.current_stream().cuda_stream
    total = torch.zeros(img, dtype=torch.float64, device=dev)
    count = torch.zeros(img, dtype=torch.int32, device=dev)
    atotal = torch.zeros((nant,) + img, dtype=torch.float64, device=dev)
    acount = torch.zeros((nant,) + img, dtype=torch.int32, device=dev)
    off, bls = torch.from_numpy(offsets).to(dev), torch.from_numpy(baselines).to(dev)
    lines = []
    bl_bytes = nbl * n * 9 + 2 * 12 * n
    ant_bytes = 2 * nbl * n * 9 + 2 * 12 * nant * n
    flags_bytes = 2 * nbl * n + 2 * 4 * nant * n

    def emit(leg, med, best, nbytes, **extra):
        bps = nbytes / (med * 1e-3)
        rec = dict(shape=a.shape, antennas=nant, dims=list(shape), leg=leg, ms_median=round(med, 3), ms_min=round(best, 3),
                   algorithmic_bytes=nbytes, GBps=round(bps / 1e9, 1), copy_GBps=round(copy_bps / 1e9, 1),
                   frac_of_copy=round(bps / copy_bps, 3), source_hash=_lib.source_hash())
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def baseline_accumulate():
        _lib.check(lib.tri_baseline_accumulate(vis.data_ptr(), _lib.TRI_VIS_C64, flags.data_ptr(), None, nbl, n,
                                               total.data_ptr(), count.data_ptr(), stream))

    def antenna_accumulate(with_vis=True):
        _lib.check(lib.tri_antenna_accumulate(vis.data_ptr() if with_vis else None, _lib.TRI_VIS_C64, flags.data_ptr(),
                                              off.data_ptr(), bls.data_ptr(), nbl, nant, n,
                                              atotal.data_ptr() if with_vis else None, acount.data_ptr(), stream))

    # the sums of one call against the sequential adds in torch, on the first positions of the first and last antenna
    antenna_accumulate()
    k = min(a.check_positions, img[2])
    ok = True
    for ant in (0, nant - 1):
        mine = torch.from_numpy(baselines[offsets[ant]:offsets[ant + 1]].astype(np.int64)).to(dev)
        exp = sequential_sum(vis[mine, :1, :1, :k], flags[mine, :1, :1, :k])
        ok = ok and torch.equal(atotal[ant, :1, :1, :k].view(torch.int64), exp[0].view(torch.int64)) and \
            torch.equal(acount[ant, :1, :1, :k], exp[1])

    # (the timed calls keep adding to the same accumulators: the same work)
    for rnd in (1, 2):
        bmed, bbest = timed(baseline_accumulate, a.repeats)
        emit("baseline_accumulate", bmed, bbest, bl_bytes, round=rnd, bytes_per_visibility=9)
        med, best = timed(antenna_accumulate, a.repeats)
        emit("antenna_accumulate", med, best, ant_bytes, round=rnd, bytes_per_visibility=round(ant_bytes / (nbl * n), 2),
             time_over_baseline=round(med / bmed, 3), bytes_over_baseline=round(ant_bytes / bl_bytes, 3),
             checked_positions=2 * k, sum_bits_and_counts_equal=bool(ok))
    med, best = timed(lambda: antenna_accumulate(False), a.repeats)
    emit("antenna_accumulate_flags_only", med, best, flags_bytes, bytes_per_visibility=round(flags_bytes / (nbl * n), 2))
    del total, count, atotal, acount
    med, best = timed(lambda: flagging.baseline_integral(vis, flags), a.repeats)
    emit("baseline_integral", med, best, bl_bytes)
    med, best = timed(lambda: flagging.antenna_integral(vis, flags, ubl), a.repeats)
    emit("antenna_integral", med, best, ant_bytes)
    # + finish (17 B per antenna position), the flagger on antennas * corr windows, the apply pass (2 B per visibility,
    # the two det lines from cache)
    med, best = timed(lambda: flagging.antenna_integrated_flagger(vis, flags, ubl, **STAGE1), max(3, a.repeats // 4))
    emit("antenna_integrated_flagger_stage1", med, best, ant_bytes + 17 * nant * n + 2 * nbl * n,
         flagged_in=round(flags.sum(dtype=torch.int64).item() / flags.numel(), 4))
    med, best = timed(lambda: flagging.extend_flags_by_antenna(flags, ubl), a.repeats)
    emit("extend_flags_by_antenna", med, best, flags_bytes + 5 * nant * n + 2 * nbl * n)
    del vis, flags
    torch.cuda.empty_cache()
    rec = demonstration(dev)
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")
    assert ok, "sum or count differs from the sequential float64 adds"


if __name__ == "__main__":
    main()
