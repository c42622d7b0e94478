"""uvcontsub_flagger.  The reference routine is plain NumPy
and its own tests do not cover it; G11 holds its output (run under this
image's NumPy).  The oracle restatement must reproduce G11 exactly; the HIP
path follows the same float32 semantics but cannot reproduce NumPy's FFT
rounding, so it is held to a flag-agreement rate."""
import numpy as np
import pytest

from conftest import load_golden


def _cases():
    d, _ = load_golden("G11_uvcontsub.npz")
    out = []
    for name in ("a", "b"):
        kw = {k[len("kw_%s_" % name):]: d[k].tolist() for k in d.files if k.startswith("kw_%s_" % name)}
        out.append((d["vis"], d["flags"], kw, d["out_" + name]))
    return out, str(d["numpy_version"])


def test_oracle_reproduces_reference():
    from oracle import oracle
    cases, npver = _cases()
    if npver.split(".")[0] != np.__version__.split(".")[0]:
        pytest.skip("fixture generated with NumPy %s" % npver)
    for vis, flags, kw, exp in cases:
        got = oracle.uvcontsub_flagger(vis, flags, **kw)
        assert np.array_equal(got, exp)
        assert got[1, 1].all()            # fully flagged product untouched


@pytest.mark.gpu
def test_gpu_uvcontsub_agreement(gpu):
    from oracle import oracle
    from tricolour_amd import flagging
    cases, _ = _cases()
    for vis, flags, kw, exp in cases:
        got = flagging.uvcontsub_flagger(vis, flags, **kw)
        assert got.shape == exp.shape and got.dtype == np.bool_
        agree = (got == exp).mean()
        assert agree >= 0.999, "flag agreement %.5f" % agree
        assert got[1, 1].all()
    # a larger random block against the oracle
    rs = np.random.RandomState(3)
    shape = (3, 2, 64, 512)
    x = np.linspace(0, 1, shape[3])
    vis = ((2 + np.cos(7 * x))[None, None, None, :] + 0.3 * rs.standard_normal(shape)
           + 1j * 0.3 * rs.standard_normal(shape)).astype(np.complex64)
    vis[..., 100] += 5
    vis[2, 0, 10] += 3
    flags = rs.uniform(size=shape) < 0.02
    kw = dict(major_cycles=5, or_original_from_cycle=1, taylor_degrees=20, sigma=10.0)
    exp = oracle.uvcontsub_flagger(vis, flags, **kw)
    got = flagging.uvcontsub_flagger(vis, flags, **kw)
    assert (got == exp).mean() >= 0.9995


# conf/default.yaml:37-45 and :106-112 (restated: the reference tree does not travel to the GPU box)
UV_SHIPPED = {
    "residual_flag_initial": dict(major_cycles=7, or_original_from_cycle=1, taylor_degrees=20, sigma=15.0),
    "residual_flag_final": dict(major_cycles=10, or_original_from_cycle=0, taylor_degrees=25, sigma=13.0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(UV_SHIPPED))
def test_gpu_uvcontsub_shipped_kwargs_mismatches_are_borderline(gpu, name):
    """Both shipped uvcontsub parameter sets.  NumPy's float64 FFT / pairwise nanmean cannot be reproduced bit for
    bit, so the claim is made precise: cycle by cycle, from the SAME starting flags, every flag
    that differs from the oracle's sits on a sample whose |vis - smooth| lies within rounding of the threshold
    sigma * mad; the number of such samples is printed.  The free-running chains must still agree >= 99.9 %."""
    from oracle import oracle
    from tricolour_amd import flagging
    kw = UV_SHIPPED[name]
    rs = np.random.RandomState(31 + len(name))
    shape = (3, 2, 96, 512)
    x = np.linspace(0, 1, shape[3])
    vis = ((2 + np.cos(7 * x) + 0.5 * np.sin(23 * x))[None, None, None, :] + 0.3 * rs.standard_normal(shape)
           + 1j * (0.2 * x[None, None, None, :] + 0.3 * rs.standard_normal(shape))).astype(np.complex64)
    vis[..., 100] += 5
    vis[..., 300:304] += 1.0                       # faint: near the threshold in later cycles
    vis[2, 0, 10] += 3
    vis[0, 1, 5, 7] = np.nan
    flags = rs.uniform(size=shape) < 0.02
    flags[1, 1] = True                             # a fully flagged product stays untouched
    cur = flags.copy()
    total_bad = 0
    for mi in range(kw["major_cycles"]):
        one = dict(kw, major_cycles=1, or_original_from_cycle=0 if mi >= kw["or_original_from_cycle"] else 1)
        exp, d = oracle.uvcontsub_flagger(vis, cur, dump=True, **one)
        got = flagging.uvcontsub_flagger(vis, cur, **one)
        bad = got != exp
        if bad.any():
            thr = np.broadcast_to(d["thr"].reshape(shape[0], shape[1], 1, 1), shape)
            rel = np.abs(d["absres"].reshape(shape) - thr)[bad] / thr[bad]
            assert rel.max() < 1e-5, "cycle %d: %d flags differ, farthest %.3g of the threshold away" % (mi, bad.sum(), rel.max())
        total_bad += int(bad.sum())
        cur = exp
    free = flagging.uvcontsub_flagger(vis, flags, **kw)
    ref = oracle.uvcontsub_flagger(vis, flags, **kw)
    nfree = int((free != ref).sum())
    print("%s: %d borderline flags over %d lock-step cycles, %d of %d differ free-running"
          % (name, total_bad, kw["major_cycles"], nfree, free.size))
    assert nfree <= 1e-3 * free.size
    assert free[1, 1].all()


@pytest.mark.gpu
def test_gpu_config4_chain(gpu):
    """BASELINE config 4 in miniature: static mask -> flag_autos -> uvcontsub
    (replaces the running flags) -> sum_threshold, device-resident, against the
    same chain evaluated with the oracle."""
    import torch
    from oracle import oracle
    from tricolour_amd.strategies import apply_strategies
    a1, a2 = np.triu_indices(3, 0)
    ubl = np.stack([np.arange(a1.size), a1, a2], axis=1)
    ants = np.array([[0., 0., 0.], [100., 0., 0.], [0., 300., 0.]])
    shape = (ubl.shape[0], 2, 48, 128)
    rs = np.random.RandomState(4)
    x = np.linspace(0, 1, shape[3])
    vis = ((3 + np.sin(5 * x))[None, None, None, :] + 0.3 * rs.standard_normal(shape)
           + 1j * 0.3 * rs.standard_normal(shape)).astype(np.complex64)
    vis[..., 33] += 6
    flags = rs.uniform(size=shape) < 0.02
    cf = np.linspace(1e9, 1.1e9, shape[3])
    cw = np.full(shape[3], cf[1] - cf[0])
    masks = [np.array([cf[60]])[:, None]]
    uv_kw = dict(major_cycles=3, or_original_from_cycle=1, taylor_degrees=20, sigma=15.0)
    st_kw = dict(outlier_nsigma=10, background_iterations=2, num_major_iterations=1)
    strategies = [dict(task="apply_static_mask", kwargs=dict(accumulation_mode="or", uvrange="")),
                  dict(task="flag_autos"),
                  dict(task="uvcontsub_flagger", kwargs=uv_kw),
                  dict(task="sum_threshold", kwargs=st_kw)]
    got = apply_strategies(strategies, torch.from_numpy(flags).cuda(), torch.from_numpy(vis).cuda(),
                           ubl=ubl, ant_pos=ants, chan_freq=cf, chan_width=cw, masked_channels=masks)
    f = oracle.apply_static_mask(flags, ubl, ants, masks, cf, cw, "or") | flags
    f = oracle.flag_autos(f, [ubl]) | f
    f = oracle.uvcontsub_flagger(vis, f, **uv_kw)
    f = oracle.sum_threshold_flagger(vis, f, **st_kw) | f
    assert (got.cpu().numpy() == f).mean() >= 0.999


UV_AB_SCRIPT = r'''
import sys, hashlib
sys.path.insert(0, %r)
import numpy as np
from tricolour_amd import flagging, _lib
rs = np.random.RandomState(8)
shape = (3, 2, 64, 512)
x = np.linspace(0, 1, shape[3])
vis = ((2 + np.cos(7 * x))[None, None, None, :] + 0.3 * rs.standard_normal(shape)
       + 1j * 0.3 * rs.standard_normal(shape)).astype(np.complex64)
vis[..., 100] += 5
vis[2, 0, 10] += 3
vis[0, 1, 5, 7] = np.nan
flags = rs.uniform(size=shape) < 0.02
flags[1, 1] = True
_lib.kernel_log_begin()
out = flagging.uvcontsub_flagger(vis, flags, major_cycles=5, or_original_from_cycle=1, taylor_degrees=20, sigma=10.0)
log = _lib.kernel_log_end()
print("DIGEST", hashlib.sha1(np.packbits(out).tobytes()).hexdigest(), int(out.sum()))
print("KERNELS", " ".join(sorted(k for k in log if k.startswith("k_uv_"))))
'''


@pytest.mark.gpu
def test_gpu_uvcontsub_vector_kernels_match_scalar(gpu):
    """The four-samples-per-thread residual / apply kernels and the scalar ones (TRI_UV_SCALAR=1, read once per
    process) give the same flags bit for bit, and the kernel log shows that each leg ran its own pair."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    digests, kernels = [], []
    for scalar in ("0", "1"):
        env = dict(os.environ)
        env["TRI_UV_SCALAR"] = scalar
        p = subprocess.run([sys.executable, "-c", UV_AB_SCRIPT % ROOT], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        digests.append([l for l in p.stdout.splitlines() if l.startswith("DIGEST")][0])
        kernels.append([l for l in p.stdout.splitlines() if l.startswith("KERNELS")][0].split()[1:])
    assert digests[0] == digests[1], digests
    assert "k_uv_resid4" in kernels[0] and "k_uv_apply4" in kernels[0] and "k_uv_resid" not in kernels[0] and "k_uv_apply" not in kernels[0], kernels
    assert "k_uv_resid" in kernels[1] and "k_uv_apply" in kernels[1] and "k_uv_resid4" not in kernels[1] and "k_uv_apply4" not in kernels[1], kernels
