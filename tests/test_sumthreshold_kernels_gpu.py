"""Every SumThreshold kernel over chunked lines against the host reference of tests/test_sumthreshold_cases.py.

tri_test_sumthreshold launches one kernel form (variant 1 k_colst_dyn, 2 k_colst_fused, 3 k_colst_mask on rows, 4
k_colst_pipe, 5 k_colst_mask on column panels) over G chunks per line, with a MAD per (image, column, chunk).  Every case
of the table in test_sumthreshold_cases (line lengths 8 .. 96, chunk layouts down to one-sample and empty chunks, column
counts around the block sizes, window lists on either side of the stage pipeline's lag formula; columns of noise, runs
at a window's threshold, exact ties and their twins one ulp above, clamped spikes, dense runs, zero and NaN MADs,
non-finite samples, subnormal and huge amplitudes) runs on every variant that accepts it.  Each call must

  * equal the reference on every sample a chunk covers (the flags are bit-exact by contract: equality, no tolerance),
  * leave the sentinel outside the chunks,
  * leave the sentinel in the image before and the image behind the n_win it was handed (n_win + 2 are allocated),
  * launch exactly the kernel its variant names, once.

The closing test holds the SumThreshold rows of the ledger (test_route_ledger.ST_KERNELS): every listed instantiation
appeared in the kernel log of a call that equalled the reference, and the comparisons made per variant are the number
the case table implies -- nothing was left out on the device.
"""
import ctypes as C

import numpy as np
import pytest

from test_route_ledger import ST_KERNELS, matches, symbol_instances
from test_sumthreshold_cases import (CASES, FAMILIES, SENTINEL, accepts, cases_of, comparisons_per_variant, make_case,
                                     reference_of)

pytestmark = pytest.mark.gpu

KERNEL_OF = {1: "k_colst_dyn", 2: "k_colst_fused<1, 2, 4, 8>", 3: "k_colst_mask<1, 2, 4, 8, false>", 4: "k_colst_pipe",
             5: "k_colst_mask<1, 2, 4, 8, true>"}
TRI_EINVAL, TRI_EUNSUPPORTED = 1, 2


def call_hook(data, mad, out, case, variant, ends=None, windows=None):
    """(rc, kernel log) of one tri_test_sumthreshold call on device tensors; `out` is (n_win + 2, L, C), the call is handed
    its second image."""
    import torch
    from tricolour_amd import _lib
    windows = case["windows"] if windows is None else windows
    ends = case["ends"] if ends is None else ends
    n_win, L, Cn = data.shape
    warr = (C.c_int64 * len(windows))(*windows)
    earr = (C.c_int64 * len(ends))(*ends)
    ms = C.c_float(0)
    _lib.kernel_log_begin()
    rc = _lib.lib().tri_test_sumthreshold(data.data_ptr(), mad.data_ptr(), out[1].data_ptr(), n_win, L, Cn, warr, len(windows),
                                          case["nsigma"], case["rho"], variant, 1, C.byref(ms), None, earr, len(ends))
    torch.cuda.synchronize()
    return rc, _lib.kernel_log_end()


class Proof:
    """What the calls of this module have shown so far: per family the mismatches, per variant the comparisons made,
    and the kernels whose calls equalled the reference."""

    def __init__(self):
        self.reports, self.compared, self.refused, self.met = {}, {}, {}, {}

    def ensure(self, fam):
        if fam in self.reports:
            return
        import torch
        from tricolour_amd import _lib
        bad = self.reports.setdefault(fam, [])
        for name in cases_of(fam):
            made = make_case(name)
            case = made["case"]
            n_win, L, Cn = made["data"].shape
            want = np.full((n_win + 2, L, Cn), SENTINEL, np.uint8)
            want[1:-1] = reference_of(made)[0]
            data = torch.tensor(made["data"], device="cuda")
            mad = torch.tensor(made["mad"], device="cuda")
            for variant in case["variants"]:
                try:
                    out = torch.full((n_win + 2, L, Cn), SENTINEL, dtype=torch.uint8, device="cuda")
                    rc, log = call_hook(data, mad, out, case, variant)
                    got = out.cpu().numpy()
                except RuntimeError as err:                  # a device fault: no further launch
                    pytest.exit("%s variant %d: %s -- nothing more is started on this device" % (name, variant, err), returncode=3)
                if variant in case["refused"]:
                    if rc != TRI_EUNSUPPORTED or log:
                        bad.append("%s variant %d: rc %d, launched %s where the hook has to refuse" % (name, variant, rc, log))
                    self.refused[variant] = self.refused.get(variant, 0) + 1
                    continue
                if rc:
                    msg = _lib.lib().tri_last_error().decode("utf-8", "replace")
                    if rc not in (TRI_EINVAL, TRI_EUNSUPPORTED):
                        pytest.exit("%s variant %d: %s -- nothing more is started on this device" % (name, variant, msg), returncode=3)
                    bad.append("%s variant %d: refused (%s)" % (name, variant, msg))
                    continue
                self.compared[variant] = self.compared.get(variant, 0) + 1
                if log != {KERNEL_OF[variant]: 1}:
                    bad.append("%s variant %d: launched %s" % (name, variant, log))
                elif not np.array_equal(got, want):
                    diff = np.argwhere(got != want)
                    i, l, c = diff[0]
                    where = "guard image" if i in (0, n_win + 1) else "kind %s" % made["kinds"][i - 1, c]
                    bad.append("%s variant %d: %d bytes differ, first at image %d line %d column %d (%s): %d for %d" % (
                        name, variant, len(diff), i - 1, l, c, where, got[i, l, c], want[i, l, c]))
                else:
                    self.met[KERNEL_OF[variant]] = self.met.get(KERNEL_OF[variant], 0) + 1


@pytest.fixture(scope="module")
def proof(gpu):
    return Proof()


@pytest.mark.parametrize("fam", FAMILIES)
def test_kernels_equal_the_reference(proof, fam):
    proof.ensure(fam)
    bad = proof.reports[fam]
    assert not bad, "%d calls of %s failed:\n  %s" % (len(bad), fam, "\n  ".join(bad[:12]))


def _tensors(name):
    import torch
    made = make_case(name)
    n_win, L, Cn = made["data"].shape
    return (made, torch.tensor(made["data"], device="cuda"), torch.tensor(made["mad"], device="cuda"),
            lambda: torch.full((n_win + 2, L, Cn), SENTINEL, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("name", ["layout[halves, L=96, rho=1.3]", "windows[32,48,64,128, L=300, thirds]", "sweep[L=96, C=64, rho=1.3]",
                                  "sweep[L=96, C=70, rho=1.3]", "windows[32,48,64,128, L=300, one]"])
def test_chunked_hook_dispatch(gpu, name):
    """Which kernel each tri_test_sumthreshold variant launches (kernel log), with two chunks and with one: variant 0
    picks what the flagger would -- the row form of the lane-mask cascade as soon as there are chunks, the stage pipeline
    for a list it takes -- and the panel form is refused with chunks."""
    made, data, mad, fresh = _tensors(name)
    case = made["case"]
    G, fusable = len(case["ends"]) - 1, case["windows"] == (1, 2, 4, 8)
    panel = fusable and G == 1 and case["C"] % 64 == 0
    want = {0: (KERNEL_OF[5] if panel else KERNEL_OF[3]) if fusable else KERNEL_OF[4],
            1: KERNEL_OF[1], 2: KERNEL_OF[2] if fusable else None, 3: KERNEL_OF[3] if fusable else None, 4: KERNEL_OF[4],
            5: KERNEL_OF[5] if panel else None}
    ref = reference_of(made)[0]
    got = {}
    for variant in range(6):
        out = fresh()
        rc, log = call_hook(data, mad, out, case, variant)
        assert rc in (0, TRI_EUNSUPPORTED), (variant, rc)
        got[variant] = None if rc else log
        if rc:
            assert not log and (out == SENTINEL).all(), variant
        else:
            assert np.array_equal(out[1:-1].cpu().numpy(), ref), variant
    assert got == {v: None if k is None else {k: 1} for v, k in want.items()}
    assert all((want[v] is not None) == accepts(case, v) for v in range(1, 6))


def test_the_panel_form_is_refused_with_chunks(gpu):
    """64 columns and windows (1, 2, 4, 8): with one chunk variant 0 is the panel form, with two it is the row form of
    the lane-mask cascade, and variant 5 is TRI_EUNSUPPORTED without a launch."""
    import torch
    made, data, _, fresh = _tensors("sweep[L=96, C=64, rho=1.3]")
    case = made["case"]
    mad = torch.ones((data.shape[0], data.shape[2], 2), dtype=torch.float64, device="cuda")
    out = fresh()
    assert call_hook(data, mad, out, case, 5, ends=[0, 48, 96]) == (TRI_EUNSUPPORTED, {}) and (out == SENTINEL).all()
    assert call_hook(data, mad, fresh(), case, 0, ends=[0, 48, 96]) == (0, {KERNEL_OF[3]: 1})
    assert call_hook(data, mad[:, :, :1].contiguous(), fresh(), case, 0, ends=[0, 96]) == (0, {KERNEL_OF[5]: 1})
    # one chunk short of the line: the panel form leaves the rows outside it alone
    out = fresh()
    assert call_hook(data, mad[:, :, :1].contiguous(), out, case, 5, ends=[3, 93]) == (0, {KERNEL_OF[5]: 1})
    got = out.cpu().numpy()
    assert (got[:, :3] == SENTINEL).all() and (got[:, 93:] == SENTINEL).all() and (got[1:-1, 3:93] <= 1).all()


def test_bad_chunk_ends_are_refused_without_a_launch(gpu):
    """Ends that decrease or leave [0, n_line] and counts outside 2 .. 256 are TRI_EINVAL before anything is launched;
    256 ends with empty chunks among them are taken."""
    import torch
    made, data, _, fresh = _tensors("layout[halves, L=96, rho=1.3]")
    case = made["case"]
    L = case["L"]
    mad = torch.ones((data.shape[0], data.shape[2], 256), dtype=torch.float64, device="cuda")      # (room for any G below)
    for ends in ([0, 50, 48], [0, 48, 97], [-1, 48, 96], [0], [48, 48, 47], list(range(0, 96)) + [96] * 161):
        for variant in (0, 1, 3, 4):
            out = fresh()
            rc, log = call_hook(data, mad, out, case, variant, ends=ends)
            assert rc == TRI_EINVAL and not log and (out == SENTINEL).all(), (ends[:4], len(ends), variant, rc, log)
    ends = sorted(list(range(0, L + 1)) * 3)[:255] + [L]
    assert len(ends) == 256 and ends[0] == 0
    out = fresh()
    rc, log = call_hook(data, mad[:, :, :255].contiguous(), out, case, 3, ends=ends)
    assert rc == 0 and log == {KERNEL_OF[3]: 1}
    got = out.cpu().numpy()
    assert (got[[0, -1]] == SENTINEL).all() and (got[1:-1] <= 1).all()


def test_every_listed_sumthreshold_instantiation_met_the_reference(proof):
    """Every instantiation the SumThreshold rows of the ledger list was launched by calls of this module that equalled
    the reference (families no selected test has asked for yet run now), nothing else of these kernels was launched, and
    per variant exactly the comparisons the case table implies were made: no case was skipped on the device but the one
    the hook documents as unsupported (nine windows on the stage pipeline), which was refused."""
    for fam in FAMILIES:
        proof.ensure(fam)
    failed = {f: len(r) for f, r in proof.reports.items() if r}
    print("comparisons per variant: %s; refused: %s; %d cases" % (sorted(proof.compared.items()), sorted(proof.refused.items()), len(CASES)))
    assert proof.compared == comparisons_per_variant(), (proof.compared, comparisons_per_variant(), failed)
    assert proof.refused == {4: 1}, proof.refused
    listed = [f for k in ST_KERNELS for f in symbol_instances(k, reachable_only=True)]
    assert sorted(listed) == sorted(KERNEL_OF.values())
    unmet = [f for f in listed if not proof.met.get(f)]
    assert not unmet, "no call that equalled the reference launched %s\nfailed calls per family: %s" % (unmet, failed)
    # a kernel counts when every call of its variant equalled the reference, not just one
    short = {KERNEL_OF[v]: (proof.met.get(KERNEL_OF[v], 0), n) for v, n in comparisons_per_variant().items() if proof.met.get(KERNEL_OF[v], 0) != n}
    assert not short and not failed, "calls that equalled the reference, of those made: %s; failed calls per family: %s" % (short, failed)
    stray = sorted(m for m in proof.met if not any(matches(k, m) for k in ST_KERNELS))
    assert not stray, stray
