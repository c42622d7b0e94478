"""The independent launch pairs inside a major iteration on two streams: same results, same kernels, ordered towards the caller.

A call on one stream gets a side lane (one more stream, a fork and a join event per calling thread).  The weight image of
the time stage (k_boxw) then runs beside the data image's kernel, and the time medians of the residual beside its
transpose.  TRI_SUBSTREAMS=0 takes the side lane away: the single-stream order.  What is held here:

  results     bit-equal to the oracle with the forks active, on the golden stage-1 cases and on a random case whose time
              radii 54 / 43 / 32 / 21 / 10 put k_boxq_deep<96, 1>, k_boxq<80, 1, 8>, k_boxq<64, 1, 8>, k_boxt<32, true, 1> and
              k_boxt<20, false, 1> each beside a k_boxw (the kernel log says that they ran)
  the switch  TRI_SUBSTREAMS=0 changes neither a flag nor the kernel log
  ordering    a consumer queued on the caller's stream without a synchronisation sees the finished result; two calls in a
              row through one workspace; two host threads with a stream each
  scratch     the result does not depend on what the workspace held
  the hook    tri_bench_boxfilter goes through the same fork

CASE is (3, 1, 128, 256): three windows, lines longer than every filter (2r + 1 = 109 at most), more than one block of 64
columns, one oracle run per seed, shared by the tests.
"""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import scratch_poison
from conftest import load_golden

pytestmark = pytest.mark.gpu

SHAPE = (3, 1, 128, 256)
STAGE1 = load_golden("G2_stage1.npz")[1]
_CASES, _EXPECTED = {}, {}


def case(seed):
    """Random visibilities with a few loud channels, rows and samples, 2 % of the channels pre-flagged, a few NaNs."""
    if seed not in _CASES:
        rs = np.random.RandomState(4100 + seed)
        vis = (rs.standard_normal(SHAPE) + 1j * rs.standard_normal(SHAPE)).astype(np.complex64)
        vis[..., rs.choice(SHAPE[3], 5, replace=False)] *= 9.0
        vis[1, 0, 40 + seed] *= 6.0
        vis[rs.uniform(size=SHAPE) < 0.002] *= 30.0
        flags = np.zeros(SHAPE, np.bool_)
        flags[..., rs.uniform(size=SHAPE[3]) < 0.02] = True
        for idx in ((0, 0, 5, 17), (2, 0, 100, 200), (1, 0, 64, 3 + seed)):
            vis[idx] = np.nan
        _CASES[seed] = (vis, flags)
    return _CASES[seed]


def expected(oracle, seed):
    if seed not in _EXPECTED:
        vis, flags = case(seed)
        exp = oracle.sum_threshold_flagger(vis, flags, **STAGE1)
        assert 0 < exp.mean() < 1
        exp.setflags(write=False)
        _EXPECTED[seed] = exp
    return _EXPECTED[seed]


def on_device(seed):
    import torch
    vis, flags = case(seed)
    return torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()


def logged_call(gpu, vd, fd):
    """(host flags, kernel log) of one call on device inputs."""
    import torch
    from tricolour_amd import _lib
    _lib.kernel_log_begin()
    try:
        out = gpu.sum_threshold_flagger(vd, fd, **STAGE1)
    finally:
        log = _lib.kernel_log_end()
    torch.cuda.synchronize()
    return out.cpu().numpy(), log


def launches(log, kernel):
    """{instantiation: launches} of the log's rows of `kernel`."""
    return {k: n for k, n in log.items() if k == kernel or k.startswith(kernel + "<")}


class substreams:
    """TRI_SUBSTREAMS set to `value` (None: unset) inside the block, as found afterwards."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("TRI_SUBSTREAMS")
        if self.value is None:
            os.environ.pop("TRI_SUBSTREAMS", None)
        else:
            os.environ["TRI_SUBSTREAMS"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("TRI_SUBSTREAMS", None)
        else:
            os.environ["TRI_SUBSTREAMS"] = self.old


@pytest.mark.parametrize("name", ["G2_stage1.npz", "G2b_radius32.npz"])
def test_golden_stage1_cases_equal_the_oracle(gpu, oracle, name):
    d, kw = load_golden(name)
    with substreams(None):
        out = gpu.sum_threshold_flagger(d["vis"], d["flags"], **kw)
    exp = oracle.sum_threshold_flagger(d["vis"], d["flags"], **kw)
    assert np.array_equal(out, exp), "%d of %d flags differ from the oracle" % ((out != exp).sum(), exp.size)


def test_every_time_stage_pair_equals_the_oracle(gpu, oracle):
    exp = expected(oracle, 0)
    with substreams(None):
        out, log = logged_call(gpu, *on_device(0))
    # the route forks: the integer weight kernel ran beside every kind of data-image kernel
    boxw, boxq, deep, boxt = (launches(log, k) for k in ("k_boxw", "k_boxq", "k_boxq_deep", "k_boxt"))
    assert set(boxw) == {"k_boxw<%d>" % (2 * r) for r in (54, 43, 32, 21, 10)}, log
    assert set(deep) == {"k_boxq_deep<96, 1>"} and set(boxq) == {"k_boxq<80, 1, 8>", "k_boxq<64, 1, 8>"}, log
    assert set(boxt) == {"k_boxt<32, true, 1>", "k_boxt<20, false, 1>"}, log
    assert sum(boxw.values()) == sum(boxq.values()) + sum(deep.values()) + sum(boxt.values())
    assert np.array_equal(out, exp), "%d of %d flags differ from the oracle" % ((out != exp).sum(), exp.size)


def test_single_stream_switch_changes_neither_flags_nor_kernels(gpu, oracle):
    vd, fd = on_device(0)
    with substreams(None):
        out, log = logged_call(gpu, vd, fd)
    before = os.environ.get("TRI_SUBSTREAMS")
    with substreams("0"):
        out0, log0 = logged_call(gpu, vd, fd)
    assert os.environ.get("TRI_SUBSTREAMS") == before
    assert log0 == log, "kernels or counts differ: %s" % sorted(set(log0.items()) ^ set(log.items()))
    assert np.array_equal(out0, out)
    assert np.array_equal(out0, expected(oracle, 0))


def test_result_is_ordered_towards_the_callers_stream(gpu, oracle):
    """A non-default stream, a consumer queued behind each call without a synchronisation, two calls with different inputs
    through the same workspace: side work of call 1 is over when its consumer, and call 2, start."""
    import torch
    from tricolour_amd import flagging
    exp = [expected(oracle, 0), expected(oracle, 1)]
    inputs = [on_device(0), on_device(1)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    consumed = []
    with substreams(None), torch.cuda.stream(s):
        flagging.release_workspace()
        for vd, fd in inputs:
            out = gpu.sum_threshold_flagger(vd, fd, **STAGE1)
            consumed.append(out.to(torch.uint8) + 0)              # queued on s behind the call
        held = {k: t.numel() for k, t in flagging._tls.ws.items()}
    s.synchronize()
    assert len(held) == 1, "both calls were to run in one workspace: %s" % (held,)
    for k, (got, want) in enumerate(zip(consumed, exp)):
        got = got.cpu().numpy().astype(np.bool_)
        assert np.array_equal(got, want), "call %d: %d of %d flags differ from the oracle" % (k + 1, (got != want).sum(), want.size)
    flagging.release_workspace()


def test_two_host_threads_with_a_stream_each(gpu, oracle):
    import torch
    from tricolour_amd import flagging
    exp = [expected(oracle, 0), expected(oracle, 1)]
    inputs = [on_device(0), on_device(1)]
    torch.cuda.synchronize()
    results, errors = {}, []

    def work(tid):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                outs = [gpu.sum_threshold_flagger(*inputs[(tid + k) % 2], **STAGE1) for k in range(3)]
            s.synchronize()
            results[tid] = [o.cpu().numpy() for o in outs]
            flagging.release_workspace()
        except BaseException as e:      # noqa: B902  (reported by the asserting thread)
            errors.append((tid, repr(e)))

    declared = flagging._declared_threads
    flagging.set_num_threads(2)
    try:
        with substreams(None):
            threads = [threading.Thread(target=work, args=(tid,)) for tid in range(2)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
    finally:
        flagging._declared_threads = declared
    assert not errors, errors
    for tid in range(2):
        for k, got in enumerate(results[tid]):
            want = exp[(tid + k) % 2]
            assert np.array_equal(got, want), "thread %d, call %d: %d flags differ from the oracle" % (tid, k + 1, (got != want).sum())


def test_result_does_not_depend_on_stale_scratch(gpu, oracle):
    """The cached workspace filled with 0xFF, then holding the leavings of a call on other inputs: the forked kernels write
    disjoint images, and everything they read was written in the same call."""
    import torch
    from tricolour_amd import flagging
    vd, fd = on_device(0)
    other = on_device(1)
    with substreams(None):
        flagging.release_workspace()
        clean = gpu.sum_threshold_flagger(vd, fd, **STAGE1).cpu().numpy()
        torch.cuda.synchronize()
        cache = flagging._tls.ws
        assert len(cache) == 1
        for t in cache.values():
            t.fill_(scratch_poison.FILL["ones"])
        torch.cuda.synchronize()
        ones = gpu.sum_threshold_flagger(vd, fd, **STAGE1).cpu().numpy()
        gpu.sum_threshold_flagger(*other, **STAGE1)
        torch.cuda.synchronize()
        stale = gpu.sum_threshold_flagger(vd, fd, **STAGE1).cpu().numpy()
        assert len(flagging._tls.ws) == 1, "the calls were to run in one workspace"
    flagging.release_workspace()
    assert np.array_equal(clean, expected(oracle, 0))
    assert np.array_equal(ones, clean), "%d flags changed with a workspace of 0xFF" % (ones != clean).sum()
    assert np.array_equal(stale, clean), "%d flags changed with another call's leavings" % (stale != clean).sum()


def test_boxfilter_hook_times_the_forked_pair(gpu):
    """tri_bench_boxfilter, time stage at r = 54 on two windows of 128 x 256: a positive time, both kernels of the pair in
    the log, and the images of the single-stream order."""
    import torch
    from tricolour_amd import _lib
    w, n, c, radius = 2, 128, 256, 54
    rs = np.random.RandomState(54)
    data = torch.from_numpy((rs.standard_normal((w, n, c)) * 3 + 10).astype(np.float32)).cuda()
    fl = (rs.uniform(size=(w, n, c)) < 0.1).astype(np.uint8)
    f4 = torch.from_numpy(np.ascontiguousarray(fl.reshape(w, n // 4, 4, c).transpose(0, 1, 3, 2))).cuda()   # TF4 words

    def run():
        ow = torch.full((w, n, c), -7.0, dtype=torch.float32, device="cuda")
        oo = torch.full((w, n, c), -7.0, dtype=torch.float32, device="cuda")
        ms = C.c_float(0)
        _lib.kernel_log_begin()
        try:
            rc = _lib.lib().tri_bench_boxfilter(data.data_ptr(), f4.data_ptr(), ow.data_ptr(), oo.data_ptr(), w, n, c, radius,
                                                0, 0, 2, C.byref(ms), torch.cuda.current_stream().cuda_stream)
        finally:
            log = _lib.kernel_log_end()
        _lib.check(rc)
        torch.cuda.synchronize()
        return ms.value, log, ow.cpu().numpy(), oo.cpu().numpy()

    with substreams(None):
        ms, log, ow, oo = run()
    with substreams("0"):
        ms0, log0, ow0, oo0 = run()
    assert ms > 0 and ms0 > 0
    assert log.get("k_boxq_deep<96, 1>") == 2 and log.get("k_boxw<108>") == 2, log
    assert log0 == log
    assert np.array_equal(ow.view(np.uint32), ow0.view(np.uint32)) and np.array_equal(oo.view(np.uint32), oo0.view(np.uint32))
    assert not (ow == -7.0).any() and not (oo == -7.0).any()
