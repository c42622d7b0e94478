"""What tests/test_boxfilter_instances_gpu.py takes for granted, checked without a GPU: the dispatcher limits it copies are
those of the sources, each case lands where its comment says by the dispatchers' own rules, and the oracle's flags of every
flagger case are neither all set nor all clear."""
import os
import re

import pytest

import test_boxfilter_instances_gpu as m
from test_route_ledger import CSRC, host_text


def _hip():
    """tricolour_amd.hip with its host files (boxfilter_host.hpp among them) spliced in."""
    return host_text()


def _define(text, name):
    found = re.findall(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


def test_the_copied_limits_are_the_sources():
    from tricolour_amd import _lib
    hip = _hip()
    assert m.TRI_EUNSUPPORTED == _lib.TRI_EUNSUPPORTED
    for name in ("LANE4_R_MAX", "BOXX_MIN_R", "BOXR_MAX_LDS_SLOTS"):
        assert getattr(m, name) == _define(hip, name), name
    with open(os.path.join(CSRC, "kernels_boxexact.hpp"), encoding="utf-8") as fh:
        assert m.BOXX_AMAX == _define(fh.read(), "BOXX_AMAX")
    # boxr_pick_ks: the radius limit and the largest ring; the spectrum pipeline's limit and its LDS budget
    assert "rad < 4 || rad > %d) return 0;" % m.BOXR_R_MAX in hip and "2 * rad >= 80 ? 80 :" in hip
    assert "boxp_pick_block(b, rad, C) > 0 && rad <= %d &&" % m.BOXR_R_MAX in hip
    assert "boxp_lds_bytes(rad, 16) <= 160 * 1024" in hip and "boxp_lds_bytes(rad, 8) <= 160 * 1024" in hip
    with open(os.path.join(CSRC, "kernels_boxpipe.hpp"), encoding="utf-8") as fh:
        pipe = fh.read()
    assert "boxp_lc(int r, int B) { return (2 * r + 2 * B + B - 1) / B * B; }" in pipe
    assert "return ((size_t)4 * (boxp_lc(r, B) + B) * 64 + (size_t)2 * B * 64) * 4;" in pipe
    # byte flags of a medium radius: the LDS kernel up to r = 40, the multi-pass kernel beyond
    assert "bt = rad <= 20 ? 128 : (rad <= 40 ? 64 : 0);" in hip
    # the candidates of the exact row filter, in the order boxx_pick_l tries them, and its rule for the 128-thread ones
    cands = re.search(r"using BoxxCodes = Ints<(.*?)>;", hip).group(1)
    assert [tuple(map(int, c)) for c in re.findall(r"(\d+) << 8 \| (\d+)", cands)] == m.BOXX_CANDS
    assert len(cands.split(",")) == len(m.BOXX_CANDS)
    assert "return first_of(BoxxCodes{}, [&](int c) {" in hip and "const int nti = c >> 8, l = c & 255;" in hip
    assert "if (nti == 128 && (P <= 128 * 17 || rad < 64)) return false;" in hip
    assert "return rad <= 128 || rad == 166 || rad == 221 || rad == 277 || rad == 397 || rad == 795;" in hip
    # the hook refuses the multi-pass family
    assert "b.unpadded = true;" in hip and "b.unpadded ? ColFamily::MultiPassUnpadded : ColFamily::MultiPass" in hip
    assert (m.ring_r_max(), m.pipe_r_max(16), m.pipe_r_max(8)) == (70, 48, 64)
    assert m.REFUSED == {"time[r=161]"} | {"spectrum[r=%d]" % r for r in (71, 107, 108, 160, 161)}
    assert {107, 108, 160, 161} <= set(m.RADII_TIME) and set(m.RADII_TIME) <= set(m.RADII_SPEC) and m.RADII_FREQ == m.RADII_TIME


def test_exact_row_cases_pick_their_candidate():
    table = dict(m.BOXX_HOOK, **m.BOXX_FORCED_256)
    assert len(table) == 2 * len(m.BOXX_CANDS)
    for frag, (r, n) in table.items():
        picked = m.boxx_pick(r, n, 256 if frag in m.BOXX_FORCED_256 else 0)
        assert picked and frag == "k_boxx<%d, %d, 1, %s>" % (picked + ("true" if m.boxx_recip(r) else "false",)), (frag, r, n, picked)
        assert r >= m.BOXX_MIN_R
    # without the switch no line length gives <256, 19, *, false>
    assert not any(m.boxx_pick(r, n) == (256, 19) for r in range(129, 400) if not m.boxx_recip(r) for n in range(4, 6400, 4))


def test_final_case_conditions():
    """The numbers the final-pass cases were derived from."""
    for name, case in m.FINAL_CASES.items():
        kw = m.final_kwargs(name)
        assert m.box_radius(kw["spike_width_freq"]) == case["r1"], name
        nbl, ncorr, T, F = case["shape"]
        assert nbl * ncorr <= 2 and ncorr * -(-T // 32) < 2048, name
    assert len(m.final_envs()) - 1 <= 3 and m.final_envs()[0] == {}
    assert set(m.CASES) == {"%s[r=%d]" % (s, r) for s, radii in (("time", m.RADII_TIME), ("frequency", m.RADII_FREQ), ("spectrum", m.RADII_SPEC))
                            for r in radii} | {"exact[%s]" % f for f in m.BOXX_HOOK} | {"final[%s]" % n for n in m.FINAL_CASES}


@pytest.mark.parametrize("name", list(m.FINAL_CASES))
def test_the_oracle_flags_of_a_final_case_are_not_trivial(oracle, name):
    assert oracle.box_radius(m.final_kwargs(name)["spike_width_freq"]) == m.FINAL_CASES[name]["r1"]
    exp, _ = m.final_expected(oracle, name)
    assert 0 < exp.mean() < 1, exp.mean()
