"""The ledger of route switches and kernels: which test runs each of them against a reference.

SWITCHES has one row per TRI_* name the library reads through getenv, KERNELS one row per __global__ kernel of
tricolour_amd/csrc.  The tests of this module (no GPU needed) hold the two tables to the sources: a switch or kernel
added, renamed or retired without a row fails here, and so does a script, test or document that sets a TRI_* name
nobody reads.  tests/test_route_matrix_gpu.py imports the tables and proves every row on the device: each `route`
switch changes the kernel log of its case as the row says and stays bit-equal to the oracle, and every `flagger`
kernel is launched by at least one oracle-checked call.

Row of SWITCHES
    cls      "route"      the switch replaces kernels: `legs` lists what must happen
             "geometry"   same kernel symbols, other launch geometry or arguments: the leg's case must launch `shapes`
             "schedule" / "print-only" / "elsewhere"   not in the matrix; `why` or `test` says where it is covered
    legs     [dict(env=..., base=..., cases={case: dict(gone=[...], new=[...], present=[...])})]
             env: the variables set (one child process per distinct env), base: the env the log is compared with
             (default: none set), gone: launched under base, not under env; new: the other way round; present:
             launched under env whatever base does.
A kernel-name fragment without '<' names a kernel whatever its template arguments ("k_reject4" is not "k_reject4_t");
with '<' it is a prefix of the instantiation ("k_median2<true, false, 16>").

Row of KERNELS
    "flagger" / "unlaunched" / "file.py::test"   as above and below
    dict(test="file.py::test", instances=[...])  the pack / unpack, scan and strategy-step kernels of the other entry
             points: `instances` lists every instantiation a launch site of the host code (tricolour_amd.hip and the
             step host files it includes: host_text) can produce, as fragments
             with their template arguments ("k_pack_v<2>", "k_pack_scan_v<4, true, false, true>"; the bare name for a
             kernel that is no template).  An entry dict(name="k_x<3>", unreachable="why") is an instantiation no public
             call can reach.  The scans below hold the lists to the launch sites, and
             tests/test_entry_kernels_gpu.py launches every reachable one in a call it compares with a host reference.
    dict(test=..., instances=[...], flagger=True)   the symbol-held rows (SYMBOL_KERNELS): the box-filter kernels
             (BOX_KERNELS) and the SumThreshold kernels (ST_KERNELS).  Launched by the flagger -- they count as `flagger`
             kernels for test_route_matrix_gpu.py (is_flagger) -- and listed by instantiation as well.  The box filters
             are launched from template functions behind with_constant() over the lists of boxfilter_host.hpp, which the
             launch-site scan cannot follow, so these rows are held to the symbol table of the built library instead (one weak
             __device_stub__ symbol per instantiation: test_box_rows_are_the_library_symbols);
             tests/test_boxfilter_instances_gpu.py launches every reachable box-filter instantiation in a call it compares
             with the oracle, tests/test_sumthreshold_kernels_gpu.py every SumThreshold one in calls over chunked lines
             that it compares with a numpy restatement of flagging.py:610-681.  Besides `unreachable`, an entry
             of the box-filter rows may be dict(name=..., switch="TRI_X"): reachable only
             under route switches that need a process of their own beyond the three that module starts (one entry:
             TRI_FILTER_DIRECT_FT acts under TRI_NO_PACKED_FLAGS=1 only); the leg of that switch in
             test_route_matrix_gpu.py, compared with the oracle, must then name exactly this instantiation as `new` or
             `present`.

Held to the launch sites (test_listed_instances_are_the_launch_sites): the pack / unpack, scan, strategy-step, Stokes and
window-count rows.  The uv-contsub rows and those of its multi-workgroup median (k_medbig_*) as well: every instantiation behind
tri_uvcontsub_flagger is met, stage by stage, by tests/test_uvcontsub_kernels_gpu.py (`also` names a second test that runs
the kernel against a reference).  Held to the symbol table: the rows of SYMBOL_KERNELS.  The open remainder: k_sir (152
instantiations), the segmented-median, rejection and line-RMS families keep rows by base name only.
"""
import glob
import itertools
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tricolour_amd", "csrc")


def _leg(env, cases, base=None):
    return dict(env=dict(env), base=dict(base or {}), cases=cases)


def _route(*legs):
    return dict(cls="route", legs=list(legs))


def _one(name, value, case, gone=(), new=(), present=()):
    return _route(_leg({name: value}, {case: dict(gone=list(gone), new=list(new), present=list(present))}))


_TILE_KERNELS = ["k_mr_predict", "k_mr_pass", "k_mr_finish"]

SWITCHES = {
    # ---- rejection of the 2-D background (background2d) ----
    "TRI_NO_TILE_MEDREJ": _route(_leg({"TRI_NO_TILE_MEDREJ": "1"}, {
        # K3t off where it is the default: the two-kernel route, and the flag copy its in-place read had made unnecessary
        "tile": dict(gone=_TILE_KERNELS + ["k_median_reject"], new=["k_median2", "k_reject4_t", "k_u8_op16<0>"], present=[]),
        # one block of 2^20 samples, four blocks in all: the sixteen-groups-in-flight form of the two-pass select
        "long_block": dict(gone=_TILE_KERNELS, new=["k_median2<true, false, 16>", "k_reject4_t"], present=[]),
    })),
    "TRI_FUSED_MEDREJ": _route(_leg({"TRI_FUSED_MEDREJ": "1"}, {
        # (the default tile route launches k_median_reject too, as its redo kernel: `present`, not `new`)
        "tile": dict(gone=_TILE_KERNELS, new=[], present=["k_median_reject"]),
        "blocks": dict(gone=["k_median2", "k_reject4_t"], new=["k_median_reject"], present=[]),
    })),
    "TRI_NO_FUSED_REJECT": _route(
        _leg({"TRI_NO_FUSED_REJECT": "1"}, {
            "tile": dict(gone=_TILE_KERNELS + ["k_median_reject"], new=["k_median2", "k_reject4"], present=[]),
            "blocks": dict(gone=["k_reject4_t"], new=["k_reject4"], present=["k_median2"]),
        }),
        _leg({"TRI_NO_FUSED_REJECT": "1", "TRI_NO_TILE_MEDREJ": "1"}, {
            "tile": dict(gone=_TILE_KERNELS + ["k_median_reject"], new=["k_median2", "k_reject4"], present=[]),
        }),
        _leg({"TRI_NO_FUSED_REJECT": "1", "TRI_FUSED_MEDREJ": "1"}, {
            "tile": dict(gone=_TILE_KERNELS + ["k_median_reject"], new=["k_median2", "k_reject4"], present=[]),
        })),
    "TRI_MEDREJ_FORCE_FALLBACK": _route(_leg({"TRI_MEDREJ_FORCE_FALLBACK": "1"}, {
        # blocks of 16384 samples: the switch alone turns the tile route on (every block then takes the redo kernel)
        "blocks": dict(gone=["k_median2", "k_reject4_t", "k_u8_op16<0>"], new=_TILE_KERNELS + ["k_median_reject"], present=[]),
        # (on the tile case the kernels are the same: the forced redo shows in tri_medrej_stats, see the GPU module)
    })),
    "TRI_MEDIAN_3PASS": _one("TRI_MEDIAN_3PASS", "1", "blocks", gone=["k_median2"], new=["k_median"]),
    "TRI_MEDIAN_NO_PREDICT": dict(cls="geometry", why="the same k_median2 instantiation, launched without its candidate scratch (arguments only)",
                                  legs=[_leg({"TRI_MEDIAN_NO_PREDICT": "1"}, {"blocks": dict(shapes=["k_median2"])})]),
    "TRI_MEDIAN_WAVE_OLD": _one("TRI_MEDIAN_WAVE_OLD", "1", "blocks", gone=["k_median_wave<8, true, 8>"], new=["k_median_wave<8, true, 1>"]),
    "TRI_BG_COPY_FLAGS": dict(cls="elsewhere", test="test_final_pass_routes_gpu.py::test_slab_final_pass_writes_the_panel_residual"),
    "TRI_NO_PACKED_FLAGS": _one("TRI_NO_PACKED_FLAGS", "1", "blocks", gone=["k_boxt", "k_boxw", "k_reject4_t", "k_colst_mask<1, 2, 4, 8, true>"],
                                new=["k_build_wo4", "k_reject4", "k_colfilter_lane4<1", "k_or_spec16"]),
    # ---- box filters ----
    "TRI_TIME_PREBUILD": _one("TRI_TIME_PREBUILD", "0", "unpacked", gone=["k_build_wo4"], new=["k_colfilter_lds<0"]),
    "TRI_FILTER_DIRECT_FT": _route(_leg({"TRI_NO_PACKED_FLAGS": "1", "TRI_FILTER_DIRECT_FT": "1"}, {
        # acts on unpacked flags with T % 4 == 0 only, which is TRI_NO_PACKED_FLAGS=1 (T % 4 == 0 packs otherwise): compared with that leg
        "blocks": dict(gone=["k_colfilter_lane4<1, true>", "k_boxqf"], new=["k_colfilter_lds<1, true, true>", "k_masked_div4<2>"], present=[]),
    }, base={"TRI_NO_PACKED_FLAGS": "1"})),
    "TRI_FILTER_MULTIPASS": _one("TRI_FILTER_MULTIPASS", "1", "blocks", gone=["k_boxt", "k_boxw"], new=["k_colfilter<0>"]),
    "TRI_FILTER_NO_LANE4": _one("TRI_FILTER_NO_LANE4", "1", "unpacked", gone=["k_colfilter_lane4"], present=["k_colfilter_lds<1"]),
    "TRI_FILTER_NO_REGRING": _one("TRI_FILTER_NO_REGRING", "1", "blocks", gone=["k_boxt", "k_boxw", "k_boxqf"],
                                  new=["k_colfilter_lane4<2", "k_colfilter_lds<2", "k_colfilter_lane4<3", "k_colfilter_lds_tf"]),
    "TRI_FILTER_NO_REGRING_F": _one("TRI_FILTER_NO_REGRING_F", "1", "blocks", gone=["k_boxqf"], new=["k_colfilter_lane4<3", "k_colfilter_lds_tf"],
                                    present=["k_boxt"]),
    "TRI_FILTER_NO_BOXW": _one("TRI_FILTER_NO_BOXW", "1", "blocks", gone=["k_boxw"], new=["k_boxt<32, true, 0>", "k_boxt<20, false, 0>"]),
    "TRI_SPEC_NO_PIPE": _one("TRI_SPEC_NO_PIPE", "1", "blocks", gone=["k_boxp_spec"], new=["k_boxt_spec"]),
    "TRI_FILTER_NO_PIPE_T": _one("TRI_FILTER_NO_PIPE_T", "1", "filters", gone=["k_boxq", "k_boxq_deep"], new=["k_boxt<80", "k_boxt<32"]),
    "TRI_FILTER_PIPE_T_B8": _one("TRI_FILTER_PIPE_T_B8", "0", "filters", gone=["k_boxq_deep", "k_boxq<56, 1, 8>"],
                                 new=["k_boxq<80, 1, 16>", "k_boxq<48, 1, 16>"]),
    "TRI_FILTER_NO_PIPE_F": _one("TRI_FILTER_NO_PIPE_F", "1", "filters", gone=["k_boxqf"], new=["k_boxf"]),
    "TRI_FILTER_PIPE_F_B8": _one("TRI_FILTER_PIPE_F_B8", "0", "filters", gone=["k_boxqf<56, 1, 8>", "k_boxqf<24, 2, 8>"],
                                 new=["k_boxqf<48, 1, 16>", "k_boxqf<16, 2, 16>"], present=["k_boxqf<80, 1, 16>"]),
    "TRI_FILTER_NO_TIN": _one("TRI_FILTER_NO_TIN", "1", "tiny", gone=["k_colfilter_lds_tf"], new=["k_colfilter_lds<1", "k_masked_div4<2>"]),
    "TRI_FILTER_NO_FUSED_DIV": _one("TRI_FILTER_NO_FUSED_DIV", "1", "tiny", gone=["k_colfilter_lds_tf"], new=["k_colfilter_lds_t", "k_masked_div4<2>"]),
    "TRI_FILTER_NO_EXACT": _one("TRI_FILTER_NO_EXACT", "1", "exact", gone=["k_boxx", "k_reject_tf"], new=["k_colfilter_lane4<3"]),
    "TRI_FILTER_NO_TF_REJECT": _one("TRI_FILTER_NO_TF_REJECT", "1", "exact", gone=["k_reject_tf", "k_median2<false, true"], new=["k_reject4_t"],
                                    present=["k_boxx"]),
    "TRI_BOXX_NTI": dict(cls="geometry", why="k_boxx with 256 instead of 128 threads per image (shorter chunks per lane)",
                         legs=[_leg({"TRI_BOXX_NTI": "256"}, {"exact": dict(shapes=["k_boxx"])})]),
    "TRI_BOXX_STATS": dict(cls="print-only", why="tri_bench_boxfilter prints the exact row filter's pass counts to stderr"),
    "TRI_INTERP_ONE_PASS": _one("TRI_INTERP_ONE_PASS", "1", "blocks", gone=["k_interp_scan", "k_interp_fix"], new=["k_colinterp"]),
    # ---- SumThreshold and the passes around it ----
    "TRI_ST_GENERIC": _one("TRI_ST_GENERIC", "1", "blocks", gone=["k_colst_mask"], new=["k_colst_pipe"]),
    "TRI_ST_REGISTER": _one("TRI_ST_REGISTER", "1", "blocks", gone=["k_colst_mask"], new=["k_colst_fused"]),
    "TRI_ST_NO_PIPE": _one("TRI_ST_NO_PIPE", "1", "st_pipe", gone=["k_colst_pipe"], new=["k_colst_dyn"]),
    "TRI_ST_NO_PANEL": _one("TRI_ST_NO_PANEL", "1", "blocks", gone=["k_colst_mask<1, 2, 4, 8, true>", "k_combine_dilate16<true>", "k_transpose<float, true>", "k_unpanel"],
                            # (the row form of k_colst_mask also serves the frequency axis and the spectra: launched either way)
                            new=["k_combine_dilate16<false>"], present=["k_colst_mask<1, 2, 4, 8, false>"]),
    "TRI_ST_BLK": dict(cls="geometry", why="the SumThreshold kernels with 64 instead of 256 columns per workgroup",
                       legs=[_leg({"TRI_ST_BLK": "64"}, {"blocks": dict(shapes=["k_colst_mask"])})]),
    "TRI_NO_FUSED_OR": _one("TRI_NO_FUSED_OR", "1", "blocks", gone=["k_colst_mask<1, 2, 4, 8, true>"], new=["k_or_spec_more16"],
                            present=["k_colst_mask<1, 2, 4, 8, false>"]),
    "TRI_NO_FUSED_DILATE": _one("TRI_NO_FUSED_DILATE", "1", "blocks", gone=["k_combine_dilate16"], new=["k_combine16", "k_unaverage16"]),
    "TRI_NO_FUSED_RESID_TF": dict(cls="elsewhere", test="test_final_pass_routes_gpu.py::test_slab_final_pass_writes_the_panel_residual"),
    "TRI_NO_FUSED_BEGIN": _one("TRI_NO_FUSED_BEGIN", "1", "blocks", gone=["k_transpose_u8w<true, true>"], new=["k_zero_flagged4"]),
    "TRI_NO_FT_SPEC_OR": _one("TRI_NO_FT_SPEC_OR", "1", "blocks", gone=["k_or_spec_ft16"], new=["k_or_spec16"]),
    "TRI_NO_AMPL_CACHE": _one("TRI_NO_AMPL_CACHE", "1", "blocks", gone=["k_amplitude4", "k_transpose_u8w<true, true>"], new=["k_prepare4"]),
    # ---- not in the matrix ----
    "TRI_SUBSTREAMS": dict(cls="schedule", why="two internal streams, the same kernels", test="test_gpu_parity.py::test_two_stream_schedule_vs_oracle"),
    "TRI_UV_SCALAR": dict(cls="elsewhere", test="test_uvcontsub.py::test_gpu_uvcontsub_vector_kernels_match_scalar"),
}

NOT_IN_MATRIX = {"TRI_SUBSTREAMS", "TRI_BOXX_STATS", "TRI_NO_FUSED_RESID_TF", "TRI_BG_COPY_FLAGS", "TRI_UV_SCALAR"}

_PARITY = "test_gpu_parity.py::"
_SCAN = "test_scan_gpu.py::"
_ROWS = "test_scan_stream_gpu.py::"
_UV = "test_uvcontsub.py::test_gpu_uvcontsub_agreement"
_LRMS = "test_line_rms.py::test_gpu_small_and_odd_shapes"
_MEDBIG = _PARITY + "test_median_kernels"
_ENTRY = "test_entry_kernels_gpu.py::test_every_listed_instantiation_met_a_host_reference"
UV_CLOSING = "test_uvcontsub_kernels_gpu.py::test_every_uvcontsub_instantiation_met_its_stage_references"
# the closing tests of the GPU modules that demand their own rows; rows that name any other test are demanded by _ENTRY's
CLOSING_TESTS = (_ENTRY, UV_CLOSING)

# the two macro-expanded launch families of the fused scan pack
SCAN_FAMILIES = {"k_pack_scan_v": "TRI_PACK_SCAN_V", "k_pack_scan_rows_v": "TRI_PACK_SCAN_ROWS_V"}


def _scan_family(kernel):
    return ["%s<%d, %s, %s, %s>" % ((kernel, nc) + tuple("true" if b else "false" for b in bits))
            for nc in (1, 2, 4) for bits in itertools.product((False, True), repeat=3)]


def _inst(test, *instances, also=None):
    row = dict(test=test, instances=list(instances))
    if also:
        row["also"] = also
    return row


_BOX = "test_boxfilter_instances_gpu.py::test_every_listed_box_instantiation_met_a_host_reference"


def _no(name, why):
    return dict(name=name, unreachable=why)


def _box(*instances):
    return dict(test=_BOX, instances=list(instances), flagger=True)


def _tf(b):
    return "true" if b else "false"


_NO_BOXW = ("launch_boxw runs behind boxw_usable() in the flagger's route only (the hook's named variants switch it off); at "
            "2r = 22 .. 30 that route is the LDS-ring kernel: boxr_pick_ks_t() takes 2r == 20 or 2r >= 32, the stage pipeline 2r >= BOXQ_MIN_2R = 56")
_NO_BOXT16 = "boxr_pick_ks_t() returns a ring size only for 2r >= 32 (32 slots or more) or 2r == 20 (20 slots)"
_NO_BOXT20 = "KS = 20 is picked at 2r == 20 only: the LDS part of the delay line is empty"
_NO_DIVIDE = "its only launch site always defers the division to k_masked_div (deferred_denom is never NULL there)"

# the box-filter families: every instantiation in the built library.  What picks each one:
BOX_ROWS = {
    # launch_boxw: 2r = 20 .. 110
    "k_boxw": _box(*[("k_boxw<%d>" % r2 if not 22 <= r2 <= 30 else _no("k_boxw<%d>" % r2, _NO_BOXW)) for r2 in range(20, 111, 2)]),
    # launch_boxt / launch_boxt_ks: <KS, LDS part present, image>
    "k_boxt": _box(*[_no("k_boxt<16, %s, %d>" % (_tf(l), i), _NO_BOXT16) for l in (False, True) for i in (0, 1)],
                   *["k_boxt<20, false, %d>" % i for i in (0, 1)], *[_no("k_boxt<20, true, %d>" % i, _NO_BOXT20) for i in (0, 1)],
                   *["k_boxt<%d, %s, %d>" % (ks, _tf(l), i) for ks in (32, 64, 80) for l in (False, True) for i in (0, 1)]),
    "k_boxt_spec": _box(*["k_boxt_spec<%d, %s>" % (ks, _tf(l)) for ks in (8, 16, 32, 64, 80) for l in (False, True)]),
    "k_boxp_spec": _box("k_boxp_spec<16, 16>", "k_boxp_spec<8, 16>"),
    # launch_boxq: <KS, image, block>
    "k_boxq": _box(*["k_boxq<%d, %d, 8>" % (ks, i) for ks in (32, 40, 48, 56, 64, 80) for i in (0, 1)],
                   *["k_boxq<%d, %d, 16>" % (ks, i) for ks in (16, 32, 48, 64, 80, 96) for i in (0, 1)]),
    "k_boxq_deep": _box(*["k_boxq_deep<%d, %d>" % (ks, i) for ks in (80, 96) for i in (0, 1)]),
    # launch_boxf, the stage pipeline: <KS, MODE, block> (no <80, 2, 8>: it would spill)
    "k_boxqf": _box(*["k_boxqf<%d, %d, 8>" % (ks, m) for ks in (16, 24, 32, 40, 48, 56, 64, 72) for m in (1, 2)], "k_boxqf<80, 1, 8>",
                    *["k_boxqf<%d, %d, 16>" % (ks, m) for ks in (16, 32, 48, 64, 80, 96) for m in (1, 2)]),
    # launch_boxf_ks: <KS, LDS part present, MODE, waves per SIMD> (KS = 32 with more than 14 LDS slots: one wave)
    "k_boxf": _box(*["k_boxf<%d, %s, %d, %d>" % (ks, _tf(l), m, 1 if ks >= 64 else 2) for ks in (8, 16, 32, 64, 80) for l in (False, True) for m in (1, 2)],
                   "k_boxf<32, true, 1, 1>", "k_boxf<32, true, 2, 1>"),
    # launch_boxx: <threads per image, chunk, MODE, verified reciprocal>
    # (<256, 19, *, false> under TRI_BOXX_NTI=256 only: r > 128 implies r >= 64, where the 128-thread candidates come first)
    "k_boxx": _box(*["k_boxx<%d, %d, %d, %s>" % (nti, l, m, _tf(rc)) for nti, l in ((128, 37), (128, 41), (256, 17), (256, 19), (256, 21), (256, 25)) for m in (1, 2) for rc in (True, False)]),
    "k_colfilter": _box("k_colfilter<0>", "k_colfilter<1>"),
    # <source (0 byte flags, 1 float images, 2 packed flags), divides itself, transposed output>
    "k_colfilter_lds": _box("k_colfilter_lds<0, true, false>", "k_colfilter_lds<1, true, false>", "k_colfilter_lds<1, false, false>",
                            dict(name="k_colfilter_lds<1, true, true>", switch="TRI_FILTER_DIRECT_FT"),
                            "k_colfilter_lds<2, true, false>", "k_colfilter_lds<2, false, false>"),
    "k_colfilter_lds_t": _box("k_colfilter_lds_t<false>", _no("k_colfilter_lds_t<true>", _NO_DIVIDE)),
    "k_colfilter_lds_tf": _box("k_colfilter_lds_tf<1>", "k_colfilter_lds_tf<2>"),
    # <source (3: the time stage's TF images), divides itself>
    "k_colfilter_lane4": _box(_no("k_colfilter_lane4<0, true>", "byte flags have no lane-per-stage kernel (launch_colfilter): only its LDS opt-in names it"),
                              "k_colfilter_lane4<1, true>", "k_colfilter_lane4<1, false>", "k_colfilter_lane4<2, true>", "k_colfilter_lane4<2, false>",
                              "k_colfilter_lane4<3, false>", _no("k_colfilter_lane4<3, true>", _NO_DIVIDE)),
}
BOX_KERNELS = tuple(BOX_ROWS)

_ST = "test_sumthreshold_kernels_gpu.py::test_every_listed_sumthreshold_instantiation_met_the_reference"


def _st(*instances):
    return dict(test=_ST, instances=list(instances), flagger=True)


# the SumThreshold family (st_launch): the two cascades exist for windows (1, 2, 4, 8) only, the lane-mask one on rows
# and on 64-column panels
ST_ROWS = {
    "k_colst_dyn": _st("k_colst_dyn"), "k_colst_pipe": _st("k_colst_pipe"), "k_colst_fused": _st("k_colst_fused<1, 2, 4, 8>"),
    "k_colst_mask": _st("k_colst_mask<1, 2, 4, 8, false>", "k_colst_mask<1, 2, 4, 8, true>"),
}
ST_KERNELS = tuple(ST_ROWS)
# the rows held to the symbol table of the built library
SYMBOL_KERNELS = BOX_KERNELS + ST_KERNELS

# "flagger": launched by sum_threshold_flagger on some route -- test_route_matrix_gpu.py must see it in an oracle-checked log
KERNELS = {
    # kernels_boxexact / boxfilter / boxline / boxpipe / boxweight: BOX_ROWS below (listed by instantiation)
    # kernels_elementwise: the flagger's passes
    "k_prepare": "flagger", "k_transpose": "flagger", "k_unpanel": "flagger", "k_transpose_u8w": "flagger",
    "k_build_wo": "flagger", "k_build_wo4": "flagger", "k_masked_div": "flagger", "k_reject": "flagger",
    "k_colinterp": "flagger", "k_interp_scan": "flagger", "k_interp_fix": "flagger", "k_sub": "flagger", "k_or": "flagger",
    "k_copy_u8": "flagger", "k_or_spec": "flagger", "k_combine": "flagger", "k_unaverage": "flagger", "k_final": "flagger",
    "k_prepare4": "flagger", "k_amplitude4": "flagger", "k_zero_flagged4": "flagger", "k_u8_op16": "flagger",
    "k_spec_rows": "flagger", "k_or_spec16": "flagger", "k_or_spec_more16": "flagger", "k_or_spec_ft16": "flagger",
    "k_combine16": "flagger", "k_combine_dilate16": "flagger", "k_unaverage16": "flagger", "k_colcount": "flagger",
    "k_final16": "flagger", "k_masked_div4": "flagger", "k_sub4": "flagger", "k_reject4_t": "flagger",
    "k_reject_tf": "flagger", "k_reject4": "flagger",
    # ... and the kernels of the other entry points
    "k_abs_c64": _PARITY + "test_hypotf_kat",
    "k_panelize": _PARITY + "test_fused_sumthreshold_kernel_vs_generic_and_oracle",
    "k_unpanel_w": _PARITY + "test_fused_sumthreshold_kernel_vs_generic_and_oracle",
    "k_fill_windows": _inst("test_packing.py::test_gpu_pack_flag_unpack", "k_fill_windows"),
    "k_pack": _inst(_ENTRY, "k_pack"), "k_pack_v": _inst(_ENTRY, "k_pack_v<1>", "k_pack_v<2>", "k_pack_v<4>"),
    "k_unpack_v": _inst(_ENTRY, "k_unpack_v<1>", "k_unpack_v<2>", "k_unpack_v<4>"), "k_unpack": _inst(_ENTRY, "k_unpack"),
    # (the template argument is the TRI_VIS_* code: 0 complex64, 1 float32)
    "k_flag_nans_zeros": _inst(_ENTRY, "k_flag_nans_zeros<0>", "k_flag_nans_zeros<1>"),
    "k_apply_bl_chan_mask": _inst(_ENTRY, "k_apply_bl_chan_mask"),
    "k_uv_count": "unlaunched", "k_uv_diff": "unlaunched",
    "k_uv_mean": _inst(UV_CLOSING, "k_uv_mean", also=_UV), "k_uv_lowpass": _inst(UV_CLOSING, "k_uv_lowpass", also=_UV),
    "k_uv_resid": _inst(UV_CLOSING, "k_uv_resid", also=_UV), "k_uv_resid4": _inst(UV_CLOSING, "k_uv_resid4", also=_UV),
    "k_uv_apply": _inst(UV_CLOSING, "k_uv_apply", also=_UV), "k_uv_apply4": _inst(UV_CLOSING, "k_uv_apply4", also=_UV),
    "k_window_counts": _inst("test_window_statistics.py::test_gpu_window_counts", "k_window_counts<true>", "k_window_counts<false>"),
    "k_stokes_intensity": _inst(_ENTRY, "k_stokes_intensity<float>", "k_stokes_intensity<double>"),
    # kernels_linerms
    "k_lrms_power": _LRMS, "k_lrms_combine": _LRMS, "k_lrms_decide": _LRMS, "k_lrms_apply": _LRMS,
    # kernels_median
    "k_median": "flagger", "k_median2": "flagger", "k_median_wave": "flagger", "k_spec_from_med": "flagger",
    # (the template argument: 16-byte loads; both forms with and without a centre in tests/test_uvcontsub_kernels_gpu.py)
    "k_medbig_range": _inst(UV_CLOSING, "k_medbig_range", also=_MEDBIG), "k_medbig_pick": _inst(UV_CLOSING, "k_medbig_pick", also=_MEDBIG),
    "k_medbig_hist": _inst(UV_CLOSING, "k_medbig_hist<true>", "k_medbig_hist<false>", also=_MEDBIG),
    "k_medbig_compact": _inst(UV_CLOSING, "k_medbig_compact<true>", "k_medbig_compact<false>", also=_MEDBIG),
    "k_medbig_select": _inst(UV_CLOSING, "k_medbig_select<true>", "k_medbig_select<false>", also=_MEDBIG),
    # kernels_reject / reject_tile
    "k_median_reject": "flagger", "k_mr_predict": "flagger", "k_mr_pass": "flagger", "k_mr_finish": "flagger",
    # kernels_scan
    # (NC in {1, 2, 4}) x STOKES x MODEL x FLAGS: the launch macros TRI_PACK_SCAN_V / TRI_PACK_SCAN_ROWS_V
    "k_pack_scan_v": _inst(_SCAN + "test_gpu_pack_scan_matches_unfused_kernels", *_scan_family("k_pack_scan_v")),
    "k_pack_scan": _inst(_SCAN + "test_gpu_pack_scan_matches_unfused_kernels", "k_pack_scan"),
    "k_unpack_scan": _inst(_SCAN + "test_gpu_unpack_scan_matches_numpy", "k_unpack_scan<4>", "k_unpack_scan<0>"),
    "k_pack_scan_rows_v": _inst(_ROWS + "test_gpu_pack_scan_rows_matches_pack_scan", *_scan_family("k_pack_scan_rows_v")),
    "k_pack_scan_rows": _inst(_ROWS + "test_gpu_pack_scan_rows_matches_pack_scan", "k_pack_scan_rows"),
    "k_unpack_scan_rows": _inst(_ROWS + "test_gpu_unpack_scan_rows_matches_unpack_scan", "k_unpack_scan_rows<4>", "k_unpack_scan_rows<0>"),
    # kernels_sir
    "k_sir": "test_sir.py::test_gpu_sir_small_and_odd_shapes",
    # kernels_sumthreshold: ST_ROWS (listed by instantiation)
    # tricolour_amd.hip
    "k_tables": "flagger", "k_gather_col_f32": "flagger", "k_gather_col_u8": "flagger", "k_normalise_flags": "flagger",
    "k_check_box_divide": _PARITY + "test_division_by_box_denominator",
}
KERNELS.update(BOX_ROWS)
KERNELS.update(ST_ROWS)


def matches(fragment, name):
    """Whether the demangled kernel name `name` (template arguments included) is the kernel `fragment` speaks of."""
    if "<" in fragment:
        return name.startswith(fragment)
    return name == fragment or name.startswith(fragment + "<")


def launches(log, fragment):
    return sum(n for name, n in log.items() if matches(fragment, name))


def base_name(name):
    return name.split("<", 1)[0]


def switch_legs(name):
    return SWITCHES[name].get("legs", [])


def named_test(where):
    """The test a KERNELS row names, or None ("flagger", "unlaunched")."""
    if isinstance(where, dict):
        return where["test"]
    return where if "::" in where else None


def is_flagger(kernel):
    """Whether sum_threshold_flagger launches the kernel on some route (the rows of SYMBOL_KERNELS say so in a field)."""
    where = KERNELS.get(kernel)
    return where == "flagger" or (isinstance(where, dict) and bool(where.get("flagger")))


def instance_rows():
    """{kernel: row} of the KERNELS rows held to the launch sites: those that list their instantiations, the box-filter
    and SumThreshold rows (held to the symbol table) apart."""
    return {k: w for k, w in KERNELS.items() if isinstance(w, dict) and not w.get("flagger")}


def symbol_instances(kernel, reachable_only=False):
    """The instantiations a row of SYMBOL_KERNELS lists (`switch` entries count as reachable)."""
    out = []
    for item in KERNELS[kernel]["instances"]:
        if not isinstance(item, dict):
            out.append(item)
        elif not (reachable_only and "unreachable" in item):
            out.append(item["name"])
    return out


def switch_met_instances():
    """{instantiation: switch} of the BOX_KERNELS entries the route matrix meets under a switch of its own."""
    return {item["name"]: item["switch"] for k in BOX_KERNELS for item in KERNELS[k]["instances"] if isinstance(item, dict) and "switch" in item}


def symbol_row_errors(symbols):
    """What differs between the rows of SYMBOL_KERNELS and a list of the library's kernel instantiations."""
    out = []
    for kernel in SYMBOL_KERNELS:
        listed, built = set(symbol_instances(kernel)), {n for n in symbols if base_name(n) == kernel}
        if listed != built:
            out.append("%s: in the library but not listed %s; listed but not in the library %s" % (kernel, sorted(built - listed), sorted(listed - built)))
    return out


def library_instances(path):
    """The kernel instantiations of a built library: one weak __device_stub__ symbol each, template arguments in the
    demangler's spelling."""
    for nm in ("nm", "/opt/rocm/llvm/bin/llvm-nm"):
        try:
            text = subprocess.run([nm, "-C", path], capture_output=True, text=True, check=True).stdout
            break
        except (OSError, subprocess.CalledProcessError):
            text = None
    assert text, "no nm to read %s with" % path
    return sorted(set(re.findall(r"__device_stub__(k_\w+(?:<[^()]*>)?)\(", text)))


def listed_instances(kernel, reachable_only=False):
    out = []
    for item in KERNELS[kernel]["instances"]:
        if isinstance(item, dict):
            if not reachable_only:
                out.append(item["name"])
        else:
            out.append(item)
    return out


def reachable_instances(closing=_ENTRY):
    """Every fragment the closing test `closing` of a GPU module has to meet: the rows that name it -- and, for
    tests/test_entry_kernels_gpu.py, also the rows that name a test which is no module's closing test."""
    assert closing in CLOSING_TESTS, closing
    mine = lambda row: row["test"] == closing or (closing == _ENTRY and row["test"] not in CLOSING_TESTS)
    return [f for k, row in sorted(instance_rows().items()) if mine(row) for f in listed_instances(k, reachable_only=True)]


# ---- the scans ----

def _sources(directory=CSRC):
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*"))):
        if os.path.isfile(path):
            with open(path, encoding="utf-8") as fh:
                out[path] = fh.read()
    return out


def host_text(directory=CSRC):
    """The host code: tricolour_amd.hip with the host files it includes (steps/step_host.hpp and one per step) spliced
    in at their include lines.  The kernel headers (kernels_*.hpp) and tri_common.hpp stay include lines."""
    def splice(m):
        name = m.group(1)
        if name == "tri_common.hpp" or os.path.basename(name).startswith("kernels_"):
            return m.group(0)
        with open(os.path.join(directory, name), encoding="utf-8") as fh:
            return fh.read()
    with open(os.path.join(directory, "tricolour_amd.hip"), encoding="utf-8") as fh:
        return re.sub(r'^#include "([^"\n]+)"[^\n]*\n', splice, fh.read(), flags=re.M)


def scan_getenv(directory=CSRC):
    texts = _sources(directory)
    texts[os.path.join(directory, "tricolour_amd.hip")] = host_text(directory)
    found = set()
    for text in texts.values():
        found.update(re.findall(r'getenv\(\s*"(TRI_[A-Z0-9_]+)"', text))
    return found


def scan_kernels(directory=CSRC):
    found = set()
    for text in _sources(directory).values():
        found.update(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", text))
    return found


def _abi_codes():
    """TRI_* enumerators of the C header with their values (template arguments are written with them)."""
    with open(os.path.join(ROOT, "include", "tricolour_amd.h"), encoding="utf-8") as fh:
        return dict(re.findall(r"^\s*(TRI_[A-Z0-9_]+)\s*=\s*(-?\d+)\s*,", fh.read(), re.M))


def _expand_launch_macros(hip):
    """Replaces every use of a function-like macro whose body launches kernels (defined and undefined again inside
    the function that uses it) by its body with the parameters substituted; the definitions themselves go."""
    define = re.compile(r"#define\s+(\w+)\(([\w\s,]*)\)((?:[^\n]*\\\n)*[^\n]*\n)")
    pos = 0
    while True:
        m = define.search(hip, pos)
        if m is None:
            return hip
        name, params, body = m.group(1), [p.strip() for p in m.group(2).split(",")], m.group(3)
        if "hipLaunchKernelGGL" not in body or name == "hipLaunchKernelGGL":
            pos = m.end()
            continue
        body = body.replace("\\\n", "\n")

        def use(u, params=params, body=body):
            args = [a.strip() for a in u.group(1).split(",")]
            if len(args) != len(params):
                return u.group(0)
            text = body
            for p, a in zip(params, args):
                text = re.sub(r"\b%s\b" % re.escape(p), a, text)
            return text
        hip = hip[:m.start()] + re.sub(r"\b%s\(([^()]*)\)" % re.escape(name), use, hip[m.end():])
        pos = m.start()


def scan_instances(directory=CSRC):
    """{kernel: set of instantiations} of the launch sites of the host code (host_text), launch macros expanded, template
    arguments in the demangler's spelling ("k_pack_scan_v<4, true, false, true>"; TRI_* codes as their numbers)."""
    hip = re.sub(r"//[^\n]*", "", host_text(directory))
    codes = _abi_codes()
    found = {}
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*(k_\w+)\s*(?:<([^<>;()]*)>)?", _expand_launch_macros(hip)):
        kernel, args = m.group(1), m.group(2)
        frag = kernel
        if args is not None:
            frag += "<%s>" % ", ".join(codes.get(a.strip(), a.strip()) for a in args.split(","))
        found.setdefault(kernel, set()).add(frag)
    return found


def names_read_by_python():
    """TRI_* names bench.py and the package read from the environment themselves."""
    found = set()
    for path in [os.path.join(ROOT, "bench.py")] + sorted(glob.glob(os.path.join(ROOT, "tricolour_amd", "*.py"))):
        with open(path, encoding="utf-8") as fh:
            for line in fh:
                if "environ" in line or "getenv" in line or re.search(r"\benv\[", line):
                    found.update(re.findall(r"""["'](TRI_[A-Z0-9_]+)["']""", line))
    return found


_COMMAND = r"(?:python[\w.]*|pytest|bash|sh|env|rocprofv3|hipcc|make|\./\S+|scripts/\S+|\$\w+|\$\{\w+\})"


def assigned_names(path, text):
    """TRI_* names `text` puts into an environment: NAME=value before a command (shell, documents), a `for` list
    whose variable is then set with $var=..., env[...] / os.environ[...] stores, dict(os.environ, NAME=...) and
    switch names kept as whole strings ("NAME" or "NAME=value") in Python."""
    found = set()
    ext = os.path.splitext(path)[1]
    if ext == ".py":
        found.update(re.findall(r"(?<![\w$])(TRI_[A-Z0-9_]+)=", text))                        # dict(os.environ, NAME="1"), "NAME=1"
        found.update(re.findall(r"""(?:env|environ)\[\s*["'](TRI_[A-Z0-9_]+)["']\s*\]\s*=[^=]""", text))
        found.update(re.findall(r"""["'](TRI_[A-Z0-9_]+)(?:=\w*)?["']""", text))
        found.update(re.findall(r"""["'](TRI_[A-Z0-9_]+)["']\s*:""", text))
    elif ext in (".md", ".rst", ".txt"):
        for m in re.finditer(r"(?<![\w$])((?:[A-Z_][A-Z0-9_]*=\S*\s+)+)" + _COMMAND, text):
            found.update(re.findall(r"(?<![\w$])(TRI_[A-Z0-9_]+)=", m.group(1)))
    else:
        found.update(re.findall(r"(?<![\w$])(TRI_[A-Z0-9_]+)=", text))
        for m in re.finditer(r"\bfor\s+(\w+)\s+in\s+([^;\n]*)", text):
            var, words = m.group(1), m.group(2)
            if re.search(r"\$\{?%s\}?=" % re.escape(var), text):
                found.update(re.findall(r"(?<![\w$])(TRI_[A-Z0-9_]+)\b", words))
    return found


def files_that_set_switches():
    paths = [os.path.join(ROOT, "bench.py")] + sorted(glob.glob(os.path.join(ROOT, "*.md")))
    for sub in ("scripts", "tests"):
        for d, _, names in os.walk(os.path.join(ROOT, sub)):
            if "golden" in d or "__pycache__" in d:
                continue
            paths += [os.path.join(d, n) for n in sorted(names) if os.path.splitext(n)[1] in (".py", ".sh", ".md", ".txt")]
    # (this file's own rows are held to the getenv scan; its scan tests spell made-up names)
    return [p for p in paths if os.path.abspath(p) != os.path.abspath(__file__)]


# error codes, dtype codes and limits of the C ABI: TRI_* tokens that are not environment variables
ABI_CONSTANTS = re.compile(r"^TRI_(OK|EINVAL|EUNSUPPORTED|EWORKSPACE|EHIP|VIS_\w+|MAX_\w+|MAD_NORMAL)$")


# ---- the tests ----

def test_every_getenv_name_has_a_row():
    found = scan_getenv()
    assert found == set(SWITCHES), "not in SWITCHES: %s; rows without a getenv: %s" % (sorted(found - set(SWITCHES)), sorted(set(SWITCHES) - found))


def test_every_kernel_has_a_row():
    found = scan_kernels()
    assert found == set(KERNELS), "not in KERNELS: %s; rows without a kernel: %s" % (sorted(found - set(KERNELS)), sorted(set(KERNELS) - found))


def test_the_scans_notice_a_change(tmp_path):
    """A renamed getenv string, an added kernel or an added instantiation in a copy of the sources changes what the
    scans find, in a step host file as in tricolour_amd.hip itself."""
    shutil.copytree(CSRC, str(tmp_path), dirs_exist_ok=True)                  # the whole tree, steps/ included
    step = tmp_path / "steps" / "linerms" / "linerms_host.hpp"
    text = step.read_text(encoding="utf-8")
    assert text.count("        hipLaunchKernelGGL(k_lrms_apply<true>,") == 1
    text = text.replace("        hipLaunchKernelGGL(k_lrms_apply<true>,",
                        "        hipLaunchKernelGGL(k_lrms_apply<7>, dim3(rows), dim3(256), 0, st);\n"
                        "    else if (is1(getenv(\"TRI_ADDED_IN_A_STEP\")))\n        hipLaunchKernelGGL(k_lrms_apply<true>,")
    step.write_text(text, encoding="utf-8")
    for path, text in _sources().items():
        text = text.replace('getenv("TRI_ST_NO_PIPE")', 'getenv("TRI_ST_NOPIPE")')
        if path.endswith("kernels_sir.hpp"):
            text += "\ntemplate <int N>\n__global__ void __launch_bounds__(64, f(N))\nk_added_later(const float* a) {}\n"
        if path.endswith("tricolour_amd.hip"):
            # one more instantiation at a literal launch site, one more use of a launch macro
            text = text.replace("        else if (ncorr == 1)\n            hipLaunchKernelGGL(k_pack_v<1>,",
                                "        else if (ncorr == 8)\n            hipLaunchKernelGGL(k_pack_v<8>, grid);\n"
                                "        else if (ncorr == 1)\n            hipLaunchKernelGGL(k_pack_v<1>,", 1)
            text = text.replace("        if (vec && ncorr == 4 && stokes) TRI_PACK_SCAN_V(4, true);",
                                "        if (vec && ncorr == 8) TRI_PACK_SCAN_V(8, false);\n"
                                "        else if (vec && ncorr == 4 && stokes) TRI_PACK_SCAN_V(4, true);", 1)
        (tmp_path / os.path.basename(path)).write_text(text, encoding="utf-8")
    assert scan_getenv(str(tmp_path)) ^ set(SWITCHES) == {"TRI_ST_NO_PIPE", "TRI_ST_NOPIPE", "TRI_ADDED_IN_A_STEP"}
    assert scan_kernels(str(tmp_path)) - set(KERNELS) == {"k_added_later"}
    before, after = scan_instances(), scan_instances(str(tmp_path))
    added = {f for k in after for f in after[k] - before.get(k, set())}
    assert added == {"k_pack_v<8>", "k_lrms_apply<7>"} | {"k_pack_scan_v<8, false, %s, %s>" % (m, f) for m in ("true", "false") for f in ("true", "false")}
    assert all(before[k] <= after[k] for k in before)


def test_rows_are_well_formed():
    for name, row in SWITCHES.items():
        cls = row["cls"]
        assert cls in ("route", "geometry", "schedule", "print-only", "elsewhere", "unreachable"), name
        if cls in ("route", "geometry"):
            assert name not in NOT_IN_MATRIX and row["legs"], name
            for leg in row["legs"]:
                assert name in leg["env"] and leg["cases"], name
                assert all(leg["env"].get(k) == v for k, v in leg["base"].items()) and name not in leg["base"], name
                for case, what in leg["cases"].items():
                    if cls == "route":
                        assert what["gone"] or what["new"], (name, case)
                    else:
                        assert what["shapes"] and row["why"], (name, case)
        elif cls == "unreachable":
            assert row["why"], name
        else:
            # nothing but these five may stay out of the matrix
            assert name in NOT_IN_MATRIX, name
            assert row.get("test") or row.get("why"), name
    assert {n for n, r in SWITCHES.items() if r["cls"] not in ("route", "geometry", "unreachable")} == NOT_IN_MATRIX
    assert {n for n, r in SWITCHES.items() if r["cls"] == "elsewhere"} == {"TRI_NO_FUSED_RESID_TF", "TRI_BG_COPY_FLAGS", "TRI_UV_SCALAR"}
    for kernel, where in KERNELS.items():
        if isinstance(where, dict):
            assert set(where) - {"flagger", "also"} == {"test", "instances"} and "::" in where["test"] and where["instances"], kernel
            assert "also" not in where or ("::" in where["also"] and where["also"] != where["test"] and kernel not in SYMBOL_KERNELS), kernel
            assert ("flagger" in where) == (kernel in SYMBOL_KERNELS) and where.get("flagger", True) is True, kernel
            assert where["test"] == {True: _BOX, False: _ST}[kernel in BOX_KERNELS] or kernel not in SYMBOL_KERNELS, kernel
            for item in where["instances"]:
                if isinstance(item, dict):
                    assert set(item) in ({"name", "unreachable"}, {"name", "switch"}) and all(item.values()), kernel
                    assert "switch" not in item or kernel in BOX_KERNELS, kernel
                else:
                    assert isinstance(item, str), kernel
            names = symbol_instances(kernel) if kernel in SYMBOL_KERNELS else listed_instances(kernel)
            assert all(base_name(n) == kernel and (n == kernel or re.match(r"^%s<[^<>]+>$" % kernel, n)) for n in names), kernel
            assert len(set(names)) == len(names), kernel
        else:
            assert where in ("flagger", "unlaunched") or "::" in where, kernel


# the kernels whose rows list their instantiations: those of kernels_scan.hpp and the pack / unpack, strategy-step,
# flag-count and Stokes kernels of kernels_elementwise.hpp
INSTANCE_KERNELS = {"k_fill_windows", "k_pack", "k_pack_v", "k_unpack_v", "k_unpack", "k_flag_nans_zeros", "k_apply_bl_chan_mask",
                    "k_window_counts", "k_stokes_intensity"}
# ... and the kernels behind tri_uvcontsub_flagger: kernels_elementwise.hpp's k_uv_* that have a launch site, kernels_median.hpp's K3d
UV_KERNELS = {"k_uv_mean", "k_uv_lowpass", "k_uv_resid", "k_uv_resid4", "k_uv_apply", "k_uv_apply4",
              "k_medbig_range", "k_medbig_hist", "k_medbig_pick", "k_medbig_compact", "k_medbig_select"}
INSTANCE_KERNELS |= UV_KERNELS


def test_instance_rows_cover_the_entry_point_kernels():
    with open(os.path.join(CSRC, "kernels_scan.hpp"), encoding="utf-8") as fh:
        scan_kernels_ = set(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", fh.read()))
    assert len(scan_kernels_) == 6
    assert set(instance_rows()) == INSTANCE_KERNELS | scan_kernels_
    uv = {k for k in KERNELS if k.startswith(("k_uv_", "k_medbig_"))}
    assert uv - UV_KERNELS == {"k_uv_count", "k_uv_diff"} and all(KERNELS[k] == "unlaunched" for k in uv - UV_KERNELS)
    for kernel in instance_rows():
        for frag in listed_instances(kernel):
            assert base_name(frag) == kernel, (kernel, frag)
            assert frag == kernel or re.match(r"^%s<[^<>]+>$" % kernel, frag), frag


def test_listed_instances_are_the_launch_sites():
    """Every instantiation a launch site of the host code produces is listed, and nothing else is."""
    found = scan_instances()
    for kernel in sorted(instance_rows()):
        listed = set(listed_instances(kernel))
        assert found.get(kernel, set()) == listed, "%s: launched but not listed %s; listed but not launched %s" % (
            kernel, sorted(found.get(kernel, set()) - listed), sorted(listed - found.get(kernel, set())))


def test_the_literal_launch_sites_alone_miss_the_macro_families():
    """The macro families are found through the macro expansion only: without it the scan sees none of their
    instantiations (so the literal scan and the expansion are both at work), and with it the full product."""
    hip = re.sub(r"//[^\n]*", "", host_text())
    for kernel, macro in SCAN_FAMILIES.items():
        literal = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*%s\s*<([^<>;()]*)>" % kernel, hip)
        assert literal and all(re.search(r"\bNC\b", a) and re.search(r"\bS\b", a) for a in literal), kernel
        assert "#define %s(NC, S)" % macro in hip and "#undef %s" % macro in hip
        product = {"%s<%d, %s, %s, %s>" % (kernel, nc, s, m, f) for nc in (1, 2, 4) for s in ("true", "false")
                   for m in ("true", "false") for f in ("true", "false")}
        assert len(product) == 24 and set(listed_instances(kernel)) == product, kernel
        assert scan_instances()[kernel] == product, kernel


def test_a_wrong_ledger_row_fails_the_scan(monkeypatch):
    """A listed instantiation the source does not launch, and a launched one that is not listed, both show."""
    found = scan_instances()
    monkeypatch.setitem(KERNELS, "k_pack_v", _inst(_ENTRY, "k_pack_v<1>", "k_pack_v<2>", "k_pack_v<4>", "k_pack_v<3>"))
    assert set(listed_instances("k_pack_v")) - found["k_pack_v"] == {"k_pack_v<3>"}
    monkeypatch.setitem(KERNELS, "k_pack_v", _inst(_ENTRY, "k_pack_v<1>", "k_pack_v<4>"))
    assert found["k_pack_v"] - set(listed_instances("k_pack_v")) == {"k_pack_v<2>"}
    with pytest.raises(AssertionError):
        test_listed_instances_are_the_launch_sites()
    monkeypatch.setitem(KERNELS, "k_pack_v", _inst(_ENTRY, "k_pack_v<1>", "k_pack_v<2>", dict(name="k_pack_v<4>", unreachable="an example")))
    test_listed_instances_are_the_launch_sites()
    assert "k_pack_v<4>" not in reachable_instances() and "k_pack_v<2>" in reachable_instances()


def test_box_rows_are_the_library_symbols():
    """The rows of SYMBOL_KERNELS (box filters and SumThreshold) against the symbol table of the built library (built
    here if it is missing, as for tests/test_abi.py): an instantiation added to a dispatcher, removed or renamed without
    its row fails here."""
    from tricolour_amd import _lib
    _lib.build()
    symbols = library_instances(_lib.LIB_PATH)
    assert len(symbols) > 300 and set(SYMBOL_KERNELS) <= {base_name(n) for n in symbols}, len(symbols)
    # (the log the GPU tests compare with spells the names as the symbol table does)
    assert "k_boxqf<40, 2, 8>" in symbols and "k_boxf<32, true, 2, 1>" in symbols and "k_boxw<110>" in symbols
    assert "k_colst_mask<1, 2, 4, 8, true>" in symbols and "k_colst_dyn" in symbols
    errors = symbol_row_errors(symbols)
    assert not errors, "\n".join(errors)


def test_a_wrong_box_row_fails_against_the_symbols(monkeypatch):
    """A row with a name too many and a row with a name missing both fail against a given symbol list, unreachable
    entries included; so does an instantiation a dispatcher gained."""
    symbols = [n for k in SYMBOL_KERNELS for n in symbol_instances(k)] + ["k_sir<4, true>", "k_pack_v<2>"]
    assert not symbol_row_errors(symbols)
    gained = symbol_row_errors(symbols + ["k_boxqf<88, 1, 8>"])
    assert len(gained) == 1 and "not listed ['k_boxqf<88, 1, 8>']" in gained[0], gained
    for lost in ("k_boxw<46>", "k_boxt<16, true, 0>"):                       # a reachable one, an unreachable one
        errors = symbol_row_errors([n for n in symbols if n != lost])
        assert len(errors) == 1 and "not in the library ['%s']" % lost in errors[0], errors
    row = KERNELS["k_boxp_spec"]
    monkeypatch.setitem(KERNELS, "k_boxp_spec", dict(row, instances=row["instances"] + ["k_boxp_spec<4, 16>"]))
    errors = symbol_row_errors(symbols)
    assert len(errors) == 1 and errors[0].startswith("k_boxp_spec:") and "not in the library ['k_boxp_spec<4, 16>']" in errors[0], errors
    monkeypatch.setitem(KERNELS, "k_boxp_spec", dict(row, instances=row["instances"][:1]))
    errors = symbol_row_errors(symbols)
    assert len(errors) == 1 and "not listed ['k_boxp_spec<8, 16>']" in errors[0], errors
    monkeypatch.setitem(KERNELS, "k_boxp_spec", dict(row, instances=[row["instances"][0], _no("k_boxp_spec<8, 16>", "an example")]))
    assert not symbol_row_errors(symbols)
    assert "k_boxp_spec<8, 16>" not in symbol_instances("k_boxp_spec", reachable_only=True)


def test_a_wrong_sumthreshold_row_fails_against_the_symbols(monkeypatch):
    """The same for the SumThreshold rows: a cascade instantiated for other windows, a lost panel form and a row that
    lists too much or too little all show, each in its own row only."""
    symbols = [n for k in SYMBOL_KERNELS for n in symbol_instances(k)] + ["k_sir<4, true>"]
    assert not symbol_row_errors(symbols)
    gained = symbol_row_errors(symbols + ["k_colst_mask<1, 2, 4, 4, false>"])
    assert len(gained) == 1 and gained[0].startswith("k_colst_mask:") and "not listed ['k_colst_mask<1, 2, 4, 4, false>']" in gained[0], gained
    for lost in ("k_colst_mask<1, 2, 4, 8, true>", "k_colst_dyn"):
        errors = symbol_row_errors([n for n in symbols if n != lost])
        assert len(errors) == 1 and "not in the library ['%s']" % lost in errors[0], errors
    row = KERNELS["k_colst_fused"]
    monkeypatch.setitem(KERNELS, "k_colst_fused", dict(row, instances=row["instances"] + ["k_colst_fused<1, 2, 2, 4>"]))
    errors = symbol_row_errors(symbols)
    assert len(errors) == 1 and errors[0].startswith("k_colst_fused:") and "not in the library ['k_colst_fused<1, 2, 2, 4>']" in errors[0], errors
    monkeypatch.setitem(KERNELS, "k_colst_mask", dict(KERNELS["k_colst_mask"], instances=["k_colst_mask<1, 2, 4, 8, false>"]))
    monkeypatch.setitem(KERNELS, "k_colst_fused", row)
    errors = symbol_row_errors(symbols)
    assert len(errors) == 1 and "not listed ['k_colst_mask<1, 2, 4, 8, true>']" in errors[0], errors


def test_sumthreshold_rows_cover_the_sumthreshold_kernels():
    """ST_KERNELS are the kernels of kernels_sumthreshold.hpp, all of them; each is still a flagger kernel."""
    with open(os.path.join(CSRC, "kernels_sumthreshold.hpp"), encoding="utf-8") as fh:
        found = set(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", fh.read()))
    assert found == set(ST_KERNELS), sorted(found ^ set(ST_KERNELS))
    assert all(is_flagger(k) for k in ST_KERNELS) and not set(ST_KERNELS) & set(BOX_KERNELS)
    assert all(base_name(n) == k for k in ST_KERNELS for n in symbol_instances(k, reachable_only=True))


def test_box_rows_cover_the_box_filter_kernels():
    """BOX_KERNELS are the kernels of the five box-filter headers, all of them; each is still a flagger kernel."""
    found = set()
    for name in ("kernels_boxexact.hpp", "kernels_boxfilter.hpp", "kernels_boxline.hpp", "kernels_boxpipe.hpp", "kernels_boxweight.hpp"):
        with open(os.path.join(CSRC, name), encoding="utf-8") as fh:
            found.update(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", fh.read()))
    assert found == set(BOX_KERNELS), sorted(found ^ set(BOX_KERNELS))
    assert all(is_flagger(k) for k in BOX_KERNELS) and not is_flagger("k_pack_v") and is_flagger("k_prepare")


def test_switch_entries_are_named_by_their_route_leg():
    """A `switch` entry is met by test_route_matrix_gpu.py: a leg of that switch must name exactly this instantiation as
    new or present, so that its oracle-checked log is known to hold it."""
    for frag, switch in switch_met_instances().items():
        named = set()
        for leg in switch_legs(switch):
            for what in leg["cases"].values():
                named.update(what.get("new", []) + what.get("present", []))
        assert SWITCHES[switch]["cls"] == "route" and frag in named, (frag, switch, sorted(named))


def _function_exists(ref):
    fname, func = ref.split("::")
    with open(os.path.join(HERE, fname), encoding="utf-8") as fh:
        return re.search(r"^def %s\(" % re.escape(func), fh.read(), re.M) is not None


def test_named_tests_exist():
    refs = {named_test(w) for w in KERNELS.values() if named_test(w)} | {r["test"] for r in SWITCHES.values() if r.get("test")}
    refs |= {w["also"] for w in KERNELS.values() if isinstance(w, dict) and w.get("also")}
    missing = sorted(r for r in refs if not _function_exists(r))
    assert not missing, missing


def test_unlaunched_kernels_have_no_launch_site():
    hip = host_text()
    for kernel, where in KERNELS.items():
        used = re.search(r"\b%s\b" % kernel, re.sub(r"//[^\n]*", "", hip)) is not None
        defined_there = re.search(r"__global__[\s\S]{0,200}?\b%s\s*\(" % kernel, hip) is not None
        if where == "unlaunched":
            assert not used, "%s has a launch site" % kernel
        elif not defined_there:
            assert used, "%s is never launched: mark it unlaunched" % kernel


def test_the_elsewhere_tests_assert_a_kernel_log():
    for name, row in SWITCHES.items():
        if row["cls"] != "elsewhere":
            continue
        with open(os.path.join(HERE, row["test"].split("::")[0]), encoding="utf-8") as fh:
            text = fh.read()
        assert name in text and "kernel_log_begin" in text, name


def test_no_file_sets_a_name_nobody_reads():
    known = set(SWITCHES) | names_read_by_python()
    bad = []
    for path in files_that_set_switches():
        with open(path, encoding="utf-8") as fh:
            text = fh.read()
        for name in sorted(assigned_names(path, text)):
            if name not in known and not ABI_CONSTANTS.match(name):
                bad.append("%s sets %s" % (os.path.relpath(path, ROOT), name))
    assert not bad, "; ".join(bad)


def test_the_assignment_scan_sees_each_form():
    assert assigned_names("x.sh", "for k in NONE TRI_A TRI_B; do\n  env $k=1 python x.py\ndone\n") == {"TRI_A", "TRI_B"}
    assert assigned_names("x.sh", "TRI_C=1 TRI_D=0 python x.py\nexport TRI_E=1\n") == {"TRI_C", "TRI_D", "TRI_E"}
    assert assigned_names("x.md", "run `TRI_F=1 python bench.py`; the loop sets TRI_G=1, a variable nobody reads") == {"TRI_F"}
    assert assigned_names("x.py", 'env["TRI_H"] = "1"\nos.environ["TRI_I"] = "1"\ne = dict(os.environ, TRI_J="1")\nK = ("TRI_K=256", "TRI_L")\n') == \
        {"TRI_H", "TRI_I", "TRI_J", "TRI_K", "TRI_L"}


def test_alternate_kernel_paths_names_are_switches():
    with open(os.path.join(HERE, "test_gpu_parity.py"), encoding="utf-8") as fh:
        text = fh.read()
    m = re.search(r'parametrize\("knob",\s*\[(.*?)\]\)\s*\ndef test_alternate_kernel_paths', text, re.S)
    assert m, "test_alternate_kernel_paths not found"
    names = set()
    for knob in re.findall(r'"([^"]+)"', m.group(1)):
        for one in knob.split(";"):
            names.add(one.partition("=")[0])
    names.discard("DEFAULT_ROUTES")
    assert len(names) > 30 and names <= set(SWITCHES), sorted(names - set(SWITCHES))
