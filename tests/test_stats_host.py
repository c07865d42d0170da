"""Time statistics, host side: the ids of the header and of abi.py, and the recurrence the
device runs (tests/stats_ref.py) against an extended-precision two-pass reference."""
import math
import os
import re

import numpy as np
import pytest

import stats_ref
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import Solver

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "aither_gfx950.h")
NAMES = ("density", "vel_x", "vel_y", "vel_z", "pressure", "temperature")
PAIRS = [("vel_x", "vel_x"), ("vel_x", "vel_y"), ("vel_x", "vel_z"), ("vel_y", "vel_y"),
         ("vel_y", "vel_z"), ("vel_z", "vel_z"), ("density", "density"),
         ("pressure", "pressure"), ("temperature", "temperature")]
OUTSIDE = (-1, 54, 63, 78, 99, 127, 182, 255, 273)
WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("pressureOutlet", 3),
        4: ("characteristic", 1)}


def _header():
    with open(HEADER) as fh:
        return fh.read()


def _const(text, name):
    return int(re.search(r"\b%s = (\d+)" % name, text).group(1))


def test_ids_of_the_header_and_abi_agree():
    text = _header()
    assert _const(text, "AGX_FIELD_STAT_SAMPLE") == 23 == abi.FIELD["stat_sample"]
    assert _const(text, "AGX_FIELD_STAT_ACCUM") == 24 == abi.FIELD["stat_accum"]
    base, end = _const(text, "AGX_STAT_BASE"), _const(text, "AGX_STAT_END")
    wbase, wend = _const(text, "AGX_WSTAT_BASE"), _const(text, "AGX_WSTAT_END")
    assert (base, end, wbase, wend) == (512, 533, 576, 594)
    assert (abi.STAT_BASE, abi.STAT_END, abi.WSTAT_BASE, abi.WSTAT_END) == (512, 533, 576, 594)
    # the cell statistics in the issue's order, the wall statistics after the wall variables
    assert sorted(abi.STAT_OUT.values()) == list(range(base, end))
    assert list(abi.STAT_OUT)[:6] == ["mean_" + n for n in NAMES]
    assert [abi.STAT_OUT[n] - base for n in ("mean_mom_x", "mean_turbulentViscosity", "mean_tke",
                                             "mean_sdr", "cov_uu", "cov_uv", "cov_ww",
                                             "var_density", "var_pressure", "var_temperature")] \
        == [6, 9, 10, 11, 12, 13, 17, 18, 19, 20]
    assert sorted(abi.WALL_STAT_OUT.values()) == list(range(wbase, wend))
    for name, wid in abi.WALL_OUT.items():
        assert abi.WALL_STAT_OUT["mean_" + name] == wbase + wid - abi.WALL_OUT["yplus"]
    assert [abi.WALL_STAT_OUT["var_" + n] - wbase for n in
            ("pressure", "shearStress_x", "shearStress_y", "shearStress_z")] == [14, 15, 16, 17]
    # six disjoint ranges, and the ids the existing tests expect to be unknown lie in none
    count = _const(text, "AGX_OUT_COUNT")
    wall_end = abi.WALL_OUT["shearStress_z"] + 1
    load_end = max(abi.LOAD_OUT.values()) + 1
    ranges = [(0, count), (64, wall_end), (abi.NODE_BASE, abi.NODE_BASE + count),
              (abi.LOAD_BASE, load_end), (base, end), (wbase, wend)]
    ranges.sort()
    for (_, hi), (lo, _) in zip(ranges, ranges[1:]):
        assert hi <= lo, ranges
    for bad in OUTSIDE:
        assert not any(lo <= bad < hi for lo, hi in ranges), bad
    # the C-ABI has gained no entry
    declared = set(re.findall(r"\bagx_(\w+)\s*\(", text.split("typedef struct agx_ctx agx_ctx;")[1]))
    assert set(abi.SYMBOLS) == declared
    assert abi.DEVICE_ONLY == ("state_fill", "state_from_cloud", "restart_unpack")


# ---- the three sample families ---------------------------------------------------------------
@pytest.fixture(scope="module")
def families(oracle):
    case = synthetic.single_block_case((8, 7, 6), stretch=1.15, bcs=WALL,
                                       equation_set="navierStokes", time_integration="rk4",
                                       cfl=0.5)
    s = Solver(oracle, case)
    g, run = case.ng, []
    for nn in range(5):
        s.step(nn)
        st = s.download("state", 0)[g:-g, g:-g, g:-g]
        x = {n: st[..., q].copy() for q, n in enumerate(NAMES[:5])}
        x["temperature"] = x["pressure"] / (x["density"] * case.gas.gas_constant)
        run.append(x)
    s.close()
    k, j, i = np.meshgrid(np.arange(6.0), np.arange(7.0), np.arange(8.0), indexing="ij")
    tiny = []
    for n in range(5):
        tiny.append({name: 1.0 + 1e-8 * np.sin(0.7 * i + 0.3 * q + 1.3 * n) *
                     np.cos(0.5 * j - 0.2 * n) * np.cos(0.9 * k + 0.1 * q * n)
                     for q, name in enumerate(NAMES)})
    same = [run[2]] * 5
    return dict(run=run, tiny=tiny, same=same)


def test_recurrence_against_the_two_pass_reference(families):
    """The measured worst case (printed) is what stats_ref records, and four times it holds."""
    worst_m = worst_c = 0.0
    for name, fam in families.items():
        wm, wc = stats_ref.worst(fam, stats_ref.WEIGHTS, PAIRS)
        print("family %-5s worst mean error %.3g, co-moment error %.3g (multiples of the bound "
              "with C = 1)" % (name, wm, wc))
        worst_m, worst_c = max(worst_m, wm), max(worst_c, wc)
    assert worst_m <= stats_ref.MEASURED_C1 * 1.0001 and worst_c <= stats_ref.MEASURED_C2 * 1.0001
    # (recorded, not loose: the constants are within a factor of two of what is measured)
    assert worst_m >= stats_ref.MEASURED_C1 / 2 and worst_c >= stats_ref.MEASURED_C2 / 2
    assert math.isclose(stats_ref.C1, 4 * stats_ref.MEASURED_C1)
    assert math.isclose(stats_ref.C2, 4 * stats_ref.MEASURED_C2)
    for fam in families.values():
        mean, cov, _ = stats_ref.west(fam, stats_ref.WEIGHTS, PAIRS)
        rmean, rcov, _ = stats_ref.two_pass(fam, stats_ref.WEIGHTS, PAIRS)
        for n in NAMES:
            assert np.abs(mean[n] - rmean[n]).max() <= stats_ref.mean_bound(
                fam, stats_ref.WEIGHTS, n)
        for a, b in PAIRS:
            assert np.abs(cov[(a, b)] - rcov[(a, b)]).max() <= stats_ref.cov_bound(
                fam, stats_ref.WEIGHTS, a, b)


def test_sums_of_squares_miss_the_bound_by_orders(families):
    fam = families["tiny"]
    _, cov, _ = stats_ref.naive(fam, stats_ref.WEIGHTS, PAIRS)
    _, wcov, _ = stats_ref.west(fam, stats_ref.WEIGHTS, PAIRS)
    _, rcov, _ = stats_ref.two_pass(fam, stats_ref.WEIGHTS, PAIRS)
    for a, b in PAIRS:
        bound = stats_ref.cov_bound(fam, stats_ref.WEIGHTS, a, b)
        assert np.abs(wcov[(a, b)] - rcov[(a, b)]).max() <= bound
        miss = float(np.abs(cov[(a, b)] - rcov[(a, b)]).max()) / bound
        assert miss > 1e3, (a, b, miss)
        # ... which leaves no digit of a variance of 1e-17
        assert np.abs(cov[(a, b)] - rcov[(a, b)]).max() > 0.5 * float(np.abs(rcov[(a, b)]).max())


def test_identical_samples_are_their_own_mean(families):
    fam = families["same"]
    mean, cov, big_w = stats_ref.west(fam, stats_ref.WEIGHTS, PAIRS)
    assert big_w == sum(stats_ref.WEIGHTS)
    for n in NAMES:
        assert np.array_equal(mean[n], fam[0][n])
    for p in PAIRS:
        assert not cov[p].any()


@pytest.mark.parametrize("family", ["run", "tiny"])
def test_doubling_every_weight_changes_no_bit(families, family):
    fam = families[family]
    m1, c1, _ = stats_ref.west(fam, stats_ref.WEIGHTS, PAIRS)
    m2, c2, _ = stats_ref.west(fam, [2.0 * w for w in stats_ref.WEIGHTS], PAIRS)
    for n in NAMES:
        assert np.array_equal(m1[n], m2[n])
    for p in PAIRS:
        assert np.array_equal(c1[p], c2[p])
