"""Time statistics collapsed along index directions, host side: the ids of the header and of
abi.py, the recurrence the device runs (tests/collapse_ref.py) against an extended-precision
two-pass reference, and solver.pool_bins."""
import math
import os
import re

import numpy as np
import pytest

import collapse_ref as cr
from aither_amd import abi
from aither_amd.solver import pool_bins

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "aither_gfx950.h")
NAMES = ("a", "b", "c")
PAIRS = [("a", "a"), ("a", "b"), ("b", "c"), ("c", "c")]
SIZES = (3, 6, 9, 67, 300, 4096)
CHUNKS = (4, 64, 100)
NBIN = 50
BIG_W = 3.75


def test_ids_of_the_header_and_abi_agree():
    with open(HEADER) as fh:
        text = fh.read()
    const = lambda name: int(re.search(r"\b%s = (\d+)" % name, text).group(1))
    assert const("AGX_CSTAT_BASE") == 1024 == abi.CSTAT_BASE
    assert const("AGX_CSTAT_COUNT") == 22 == abi.CSTAT_COUNT == len(abi.CSTAT_NAMES)
    assert const("AGX_CSTAT_END") == 2048
    assert abi.CSTAT_NAMES[:21] == tuple(abi.STAT_OUT) and abi.CSTAT_NAMES[21] == "volume"
    for n, name in enumerate(abi.STAT_OUT):
        assert abi.STAT_OUT[name] == abi.STAT_BASE + n
        assert abi.cstat_id(5, name) == 1024 + 32 * 5 + n
    assert abi.cstat_id(7, "volume") == 1024 + 32 * 7 + 21
    assert [abi.cstat_mask(o) for o in ("i", "j", "ij", "k", "ik", "kj", "ijk")] == \
        [1, 2, 3, 4, 5, 6, 7]
    for bad in ("", "x", "ii", "ijkk"):
        with pytest.raises(ValueError):
            abi.cstat_mask(bad)
    # the range lies above every other one, and every second moment names two means
    assert abi.CSTAT_BASE >= max(abi.WSTAT_END, abi.STAT_END)
    assert list(abi.STAT_PAIRS) == list(abi.STAT_OUT)[12:]
    assert all(m in abi.STAT_OUT for p in abi.STAT_PAIRS.values() for m in p)
    # the chunk the device pools the collapsed (j, k) positions in
    with open(os.path.join(os.path.dirname(HERE), "aither_amd", "csrc", "agx_stats.hpp")) as fh:
        assert int(re.search(r"CSTAT_CHUNK = (\d+)", fh.read()).group(1)) == abi.CSTAT_CHUNK


# ---- the three families --------------------------------------------------------------------------
def family(kind, n, seed=0):
    """NBIN bins of n cells: (vol, means, coms).  Volumes of a stretched grid (ratio 1.15, capped
    at 1e3) with a random factor."""
    rng = np.random.default_rng(1000 * seed + n)
    grow = np.minimum(1.15 ** np.arange(n), 1.0e3)
    vol = grow * rng.uniform(0.5, 1.5, (NBIN, n))
    if kind == "random":
        means = {k: rng.uniform(-1.0, 1.0, (NBIN, n)) + 0.3 * q for q, k in enumerate(NAMES)}
        coms = {p: rng.uniform(-1.0, 1.0, (NBIN, n)) for p in PAIRS}
    elif kind == "tiny":
        means = {k: 1.0 + 1e-8 * rng.uniform(-1.0, 1.0, (NBIN, n)) for k in NAMES}
        coms = {p: 1e-16 * rng.uniform(0.0, 1.0, (NBIN, n)) for p in PAIRS}
    else:
        means = {k: np.repeat(rng.uniform(-1.0, 1.0, (NBIN, 1)), n, axis=1) for k in NAMES}
        coms = {p: np.repeat(rng.uniform(-1.0, 1.0, (NBIN, 1)), n, axis=1) for p in PAIRS}
    return vol, means, coms


FORMS = [("west_space", cr.west_space)] + \
    [("chunked %d" % ch, lambda *a, ch=ch: cr.chunked(*a, chunk=ch)) for ch in CHUNKS]


def test_recurrence_against_the_two_pass_reference():
    """The measured worst case (printed) is what collapse_ref records, and four times it holds."""
    worst_m = worst_c = 0.0
    for kind in ("random", "tiny", "same"):
        for n in SIZES:
            fam = family(kind, n)
            for label, form in FORMS:
                wm, wc = cr.reached(form(*fam, BIG_W), *fam, BIG_W, c1=1.0, c2=1.0)
                print("family %-6s N %4d %-11s mean %.3g, co-moment %.3g of the bound with C = 1"
                      % (kind, n, label, wm, wc))
                worst_m, worst_c = max(worst_m, wm), max(worst_c, wc)
                hm, hc = cr.reached(form(*fam, BIG_W), *fam, BIG_W)
                assert hm <= 1.0 and hc <= 1.0, (kind, n, label, hm, hc)
    print("worst: means %.3g, co-moments %.3g" % (worst_m, worst_c))
    assert worst_m <= cr.MEASURED_C1 * 1.0001 and worst_c <= cr.MEASURED_C2 * 1.0001
    # (recorded, not loose: the constants are within a factor of two of what is measured)
    assert worst_m >= cr.MEASURED_C1 / 2 and worst_c >= cr.MEASURED_C2 / 2
    assert math.isclose(cr.C1, 4 * cr.MEASURED_C1) and math.isclose(cr.C2, 4 * cr.MEASURED_C2)


def _same(got, fam):
    vol, means, coms = fam
    _, m, cov = got
    for k in means:
        assert np.array_equal(m[k], means[k][..., 0]), k
    for p in coms:
        assert np.array_equal(cov[p], coms[p][..., 0] / BIG_W), p


@pytest.mark.parametrize("n", SIZES)
def test_identical_cells_are_exact(n):
    """M = m and cov = C / W bit for bit, whatever the volumes: serial, chunked at every chunk
    length, and two halves joined by pool_bins."""
    fam = family("same", n)
    _same(cr.west_space(*fam, BIG_W), fam)
    for ch in CHUNKS + (1, 2, n):
        _same(cr.chunked(*fam, BIG_W, chunk=ch), fam)
    for p in PAIRS:
        assert not cr.serial(*fam)[3][p].any()          # D = 0 exactly
    cut = n // 2 + 1
    halves = []
    for sl in (slice(0, cut), slice(cut, n)):
        sub = (fam[0][..., sl], {k: m[..., sl] for k, m in fam[1].items()},
               {p: c[..., sl] for p, c in fam[2].items()})
        halves.append(cr.west_space(*sub, BIG_W))
    _same(pool_bins(halves), fam)


def test_sums_of_squares_miss_the_bound_by_orders():
    for n in SIZES:
        fam = family("tiny", n)
        wm, wc = cr.reached(cr.west_space(*fam, BIG_W), *fam, BIG_W)
        assert wm <= 1.0 and wc <= 1.0
        _, miss = cr.reached(cr.naive(*fam, BIG_W), *fam, BIG_W)
        print("N %4d: sums of squares miss the co-moment bound by %.3g" % (n, miss))
        assert miss > 1e3, (n, miss)


def test_a_count_weighted_average_misses_on_a_stretched_grid():
    """The volumes grow by 1.15 per cell and the means vary with them: the unweighted average
    is another number."""
    for n in SIZES:
        vol, means, coms = family("random", n)
        means = {k: m + 0.01 * np.log(vol) for k, m in means.items()}
        fam = (vol, means, coms)
        wm, wc = cr.reached(cr.count_mean(*fam, BIG_W), *fam, BIG_W)
        assert wm > 1e6 and wc > 1e6, (n, wm, wc)
        # ... and on a uniform grid it is the same number
        flat = (np.full_like(vol, 0.37), means, coms)
        wm, wc = cr.reached(cr.count_mean(*flat, BIG_W), *flat, BIG_W)
        assert wm <= 1.0 and wc <= 1.0


@pytest.mark.parametrize("kind", ["random", "tiny"])
def test_pool_bins_of_a_split_bin(kind):
    """A bin split at any point and joined by pool_bins is the unsplit bin within the bound."""
    n = 67
    fam = family(kind, n)
    worst = (0.0, 0.0)
    for cut in range(1, n):
        parts = []
        for sl in (slice(0, cut), slice(cut, n)):
            sub = (fam[0][..., sl], {k: m[..., sl] for k, m in fam[1].items()},
                   {p: c[..., sl] for p, c in fam[2].items()})
            parts.append(cr.west_space(*sub, BIG_W))
        got = pool_bins(parts)
        assert np.allclose(got[0], fam[0].sum(axis=-1), rtol=n * cr.ULP, atol=0.0)
        wm, wc = cr.reached(got, *fam, BIG_W)
        assert wm <= 1.0 and wc <= 1.0, (cut, wm, wc)
        worst = max(worst[0], wm), max(worst[1], wc)
    print("%s: split bins reach %.3g (means) and %.3g (co-moments) of the bound" % ((kind,) + worst))
    # three parts, and the names of abi.STAT_PAIRS as keys
    named = {"mean_vel_x": "a", "mean_vel_y": "b"}
    parts = []
    for sl in (slice(0, 20), slice(20, 41), slice(41, n)):
        sub = (fam[0][..., sl], {k: m[..., sl] for k, m in fam[1].items()},
               {p: c[..., sl] for p, c in fam[2].items()})
        v, m, c = cr.west_space(*sub, BIG_W)
        parts.append((v, {k: m[x] for k, x in named.items()}, {"cov_uv": c[("a", "b")]}))
    v, m, c = pool_bins(parts)
    got = (v, {"a": m["mean_vel_x"], "b": m["mean_vel_y"]}, {("a", "b"): c["cov_uv"]})
    sub = (fam[0], {k: fam[1][k] for k in "ab"}, {("a", "b"): fam[2][("a", "b")]})
    wm, wc = cr.reached(got, *sub, BIG_W)
    assert wm <= 1.0 and wc <= 1.0


def test_every_layer_offers_the_call():
    from aither_amd.solver import MultigridSolver, Solver
    assert callable(Solver.stats_collapse) and callable(MultigridSolver.stats_collapse)
    with open(os.path.join(os.path.dirname(HERE), "include", "aither_gfx950.hpp")) as fh:
        hpp = fh.read()
    assert "CollapsedStatisticId(int mask, int n) { return AGX_CSTAT_BASE + 32 * mask + n; }" in hpp
    assert "void CollapsedStatistics(int block, int mask, const std::vector<int32_t> &ids," in hpp
