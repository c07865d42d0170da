"""Spectra along homogeneous directions, host side: the field ids of the header and of abi.py,
the layers that offer the calls, the payload helpers, correlation and pool_spectra, the plan's
arithmetic under the sanitizers and against its Python copy, the teeth of the mean
subtraction, and the measurement of the bound's constant on the float64 restatement
(tests/spectra_ref.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import spectra_ref as sr
from aither_amd import abi, solver
from aither_amd.solver import MultigridSolver, PhasedSolver, Solver

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")
IDS = {"spectra_plan": 29, "spectra_sample": 30, "spectra_accum": 31, "spectra_values": 32}
METHODS = ("spectra_plan", "spectra_sample", "spectra", "spectra_download", "spectra_upload",
           "spectra_reset", "spectra_clear")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_the_header_and_abi_carry_the_four_ids():
    text = _read("include", "aither_gfx950.h")
    for name, value in IDS.items():
        assert int(re.search(r"\bAGX_FIELD_%s = (\d+)" % name.upper(), text).group(1)) == value
        assert abi.FIELD[name] == value == abi.SPECTRA_FIELD[name]
        assert name not in abi.FIELD and abi.FIELD.get(name) is None
    assert abi.SPECTRA_FIELD == IDS
    assert len(abi.FIELD) == 23 and sorted(abi.FIELD.values()) == list(range(23))
    assert abi.FIELD["series_locate"] == 28 and abi.FIELD["stat_accum"] == 24
    with pytest.raises(KeyError):
        abi.FIELD["series"]
    with pytest.raises(KeyError):
        abi.FIELD["spectra"]
    assert "spectra" not in _read("aither_amd", "csrc", "exports.map")
    limit = int(re.search(r"#define AGX_SPECTRA_MAX_N (\d+)", text).group(1))
    assert limit == abi.SPECTRA_MAX_N == sr.MAX_N >= 1024
    plan = _read("aither_amd", "csrc", "agx_spectra_plan.hpp")
    assert int(re.search(r"SPECTRA_MAX_N = (\d+)", plan).group(1)) == limit


def test_every_layer_offers_the_calls():
    for cls in (Solver, PhasedSolver, MultigridSolver):
        for m in METHODS:
            assert callable(getattr(cls, m)), (cls.__name__, m)
    assert callable(solver.pool_spectra) and callable(solver.correlation)
    hpp = _read("include", "aither_gfx950.hpp")
    for call, field in (("SetSpectraPlan", "PLAN"), ("SampleSpectra(double w)", "SAMPLE"),
                        ("Spectra(int block", "VALUES"), ("SpectraPayload", "ACCUM"),
                        ("ClearSpectra", "PLAN")):
        assert "void " + call in hpp, call
        assert "AGX_FIELD_SPECTRA_" + field in hpp
    make = _read("aither_amd", "csrc", "Makefile")
    assert "agx_spectra.hpp" in make and "agx_spectra_plan.hpp" in make
    assert '#include "agx_spectra.hpp"' in _read("aither_amd", "csrc", "agx_api.hip")


def test_payload_helpers():
    names = ["vel_x", "pressure", "temperature"]
    p = abi.spectra_plan(names, [("vel_x", "pressure"), (2, 0)], along="k", over="ij")
    assert p.tolist() == [2, 3, 3, 2, abi.OUT["vel_x"], abi.OUT["pressure"],
                          abi.OUT["temperature"], 0, 1, 2, 0]
    assert abi.spectra_plan_parse(p) == (names, [(0, 1), (2, 0)], "k", "ij")
    assert abi.spectra_plan([]).tolist() == [0, 0, 0, 0]
    assert abi.spectra_plan(["density"], along="j").tolist() == [1, 0, 1, 0, abi.OUT["density"]]
    assert abi.spectra_shape((8, 7, 5), "i", "") == ((5, 7), 5)
    assert abi.spectra_shape((8, 7, 5), "j", "k") == ((8,), 4)
    assert abi.spectra_shape((8, 7, 5), "k", "ij") == ((), 3)
    body = np.arange(5 * 2 * 4, dtype=np.float64)
    payload = np.concatenate([p, [3.5, 4.0, 2.0, 4.0], body])
    assert len(payload) == abi.spectra_accum_size(3, 2, 2, 4)
    plan, big_w, samples, s = abi.spectra_accum_split(payload)
    assert plan.tolist() == p.tolist() and (big_w, samples) == (3.5, 4.0)
    assert s.shape == (5, 2, 4) and s.ravel().tolist() == body.tolist()


def test_correlation_is_the_circular_two_point_correlation():
    rng = np.random.default_rng(5)
    for n in (2, 3, 8, 67):
        x = rng.standard_normal((2, 1, 1, n)) + np.array([0.5, -2.0])[:, None, None, None]
        # (lines along i of a 1 x 1 x n block)
        ref, _, _ = sr.reference([x], [1.0], [(0, 1)], "i", "")
        ref = ref.astype(np.float64).reshape(3, n // 2 + 1)
        got = solver.correlation(ref, n)
        assert got.shape == (3, n)
        for q, (a, b) in enumerate(((0, 0), (1, 1), (0, 1))):
            xa, xb = x[a].ravel(), x[b].ravel()
            direct = np.array([0.5 * np.mean(xa * np.roll(xb, -r) + xb * np.roll(xa, -r))
                               for r in range(n)])
            assert np.abs(got[q] - direct).max() <= 64 * n * sr.ULP * np.abs(direct).max()


def test_pool_spectra_is_one_pooled_computation():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, 3, 6, 8))          # lines along i, pooled over j
    whole, _, _ = sr.reference([x], [1.0], [(0, 1)], "i", "j")
    lo, _, _ = sr.reference([x[:, :, :4]], [1.0], [(0, 1)], "i", "j")
    hi, _, _ = sr.reference([x[:, :, 4:]], [1.0], [(0, 1)], "i", "j")
    got, weight = solver.pool_spectra([(lo.astype(np.float64), 2.0, 4),
                                       (hi.astype(np.float64), 2.0, 2)])
    assert weight == 12.0
    scale = np.abs(whole).max()
    assert np.abs(got - whole).max() <= 8 * sr.ULP * scale
    same, _ = solver.pool_spectra([(got, 1.0, 3), (got, 5.0, 7), (got, 0.5, 1)])
    assert np.array_equal(same, got)


def test_the_plan_arithmetic_under_the_sanitizers():
    subprocess.run(["make", "-C", CPP, "-f", "spectra.mk"], check=True, capture_output=True)
    exe = os.path.join(CPP, "spectra_plan")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.search(r"spectra_plan: \d+ plans walked", run.stdout)
    # the Python copy of the arithmetic (the restatement's) is the header's
    for ext in ((8, 7, 5), (67, 3, 2), (2, 3, 130), (256, 20, 9), (9, 256, 20), (1024, 5, 2),
                (66, 9, 6), (13, 37, 1)):
        for along in range(3):
            for over in range(8):
                if over >> along & 1:
                    continue
                for nvar in (1, 3, 6):
                    out = subprocess.run([exe, "shape", *map(str, ext), str(along), str(over),
                                          str(nvar)], capture_output=True, text=True, check=True)
                    s = sr.shape(ext, along, over, nvar)
                    if s is None:
                        assert out.stdout.strip() == "refused"
                        continue
                    mine = [s[k] for k in ("tl", "nt1", "ng", "steps", "nchunk", "nfix", "nbin",
                                           "nrec", "lines")]
                    mine += [sr.record_lines(s, r) for r in range(s["nrec"])]
                    assert [int(v) for v in out.stdout.split()] == mine, (ext, along, over, nvar)
    out = subprocess.run([exe, "shape", "1025", "2", "2", "0", "0", "1"], capture_output=True,
                         text=True, check=True)
    assert out.stdout.strip() == "refused" and sr.shape((1025, 2, 2), 0, 0, 1) is None


def test_a_subset_plan_restates_to_the_same_bits():
    """The grouping of lines into records does not depend on the number of variables: at
    256 x 40 x 1 along i over j the LDS limits the tile, and the restatement of a plan of three
    variables, of one of them and of six agrees bit for bit on what they share."""
    shapes = [sr.shape((256, 40, 1), 0, 2, nvar) for nvar in (1, 2, 3, 6)]
    assert all(s == shapes[0] for s in shapes) and shapes[0]["tl"] == 4
    rng = np.random.default_rng(9)
    x = rng.standard_normal((6, 1, 40, 256))
    six = sr.restate([x], [1.0], [(0, 1)], "i", "j")
    three = sr.restate([x[:3]], [1.0], [(0, 1)], "i", "j")
    one = sr.restate([x[:1]], [1.0], [], "i", "j")
    assert np.array_equal(one[0], three[0]) and np.array_equal(three[:3], six[:3])
    assert np.array_equal(three[3], six[6])


FAMILIES = ("random", "pressure", "harmonic")
SIZES = (2, 3, 7, 8, 16, 67, 130, 256)
WEIGHTS = (1.0, 0.5, 2.0, 0.25, 1.0)


def family(name, n, lines, rng):
    """One sample x[2, 1, lines, n]: lines along i of a block n x lines x 1."""
    if name == "random":
        return rng.standard_normal((2, 1, lines, n))
    if name == "pressure":
        return 1.0 + 1e-8 * rng.standard_normal((2, 1, lines, n))
    m0 = max(1, n // 3)
    phase = rng.uniform(0, 2 * np.pi, (2, 1, lines, 1))
    amp = rng.uniform(0.5, 2.0, (2, 1, lines, 1))
    return 3.0 + amp * np.cos(2 * np.pi * m0 * np.arange(n) / n + phase)


def test_the_raw_transform_misses_the_bound_by_orders():
    """The teeth: without the mean subtracted the float64 transform of 1 + 1e-8 noise misses
    the bound by orders of magnitude; with it, it holds."""
    rng = np.random.default_rng(7)
    for n in (3, 256):
        x = family("pressure", n, 1, rng)
        ref, a1, mu = sr.reference([x], [1.0], [(0, 1)], "i", "")
        lim = sr.bound(a1, mu, [(0, 1)], n, 1, 1)
        raw = sr.line_spectra(x, [(0, 1)], 0, shift=False)
        good = sr.line_spectra(x, [(0, 1)], 0)
        # (the modes m >= 1: entry 0 is the product of the means either way)
        share_raw = sr.reached(raw[..., 1:], ref[..., 1:], lim[..., 1:])
        share_good = sr.reached(good[..., 1:], ref[..., 1:], lim[..., 1:])
        print(f"N = {n}: raw transform {share_raw:.3g} of the bound, shifted {share_good:.3g}")
        assert share_good <= 1.0
        assert share_raw > 1e3


def test_the_bound_constant_is_what_the_restatement_reaches():
    """c1 measured on the float64 restatement (never on the device): the largest error over
    (N + L + n) ulp A'A' over the sizes, families, poolings and weights of the record."""
    rng = np.random.default_rng(8)
    worst = {}
    for n in SIZES:
        for fam in FAMILIES:
            for over, lines in (("", 1), ("j", 5)):
                # (the five weights of the record, and a single sample: the smallest bound)
                for weights in (WEIGHTS, WEIGHTS[:1]):
                    xs = [family(fam, n, 5, rng) for _ in weights]
                    ref, a1, mu = sr.reference(xs, weights, [(0, 1)], "i", over)
                    got = sr.restate(xs, list(weights), [(0, 1)], "i", over)
                    unit = sr.bound(a1, mu, [(0, 1)], n, lines, len(weights), c1=1.0)
                    share = sr.reached(got, ref, unit)
                    worst[n] = max(worst.get(n, 0.0), share)
    print("c1 reached per N:", {n: round(v, 3) for n, v in worst.items()})
    top = max(worst.values())
    assert top <= sr.MEASURED_C1, worst
    # (the record is the measurement, not a loose cap)
    assert top >= 0.5 * sr.MEASURED_C1, worst
    assert sr.C1 == 4 * sr.MEASURED_C1
