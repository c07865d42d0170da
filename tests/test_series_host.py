"""Time series at chosen cells and wall faces, host side: the field ids of the header and of
abi.py, the layers that offer the calls, the payload helpers, the numpy reference of the
nearest-cell search (tests/series_ref.py) and the ring arithmetic under the sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import series_ref
from aither_amd import abi, solver
from aither_amd.solver import MultigridSolver, PhasedSolver, Solver

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")
IDS = {"series_plan": 25, "series_sample": 26, "series_rows": 27, "series_locate": 28}
# literal copies: the C-ABI gains no entry and no device-only name
SYMBOLS = [
    "last_error", "version", "ctx_create", "ctx_destroy", "ctx_set_stream", "config_set",
    "block_create", "block_set_bcs", "conn_create", "setup_finalize", "state_upload",
    "field_download", "field_upload", "output_pack", "restart_pack", "state_fill",
    "state_from_cloud", "restart_unpack", "plot3d_metrics", "nearest_wall_distance",
    "mg_restrict", "mg_matrix_residual", "mg_invert_diagonal", "mg_save_update",
    "mg_reset_diagonal", "mg_prolong", "store_time_n", "iterate", "phase_bc_faces",
    "phase_bc_edges", "phase_residual", "phase_explicit_update", "phase_implicit_begin",
    "phase_relax_forward", "phase_relax_backward", "phase_matrix_residual",
    "phase_implicit_update", "halo_swap_local", "halo_count", "halo_pack", "halo_unpack",
    "set_exchange", "rccl_unique_id", "rccl_exchange_create", "halo_exchange", "timing_enable",
    "timing_get", "timing_reset", "sync"]
BLOCK_FIELDS = {
    "state", "residual", "dt", "spec_radius", "cons_n", "update", "diagonal", "temperature",
    "viscosity", "cons_nm1", "vel_grad", "temp_grad", "dens_grad", "press_grad", "volume",
    "center", "farea_i", "farea_j", "farea_k", "width_i", "width_j", "width_k", "wall_dist"}
METHODS = ("series_plan", "series_sample", "series_rows", "series_drop", "series_clear",
           "series_locate")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_the_header_and_abi_carry_the_four_ids():
    text = _read("include", "aither_gfx950.h")
    for name, value in IDS.items():
        assert int(re.search(r"\bAGX_FIELD_%s = (\d+)" % name.upper(), text).group(1)) == value
        assert abi.FIELD[name] == value == abi.SERIES_FIELD[name]
        assert name not in abi.FIELD and abi.FIELD.get(name) is None
    assert abi.SERIES_FIELD == IDS
    # iteration sees the block-shaped fields only, as before
    assert set(abi.FIELD) == BLOCK_FIELDS and len(abi.FIELD) == 23
    assert sorted(abi.FIELD.values()) == list(range(23))
    assert abi.FIELD["stat_sample"] == 23 and abi.FIELD["stat_accum"] == 24
    with pytest.raises(KeyError):
        abi.FIELD["series"]
    # the C-ABI is what it was
    assert list(abi.SYMBOLS) == SYMBOLS
    assert abi.DEVICE_ONLY == ("state_fill", "state_from_cloud", "restart_unpack")
    declared = set(re.findall(r"\bagx_(\w+)\s*\(", text.split("typedef struct agx_ctx agx_ctx;")[1]))
    assert declared == set(SYMBOLS)
    exports = _read("aither_amd", "csrc", "exports.map")
    assert "series" not in exports


def test_every_layer_offers_the_calls():
    for cls in (Solver, PhasedSolver, MultigridSolver):
        for m in METHODS:
            assert callable(getattr(cls, m)), (cls.__name__, m)
    assert callable(solver.pool_series)
    hpp = _read("include", "aither_gfx950.hpp")
    for call, field in (("SetSeriesPlan", "PLAN"), ("SampleSeries(double t)", "SAMPLE"),
                        ("SeriesRows", "ROWS"), ("DropSeriesRows", "ROWS"),
                        ("LocateCells", "LOCATE")):
        assert "void " + call in hpp, call
        assert "AGX_FIELD_SERIES_" + field in hpp
    # the library is built from the new kernels
    assert "agx_series.hpp" in _read("aither_amd", "csrc", "Makefile")
    assert '#include "agx_series.hpp"' in _read("aither_amd", "csrc", "agx_api.hip")


def test_plan_and_rows_payloads_round_trip():
    # cells: hand-made payload
    names = ["pressure", "vel_x", "velGrad_uy"]
    pts = [(0, 0, 0), (6, 4, 2), (6, 4, 2), (3, 1, 0)]
    plan = abi.series_plan(names, pts, 5)
    hand = [0, 4, 3, 5, abi.OUT["pressure"], abi.OUT["vel_x"], abi.OUT["velGrad_uy"],
            0, 0, 0, 6, 4, 2, 6, 4, 2, 3, 1, 0]
    assert plan.dtype == np.float64 and plan.tolist() == [float(v) for v in hand]
    back = abi.series_plan_parse(hand)
    assert back[0] == names and back[1].tolist() == [list(p) for p in pts]
    assert back[2:] == (5, "cells")
    # wall faces
    plan = abi.series_plan(["shearStress_x", "pressure"], [3, 0, 3], 7, kind="wall")
    assert plan.tolist() == [1.0, 3.0, 2.0, 7.0, 75.0, 70.0, 3.0, 0.0, 3.0]
    back = abi.series_plan_parse(plan)
    assert back[0] == ["shearStress_x", "pressure"] and back[1].tolist() == [3, 0, 3]
    assert back[2:] == (7, "wall")
    # no points: the payload that discards a plan
    assert abi.series_plan([], [], 1).tolist() == [0.0, 0.0, 0.0, 1.0]
    # rows: {P, V, rows, capacity}, then rows x {t, [v][p]}; the buffer holds `capacity` rows
    npts, nvar, cap = 3, 2, 4
    hand = np.array([npts, nvar, 2, cap,
                     0.5, 11, 12, 13, 21, 22, 23,
                     0.75, 111, 112, 113, 121, 122, 123] + [-7.0] * 14)
    assert hand.size == abi.series_rows_size(npts, nvar, cap)
    t, v = abi.series_rows_split(hand)
    assert t.tolist() == [0.5, 0.75] and v.shape == (2, nvar, npts)
    assert v[1].tolist() == [[111, 112, 113], [121, 122, 123]] and v[0, 1, 2] == 23
    assert np.array_equal(abi.series_rows_join(t, v, cap), hand[:4 + 2 * 7])
    t0, v0 = abi.series_rows_split(np.array([npts, nvar, 0, cap], dtype=float))
    assert t0.shape == (0,) and v0.shape == (0, nvar, npts)


def test_pool_series_keeps_the_nearest_and_the_lower_block():
    a = np.array([[0, 1, 1, 1, 4.0], [0, 2, 2, 2, 1.0], [0, 0, 0, 0, 2.0]])
    b = np.array([[1, 5, 5, 5, 3.0], [1, 6, 6, 6, 1.0], [1, 7, 7, 7, 9.0]])
    for parts in ([a, b], [b, a]):
        got = solver.pool_series(parts)
        assert got.tolist() == [b[0].tolist(), a[1].tolist(), a[2].tolist()]
    assert np.array_equal(series_ref.join({0: a[:, 1:], 1: b[:, 1:]}), solver.pool_series([a, b]))
    # the records of the two blocks back in the caller's order
    where = solver.pool_series([a, b])
    t = np.array([0.1, 0.2])
    rec_a = {0: (t, np.array([[[10.0, 20.0]], [[11.0, 21.0]]]))}      # points 1 and 2
    rec_b = {1: (t, np.array([[[30.0]], [[31.0]]]))}                  # point 0
    w2, t2, vals = solver.pool_series([a, b], records=[rec_a, rec_b])
    assert np.array_equal(w2, where) and np.array_equal(t2, t)
    assert vals.tolist() == [[[30.0, 10.0, 20.0]], [[31.0, 11.0, 21.0]]]


def test_reference_nearest_and_its_tie_rule():
    rng = np.random.default_rng(7)
    center = rng.random((3, 4, 5, 3))
    pts = np.concatenate([rng.random((40, 3)), 50.0 * rng.standard_normal((10, 3))])
    assert np.array_equal(series_ref.nearest(center, pts), series_ref.nearest_loop(center, pts))
    # exact ties on the power-of-two box: face midpoints 2 cells, edges 4, corners 8
    center, pts = series_ref.tie_box()
    got = series_ref.nearest(center, pts)
    assert np.array_equal(got, series_ref.nearest_loop(center, pts))
    flat = center.reshape(-1, 3)
    ties = []
    for x, row in zip(pts, got):
        d2 = ((flat - x) ** 2).sum(axis=1)
        tied = np.flatnonzero(d2 == d2.min())
        ties.append(tied.size)
        q = int(row[0] + 4 * (row[1] + 3 * row[2]))
        assert q == tied.min() and row[3] == d2.min()
    assert {1, 2, 4, 8} <= set(ties)


def test_reference_ring_chronology():
    ring = series_ref.Ring(3)
    for t in (0.0, 1.0, 2.0):
        ring.sample(t)
    with pytest.raises(OverflowError):
        ring.sample(3.0)
    ring.drop(2)
    ring.sample(3.0)
    ring.sample(4.0)
    assert ring.rows == [2.0, 3.0, 4.0]
    with pytest.raises(ValueError):
        ring.drop(4)


def test_ring_arithmetic_under_the_sanitizers():
    """tests/cpp/series_ring.cpp: csrc/agx_series_ring.hpp -- head, count, drop and the
    chronological unroll -- beside a std::deque, built with the address and
    undefined-behaviour sanitizers and run on the CPU."""
    subprocess.check_call(["make", "-C", CPP, "-f", "series.mk", "series_ring"],
                          stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(CPP, "series_ring")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"series_ring OK" in r.stdout
