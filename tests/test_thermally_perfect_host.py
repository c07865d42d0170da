"""Thermally perfect gas, host side (no GPU): the fixture of the reference's thermallyPerfect
case, the case build, the numpy restatement of the model (aither_amd.case.fluid), the two
thermally perfect libraries (load and exports only) -- and the CPU oracle's own statement of
the model (oracle/oracle.c), pinned on the reference's thermallyPerfect truth, which is what
the parity tests of tests/test_thermally_perfect_gpu.py hold the device to."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aither_amd
from aither_amd import abi
from aither_amd.case import fluid, synthetic
from aither_amd.case.builder import build_case, config_struct
from aither_amd.case.inputfile import parse_input
from aither_amd.solver import Solver

HERE = os.path.dirname(os.path.abspath(__file__))
TP_DIR = os.path.join(HERE, "golden", "thermallyPerfect")
TP_INP = os.path.join(TP_DIR, "thermallyPerfect.inp")
CASES = os.path.join(HERE, "golden", "cases")
TRUTH = [5.8177e-01, 3.8066e-01, 4.8670e-01, 1.0000e+00, 5.9931e-01, 1.2830e-06, 3.5031e-04]


def test_fixture_digests_and_truth_record():
    spec = json.load(open(os.path.join(TP_DIR, "truth.json")))
    assert spec["truth"] == TRUTH
    assert spec["iterations"] == 20 and spec["ignore"] == [3] and spec["line"] == 468
    for f in ("thermallyPerfect.inp", "thermallyPerfect.xyz"):
        data = open(os.path.join(TP_DIR, f), "rb").read()
        assert hashlib.sha256(data).hexdigest() == spec["sha256"][f], f
    out = subprocess.check_output([sys.executable, os.path.join(TP_DIR, "make_fixture.py"),
                                   "--manifest"], text=True)
    assert "matches truth.json" in out


def test_truth_deck_builds_thermally_perfect():
    case = build_case(TP_INP)
    assert case.n_eq == 7 and case.ng == 1 and len(case.blocks) == 1
    assert tuple(case.blocks[0].geom.n) == (120, 150, 1)
    cfg = config_struct(case)
    assert cfg.thermodynamic_model == abi.THERMO["thermallyPerfect"] == 1
    assert cfg.gas.n_vib == 1 and cfg.gas.theta_v[0] == 3056.0 / 2000.0
    assert list(cfg.gas.theta_v[1:]) == [0.0] * (abi.MAX_VIB - 1)
    # a_ref and R stay the calorically perfect ones (input.cpp:608-613)
    cpg = fluid.make_gas("air", 2000.0, 0.4, 1.0)
    assert cfg.gas.a_ref == cpg.a_ref and cfg.gas.gas_constant == cpg.gas_constant


@pytest.mark.parametrize("name", sorted(os.listdir(CASES)))
def test_existing_decks_stay_calorically_perfect(name):
    path = os.path.join(CASES, name, name + ".inp")
    deck = parse_input(path)
    deck.multigrid_levels = 1       # (the finest level; the gas does not depend on it)
    cfg = config_struct(build_case(path, deck=deck))
    assert cfg.thermodynamic_model == 0 and cfg.gas.n_vib == 0
    assert list(cfg.gas.theta_v) == [0.0] * abi.MAX_VIB


def test_validate_accepts_thermally_perfect_by_name_only():
    deck = synthetic.make_deck(thermodynamic_model="thermallyPerfect")
    deck.validate()
    deck.thermodynamic_model = "frozenChemistry"
    with pytest.raises(NotImplementedError, match="thermodynamicModel frozenChemistry"):
        deck.validate()


@pytest.fixture
def air():
    return fluid.make_gas("air", 2000.0, 0.4, 1.0, "thermallyPerfect")


def test_cv_limits(air):
    r, n = air.gas_constant, air.n
    # T -> 0: the vibrational mode is frozen; T -> infinity: fully excited (+R)
    assert abs(fluid.cv(air, 1.0e-3) / (n * r) - 1.0) < 1e-14
    assert abs(fluid.cv(air, 1.0e5) / ((n + 1.0) * r) - 1.0) < 1e-9
    t = np.geomspace(1.0e-3, 1.0e5, 400)
    c = fluid.cv(air, t)
    assert np.all(c >= n * r) and np.all(c <= (n + 1.0) * r)
    np.testing.assert_allclose(fluid.cp(air, t), c + r, rtol=1e-15)
    np.testing.assert_allclose(fluid.gamma(air, t), (c + r) / c, rtol=1e-15)
    # without vibrational modes: the calorically perfect constants
    cpg = fluid.make_gas("air", 2000.0, 0.4, 1.0)
    assert np.all(fluid.cv(cpg, t) == n * r)


def test_energy_derivative_is_cv(air):
    t = np.geomspace(0.01, 50.0, 200)
    h = 1.0e-5 * t
    de = (fluid.spec_energy(air, t + h) - fluid.spec_energy(air, t - h)) / (2.0 * h)
    np.testing.assert_allclose(de, fluid.cv(air, t), rtol=1e-8)


def test_temperature_from_energy_inverts_spec_energy(air):
    t = np.geomspace(0.01, 50.0, 2001)
    got = fluid.temperature_from_energy(air, fluid.spec_energy(air, t))
    np.testing.assert_allclose(got, t, rtol=1e-13, atol=0.0)


def test_tp_libraries_export_exactly_the_c_abi():
    for path in (aither_amd.TP_LIB_PATH, aither_amd.RANS_TP_LIB_PATH):
        assert os.path.exists(path), "not built: run __graft_entry__.build()"
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        names = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
        assert names and all(n.startswith("agx_") for n in names)
        assert {n[4:] for n in names} == set(abi.SYMBOLS)


def test_all_four_libraries_load_global_in_one_process():
    code = ("import ctypes, sys\n"
            "libs = [ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL) for p in sys.argv[1:]]\n"
            "for l in libs:\n"
            "    l.agx_version.restype = ctypes.c_char_p\n"
            "print('|'.join(l.agx_version().decode() for l in libs))\n")
    paths = [aither_amd.LIB_PATH, aither_amd.RANS_LIB_PATH, aither_amd.TP_LIB_PATH,
             aither_amd.RANS_TP_LIB_PATH]
    out = subprocess.check_output([sys.executable, "-c", code, *paths], text=True)
    versions = out.strip().split("|")
    assert len(versions) == 4 and all("gfx950" in v for v in versions)
    assert ["thermallyPerfect" in v for v in versions] == [False, False, True, True]


def test_loader_picks_the_library_of_the_model():
    assert aither_amd.lib_path(5) == aither_amd.LIB_PATH
    assert aither_amd.lib_path(7) == aither_amd.RANS_LIB_PATH
    assert aither_amd.lib_path(5, "thermallyPerfect") == aither_amd.TP_LIB_PATH
    assert aither_amd.lib_path(7, "thermallyPerfect") == aither_amd.RANS_TP_LIB_PATH
    with pytest.raises(ValueError, match="thermodynamic_model"):
        aither_amd.load(5, "thermallyImperfect")
    with pytest.raises(ValueError, match="n_eq"):
        aither_amd.lib_path(6, "thermallyPerfect")
    api = aither_amd.load(7, "thermallyPerfect")
    assert b"thermallyPerfect" in api.version()
    assert aither_amd.load(7, "thermallyPerfect") is api and aither_amd.load(7) is not api
    # the environment overrides, as for the other two libraries
    code = "import aither_amd; print(aither_amd.lib_path(5, 'thermallyPerfect'))"
    env = dict(os.environ, AGX_TP_LIB="/elsewhere/libtp.so")
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env,
                                  cwd=os.path.dirname(HERE))
    assert out.strip() == "/elsewhere/libtp.so"


# ---- the oracle's thermally perfect gas -------------------------------------------------
TP, CP = "thermallyPerfect", "caloricallyPerfect"


def test_oracle_reproduces_the_thermally_perfect_truth(oracle):
    """20 free-running iterations of the reference's thermallyPerfect deck through the oracle:
    the reference's own 1 % (regressionTests.py:108-112) and every printed digit; index 3 is
    ignored as recorded.  (As a calorically perfect gas the deck gives 6.1462e-01 for the
    first entry against 5.8177e-01.)  The oracle's energy -> temperature root is Ridders'
    method iterated to round-off instead of the reference's 1e-8: it moves no digit."""
    spec = json.load(open(os.path.join(TP_DIR, "truth.json")))
    sol = Solver(oracle, build_case(TP_INP))
    out = sol.run(spec["iterations"])
    sol.close()
    for idx, (g, t) in enumerate(zip(out["norm"], spec["truth"])):
        if idx in spec["ignore"]:
            continue
        assert abs(g - t) <= 0.01 * t, (idx, g, t)
        assert f"{g:.4e}" == f"{t:.4e}", (idx, g, t)


def _temperature_sweep(case):
    """the case's state with T = 0.1 .. 5 t_ref over its physical cells (air at t_ref =
    288.15 K: theta / T = 106 .. 2.1)"""
    gas, g = case.gas, case.ng
    st = case.blocks[0].state.copy()
    inner = st[g:-g, g:-g, g:-g]
    t = np.geomspace(0.1, 5.0, inner[..., 0].size).reshape(inner.shape[:3])
    inner[..., 4] = inner[..., 0] * gas.gas_constant * t
    return st, inner, t


def test_oracle_output_pack_pointwise(oracle):
    """T, sos, mach, energy, enthalpy, cp, cv of ora_output_pack against the numpy model --
    the sweep test_output_pack_pointwise makes on the device."""
    case = synthetic.single_block_case((16, 12, 10), thermodynamic_model=TP,
                                       time_integration="explicitEuler", cfl=0.3)
    gas = case.gas
    st, inner, _ = _temperature_sweep(case)
    sol = Solver(oracle, case)
    sol.upload("state", 0, st)
    names = ["temperature", "sos", "mach", "energy", "enthalpy", "cp", "cv"]
    got = dict(zip(names, sol.output_pack(0, names)))
    sol.close()
    rho, p = inner[..., 0], inner[..., 4]
    tt = p / (rho * gas.gas_constant)
    a_r, t_r = gas.a_ref, gas.t_ref
    v2 = (inner[..., 1:4] ** 2).sum(-1)
    cs = np.sqrt(fluid.gamma(gas, tt) * p / rho)
    e = fluid.spec_energy(gas, tt) + 0.5 * v2
    want = dict(temperature=tt * t_r, sos=cs * a_r, mach=np.sqrt(v2) / cs, energy=e * a_r ** 2,
                enthalpy=(e + p / rho) * a_r ** 2, cp=fluid.cp(gas, tt) * a_r ** 2 / t_r,
                cv=fluid.cv(gas, tt) * a_r ** 2 / t_r)
    for n in names:
        np.testing.assert_allclose(got[n], want[n], rtol=1e-12, atol=0.0, err_msg=n)
    cvs = want["cv"] / (a_r ** 2 / t_r) / gas.gas_constant
    assert cvs.min() < gas.n + 1e-6 and cvs.max() > gas.n + 0.6


def test_oracle_temperature_from_energy_root(oracle):
    """The oracle's energy -> temperature root: conserved variables whose energy is the numpy
    model's spec_energy(T), T = 0.1 .. 5 t_ref, go in as the state at time n of an RK stage
    with a zero residual (u = consVarsN - dt / V alpha R, procBlock.cpp:935-950); the
    primitive state that comes out has T to 1e-13."""
    case = synthetic.single_block_case((16, 12, 10), thermodynamic_model=TP,
                                       time_integration="rk4", cfl=0.5)
    gas = case.gas
    st, inner, t = _temperature_sweep(case)
    cons = np.empty_like(inner)
    cons[..., 0] = inner[..., 0]
    cons[..., 1:4] = inner[..., 0:1] * inner[..., 1:4]
    cons[..., 4] = inner[..., 0] * (fluid.spec_energy(gas, t) + 0.5 * (inner[..., 1:4] ** 2).sum(-1))
    sol = Solver(oracle, case)
    g = case.ng
    sol.upload("cons_n", 0, cons)
    sol.upload("residual", 0, np.zeros_like(cons))
    sol.upload("dt", 0, np.ones(cons.shape[:3] + (1,)))
    l2, linf = np.zeros(5), abi.Linf()
    oracle.check(oracle.phase_explicit_update(sol.ctx, 0, l2.ctypes.data_as(abi.c_dp),
                                              C.byref(linf)), "explicit_update")
    new = sol.download("state", 0)[g:-g, g:-g, g:-g]
    sol.close()
    got = new[..., 4] / (new[..., 0] * gas.gas_constant)
    np.testing.assert_allclose(got, t, rtol=1e-13, atol=0.0)
    np.testing.assert_allclose(new[..., :4], inner[..., :4], rtol=1e-15, atol=1e-300)


ORACLE_WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
               4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
ORACLE_DECKS = {
    "weno_visc_lusgs": dict(bcs=ORACLE_WALL, equation_set="navierStokes",
                            face_reconstruction="weno", limiter="none", inviscid_flux="ausm",
                            time_integration="implicitEuler", matrix_sweeps=2, cfl=10.0),
    "rans_blusgs": dict(bcs=ORACLE_WALL, equation_set="rans", turbulence_model="sst2003",
                        time_integration="implicitEuler", matrix_solver="blusgs", cfl=10.0),
    "roe_bdf2_dplur": dict(time_integration="bdf2", nonlinear_iterations=2, dt=2.0e-5,
                           dual_time_cfl=100.0, matrix_solver="dplur", matrix_sweeps=3),
}


def _oracle_run(oracle, case, steps=2):
    sol = Solver(oracle, case)
    for nn in range(steps):
        sol.step(nn)
    out = (sol.download("state", 0).copy(), sol.download("residual", 0).copy(),
           np.array([h["l2"] for h in sol.history]), [h["matrix"] for h in sol.history])
    sol.close()
    return out


@pytest.mark.parametrize("kind", sorted(ORACLE_DECKS))
def test_oracle_frozen_is_calorically_perfect_bit_for_bit(oracle, kind):
    """A thermally perfect gas without a vibrational mode IS the calorically perfect one: the
    oracle gives the same bits for both configs (the oracle-side twin of the device's
    test_no_vibration_* tests)."""
    make = lambda m: synthetic.single_block_case((10, 9, 8), stretch=1.2,
                                                 thermodynamic_model=m, **ORACLE_DECKS[kind])
    frozen = make(TP)
    frozen.gas.theta_v = []
    cfg = config_struct(frozen)
    assert cfg.thermodynamic_model == abi.THERMO[TP] and cfg.gas.n_vib == 0
    a, b = _oracle_run(oracle, make(CP)), _oracle_run(oracle, frozen)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3] == b[3]
    # ... and with the mode the same deck is another computation
    c = _oracle_run(oracle, make(TP))
    assert not np.array_equal(a[1], c[1])


def _ora_config_set(oracle, cfg):
    ctx = C.c_void_p()
    oracle.check(oracle.ctx_create(0, 0, C.byref(ctx)), "ctx_create")
    try:
        rc = oracle.config_set(ctx, C.byref(cfg))
        return rc, (oracle.last_error() or b"") if rc else b""
    finally:
        oracle.ctx_destroy(ctx)


def test_oracle_config_refusals(oracle):
    """ora_config_set refuses what the oracle does not restate, instead of running it as a
    calorically perfect gas."""
    case = synthetic.single_block_case((6, 5, 4), thermodynamic_model=TP,
                                       time_integration="implicitEuler", cfl=5.0)
    cfg = config_struct(case)
    assert _ora_config_set(oracle, cfg)[0] == 0
    cfg.gas.n_vib = 0                                  # (the frozen gas of the tests above)
    assert _ora_config_set(oracle, cfg)[0] == 0
    cfg.gas.n_vib = abi.MAX_VIB + 1
    rc, msg = _ora_config_set(oracle, cfg)
    assert rc != 0 and b"n_vib" in msg and b"AGX_MAX_VIB" in msg, msg
    cfg.gas.n_vib = -1
    rc, msg = _ora_config_set(oracle, cfg)
    assert rc != 0 and b"n_vib" in msg, msg
    cfg.gas.n_vib = 1
    cfg.thermodynamic_model = abi.THERMO[CP]
    rc, msg = _ora_config_set(oracle, cfg)
    assert rc != 0 and b"calorically perfect" in msg and b"n_vib" in msg, msg
    cfg.thermodynamic_model = 2
    rc, msg = _ora_config_set(oracle, cfg)
    assert rc != 0 and b"thermodynamic_model 2" in msg, msg
    cfg.thermodynamic_model = abi.THERMO[TP]
    cfg.gas.theta_v[0] = 0.0
    rc, msg = _ora_config_set(oracle, cfg)
    assert rc != 0 and b"theta_v" in msg, msg
    cfg.thermodynamic_model = abi.THERMO[CP]
    cfg.gas.n_vib = 0
    assert _ora_config_set(oracle, cfg)[0] == 0


def test_oracle_model_takes_effect_on_a_hot_case(oracle):
    """The parity tests of tests/test_thermally_perfect_gpu.py can fail: a hot case of
    tests/tp_cases.py (vibrational share of cv >= 0.10 in every cell, asserted by its helper)
    run through the oracle thermally and calorically perfect gives residuals that differ by
    more than 1e-3 relative -- seven orders above the parity bound."""
    import tp_cases
    deck = tp_cases.FIVE["weno_ausm_visc_lusgs"]
    tp = _oracle_run(oracle, tp_cases.hot_single(TP, **deck), steps=3)
    cp = _oracle_run(oracle, tp_cases.hot_single(CP, **deck), steps=3)
    d = np.abs(tp[2][-1] - cp[2][-1]) / np.abs(cp[2][-1])
    assert d.max() > 1e-3, d
    # the first residual, from the same initial state: the fluxes alone
    d0 = np.abs(tp[2][0] - cp[2][0]) / np.abs(cp[2][0])
    assert d0.max() > 1e-3, d0
    # and the condition holds for every case the GPU module runs (cheap: numpy only)
    for kw in tp_cases.FIVE.values():
        tp_cases.hot_single(**kw)
    for name in tp_cases.RANS:
        tp_cases.rans_case(name)
    with pytest.raises(AssertionError):
        tp_cases.excited(synthetic.single_block_case((6, 5, 4), thermodynamic_model=TP))
