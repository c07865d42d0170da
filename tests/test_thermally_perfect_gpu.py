"""Thermally perfect gas on the MI355X (libaither_gfx950_tp.so, libaither_gfx950_rans_tp.so).

First line of defence: parity of the two libraries with the CPU oracle WITH THE VIBRATIONAL
MODE ACTIVE (test_tp_* below): the oracle carries the model as an independent restatement of
the reference, pinned on the reference's thermallyPerfect truth
(tests/test_thermally_perfect_host.py), and every row of DESIGN section 8's device-site table is
reached by a hot (~2000 K) case of tests/tp_cases.py at parity_utils.RTOL.

Beside it: the reference's truth reproduced by the HIP library alone; each library's refusal
of the other model; the device thermodynamics pointwise and through one explicit update
against the numpy restatement (aither_amd.case.fluid).  Second line of defence: with no
vibrational mode, where the model is the calorically perfect gas, the `_tp` builds against
their calorically perfect siblings (test_no_vibration_*)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import aither_amd
from aither_amd import abi
from aither_amd.case import fluid, synthetic
from aither_amd.case.builder import build_case, config_struct
from aither_amd.case.inputfile import parse_input
from aither_amd.solver import MultigridSolver, Solver
from parity_utils import RTOL, assert_components, flux_scale, rel_err, run_pair
import tp_cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TP_DIR = os.path.join(HERE, "golden", "thermallyPerfect")
TP_INP = os.path.join(TP_DIR, "thermallyPerfect.inp")
TP, CP = "thermallyPerfect", "caloricallyPerfect"

FARFIELD = {s: ("characteristic", 1) for s in range(1, 7)}
WALL_J = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("pressureOutlet", 3),
          4: ("characteristic", 1)}
WALL_ISO = {3: ("viscousWall", 4), 4: ("viscousWall", 2),
            1: ("characteristic", 1), 2: ("characteristic", 1)}
RANS_WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
             4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}


def test_reference_truth():
    """20 free-running iterations of the reference's thermallyPerfect deck (SST 2003, LU-SGS,
    supersonic ramp, air with a vibrational mode) reproduce its truth vector
    (regressionTests.py:463-471) to the printed digits."""
    spec = json.load(open(os.path.join(TP_DIR, "truth.json")))
    sol = Solver(aither_amd.load(7, TP), build_case(TP_INP))
    out = sol.run(spec["iterations"])
    sol.close()
    for idx, (got, t) in enumerate(zip(out["norm"], spec["truth"])):
        if idx in spec["ignore"]:
            continue
        assert f"{got:.4e}" == f"{t:.4e}", (idx, got, t)


def _config_set(api, cfg):
    ctx = C.c_void_p()
    api.check(api.ctx_create(0, 0, C.byref(ctx)), "ctx_create")
    try:
        rc = api.config_set(ctx, C.byref(cfg))
        return rc, api.last_error() or b""
    finally:
        api.ctx_destroy(ctx)


@pytest.mark.parametrize("n_eq", [5, 7])
def test_each_library_refuses_the_other_model(n_eq):
    kw = dict(equation_set="rans", turbulence_model="sst2003", bcs=RANS_WALL) if n_eq == 7 else {}
    case = synthetic.single_block_case((6, 5, 4), thermodynamic_model=TP,
                                       time_integration="implicitEuler", cfl=5.0, **kw)
    cfg = config_struct(case)
    tp, cp = aither_amd.load(n_eq, TP), aither_amd.load(n_eq, CP)
    rc, msg = _config_set(tp, cfg)
    assert rc == 0, msg
    rc, msg = _config_set(cp, cfg)
    assert rc != 0 and b"_tp.so" in msg, msg
    cfg.thermodynamic_model = abi.THERMO[CP]
    cfg.gas.n_vib = 0
    rc, msg = _config_set(cp, cfg)
    assert rc == 0, msg
    rc, msg = _config_set(tp, cfg)
    assert rc != 0 and b"thermally perfect" in msg, msg
    cfg.thermodynamic_model = abi.THERMO[TP]
    cfg.gas.n_vib = abi.MAX_VIB + 1
    rc, msg = _config_set(tp, cfg)
    assert rc != 0 and b"n_vib" in msg, msg


def _rho_e(gas, s):
    """rho E of primitive states [..., rho u v w p] with the numpy model"""
    t = s[..., 4] / (s[..., 0] * gas.gas_constant)
    return s[..., 0] * (fluid.spec_energy(gas, t) + 0.5 * (s[..., 1:4] ** 2).sum(-1))


def test_output_pack_pointwise():
    """Temperature, sos, mach, energy, enthalpy, cp and cv of states whose T spans 0.1-5
    t_ref (air at t_ref = 288.15 K: theta / T = 106 .. 2.1) against the numpy model."""
    case = synthetic.single_block_case((16, 12, 10), thermodynamic_model=TP,
                                       time_integration="explicitEuler", cfl=0.3)
    gas, g = case.gas, case.ng
    st = case.blocks[0].state.copy()
    inner = st[g:-g, g:-g, g:-g]
    t = np.geomspace(0.1, 5.0, inner[..., 0].size).reshape(inner.shape[:3])
    inner[..., 4] = inner[..., 0] * gas.gas_constant * t
    sol = Solver(aither_amd.load(5, TP), case)
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
    # the range runs from the frozen mode (cv = n R) to a mostly excited one (cv ~ (n + 0.7) R)
    cvs = want["cv"] / (a_r ** 2 / t_r) / gas.gas_constant
    assert cvs.min() < gas.n + 1e-6 and cvs.max() > gas.n + 0.6


def test_explicit_update_takes_temperature_from_energy():
    """One explicit Euler step (procBlock.cpp:892): rho E of the new primitive state, formed
    by the numpy model, equals rho E_old - dt / V R_E -- the device's energy -> temperature
    root checked directly, at T ~ 6 t_ref where the vibrational energy is ~10 % of e."""
    case = synthetic.single_block_case((10, 9, 8), stretch=1.1, bcs=WALL_J,
                                       equation_set="navierStokes", thermodynamic_model=TP,
                                       time_integration="explicitEuler", cfl=0.3)
    gas, g = case.gas, case.ng
    ni, nj, nk = case.blocks[0].geom.n
    st = case.blocks[0].state.copy()
    st[..., 4] *= 6.0
    sol = Solver(aither_amd.load(5, TP), case)
    sol.upload("state", 0, st)
    old = sol.download("state", 0)[g:-g, g:-g, g:-g]
    sol.step(0)
    new = sol.download("state", 0)[g:-g, g:-g, g:-g]
    res = sol.download("residual", 0)
    dt = sol.download("dt", 0)[..., 0]
    sol.close()
    vol = np.asarray(case.blocks[0].geom.vol.a).reshape(nk + 2 * g, nj + 2 * g, ni + 2 * g)
    vol = vol[g:-g, g:-g, g:-g]
    want = _rho_e(gas, old) - dt / vol * res[..., 4]
    got = _rho_e(gas, new)
    assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()
    # (the momentum update, for the record: the same step)
    np.testing.assert_allclose(new[..., 0] * new[..., 1],
                               old[..., 0] * old[..., 1] - dt / vol * res[..., 1],
                               rtol=0, atol=1e-12 * np.abs(old[..., 0] * old[..., 1]).max())


# ---- no vibrational mode: the thermally perfect build against its calorically perfect
# sibling, per time step from identical inputs (as tests/parity_utils.run_pair does
# against the oracle) -------------------------------------------------------------------
SYNC_FIELDS = ("state", "cons_n", "cons_nm1", "update")


def _frozen(case):
    """the case's gas as a thermally perfect gas without vibrational modes"""
    case.gas.theta_v = []
    return case


def _stagnation_case(model):
    return tp_cases.stagnation_case(model)


def _pair(n_eq, make, steps=3, outputs=False):
    c_cp, c_tp = make(CP), _frozen(make(TP))
    sc, st = Solver(aither_amd.load(n_eq, CP), c_cp), Solver(aither_amd.load(n_eq, TP), c_tp)
    ng = c_cp.ng
    rfloor = 1.0e-3 * flux_scale(c_cp)
    nfloor = rfloor * np.sqrt(c_cp.total_cells)
    nh = 0
    for nn in range(steps):
        if nn > 0:
            for gb in sc.block_ids:
                for f in SYNC_FIELDS:
                    st.upload(f, gb, sc.download(f, gb))
                sc.upload("state", gb, sc.download("state", gb))
            st.l2_first = None if sc.l2_first is None else sc.l2_first.copy()
        # (the floors of the norms and the residual: from the state the step starts with)
        start = [sc.download("state", gb) for gb in sc.block_ids]
        sc.step(nn), st.step(nn)
        assert len(sc.history) == len(st.history)
        ref = [sc.download("state", gb) for gb in sc.block_ids]
        for hc, ht in zip(sc.history[nh:], st.history[nh:]):
            e = rel_err(ht["l2"][None, :], hc["l2"][None, :], nfloor)
            assert e < RTOL, ("L2", nn, e)
            assert_components(c_cp, "l2", ht["l2"][None, :], hc["l2"][None, :], start, (nn,))
        nh = len(sc.history)
        # every component on its own scale (parity_utils.component_err), over all blocks
        core = lambda x: x[ng:-ng, ng:-ng, ng:-ng]
        assert_components(c_cp, "state", [core(st.download("state", gb)) for gb in sc.block_ids],
                          [core(x) for x in ref], ref, (nn,))
        assert_components(c_cp, "residual", [st.download("residual", gb) for gb in sc.block_ids],
                          [sc.download("residual", gb) for gb in sc.block_ids], start, (nn,))
        for gb in sc.block_ids:
            for f in ("state", "residual", "dt"):
                a, b = st.download(f, gb), sc.download(f, gb)
                if f == "state":
                    a, b = a[ng:-ng, ng:-ng, ng:-ng], b[ng:-ng, ng:-ng, ng:-ng]
                e = rel_err(a, b, rfloor if f == "residual" else 0.0)
                assert e < RTOL, (f, gb, nn, e)
    if outputs:
        names = ["density", "pressure", "mach", "sos", "temperature", "energy", "enthalpy",
                 "cp", "cv", "viscosity"]
        for x, y, n in zip(st.output_pack(0, names), sc.output_pack(0, names), names):
            assert np.abs(x - y).max() <= RTOL * np.abs(y).max(), n
    sc.close(), st.close()


FIVE = {
    "muscl_roe_rk4": dict(n=(10, 9, 8), stretch=1.2, skew=0.01, time_integration="rk4",
                          cfl=0.5),
    "weno_ausm_visc_lusgs": dict(n=(10, 9, 8), stretch=1.2, bcs=WALL_J,
                                 equation_set="navierStokes", face_reconstruction="weno",
                                 limiter="none", inviscid_flux="ausm",
                                 time_integration="implicitEuler", matrix_solver="lusgs",
                                 cfl=10.0),
    "dplur_muscl_ausm": dict(n=(10, 9, 8), stretch=1.1, bcs=FARFIELD, inviscid_flux="ausm",
                             limiter="none", time_integration="implicitEuler",
                             matrix_solver="dplur", matrix_sweeps=4, cfl=50.0),
    "wenoz_roe_bdf2_dual": dict(n=(10, 9, 8), stretch=1.1, face_reconstruction="wenoZ",
                                limiter="none", time_integration="bdf2",
                                nonlinear_iterations=3, dt=2.0e-5, dual_time_cfl=100.0,
                                matrix_sweeps=2),
    "bdplur_visc_iso_wall": dict(n=(9, 9, 8), stretch=1.15, bcs=WALL_ISO,
                                 equation_set="navierStokes", time_integration="implicitEuler",
                                 matrix_solver="bdplur", matrix_sweeps=3, cfl=5.0),
}
RANS = {
    "sst_blusgs": dict(matrix_solver="blusgs", matrix_sweeps=2),
    "sst_bdplur": dict(matrix_solver="bdplur", matrix_sweeps=3, inviscid_flux="ausm"),
    "wilcox2006_lusgs": dict(turbulence_model="kOmegaWilcox2006", matrix_solver="lusgs",
                             matrix_sweeps=2),
    "sst_wall_law": dict(matrix_solver="lusgs", wall_treatment="wallLaw"),
}


@pytest.mark.parametrize("name", sorted(FIVE))
def test_no_vibration_matches_calorically_perfect(name):
    _pair(5, lambda m: synthetic.single_block_case(thermodynamic_model=m, **FIVE[name]),
          outputs=name == "weno_ausm_visc_lusgs")


def test_no_vibration_stagnation_inlet_nonreflecting_outlet():
    _pair(5, _stagnation_case)


@pytest.mark.parametrize("name", sorted(RANS))
def test_no_vibration_matches_calorically_perfect_rans(name):
    deck = dict(n=(9, 8, 7), stretch=1.2, bcs=RANS_WALL, equation_set="rans",
                turbulence_model="sst2003", time_integration="implicitEuler", cfl=10.0)
    deck.update(RANS[name])
    _pair(7, lambda m: synthetic.single_block_case(thermodynamic_model=m, **deck))


def test_no_vibration_multigrid_v_cycle():
    kw = dict(n=(12, 10, 8), nblocks=1, axis="i", stretch=1.1, levels=2, cycle="V",
              time_integration="implicitEuler", matrix_solver="dplur", matrix_sweeps=4,
              cfl=40.0)
    cc, tc = synthetic.multigrid_levels(thermodynamic_model=CP, **kw)
    ct, tt = synthetic.multigrid_levels(thermodynamic_model=TP, **kw)
    for c in ct:
        _frozen(c)
    sc = MultigridSolver(aither_amd.load(5, CP), cc, tc)
    st = MultigridSolver(aither_amd.load(5, TP), ct, tt)
    oc, ot = sc.step(0), st.step(0)
    assert rel_err(ot["l2"][None, :], oc["l2"][None, :]) < RTOL
    g = cc[0].ng
    a = st.download("state", 0)[g:-g, g:-g, g:-g]
    b = sc.download("state", 0)[g:-g, g:-g, g:-g]
    assert rel_err(a, b) < RTOL
    sc.close(), st.close()


def test_the_model_takes_effect():
    """The truth deck switched to caloricallyPerfect on the plain rans library: residuals
    differ from the thermally perfect ones by more than 1e-3 relative."""
    tp = Solver(aither_amd.load(7, TP), build_case(TP_INP))
    deck = parse_input(TP_INP)
    deck.thermodynamic_model = CP
    cp = Solver(aither_amd.load(7, CP), build_case(TP_INP, deck=deck))
    for nn in range(3):
        tp.step(nn), cp.step(nn)
    a, b = tp.history[-1]["l2"], cp.history[-1]["l2"]
    tp.close(), cp.close()
    d = np.abs(a - b) / np.abs(b)
    assert np.max(d[:5]) > 1e-3, d


# ---- the vibrational mode active: the `_tp` libraries against the oracle -----------------
# parity_utils.run_pair unchanged: per time step from identical inputs, state / residual /
# dt, L2 and Linf norms and the derived matrix-residual bound, all at parity_utils.RTOL.
# Every case comes from tests/tp_cases.py, which asserts that the mode is excited in every
# cell and names the rows of DESIGN section 8's device-site table the case reaches.
def _report(name, sg, so, case):
    """worst relative error of the last step, printed (-s) for DESIGN section 8"""
    g = case.ng
    rfloor = 1.0e-3 * flux_scale(case)
    worst = {}
    for gb in sg.block_ids:
        for f in ("state", "residual", "dt"):
            a, b = sg.download(f, gb), so.download(f, gb)
            if f == "state":
                a, b = a[g:-g, g:-g, g:-g], b[g:-g, g:-g, g:-g]
            worst[f] = max(worst.get(f, 0.0), rel_err(a, b, rfloor if f == "residual" else 0.0))
    print("TP-PARITY", name, " ".join(f"{k}={v:.2e}" for k, v in worst.items()))


# (stacked blocks lie one period of the perturbation apart: at step 0 the maxima of the two
# blocks agree to round-off, the L-inf location of that entry -- one of two -- is undecided)
STACKED_UNDECIDED = 1 / 2


def _run(name, n_eq, oracle, case, steps=3, **kw):
    sg, so = run_pair(aither_amd.load(n_eq, TP), oracle, case, steps, **kw)
    _report(name, sg, so, case)
    sg.close(), so.close()


def test_tp_truth_deck_per_iteration(oracle):
    """The truth deck itself (Roe + minmod MUSCL, SST 2003, LU-SGS, supersonic ramp), per
    iteration from identical inputs: localises what the five-digit truth only sums up."""
    _run("truth_deck", 7, oracle, tp_cases.excited(build_case(TP_INP)))


@pytest.mark.parametrize("name", sorted(tp_cases.FIVE))
def test_tp_five_equation_parity(oracle, name):
    _run(name, 5, oracle, tp_cases.hot_single(**tp_cases.FIVE[name]))


def test_tp_stagnation_inlet_nonreflecting_outlet_parity(oracle):
    """stagnation inlet gamma(T_interior), nonreflecting outlet gamma(T_n)
    (ghostStates.cpp:538-558, 633) -- _stagnation_case, unfrozen and hot"""
    _run("stagnation", 5, oracle, tp_cases.excited(tp_cases.stagnation_case(TP, tp_cases.HOT)))


@pytest.mark.parametrize("name", sorted(tp_cases.RANS))
def test_tp_rans_parity(oracle, name):
    _run(name, 7, oracle, tp_cases.rans_case(name))


@pytest.mark.parametrize("vel", tp_cases.RANS_BOX_VELOCITIES)
def test_tp_rans_inlet_and_supersonic_boundaries_parity(oracle, vel):
    _run(f"rans_box_{vel[0]:.0f}", 7, oracle, tp_cases.rans_box_case(vel))


@pytest.mark.parametrize("tag,solver", tp_cases.WALL_LAW)
def test_tp_wall_law_parity(oracle, tag, solver):
    _run(f"wall_law_{tag}_{solver}", 7, oracle, tp_cases.wall_law_case(tag, solver))


def test_tp_stacked_blocks_parity_five(oracle):
    _run("stacked_blusgs_visc", 5, oracle, tp_cases.stacked_five(), steps=2,
         linf_undecided=STACKED_UNDECIDED)


def test_tp_stacked_blocks_parity_rans(oracle):
    _run("stacked_rans_lusgs", 7, oracle, tp_cases.stacked_rans(), steps=2,
         linf_undecided=STACKED_UNDECIDED)


def _multigrid(n_eq, oracle, make, matrix_rtol, update_by_largest):
    cg, tg = make()
    co, to = make()
    sg = MultigridSolver(aither_amd.load(n_eq, TP), cg, tg)
    so = MultigridSolver(oracle, co, to)
    g, levels, nblocks = cg[0].ng, len(cg), len(cg[0].blocks)
    worst = dict(l2=0.0, matrix=0.0, state=0.0, update=0.0)
    for nn in range(3):
        og, oo = sg.step(nn), so.step(nn)
        worst["l2"] = max(worst["l2"], float((np.abs(og["l2"] - oo["l2"]) / oo["l2"]).max()))
        worst["matrix"] = max(worst["matrix"], abs(og["matrix"] - oo["matrix"]) / oo["matrix"])
        print("TP-PARITY multigrid", n_eq, nn, worst)
        assert np.allclose(og["l2"], oo["l2"], rtol=1e-9, atol=1e-12 * oo["l2"].max())
        assert abs(og["matrix"] - oo["matrix"]) <= matrix_rtol * oo["matrix"]
        scale = max(np.abs(so.download("update", gb, lev)).max()
                    for lev in range(levels) for gb in range(nblocks))
        for lev in range(levels):
            for gb in range(nblocks):
                a = sg.download("state", gb, lev)[g:-g, g:-g, g:-g]
                b = so.download("state", gb, lev)[g:-g, g:-g, g:-g]
                e = rel_err(a, b)
                worst["state"] = max(worst["state"], e)
                assert e < 1e-9, (nn, lev, gb, "state", e)
                a = sg.download("update", gb, lev)[g:-g, g:-g, g:-g]
                b = so.download("update", gb, lev)[g:-g, g:-g, g:-g]
                e = (np.abs(a - b).max() / scale) if update_by_largest else rel_err(a, b)
                worst["update"] = max(worst["update"], e)
                assert e < 1e-9, (nn, lev, gb, "update", e)
    print("TP-PARITY multigrid", n_eq, "final", worst)
    sg.close(), so.close()


def test_tp_multigrid_five_equations_parity(oracle):
    """W cycle, three levels, two blocks, DPLUR: the bounds of test_multigrid_synthetic_parity"""
    _multigrid(5, oracle, tp_cases.multigrid_five, 1e-8, False)


def test_tp_multigrid_seven_equations_parity(oracle):
    """W cycle, three levels, two blocks, SST + BLU-SGS: the bounds (and the update's scale)
    of test_multigrid_seven_equations_parity"""
    _multigrid(7, oracle, tp_cases.multigrid_rans, 1e-7, True)


def test_tp_outputs_parity(oracle):
    """k_output_pack (every thermodynamic name plus viscosity), the restart pack and the
    temperature / viscosity / gradient fields of the device against the oracle's, hot."""
    case = tp_cases.hot_single(**tp_cases.FIVE["weno_ausm_visc_lusgs"])
    agx = aither_amd.load(5, TP)
    sg, so = run_pair(agx, oracle, case, 1)
    # both hold their own state after the step: give the device the oracle's, bit for bit
    sg.upload("state", 0, so.download("state", 0))
    names = ["density", "pressure", "mach", "sos", "temperature", "energy", "enthalpy",
             "cp", "cv", "viscosity"]
    for x, y, n in zip(sg.output_pack(0, names), so.output_pack(0, names), names):
        e = np.abs(x - y).max() / np.abs(y).max()
        print("TP-PARITY output", n, f"{e:.2e}")
        assert e < RTOL, (n, e)
    x, y = sg.restart_pack(0), so.restart_pack(0)
    assert rel_err(x, y) < RTOL
    sg.close(), so.close()
    # the fields, as test_temperature_viscosity_fields: the oracle's arrays belong to the
    # state its last residual saw
    sg, so2 = Solver(agx, case), Solver(oracle, case)
    oracle.check(oracle.phase_bc_faces(so2.ctx)); oracle.check(oracle.phase_bc_edges(so2.ctx))
    oracle.check(oracle.phase_residual(so2.ctx, 0, case.deck.cfl(0)))
    sg.upload("state", 0, so2.download("state", 0))
    g = case.ng
    for f in ("temperature", "viscosity"):
        a, b = sg.download(f, 0), so2.download(f, 0)
        inner = (slice(g, -g),) * 3
        assert rel_err(a[inner], b[inner]) < RTOL, f
        assert rel_err(a[g:-g, g:-g, :], b[g:-g, g:-g, :]) < RTOL, f
    for f in ("vel_grad", "temp_grad", "dens_grad", "press_grad"):
        a, b = sg.download(f, 0), so2.download(f, 0)
        assert np.abs(b).max() > 0 and rel_err(a, b) < RTOL, f
    sg.close(), so2.close()
