"""The nodal function file on the device (agx_output_pack with AGX_NODE_BASE + AGX_OUT_*,
k_node_grads + k_node_pack): the payload of the reference's WriteNodeFun (output.cpp:452-469)
against the numpy restatement of tests/node_ref.py, fed with the fields downloaded AFTER the
call (so the ghost cells are those the kernels read); every node of every variable is compared.

Ceilings: those of tests/test_output_pack.py:100-103 -- 1e-10 of the variable's largest
magnitude for everything but gradients and residuals, 1e-8 for those.  The kernels and the
restatement read the same numbers and differ in fused multiply-adds and the rounding of 8 to 12
terms only: the largest ratios seen over all the cases here are 4.8e-16 and 3.2e-13 (DESIGN
section 8 f1 lists them per case), and TOL_STATE / TOL_GRAD below are a decade above those.  A variable whose reference is identically
zero must be exactly zero.

The number of ghost layers is the deck's (input.cpp:1127-1143: WENO 3, MUSCL 2, constant
reconstruction 1); the rules read the first layer only, and all three occur below.
"""
import ctypes as C

import numpy as np
import pytest

import node_ref
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import Solver
from test_output_pack import LAMINAR as LAMINAR_NAMES, WALL

pytestmark = pytest.mark.gpu

TOL_STATE, TOL_GRAD = 5e-15, 4e-12
# the deck of _case("laminar") / _case("rans") of tests/test_output_pack.py
LAMINAR = dict(stretch=1.2, skew=0.01, bcs=WALL, equation_set="navierStokes",
               face_reconstruction="weno", limiter="none", inviscid_flux="ausm",
               time_integration="bdf2", matrix_solver="lusgs", nonlinear_iterations=2,
               dt=2.0e-6, cfl=-1.0)
RANS = dict(stretch=1.15, bcs=WALL, equation_set="rans", turbulence_model="sst2003",
            time_integration="bdf2", matrix_solver="lusgs", nonlinear_iterations=2, dt=2.0e-6,
            cfl=-1.0)
RANS_NAMES = [n for n in abi.OUT if n not in node_ref.NOT_AT_NODES]


def _lib(n_eq=5, model="caloricallyPerfect"):
    import aither_amd
    return aither_amd.load(n_eq, model)


def _stepped(lib, case):
    sol = Solver(lib, case)
    sol.step(0), sol.step(1)
    return sol


def _hold_block_to_restatement(sol, gb, names, turbulent=False, what="node_pack"):
    case = sol.case
    got = sol.node_pack(gb, names)
    ni, nj, nk = case.blocks[gb].geom.n
    assert got.shape == (len(names), nk + 1, nj + 1, ni + 1)
    assert np.isfinite(got).all()
    ref = node_ref.node_vars(node_ref.download_fields(sol, gb), case.gas, case.ng,
                             global_pos=case.blocks[gb].global_pos, turbulent=turbulent)
    node_ref.compare(got, ref, names, TOL_STATE, TOL_GRAD, what=what)
    return got


@pytest.mark.parametrize("n", [(5, 4, 3), (6, 4, 1)])
def test_laminar_every_name(n):
    """(6, 4, 1): every node is a boundary node, as in most of the reference's own cases"""
    sol = _stepped(_lib(), synthetic.single_block_case(n, **LAMINAR))
    assert len(LAMINAR_NAMES) == 48
    got = _hold_block_to_restatement(sol, 0, LAMINAR_NAMES, what=f"laminar {n}")
    row = dict(zip(LAMINAR_NAMES, got))
    assert np.abs(row["velGrad_uy"]).max() > 0.0 and np.abs(row["resid_energy"]).max() > 0.0
    for name in ("tke", "sdr") + node_ref.NOT_AT_NODES:
        assert np.all(row[name] == 0.0), name
    sol.close()


def test_rans_every_name_but_the_four_refused():
    sol = _stepped(_lib(7), synthetic.single_block_case((5, 4, 3), **RANS))
    got = _hold_block_to_restatement(sol, 0, RANS_NAMES, turbulent=True, what="rans")
    row = dict(zip(RANS_NAMES, got))
    assert np.abs(row["tke"]).max() > 0.0 and np.abs(row["omegaGrad_y"]).max() > 0.0
    for name in node_ref.NOT_AT_NODES:
        with pytest.raises(RuntimeError, match="the reference averages eddyViscosity_, f1_, f2_ "
                                               "with their ghost cells"):
            sol.node_pack(0, ["density", name])
    sol.close()


def test_thermally_perfect_node_thermodynamics():
    """hot case of tests/tp_cases.py, vibrational mode active: sos / mach / energy / enthalpy
    with T of the node state, cp / cv at the averaged temperature"""
    import tp_cases
    kw = {k: v for k, v in LAMINAR.items() if k not in ("time_integration", "dt", "cfl",
                                                        "nonlinear_iterations")}
    case = tp_cases.hot_single(n=(5, 4, 3), time_integration="implicitEuler", cfl=5.0, **kw)
    sol = _stepped(_lib(5, "thermallyPerfect"), case)
    names = ["temperature", "cp", "cv", "sos", "mach", "energy", "enthalpy", "viscosity"]
    got = _hold_block_to_restatement(sol, 0, names, what="thermallyPerfect")
    gas = case.gas
    cv_frozen = gas.n * gas.gas_constant * gas.a_ref ** 2 / gas.t_ref
    assert got[names.index("cv")].min() > 1.05 * cv_frozen
    sol.close()


def test_two_blocks_across_a_local_connection():
    """two (4, 3, 2) blocks stacked along i, MUSCL (two ghost layers).  At the nodes strictly
    inside the shared face both blocks average the same eight cells: the state-derived
    variables agree to 1e-12 relative, whatever node_ref says."""
    case = synthetic.stacked_blocks_case((4, 3, 2), nblocks=2, axis="i", stretch=1.15, bcs=WALL,
                                         equation_set="navierStokes",
                                         time_integration="implicitEuler", matrix_solver="lusgs",
                                         cfl=5.0)
    assert case.ng == 2
    sol = _stepped(_lib(), case)
    got = [_hold_block_to_restatement(sol, gb, LAMINAR_NAMES, what=f"block {gb}")
           for gb in (0, 1)]
    for name in node_ref.STATE_DERIVED:
        q = LAMINAR_NAMES.index(name)
        a, b = got[0][q][1:-1, 1:-1, -1], got[1][q][1:-1, 1:-1, 0]
        assert a.size == 2
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), name
    sol.close()


def test_one_ghost_layer():
    case = synthetic.single_block_case((4, 3, 2), stretch=1.2, skew=0.01, bcs=WALL,
                                       equation_set="navierStokes",
                                       face_reconstruction="constant",
                                       time_integration="implicitEuler", matrix_solver="lusgs",
                                       cfl=5.0)
    assert case.ng == 1
    sol = _stepped(_lib(), case)
    _hold_block_to_restatement(sol, 0, LAMINAR_NAMES, what="one ghost layer")
    sol.close()


def _raw(sol, gb, ids, n=None, size=8192):
    arr = (C.c_int32 * len(ids))(*ids)
    out = np.zeros(size)
    sol.api.check(sol.api.output_pack(sol.ctx, sol.block_ids[gb], len(ids) if n is None else n,
                                      arr, out.ctypes.data_as(abi.c_dp)), "output_pack")
    return out


def test_contract_order_refusals_determinism_and_no_side_effects():
    def make():
        return _stepped(_lib(), synthetic.single_block_case((5, 4, 3), **LAMINAR))
    sol, plain = make(), make()
    full = sol.node_pack(0, LAMINAR_NAMES)
    # two identical calls: the same bits (a gather, no atomics)
    assert np.array_equal(sol.node_pack(0, LAMINAR_NAMES), full)
    # a subset in another order: variable-major, in the caller's order
    sub = ["pressGrad_z", "pressure", "density", "resid_mom_x", "mach", "wallDistance"]
    z = sol.node_pack(0, sub)
    for q, name in enumerate(sub):
        assert np.array_equal(z[q], full[LAMINAR_NAMES.index(name)]), name
    # refusals, by their message
    node, cell, wall = abi.NODE_OUT["density"], abi.OUT["density"], abi.WALL_OUT["density"]
    with pytest.raises(RuntimeError, match="cell and node variables in one call"):
        _raw(sol, 0, [node, cell])
    with pytest.raises(RuntimeError, match="node and wall variables in one call"):
        _raw(sol, 0, [wall, node])
    for bad in (127, 128 + 54, 255):
        with pytest.raises(RuntimeError, match="unknown output variable"):
            _raw(sol, 0, [bad])
    with pytest.raises(RuntimeError, match="nvar 55 out of range"):
        _raw(sol, 0, [node] * 55)
    with pytest.raises(RuntimeError, match="nvar 0 out of range"):
        _raw(sol, 0, [node], n=0)
    euler = synthetic.single_block_case((4, 3, 2), equation_set="euler",
                                        time_integration="implicitEuler", cfl=5.0)
    s2 = Solver(_lib(), euler)
    with pytest.raises(RuntimeError, match="only kept for viscous runs"):
        s2.node_pack(0, ["viscosity"])
    assert np.isfinite(s2.node_pack(0, ["density", "velGrad_ux"])).all()
    s2.close()
    # the cell payload is the same before and after a nodal call, bit for bit
    names = ["density", "velGrad_vx", "tempGrad_y", "resid_energy", "pressure"]
    before = plain.output_pack(0, names)
    assert np.array_equal(sol.output_pack(0, names), before)
    sol.node_pack(0, sub)
    assert np.array_equal(sol.output_pack(0, names), before)
    # ... and two further iterations give the run that never made a nodal call
    for nn in (2, 3):
        a, b = sol.step(nn), plain.step(nn)
        assert np.array_equal(a["l2"], b["l2"]) and a["linf"] == b["linf"]
    assert np.array_equal(sol.download("state", 0), plain.download("state", 0))
    sol.close(), plain.close()
