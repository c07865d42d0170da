"""Wall-surface output on the device (agx_output_pack with AGX_WALL_*, k_wall_pack): the payload
of the reference's wall function file (WriteWallFun, output.cpp:472-571) against the numpy
restatement of tests/wall_ref.py, fed with the fields downloaded after the call; every face of
every viscousWall surface is compared.  Tolerances: those of tests/test_output_pack.py:100-103
for the same kind of quantity (1e-10 of the variable's largest magnitude for what is formed from
the state alone, 1e-8 for what is formed from gradients)."""
import ctypes as C

import numpy as np
import pytest

import wall_ref
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import Solver
from conftest import golden_case

pytestmark = pytest.mark.gpu

ALL = list(abi.WALL_OUT)
# isothermal and moving (tag 4) and constant heat flux (5) on two opposite sides, adiabatic
# (2) on a side of another direction: the edge ghost cells between two walls are read
WALLS = {3: ("viscousWall", 4), 4: ("viscousWall", 5), 1: ("viscousWall", 2),
         2: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
LAMINAR = dict(equation_set="navierStokes", face_reconstruction="weno", limiter="none",
               inviscid_flux="ausm", time_integration="implicitEuler", matrix_solver="lusgs",
               cfl=5.0)


def _lib(n_eq=5, model="caloricallyPerfect"):
    import aither_amd
    return aither_amd.load(n_eq, model)


def _hold_block_to_restatement(sol, gb, fourth=False):
    case = sol.case
    got = sol.wall_pack(gb, ALL)
    fields = wall_ref.download_fields(sol, gb)
    gas = wall_ref.GasRef(case.gas)
    surfs = sol.wall_surfaces(gb)
    ref = {n: [] for n in ALL}
    for q, surf in enumerate(surfs):
        w = wall_ref.wall_vars(fields, surf, gas, case.ng, fourth=fourth)
        for n in ALL:
            assert got[n][q].shape == surf["shape"], (n, q)
            ref[n].append(w[n])
    wall_ref.compare(got, ref)
    for n in ("tke", "sdr", "viscosityRatio"):
        assert all(np.all(a == 0.0) for a in got[n]), n
    return got


@pytest.mark.parametrize("recon", ["central", "centralFourth"])
def test_laminar_walls_on_three_sides(recon):
    case = synthetic.single_block_case((12, 9, 7), stretch=1.2, skew=0.01, bcs=WALLS,
                                       viscous_face_reconstruction=recon, **LAMINAR)
    sol = Solver(_lib(), case)
    sol.step(0), sol.step(1)
    assert [w["side"] for w in sol.wall_surfaces(0)] == [1, 3, 4]
    got = _hold_block_to_restatement(sol, 0, fourth=recon == "centralFourth")
    # the three thermal wall types give three different payloads
    assert np.abs(got["heatFlux"][1]).max() > 0.0 and np.abs(got["heatFlux"][2]).max() > 0.0
    sol.close()


def test_wall_across_a_block_connection():
    """two blocks stacked along k, walls on j-min (isothermal) and i-min (adiabatic) of both:
    the faces next to the connection read ghost cells the local halo swap filled"""
    bcs = {3: ("viscousWall", 4), 1: ("viscousWall", 2), 2: ("characteristic", 1),
           4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
    case = synthetic.stacked_blocks_case((8, 7, 6), nblocks=2, axis="k", stretch=1.15, bcs=bcs,
                                         **LAMINAR)
    sol = Solver(_lib(), case)
    sol.step(0), sol.step(1)
    for gb in (0, 1):
        assert [w["side"] for w in sol.wall_surfaces(gb)] == [1, 3]
        _hold_block_to_restatement(sol, gb)
    sol.close()


def test_thermally_perfect_laminar_walls():
    """hot case of tests/tp_cases.py on the _tp library; cp(T) of thermodynamic.hpp:125-189 is
    restated in wall_ref.GasRef.cp (it enters through the turbulent conductivity, which is 0
    in a laminar run: the laminar conductivity is Sutherland's, transport.cpp:124-132)"""
    import tp_cases
    case = tp_cases.hot_single(n=(10, 9, 7), stretch=1.2, skew=0.01, bcs=WALLS, **LAMINAR)
    sol = Solver(_lib(5, "thermallyPerfect"), case)
    sol.step(0), sol.step(1)
    gas = wall_ref.GasRef(case.gas)
    assert gas.theta_v and gas.cp(np.array([7.0]))[0] > 1.05 * gas.R * (gas.n + 1.0)
    _hold_block_to_restatement(sol, 0)
    sol.close()


def test_rans_low_re_wall():
    """the SST case of tests/test_output_pack.py: tke, sdr the (limited) central face value,
    viscosityRatio = mut / (mu + EPS), the gradient-derived variables against the restatement
    with the eddy viscosity recovered from the payload (the eddy viscosity itself is the
    residual kernel's device function, pinned by the parity tests)"""
    from test_output_pack import _case
    case = _case("rans")
    sol = Solver(_lib(7), case)
    sol.step(0), sol.step(1)
    got = sol.wall_pack(0, ALL)
    fields = wall_ref.download_fields(sol, 0)
    gas = wall_ref.GasRef(case.gas, turb_prandtl=0.9)
    surfs = sol.wall_surfaces(0)
    assert [w["side"] for w in surfs] == [3]
    ref = {n: [] for n in ALL}
    for q, surf in enumerate(surfs):
        w = wall_ref.wall_vars(fields, surf, gas, case.ng, mut_ratio=got["viscosityRatio"][q],
                               turbulent=True)
        for n in ALL:
            ref[n].append(w[n])
    wall_ref.compare(got, ref)
    for n in ("tke", "sdr"):
        for a, r in zip(got[n], ref[n]):
            assert np.abs(a - r).max() <= 1e-10 * np.abs(r).max(), n
    ratio = got["viscosityRatio"][0]
    assert np.isfinite(ratio).all() and (ratio >= 0.0).all()
    sol.close()


def test_wall_law_surfaces_hand_out_the_stored_wall_data():
    """golden wallLaw case, two steps.  There is no independent solve of the wall law here:
    shapes and order, the identities between the stored quantities, and the low-Re restatement
    on the faces the stored y+ < 10 switches to it (their number is printed)."""
    case = golden_case("wallLaw")
    sol = Solver(_lib(7), case)
    with pytest.raises(RuntimeError, match="no wall data before the first residual"):
        for gb in range(len(case.blocks)):
            if sol.wall_surfaces(gb):
                sol.wall_pack(gb, ["yplus"])
    sol.step(0), sol.step(1)
    gas = wall_ref.GasRef(case.gas)
    tau_sc = gas.mu_ref / gas.scaling * gas.a_ref / gas.l_ref
    n_low = n_all = 0
    for gb in range(len(case.blocks)):
        surfs = sol.wall_surfaces(gb)
        if not surfs:
            continue
        got = sol.wall_pack(gb, ALL)
        fields = wall_ref.download_fields(sol, gb)
        for q, surf in enumerate(surfs):
            for n in ALL:
                assert got[n][q].shape == surf["shape"] and np.isfinite(got[n][q]).all(), n
            utau = got["frictionVelocity"][q] / gas.a_ref
            rho = got["density"][q] / gas.rho_ref
            mag = got["shearStress"][q] / tau_sc
            np.testing.assert_allclose(utau * utau * rho, mag, rtol=1e-12)
            comps = np.stack([got["shearStress_" + c][q] for c in "xyz"], -1)
            np.testing.assert_allclose(np.sqrt((comps ** 2).sum(-1)), got["shearStress"][q],
                                       rtol=1e-12)
            low = got["yplus"][q] < 10.0
            n_low += int(low.sum())
            n_all += low.size
            if low.any():
                w = wall_ref.wall_vars(fields, surf, gas, case.ng,
                                       mut_ratio=got["viscosityRatio"][q], turbulent=True)
                for n in wall_ref.GRAD_NAMES + wall_ref.STATE_NAMES:
                    tol = 1e-10 if n in wall_ref.STATE_NAMES else 1e-8
                    scale = np.abs(w[n]).max()
                    assert np.abs(got[n][q] - w[n])[low].max() <= tol * scale, n
    print(f"wallLaw: {n_low} of {n_all} wall faces have y+ < 10 (low-Re treatment)")
    assert n_all > 0
    sol.close()


def _raw(sol, gb, ids, n=None, size=4096):
    arr = (C.c_int32 * len(ids))(*ids)
    out = np.zeros(size)
    sol.api.check(sol.api.output_pack(sol.ctx, sol.block_ids[gb], len(ids) if n is None else n,
                                      arr, out.ctypes.data_as(abi.c_dp)), "output_pack")
    return out


def test_contract_order_subsets_refusals_and_no_side_effects():
    def make():
        case = synthetic.single_block_case((10, 8, 6), stretch=1.2, skew=0.01, bcs=WALLS,
                                           **LAMINAR)
        s = Solver(_lib(), case)
        s.step(0), s.step(1)
        return s
    sol, plain = make(), make()
    full = sol.wall_pack(0, ALL)
    # caller's order, a repeated id, and a subset bit for bit
    surfs = sol.wall_surfaces(0)
    total = sum(int(np.prod(w["shape"])) for w in surfs)
    ids = [abi.WALL_OUT[n] for n in ("heatFlux", "yplus", "heatFlux", "shearStress_z")]
    raw = _raw(sol, 0, ids)[:4 * total].reshape(4, total)
    flat = lambda n: np.concatenate([a.ravel() for a in full[n]])
    assert np.array_equal(raw[0], flat("heatFlux")) and np.array_equal(raw[2], raw[0])
    assert np.array_equal(raw[1], flat("yplus")) and np.array_equal(raw[3], flat("shearStress_z"))
    # refusals, by their message
    with pytest.raises(RuntimeError, match="cell and wall variables in one call"):
        _raw(sol, 0, [abi.OUT["density"], abi.WALL_OUT["density"]])
    for bad in (99, 54, 63, 78, -1):
        with pytest.raises(RuntimeError, match="unknown output variable"):
            _raw(sol, 0, [bad])
    with pytest.raises(RuntimeError, match="nvar 15 out of range"):
        _raw(sol, 0, [abi.WALL_OUT["yplus"]] * 15)
    with pytest.raises(RuntimeError, match="nvar 0 out of range"):
        _raw(sol, 0, [abi.WALL_OUT["yplus"]], n=0)
    rows = _raw(sol, 0, [abi.WALL_OUT["yplus"]] * 14)[:14 * total].reshape(14, total)
    assert all(np.array_equal(r, flat("yplus")) for r in rows)
    no_wall = synthetic.single_block_case((8, 6, 5), bcs={1: ("characteristic", 1)}, **LAMINAR)
    s2 = Solver(_lib(), no_wall)
    with pytest.raises(RuntimeError, match="has no viscousWall surface"):
        _raw(s2, 0, [abi.WALL_OUT["yplus"]])
    s2.close()
    euler = synthetic.single_block_case((8, 6, 5), bcs={3: ("viscousWall", 2)},
                                        equation_set="euler", time_integration="implicitEuler",
                                        cfl=5.0)
    s3 = Solver(_lib(), euler)
    with pytest.raises(RuntimeError, match="need a viscous context"):
        _raw(s3, 0, [abi.WALL_OUT["yplus"]])
    s3.close()
    # the cell payload is the same before and after a wall call, bit for bit
    names = ["density", "velGrad_vx", "tempGrad_y", "resid_energy", "pressure"]
    before = plain.output_pack(0, names)
    assert np.array_equal(sol.output_pack(0, names), before)
    sol.wall_pack(0, ["shearStress"])
    assert np.array_equal(sol.output_pack(0, names), before)
    # ... and one more step gives the run without the wall calls
    a, b = sol.step(2), plain.step(2)
    assert np.array_equal(a["l2"], b["l2"]) and a["linf"] == b["linf"]
    assert np.array_equal(sol.download("state", 0), plain.download("state", 0))
    sol.close(), plain.close()
