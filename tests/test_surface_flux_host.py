"""Boundary fluxes and the block balance, host side: the numpy restatement of the two inviscid
fluxes (tests/flux_ref.py) is proven on the CPU oracle, the invariant the feature rests on --
the residual summed over a block is the sum of the outward fluxes through its boundary -- is
stated on the oracle alone, and the id ranges are shown to be free."""
import numpy as np
import pytest

import flux_cases
import flux_ref
import les_ref
import parity_utils
from aither_amd import abi
from aither_amd.solver import Solver


def _oracle_f1(oracle, flux):
    """F1 as euler with constant reconstruction after one residual of the oracle: the case,
    the ghost-padded state the residual saw, the residual, the host geometry's face areas"""
    case = flux_cases.f1(**flux_cases.EULER, **flux_cases.SCHEMES["constant_" + flux])
    s = Solver(oracle, case)
    les_ref.residual_once(s)
    state, resid = s.download("state", 0), s.download("residual", 0)
    s.close()
    g = case.blocks[0].geom
    fareas = {d: g.farea["ijk"[d]].a for d in range(3)}
    return case, state, resid, fareas


def _cell_error(case, state, resid, fareas, flux, **variant):
    """per equation: max over the cells of |oracle residual - telescoped restated fluxes| over
    the equation's flux scale times the largest face area"""
    g = case.blocks[0].geom
    faces = flux_ref.all_face_fluxes(state, fareas, g.ng, g.n, case.gas, flux, **variant)
    ref = flux_ref.telescoped(faces, g.n)
    scale = flux_ref.equation_scales(case) * parity_utils.flux_scale(case)
    return np.abs(resid - ref).max(axis=(0, 1, 2)) / scale, faces


@pytest.mark.parametrize("flux,broken", [("roe", dict(harten=False)),
                                         ("ausm", dict(swap_pressure_weights=True))])
def test_restated_fluxes_telescope_to_the_oracles_residual(oracle, flux, broken):
    case, state, resid, fareas = _oracle_f1(oracle, flux)
    err, _ = _cell_error(case, state, resid, fareas, flux)
    print(f"F1 euler constant {flux}: |oracle - restatement| / flux scale per equation {err}")
    assert err.max() <= 1e-12, err
    # a deliberate error in the restatement is seen: the field runs through Mach 1 (the Harten
    # fix is taken) and its pressure varies across every face (fl != fr)
    bad, _ = _cell_error(case, state, resid, fareas, flux, **broken)
    print(f"F1 euler constant {flux} with {broken}: {bad}")
    assert bad.max() > 1e-6, bad


@pytest.mark.parametrize("flux", ["roe", "ausm"])
def test_balance_holds_on_the_oracle(oracle, flux):
    """sum of the oracle's residual = sum over the surfaces of sigma F |A| of the restated
    fluxes, per equation, to RTOL of the flux scale times the block's boundary area; every
    surface contributes (two on j-min), and dropping one breaks it"""
    case, state, resid, fareas = _oracle_f1(oracle, flux)
    g = case.blocks[0].geom
    faces = flux_ref.all_face_fluxes(state, fareas, g.ng, g.n, case.gas, flux)
    surfs = flux_ref.host_surfaces(case, 0)
    assert [s["side"] for s in surfs] == [1, 2, 3, 3, 4, 5, 6]
    assert sorted(int(np.prod(s["shape"])) for s in surfs) == [54, 66, 90, 90, 120, 300, 300]
    per_surface = np.array([flux_ref.surface_sums(s, faces) for s in surfs])
    total = per_surface.sum(0)
    rsum = resid.reshape(-1, 5).sum(0)
    tol = parity_utils.RTOL * flux_ref.equation_scales(case) * flux_ref.boundary_area(case, 0)
    print(f"F1 oracle {flux}: residual sums {rsum}\n  flux sums {total}\n  tolerance {tol}")
    assert np.all(np.abs(rsum - total) <= tol)
    area = sum(flux_ref.surface_area(s, fareas[(s["side"] - 1) // 2], g.ng) for s in surfs)
    assert abs(area - flux_ref.boundary_area(case, 0)) <= 1e-13 * area
    for q in range(len(surfs)):
        short = total - per_surface[q]
        assert np.any(np.abs(rsum - short) > tol), q


def test_id_ranges_are_free():
    flux, budget = set(abi.FLUX_OUT.values()), set(abi.BUDGET_OUT.values())
    assert flux == set(range(abi.FLUX_BASE, abi.FLUX_END)) and len(abi.FLUX_OUT) == 15
    assert budget == set(range(abi.BUDGET_BASE, abi.BUDGET_END)) and len(abi.BUDGET_OUT) == 15
    assert (abi.FLUX_BASE, abi.FLUX_END, abi.BUDGET_BASE, abi.BUDGET_END) == (384, 399, 448, 463)
    taken = set(abi.OUT.values()) | set(range(0, 54)) | set(abi.WALL_OUT.values()) | \
        set(abi.NODE_OUT.values()) | set(abi.LOAD_OUT.values()) | \
        set(range(abi.STAT_BASE, abi.STAT_END)) | set(range(abi.WSTAT_BASE, abi.WSTAT_END)) | \
        set(range(abi.CSTAT_BASE, 2048))
    # the ids the existing tests pin as unknown
    unknown = {54, 63, 78, 99, 127, 182, 255, 273, 533, 575, 594, 1023, 2048}
    for ids in (flux, budget):
        assert not ids & taken and not ids & unknown
    assert not flux & budget
    names = list(abi.FLUX_OUT)
    assert names[0] == "area" and names[1:8] == ["inviscid_" + e for e in abi.EQUATIONS]
    assert names[8:] == ["viscous_" + e for e in abi.EQUATIONS]
    assert abi.EQUATIONS == ("mass", "mom_x", "mom_y", "mom_z", "energy", "tke", "sdr")
    names = list(abi.BUDGET_OUT)
    assert names[0] == "volume" and names[1:8] == ["total_" + e for e in abi.EQUATIONS]
    assert names[8:] == ["residual_" + e for e in abi.EQUATIONS]
    assert abi.FLUX_OUT["viscous_sdr"] == 398 and abi.BUDGET_OUT["residual_sdr"] == 462


def test_pool_fluxes_adds_blocks_and_filters():
    from aither_amd.solver import pool_fluxes
    surfs = [dict(tag=1, bc_type="characteristic"), dict(tag=1001, bc_type="interblock")]
    other = [dict(tag=2000, bc_type="interblock"), dict(tag=2, bc_type="viscousWall")]
    a = {"inviscid_mass": np.array([1.5, -4.0])}
    b = {"inviscid_mass": np.array([4.0, 0.25])}
    assert pool_fluxes([(surfs, a), (other, b)]) == {"inviscid_mass": 1.75}
    assert pool_fluxes([(surfs, a), (other, b)], bc_types=["interblock"]) == {"inviscid_mass": 0.0}
    assert pool_fluxes([(surfs, a), (other, b)], tags=[2]) == {"inviscid_mass": 0.25}
