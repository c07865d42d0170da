"""Wall-surface output (WriteWallFun, output.cpp:472-571), host side: the ids of the header
and abi.WALL_OUT, Solver.wall_surfaces, and the numpy restatement the GPU tests hold the
device to (tests/wall_ref.py) on a field where the answer is known."""
import os
import re

import numpy as np

import wall_ref
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import Solver
from conftest import ROOT, golden_case

HEADER_NAMES = ["YPLUS", "SHEAR_STRESS", "VISCOSITY_RATIO", "HEAT_FLUX", "FRICTION_VELOCITY",
                "DENSITY", "PRESSURE", "TEMPERATURE", "VISCOSITY", "TKE", "SDR", "SHEAR_X",
                "SHEAR_Y", "SHEAR_Z"]
ABI_NAMES = ["yplus", "shearStress", "viscosityRatio", "heatFlux", "frictionVelocity", "density",
             "pressure", "temperature", "viscosity", "tke", "sdr", "shearStress_x",
             "shearStress_y", "shearStress_z"]


def _wall_enum():
    with open(os.path.join(ROOT, "include", "aither_gfx950.h")) as fh:
        text = fh.read()
    body = re.search(r"enum \{ (AGX_WALL_YPLUS = (\d+),.*?AGX_WALL_END) \};", text, re.S)
    assert body, "the header has no AGX_WALL_* enum"
    body_text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    names = [n.strip().split("=")[0].strip() for n in body_text.split(",")]
    base = int(body.group(2))
    return {n: base + q for q, n in enumerate(names)}


def test_wall_ids_match_the_header_and_stay_clear_of_the_cell_ids():
    enum = _wall_enum()
    assert list(enum) == ["AGX_WALL_" + n for n in HEADER_NAMES] + ["AGX_WALL_END"]
    assert list(abi.WALL_OUT) == ABI_NAMES
    for h, a in zip(HEADER_NAMES, ABI_NAMES):
        assert abi.WALL_OUT[a] == enum["AGX_WALL_" + h], a
    with open(os.path.join(ROOT, "include", "aither_gfx950.h")) as fh:
        count = int(re.search(r"AGX_OUT_COUNT = (\d+)", fh.read()).group(1))
    assert max(abi.OUT.values()) < count <= min(abi.WALL_OUT.values())
    assert not set(abi.OUT.values()) & set(abi.WALL_OUT.values())
    assert 99 >= enum["AGX_WALL_END"] and 99 not in abi.OUT.values()


def test_wall_surfaces_order_and_shapes(oracle):
    ni, nj, nk = 7, 6, 5
    bcs = {1: ("viscousWall", 5), 3: ("viscousWall", 4), 4: ("viscousWall", 2),
           6: ("viscousWall", 2), 2: ("characteristic", 1), 5: ("characteristic", 1)}
    case = synthetic.single_block_case((ni, nj, nk), bcs=bcs, equation_set="navierStokes",
                                       time_integration="implicitEuler", cfl=5.0)
    s = Solver(oracle, case)
    surfs = s.wall_surfaces(0)
    # the order the library gets them in: the block's sorted surface list (boundarySurface
    # operator<), which is the order of wallData_ (procBlock.cpp:76-85)
    assert [w["side"] for w in surfs] == [1, 3, 4, 6]
    assert [w["tag"] for w in surfs] == [5, 4, 2, 2]
    assert [w["shape"] for w in surfs] == [(nk, nj, 1), (nk, 1, ni), (nk, 1, ni), (1, nj, ni)]
    assert surfs[0]["range"] == (0, 0, 0, nj, 0, nk)
    assert surfs[3]["range"] == (0, ni, 0, nj, nk, nk)
    s.close()
    case = golden_case("wallLaw")
    s = Solver(oracle, case)
    for gb, blk in enumerate(case.blocks):
        want = [x for x in blk.surfaces if x.bc_type == "viscousWall"]
        got = s.wall_surfaces(gb)
        assert len(got) == len(want)
        for w, x in zip(got, want):
            assert w["side"] == x.surface_type()
            assert w["range"] == (x.imin, x.imax, x.jmin, x.jmax, x.kmin, x.kmax)
            assert int(np.prod(w["shape"])) == max(x.imax - x.imin, 1) * \
                max(x.jmax - x.jmin, 1) * max(x.kmax - x.kmin, 1)
    assert sum(len(s.wall_surfaces(gb)) for gb in range(len(case.blocks))) >= 1
    s.close()


class _Gas:
    gas_constant, n = 1.0 / 1.4, 2.5
    visc_c1, visc_s, cond_c1, cond_s = 1.458e-6, 110.4, 2.495e-3, 194.0
    t_ref, rho_ref, l_ref, a_ref = 288.15, 1.225, 1.0, 340.0
    theta_v = []


def _affine_fields(n, ng, M, G, gvec):
    """A uniform lattice under x = M xi (sheared, non-orthogonal) with u = G^T x + u0 and
    T = g . x + T0 in physical and ghost cells: [k, j, i, c] arrays like the downloads."""
    ni, nj, nk = n
    h = np.array([0.1, 0.07, 0.05])
    E = M * h[None, :]                       # columns: the edge vectors of a cell
    shape = (nk + 2 * ng, nj + 2 * ng, ni + 2 * ng)
    kk, jj, ii = np.meshgrid(*[np.arange(s) - ng + 0.5 for s in shape], indexing="ij")
    cen = ii[..., None] * E[:, 0] + jj[..., None] * E[:, 1] + kk[..., None] * E[:, 2]
    vel = cen @ G + np.array([3.0, -1.0, 0.5])          # u_c = sum_r x_r G[r, c]
    temp = 1.0 + cen @ gvec
    rho = 1.1 + 0.0 * temp
    state = np.concatenate([rho[..., None], vel, (rho * _Gas.gas_constant * temp)[..., None]], -1)
    f = {"state": state, "temperature": temp[..., None],
         "viscosity": (0.9 + 0.2 * temp)[..., None],
         "volume": np.full(shape + (1,), abs(np.linalg.det(E))),
         "wall_dist": np.full(shape + (1,), 0.01)}
    for d, name in enumerate("ijk"):
        a = np.cross(E[:, (d + 1) % 3], E[:, (d + 2) % 3])
        fs = list(shape)
        fs[2 - d] += 1
        f["farea_" + name] = np.broadcast_to(
            np.concatenate([a / np.linalg.norm(a), [np.linalg.norm(a)]]), tuple(fs) + (4,)).copy()
        f["width_" + name] = np.full(shape + (1,), h[d])
    return f


def test_restatement_is_exact_on_a_linear_field_over_an_affine_grid():
    n, ng = (6, 5, 4), 2
    M = np.array([[1.0, 0.3, -0.2], [0.1, 1.0, 0.25], [-0.15, 0.2, 1.0]])
    G = np.array([[0.7, -1.1, 0.4], [2.0, 0.3, -0.6], [-0.9, 1.3, 0.8]])
    gvec = np.array([0.02, -0.03, 0.015])
    fields = _affine_fields(n, ng, M, G, gvec)
    gas = wall_ref.GasRef(_Gas)
    ni, nj, nk = n
    ranges = {1: (0, 0, 0, nj, 0, nk), 2: (ni, ni, 0, nj, 0, nk), 3: (0, ni, 0, 0, 0, nk),
              4: (0, ni, nj, nj, 0, nk), 5: (0, ni, 0, nj, 0, 0), 6: (0, ni, 0, nj, nk, nk)}
    for side, rng in ranges.items():
        for fourth in (False, True):
            surf = wall_ref.surface_of(side, rng)
            w = wall_ref.wall_vars(fields, surf, gas, ng, fourth=fourth)
            assert w["velGrad"].shape == surf["shape"] + (3, 3)
            assert np.abs(w["velGrad"] - G).max() <= 1e-12 * np.abs(G).max(), side
            assert np.abs(w["tempGrad"] - gvec).max() <= 1e-12 * np.abs(gvec).max(), side
            # shearStress_ = lambda tr(G) n + mu (G + G^T) n  (TauNormal, utility.cpp:426-436)
            mu, nrm = w["mu"], w["normal"]
            want = (-(2.0 / 3.0) * mu * np.trace(G))[..., None] * nrm + \
                mu[..., None] * (nrm @ (G + G.T))
            assert np.abs(w["tau"] - want).max() <= 1e-12 * np.abs(want).max(), side
            sc = gas.mu_ref / gas.scaling * gas.a_ref / gas.l_ref
            np.testing.assert_allclose(w["shearStress"], np.sqrt((want ** 2).sum(-1)) * sc,
                                       rtol=1e-12)
            np.testing.assert_allclose(w["shearStress_y"], want[..., 1] * sc, rtol=1e-11,
                                       atol=1e-12 * np.abs(want).max() * sc)
            # linear fields: the two- and the four-cell face values agree
            t_face = w["temperature"] / gas.t_ref
            k = gas.conductivity(t_face) * gas.scaling
            np.testing.assert_allclose(w["heatFlux"], k * (nrm @ gvec) * gas.mu_ref * gas.t_ref
                                       / gas.l_ref, rtol=1e-11)
            assert np.all(w["tke"] == 0.0) and np.all(w["viscosityRatio"] == 0.0)


def test_restatement_on_oracle_fields_is_finite_and_consistent(oracle):
    bcs = {3: ("viscousWall", 4), 4: ("viscousWall", 5), 1: ("viscousWall", 2),
           2: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
    case = synthetic.single_block_case((9, 8, 7), stretch=1.2, skew=0.01, bcs=bcs,
                                       equation_set="navierStokes", face_reconstruction="weno",
                                       limiter="none", inviscid_flux="ausm",
                                       time_integration="implicitEuler", cfl=5.0)
    s = Solver(oracle, case)
    s.step(0), s.step(1)
    fields = wall_ref.download_fields(s, 0, host_geometry=True)
    gas = wall_ref.GasRef(case.gas)
    surfs = s.wall_surfaces(0)
    assert [w["side"] for w in surfs] == [1, 3, 4]
    for surf in surfs:
        w = wall_ref.wall_vars(fields, surf, gas, case.ng)
        for name in abi.WALL_OUT:
            assert w[name].shape == surf["shape"] and np.isfinite(w[name]).all(), name
        utau, rho = w["frictionVelocity"] / gas.a_ref, w["density"] / gas.rho_ref
        tau = w["shearStress"] / (gas.mu_ref / gas.scaling * gas.a_ref / gas.l_ref)
        np.testing.assert_allclose(utau * utau * rho, tau, rtol=1e-13)
        comps = np.stack([w["shearStress_" + c] for c in "xyz"], -1)
        np.testing.assert_allclose(np.sqrt((comps ** 2).sum(-1)), w["shearStress"], rtol=1e-13)
        # y+ = y u_tau rho / (mu + mut) with the wall distance of the wall-adjacent cell
        g, d = case.ng, (surf["side"] - 1) // 2
        wd = fields["wall_dist"][g:-g, g:-g, g:-g, 0]
        sl = [slice(None)] * 3
        sl[2 - d] = slice(0, 1) if surf["side"] % 2 == 1 else slice(-1, None)
        mu = w["viscosity"] / gas.mu_ref * gas.scaling
        np.testing.assert_allclose(w["yplus"], wd[tuple(sl)] * utau * rho / mu, rtol=1e-13)
        assert (w["yplus"] > 0.0).all()
    s.close()
