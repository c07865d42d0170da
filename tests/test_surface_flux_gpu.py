"""Boundary fluxes and the block balance on the device (agx_output_pack with AGX_FLUX_* and
AGX_BUDGET_*; k_surface_flux, k_surface_flux_visc, k_block_budget).  Three kinds of check, none
of which shares the surface kernels' code path: the balance (the residual summed over a block
against the fluxes through its boundary), the antisymmetry of the two sides of a local
connection, and numpy restatements (tests/flux_ref.py for the inviscid fluxes, tests/les_ref.py
for the viscous ones, tests/loads_ref.py / wall_ref.py at walls).

The tolerance throughout is parity_utils.RTOL (1e-10) of the equation's flux scale times the
total boundary area of the block(s) (flux_ref.equation_scales, flux_ref.boundary_area), never
of a surface's own sum.  Values are compared nondimensionally: what the library returns over
the factors the header states (flux_ref.factors).  The totals and the volume are plain sums of
N <= 1800 positive or cancelling terms of the downloaded fields: (N + 64) 2^-52 of the sum of
the terms' magnitudes covers any summation order plus the roundings of forming a term."""
import ctypes as C
import math

import numpy as np
import pytest

import flux_cases
import flux_ref
import les_cases
import les_ref
import loads_ref
import parity_utils
import probe
import wall_ref
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import Solver, pool_fluxes

pytestmark = pytest.mark.gpu

RTOL = parity_utils.RTOL
EPS52 = 2.0 ** -52
EQ = abi.EQUATIONS
FARFIELD = {s: ("characteristic", 1) for s in range(1, 7)}


def _lib(n_eq=5, model="caloricallyPerfect"):
    import aither_amd
    return aither_amd.load(n_eq, model)


def _tolerance(case, blocks=None):
    """RTOL x flux scale x boundary area of the listed blocks (default: all), per equation"""
    blocks = range(len(case.blocks)) if blocks is None else blocks
    area = sum(flux_ref.boundary_area(case, gb) for gb in blocks)
    return RTOL * flux_ref.equation_scales(case) * area


def _nondim(sol, got, prefix, factor):
    """[nsurf, n_eq] (or [n_eq]) of the values prefix_e over the factor of equation e"""
    n_eq = sol.cfg.n_eq
    return np.stack([np.asarray(got[f"{prefix}_{EQ[e]}"]) / factor[e] for e in range(n_eq)], -1)


def _read(sol, gb):
    """every flux and budget value of block gb, nondimensional: area [nsurf], inviscid and
    viscous [nsurf, n_eq], volume, total and residual [n_eq]"""
    gas, n_eq = sol.case.gas, sol.cfg.n_eq
    f_flux, f_total = flux_ref.factors(gas, n_eq)
    flux, bud = sol.surface_fluxes(gb), sol.block_budget(gb)
    nsurf = len(sol.flux_surfaces(gb))
    assert len(flux) == 1 + 2 * n_eq and len(bud) == 1 + 2 * n_eq
    assert all(v.shape == (nsurf,) for v in flux.values())
    return dict(area=flux["area"] / gas.l_ref ** 2, volume=bud["volume"] / gas.l_ref ** 3,
                inviscid=_nondim(sol, flux, "inviscid", f_flux),
                viscous=_nondim(sol, flux, "viscous", f_flux),
                total=_nondim(sol, bud, "total", f_total),
                residual=_nondim(sol, bud, "residual", f_flux))


def _hold_balance(sol, what):
    """after a residual: for every block and every e < 5 the residual sum equals the net
    outward flux over ALL its surfaces; the residual sums, the totals and the volume equal
    numpy sums of the downloaded fields.  Returns {gb: _read}."""
    case, g = sol.case, sol.case.ng
    out = {}
    for gb in sorted(sol.block_ids):
        tol = _tolerance(case, [gb])
        surfs = sol.flux_surfaces(gb)
        assert len(surfs) == len(case.blocks[gb].surfaces)      # (one rank: none left out)
        got = out[gb] = _read(sol, gb)
        net = (got["inviscid"] + got["viscous"]).sum(0)
        bad = []
        for e in range(5):
            err = abs(got["residual"][e] - net[e])
            print(f"{what} block {gb} {EQ[e]}: residual sum {got['residual'][e]:.17g} flux sum "
                  f"{net[e]:.17g} |diff| {err:.3e} tol {tol[e]:.3e}")
            if not err <= tol[e]:
                bad.append((EQ[e], err, tol[e]))
        assert not bad, (what, gb, bad)
        resid = sol.download("residual", gb)
        rsum = np.array([math.fsum(resid[..., e].ravel()) for e in range(resid.shape[-1])])
        assert np.all(np.abs(got["residual"] - rsum) <= tol), (got["residual"], rsum, tol)
        state = sol.download("state", gb)[g:-g, g:-g, g:-g]
        vol = sol.geometry("volume", gb)[g:-g, g:-g, g:-g, 0]
        terms = flux_ref.conserved(state, case.gas) * vol[..., None]
        n = vol.size
        assert abs(got["volume"] - math.fsum(vol.ravel())) <= (n + 64) * EPS52 * vol.sum()
        for e in range(terms.shape[-1]):
            want, mag = math.fsum(terms[..., e].ravel()), np.abs(terms[..., e]).sum()
            assert abs(got["total"][e] - want) <= (n + 64) * EPS52 * mag, (what, gb, EQ[e])
        assert got["total"][0] > 0.0 and got["volume"] > 0.0
    return out


def _after_residual(lib, case):
    sol = Solver(lib, case)
    les_ref.residual_once(sol)
    return sol


# ---- 1. the balance ----------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["constant_roe", "constant_ausm", "muscl_vanalbada_roe",
                                    "muscl_vanalbada_ausm", "muscl_minmod_roe",
                                    "muscl_minmod_ausm"])
def test_balance_f1_euler(scheme):
    sol = _after_residual(_lib(), flux_cases.f1(**flux_cases.EULER, **flux_cases.SCHEMES[scheme]))
    got = _hold_balance(sol, "F1 euler " + scheme)[0]
    surfs = sol.flux_surfaces(0)
    assert [s["side"] for s in surfs] == [1, 2, 3, 3, 4, 5, 6]
    assert [int(np.prod(s["shape"])) for s in surfs][-2:] == [300, 300]    # two chunks each
    assert np.all(got["viscous"] == 0.0)                       # an inviscid context
    open_ = [q for q, s in enumerate(surfs) if "Wall" not in s["bc_type"]]
    assert len(open_) == 4 and np.all(np.abs(got["inviscid"][open_, 0]) > 0.0)
    sol.close()


@pytest.mark.parametrize("name,deck", [
    ("muscl_roe", dict(flux_cases.SCHEMES["muscl_vanalbada_roe"])),
    ("weno_ausm", dict(flux_cases.SCHEMES["weno_ausm"])),
    ("fourth", dict(flux_cases.SCHEMES["muscl_vanalbada_roe"],
                    viscous_face_reconstruction="centralFourth"))])
def test_balance_f1_navier_stokes(name, deck):
    case = flux_cases.f1(**flux_cases.NS, **deck)
    assert case.ng == (3 if name == "weno_ausm" else 2)
    sol = _after_residual(_lib(), case)
    got = _hold_balance(sol, "F1 navierStokes " + name)[0]
    walls = [q for q, s in enumerate(sol.flux_surfaces(0)) if s["bc_type"] == "viscousWall"]
    assert len(walls) == 2
    assert np.all(got["viscous"][:, 0] == 0.0)                 # no viscous mass flux
    assert np.all(np.abs(got["viscous"][walls, 1:5]).max(1) > 0.0)
    sol.close()


@pytest.mark.parametrize("form", ["ns", "les", "tp"])
def test_balance_f3(form):
    make, lib = flux_cases.F3[form]
    sol = _after_residual(_lib(*lib), make())
    _hold_balance(sol, "F3 " + form)
    sol.close()


@pytest.mark.parametrize("deck", ["rans", "wall_law"])
def test_balance_f4(deck):
    sol = Solver(_lib(7), flux_cases.F4[deck]())
    if deck == "wall_law":
        # wall-law faces: refused before the first residual, like the wall variables
        gb = next(gb for gb in sorted(sol.block_ids) if sol.wall_surfaces(gb))
        with pytest.raises(RuntimeError, match="no wall data before the first residual"):
            sol.surface_fluxes(gb, ["area"])
    les_ref.residual_once(sol)
    _hold_balance(sol, "F4 " + deck)
    sol.close()


# ---- 2. per surface against numpy ------------------------------------------------------------------
@pytest.mark.parametrize("flux", ["roe", "ausm"])
def test_inviscid_values_per_surface_against_the_restatement(flux):
    case = flux_cases.f1(**flux_cases.EULER, **flux_cases.SCHEMES["constant_" + flux])
    sol = _after_residual(_lib(), case)
    got = _read(sol, 0)
    g, n = case.ng, case.blocks[0].geom.n
    # (an euler context: the ghost cells hold the inviscid fill the call made)
    state = sol.download("state", 0)
    fareas = {d: sol.geometry("farea_" + "ijk"[d], 0) for d in range(3)}
    faces = flux_ref.all_face_fluxes(state, fareas, g, n, case.gas, flux)
    tol = _tolerance(case)
    for q, s in enumerate(sol.flux_surfaces(0)):
        ref = flux_ref.surface_sums(s, faces)
        err = np.abs(got["inviscid"][q] - ref)
        print(f"F1 {flux} surface {q} (side {s['side']} {s['bc_type']}): {got['inviscid'][q]} "
              f"restated {ref} |diff| {err}")
        assert np.all(err <= tol), (q, err, tol)
        area = flux_ref.surface_area(s, fareas[(s["side"] - 1) // 2], g)
        nf = int(np.prod(s["shape"]))
        assert abs(got["area"][q] - area) <= (nf + 16) * EPS52 * area
    sol.close()


def _viscous_reference(sol, gb, cw, fourth=False):
    """- sigma sum F_visc |A| of every surface of block gb from les_ref.faces on the downloaded
    fields (the ghost cells as the flux call left them): [nsurf, 5]"""
    case = sol.case
    geom = case.blocks[gb].geom
    fields = wall_ref.download_fields(sol, gb)
    gas = wall_ref.GasRef(case.gas)
    per_d = {d: les_ref.faces(fields, gas, geom.n, case.ng, d, fourth=fourth, cw=cw)["flux"]
             for d in range(3)}                                  # [i, j, k, 5]
    out = []
    for s in sol.flux_surfaces(gb):
        d = (s["side"] - 1) // 2
        r = s["range"]
        lo, hi = [r[0], r[2], r[4]], [r[1], r[3], r[5]]
        hi[d] = lo[d] + 1
        f = per_d[d][lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        out.append([-flux_ref.sigma(s["side"]) * math.fsum(f[..., e].ravel()) for e in range(5)])
    return np.array(out)


@pytest.mark.parametrize("name,make,lib,cw", [
    ("F3 ns", flux_cases.F3["ns"][0], (5,), 0.0),
    ("F3 les", flux_cases.F3["les"][0], (5,), les_ref.CW),
    ("F3 tp", flux_cases.F3["tp"][0], (5, "thermallyPerfect"), les_ref.CW),
    ("A ns", lambda: les_cases.deck_a(eq=les_cases.NS), (5,), 0.0),
    ("A les", lambda: les_cases.deck_a(eq=les_cases.LES), (5,), les_ref.CW)])
def test_viscous_values_of_non_wall_surfaces_against_the_restatement(name, make, lib, cw):
    sol = _after_residual(_lib(*lib), make())
    got = _read(sol, 0)
    ref = _viscous_reference(sol, 0, cw)
    tol = _tolerance(sol.case)[:5]
    checked = 0
    for q, s in enumerate(sol.flux_surfaces(0)):
        if s["bc_type"] == "viscousWall":
            continue
        err = np.abs(got["viscous"][q] - ref[q])
        print(f"{name} surface {q} (side {s['side']}): viscous {got['viscous'][q]} restated "
              f"{ref[q]} |diff| {err}")
        assert np.all(err <= tol), (q, err, tol)
        assert np.abs(ref[q][1:]).max() > 0.0
        checked += 1
    assert checked == (6 if name.startswith("A") else 4)
    if name.startswith("A"):       # j-surfaces of 396 faces, k-surfaces of 594: 2 and 3 chunks
        assert sorted(int(np.prod(s["shape"])) for s in sol.flux_surfaces(0)) == \
            [54, 54, 396, 396, 594, 594]
    sol.close()


@pytest.mark.parametrize("name,make,lib", [
    ("F3 ns", flux_cases.F3["ns"][0], (5,)), ("F3 les", flux_cases.F3["les"][0], (5,)),
    ("F3 tp", flux_cases.F3["tp"][0], (5, "thermallyPerfect")),
    ("F1 ns", lambda: flux_cases.f1(**flux_cases.NS,
                                    **flux_cases.SCHEMES["muscl_vanalbada_roe"]), (5,))])
def test_wall_surfaces_against_the_wall_loads(name, make, lib):
    """viscous momentum = viscousForce; viscous energy = heatLoad on a wall at rest, heatLoad +
    sum (tau . u_wall) m |A| on the moving wall (tag 4), tau restated by wall_ref -- each
    value over its own factor, as nondimensional sums (the energy flux is in watts, heatLoad
    keeps the factor of the wall file's heatFlux)"""
    sol = _after_residual(_lib(*lib), make())
    case = sol.case
    gas, g = case.gas, case.ng
    got = _read(sol, 0)
    f_flux, _ = flux_ref.factors(gas, 5)
    loads = sol.wall_loads(0, loads_ref.NO_MOMENTS)
    load_surfs = sol.load_surfaces(0)
    tol = _tolerance(case)
    fields = wall_ref.download_fields(sol, 0)
    ratio = sol.wall_pack(0, ["viscosityRatio"])["viscosityRatio"]
    les = name.endswith("les") or name.endswith("tp")
    walls = 0
    for q, s in enumerate(sol.flux_surfaces(0)):
        if s["bc_type"] != "viscousWall":
            continue
        lq = next(i for i, t in enumerate(load_surfs) if t["range"] == s["range"])
        force = np.array([loads[f"viscousForce_{c}"][lq] for c in "xyz"]) / f_flux[1:4]
        err = np.abs(got["viscous"][q][1:4] - force)
        print(f"{name} wall {q} (side {s['side']}, tag {s['tag']}): viscous momentum "
              f"{got['viscous'][q][1:4]} viscousForce {force} |diff| {err}")
        assert np.all(err <= tol[1:4])
        # (heatLoad carries the factor of the wall file's heatFlux, mu_ref t_ref / l_ref, times
        # l_ref^2; the energy flux the factor of rho E times a_ref l_ref^2: both to the same
        # nondimensional sum)
        energy = loads["heatLoad"][lq] / (wall_ref.GasRef(gas).mu_ref * gas.t_ref * gas.l_ref)
        moving = s["tag"] == 4
        if moving:
            u_wall = np.array([5.0, 0.0, 0.0]) / gas.a_ref            # synthetic.make_deck
            wq = sum(1 for t in sol.flux_surfaces(0)[:q] if t["bc_type"] == "viscousWall")
            wv = wall_ref.wall_vars(fields, s, wall_ref.GasRef(gas), g,
                                    mut_ratio=ratio[wq] if les else None)
            d = (s["side"] - 1) // 2
            fa = fields["farea_" + "ijk"[d]][flux_ref_window(s, g)][..., 3]
            energy += loads_ref.sigma(s["side"]) * math.fsum(((wv["tau"] * u_wall).sum(-1) *
                                                               fa).ravel())
        err = abs(got["viscous"][q][4] - energy)
        print(f"  viscous energy {got['viscous'][q][4]:.17g} heatLoad"
              f"{' + tau . u_wall' if moving else ''} {energy:.17g} |diff| {err:.3e}")
        assert err <= tol[4]
        walls += 1
    assert walls == 2
    sol.close()


def flux_ref_window(surf, ng):
    return tuple(slice(s.start + ng, s.stop + ng) for s in flux_ref.surface_window(surf))


# ---- 3. the connection ------------------------------------------------------------------------------
@pytest.mark.parametrize("eq", ["euler", "navierStokes"])
def test_connection_sides_cancel_and_the_pool_is_the_outer_boundary(eq):
    deck = dict(flux_cases.EULER if eq == "euler" else flux_cases.NS,
                **flux_cases.SCHEMES["muscl_vanalbada_roe"])
    two = _after_residual(_lib(), flux_cases.f2(**deck))
    got = _hold_balance(two, "F2 " + eq)
    surfs = [two.flux_surfaces(gb) for gb in (0, 1)]
    tol = _tolerance(two.case)
    up = next(q for q, s in enumerate(surfs[0]) if s["bc_type"] == "interblock")
    lo = next(q for q, s in enumerate(surfs[1]) if s["bc_type"] == "interblock")
    assert surfs[0][up]["side"] == 2 and surfs[1][lo]["side"] == 1
    # (the viscous values of the two sides are held in the inviscid context, where both are
    # zero: in a viscous one each block evaluates the faces on the rim of the patch with its
    # own edge ghost cells, as its residual does -- tests/test_les_ref_host.py shows the same
    # of the reference's residual -- and the two sides differ there; they are printed)
    for kind in ("inviscid", "viscous"):
        a, b = got[0][kind][up], got[1][kind][lo]
        print(f"F2 {eq} {kind}: block 0 i-max {a}\n   block 1 i-min {b}")
        if kind == "inviscid" or eq == "euler":
            assert np.all(np.abs(a + b) <= tol)
    assert np.all(np.abs(got[0]["inviscid"][up]) > 0.0)
    assert abs(got[0]["area"][up] - got[1]["area"][lo]) <= 64 * EPS52 * got[0]["area"][up]
    # pool_fluxes over both blocks: the connection cancels, the rest is the two residual sums
    f_flux, _ = flux_ref.factors(two.case.gas, 5)
    pooled = pool_fluxes([(two.flux_surfaces(gb), two.surface_fluxes(gb)) for gb in (0, 1)])
    for e in range(5):
        net = (pooled[f"inviscid_{EQ[e]}"] + pooled[f"viscous_{EQ[e]}"]) / f_flux[e]
        rsum = got[0]["residual"][e] + got[1]["residual"][e]
        assert abs(net - rsum) <= tol[e], (EQ[e], net, rsum)
    if eq == "euler":
        # ... and the outer surfaces give what the one block gives (its faces see the same
        # cells: a boundary face's stencil runs across the boundary, not along the cut)
        one = _after_residual(_lib(), flux_cases.f1(**deck))
        ref = _read(one, 0)
        parts = flux_cases.f2_parts(one.flux_surfaces(0), surfs)
        assert [len(p) for p in parts] == [1, 1, 1, 1, 2, 2, 2]
        for q, p in enumerate(parts):
            mine = sum(got[gb]["inviscid"][s] for gb, s in p)
            assert np.all(np.abs(mine - ref["inviscid"][q]) <= tol), q
            area = sum(got[gb]["area"][s] for gb, s in p)
            assert abs(area - ref["area"][q]) <= 1e-13 * area
        one.close()
    two.close()


# ---- 4. uniform free stream -----------------------------------------------------------------------
@pytest.mark.parametrize("n_eq", [5, 7])
def test_uniform_free_stream_closed_form(n_eq):
    """a closed box of characteristic boundaries in its own free stream: every surface gives
    mass = rho v . sum sigma A, rho k v . sum sigma A and rho omega v . sum sigma A, and
    nothing viscous"""
    kw = dict(equation_set="rans", turbulence_model="sst2003", time_integration="implicitEuler",
              cfl=5.0) if n_eq == 7 else dict(flux_cases.NS)
    case = synthetic.single_block_case((6, 5, 4), stretch=1.2, skew=0.02, amplitude=0.0,
                                       bcs=FARFIELD, **kw)
    sol = _after_residual(_lib(n_eq), case)
    got = _read(sol, 0)
    g = case.ng
    s0 = case.blocks[0].state[g, g, g]
    tol = _tolerance(case)
    for q, s in enumerate(sol.flux_surfaces(0)):
        d = (s["side"] - 1) // 2
        fa = sol.geometry("farea_" + "ijk"[d], 0)[flux_ref_window(s, g)]
        a_vec = flux_ref.sigma(s["side"]) * np.array(
            [math.fsum((fa[..., c] * fa[..., 3]).ravel()) for c in range(3)])
        mass = s0[0] * float(s0[1:4] @ a_vec)
        want = {0: mass}
        if n_eq == 7:
            want.update({5: mass * s0[5], 6: mass * s0[6]})
        for e, w in want.items():
            err = abs(got["inviscid"][q][e] - w)
            print(f"free stream ({n_eq} eq) side {s['side']} {EQ[e]}: {got['inviscid'][q][e]:.17g} "
                  f"closed form {w:.17g} |diff| {err:.3e} tol {tol[e]:.3e}")
            assert err <= tol[e]
        assert np.all(np.abs(got["viscous"][q]) <= tol)
    assert abs(got["inviscid"][:, 0].sum()) <= tol[0]          # a closed surface
    sol.close()


# ---- 5. determinism and the id rules -----------------------------------------------------------------
def _raw(sol, gb, ids, n=None, size=512):
    arr = (C.c_int32 * len(ids))(*ids)
    out = np.zeros(size)
    sol.api.check(sol.api.output_pack(sol.ctx, sol.block_ids[gb], len(ids) if n is None else n,
                                      arr, out.ctypes.data_as(abi.c_dp)), "output_pack")
    return out


def test_determinism_and_id_rules():
    names_f = [n for n in abi.FLUX_OUT if not n.endswith(("_tke", "_sdr"))]
    names_b = [n for n in abi.BUDGET_OUT if not n.endswith(("_tke", "_sdr"))]
    case = flux_cases.f1(**flux_cases.NS, **flux_cases.SCHEMES["muscl_vanalbada_roe"])
    sol = Solver(_lib(), case)
    # before the first residual: the totals are there, the residual sums are refused by name
    assert sol.block_budget(0, ["volume", "total_mass"])["volume"] > 0.0
    with pytest.raises(RuntimeError, match="no residual has been formed yet"):
        sol.block_budget(0, ["residual_mass"])
    les_ref.residual_once(sol)
    nsurf = len(sol.flux_surfaces(0))
    for out, names, cols in ((abi.FLUX_OUT, names_f, nsurf), (abi.BUDGET_OUT, names_b, 1)):
        ids = [out[n] for n in names]
        full = _raw(sol, 0, ids)[:len(ids) * cols].reshape(len(ids), cols)
        assert np.array_equal(full, _raw(sol, 0, ids)[:len(ids) * cols].reshape(len(ids), cols))
        assert np.all(full[0] > 0.0)
        # a permuted subset and a repeated id are rows of the full call, bit for bit
        pick = [names[7], names[0], names[10], names[3], names[7]]
        raw = _raw(sol, 0, [out[n] for n in pick])[:5 * cols].reshape(5, cols)
        for row, n in zip(raw, pick):
            assert np.array_equal(row, full[names.index(n)]), n
        rows = _raw(sol, 0, [ids[2]] * 15)[:15 * cols].reshape(15, cols)
        assert all(np.array_equal(r, full[2]) for r in rows)
    flux, bud = abi.FLUX_OUT["area"], abi.BUDGET_OUT["volume"]
    for other, ident in (("cell", abi.OUT["density"]), ("wall", abi.WALL_OUT["yplus"]),
                         ("node", abi.NODE_OUT["density"]), ("load", abi.LOAD_OUT["area"]),
                         ("statistics", abi.STAT_OUT["mean_density"]),
                         ("collapsed statistics", abi.cstat_id(7, "volume")),
                         ("budget", bud)):
        with pytest.raises(RuntimeError, match=f"{other} and flux variables in one call"):
            _raw(sol, 0, [ident, flux])
    with pytest.raises(RuntimeError, match="cell and budget variables in one call"):
        _raw(sol, 0, [bud, abi.OUT["density"]])
    for ident in (flux, bud):
        with pytest.raises(RuntimeError, match="nvar 16 out of range"):
            _raw(sol, 0, [ident] * 16)
    for bad in (383, 399, 447, 463):
        with pytest.raises(RuntimeError, match=f"unknown output variable {bad}"):
            _raw(sol, 0, [bad])
    for n in ("inviscid_tke", "viscous_sdr"):
        with pytest.raises(RuntimeError, match=r"flux variable \d+ \(tke, sdr\) is not kept by "
                                               r"the 5-equation libraries"):
            _raw(sol, 0, [abi.FLUX_OUT[n]])
    with pytest.raises(RuntimeError, match=r"budget variable \d+ \(tke, sdr\) is not kept by "
                                           r"the 5-equation libraries"):
        _raw(sol, 0, [abi.BUDGET_OUT["total_sdr"]])
    sol.close()


class _FluxProber(probe.Prober):
    """probe.Prober with a kind of its own: a flux call and a budget call on every block after
    every hooked entry; a refused flux call must carry the FILL_OPEN message, a budget call is
    never refused"""

    def __init__(self):
        super().__init__("flux")
        self.refused_at = set()

    def _flux(self, s, lev, label, obs):
        for gb in s.block_ids:
            obs[(lev, gb, "budget")] = np.array(list(
                s.block_budget(gb, ["volume", "total_mass", "total_energy"]).values()))
            try:
                obs[(lev, gb, "flux")] = np.stack(list(s.surface_fluxes(gb).values()))
            except RuntimeError as exc:
                assert probe.FILL_OPEN.search(str(exc)), str(exc)
                self.refused_at.add(label)


@pytest.mark.parametrize("deck", [
    dict(equation_set="navierStokes", time_integration="implicitEuler", matrix_solver="lusgs",
         matrix_sweeps=2, cfl=5.0, bcs=loads_ref.WALLS),
    dict(time_integration="rk4", cfl=0.5)])
def test_flux_reads_between_the_phases(deck):
    """the positions of probe.REFUSED_AT are refused for the flux ids -- in a viscous and in an
    inviscid context alike -- and legal for the budget ids; the run stays bit-identical"""
    make = lambda: synthetic.single_block_case((7, 6, 5), stretch=1.2, skew=0.01, **deck)
    lib = _lib()
    base = probe.run(lib, make, "phased")[0]
    prober = _FluxProber()
    top = probe.PhasedSolver(probe.ProbingApi(lib, prober), make(), 0, None, None)
    final = {}
    try:
        prober.solvers = [top]
        for nn in range(2):
            top.step(nn)
        prober.solvers = []
        g = top.case.ng
        for f in ("state", "update"):
            final[(0, 0, f)] = top.download(f, 0)[g:-g, g:-g, g:-g]
        for f in ("residual", "dt", "cons_n", "cons_nm1"):
            final[(0, 0, f)] = top.download(f, 0)
        for q, h in enumerate(top.history):
            final[("history", q, "l2")] = np.array(h["l2"])
            final[("history", q, "linf")] = np.array(h["linf"], dtype=float)
            final[("history", q, "matrix")] = np.array(h["matrix"])
    finally:
        top.close()
    assert probe.differences(base, final) == {}
    want = {label for label, kind in probe.expected_refusals(prober.labels)}
    assert want and prober.refused_at == want, (sorted(prober.refused_at), sorted(want))
    assert all((0, 0, "budget") in prober.seen[pos] for pos in range(len(prober.labels)))
    answered = [pos for pos, obs in prober.seen.items() if (0, 0, "flux") in obs]
    assert len(answered) == sum(1 for label in prober.labels if label not in want)


# ---- 6. bit-identity ------------------------------------------------------------------------------
def _run(lib, make, reads):
    sol = Solver(lib, make())
    deck = sol.case.deck
    record = []
    for nn in range(2):
        sol.store_time_n(nn)
        for mm in range(deck.nonlinear_iterations):
            l2, linf, mres = sol.iterate(mm, deck.cfl(nn))
            record.append(np.concatenate([l2, [linf.linf, linf.block, linf.i, linf.j, linf.k,
                                               linf.eqn, mres]]))
            if reads:
                for gb in sorted(sol.block_ids):
                    flux, bud = sol.surface_fluxes(gb), sol.block_budget(gb)
                    assert np.all(np.isfinite(np.stack(list(flux.values()))))
                    assert np.all(np.isfinite(list(bud.values())))
    out = dict(record=np.array(record))
    g = sol.case.ng
    for gb in sorted(sol.block_ids):
        # (the physical cells: the ghost cells are whatever the last fill left)
        out[("state", gb)] = sol.download("state", gb)[g:-g, g:-g, g:-g]
        out[("residual", gb)] = sol.download("residual", gb)
    d2 = None
    if deck.is_implicit():
        try:
            sol.download("diagonal", 0)
            d2 = False
        except RuntimeError as exc:
            d2 = bool(probe.NOT_HELD["d2_diagonal"].search(str(exc)))
    sol.close()
    return out, d2


@pytest.mark.parametrize("name", ["lusgs_d2", "rk4"])
def test_run_with_reads_after_every_iteration_is_bit_identical(name):
    if name == "lusgs_d2":
        make = lambda: synthetic.single_block_case(
            (12, 9, 7), stretch=1.2, skew=0.01, bcs=loads_ref.WALLS, matrix_sweeps=2,
            **loads_ref.LAMINAR)
    else:
        make = lambda: flux_cases.f1(**flux_cases.EULER,
                                     **flux_cases.SCHEMES["muscl_vanalbada_roe"])
    lib = _lib()
    plain, d2 = _run(lib, make, False)
    read, _ = _run(lib, make, True)
    if name == "lusgs_d2":
        assert d2 is True                # the diagonal-ordered LU-SGS path was the one taken
    assert plain.keys() == read.keys()
    for key in plain:
        assert np.array_equal(plain[key], read[key]), key
