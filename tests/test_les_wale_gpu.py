"""Large-eddy simulation with the WALE subgrid model on the device (equationSet
largeEddySimulation, turbulenceModel wale; the 5-equation libraries, explicit time integration).

No deck of the reference's test cases selects the model and the CPU oracle does not carry it:
the device is held to the numpy restatement of tests/les_ref.py, fed with the fields downloaded
after the call (tests/test_les_ref_host.py proves the restatement on the oracle and on closed
forms, and shows that every deck used here can see a missing or mis-scaled eddy viscosity), and
to the library's other kernel form.  The decks are those of tests/les_cases.py."""
import numpy as np
import pytest

import les_cases
import les_ref
import loads_ref
import parity_utils
import wall_ref
from aither_amd import abi
from aither_amd.solver import Solver

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
WALL_NAMES = list(wall_ref.STATE_NAMES + wall_ref.GRAD_NAMES) + ["viscosityRatio"]


def _lib(name):
    import aither_amd
    return aither_amd.load(5, "thermallyPerfect" if name == "E" else "caloricallyPerfect")


def _solver(monkeypatch, name, eq, form, lib=None, **kw):
    """form: "tile" (what the library selects itself) or "gather" (AGX_VISC=gather, read when
    the context is created)"""
    if form == "gather":
        monkeypatch.setenv("AGX_VISC", "gather")
    else:
        monkeypatch.delenv("AGX_VISC", raising=False)
    return Solver(lib or _lib(name), les_cases.DECKS[name](eq=eq, **kw))


def _cells(sol, field):
    return [sol.download(field, gb) for gb in sorted(sol.block_ids)]


def _restated(sol, name):
    """per block: (les, laminar, increment) of the restatement on the fields the device holds"""
    case = sol.case
    gas = wall_ref.GasRef(case.gas)
    out = []
    for gb in sorted(sol.block_ids):
        fields = wall_ref.download_fields(sol, gb)
        out.append(les_ref.increment(fields, gas, case.blocks[gb].geom.n, case.ng,
                                     fourth=les_cases.FOURTH[name],
                                     visc_cfl_coeff=case.deck.viscous_cfl_coefficient()) +
                   (fields,))
    return out


def _hold_residual_to_restatement(les, ns, name, form, cfl):
    """residual, spectral radius, dt and the function-file variables of every block, after one
    residual of both contexts"""
    case = les.case
    g = case.ng
    gas = wall_ref.GasRef(case.gas)
    for gb, (ref_les, ref_lam, inc, fields) in zip(sorted(les.block_ids), _restated(les, name)):
        assert np.array_equal(les.download("state", gb), ns.download("state", gb))
        # 2. residual(LES) - residual(navierStokes) against the restatement's WALE increment
        r_les, r_ns = les.download("residual", gb), ns.download("residual", gb)
        diff = r_les - r_ns
        assert np.all(diff[..., 0] == 0.0)
        for e in range(1, 5):
            scale = np.abs(inc["residual"][..., e]).max()
            tol = 1e-8 * scale + 16.0 * ULP * np.abs(r_les[..., e]).max()
            err = np.abs(diff[..., e] - inc["residual"][..., e]).max()
            print(f"deck {name} {form} block {gb}: residual increment {e}: |diff| {err:.3e} "
                  f"tol {tol:.3e} (increment {scale:.3e})")
            assert scale > 0.0 and err <= tol, (e, err, tol)
        # 3. the spectral radius the same way
        s_les = les.download("spec_radius", gb)[..., 0]
        s_ns = ns.download("spec_radius", gb)[..., 0]
        scale = np.abs(inc["spec_radius"]).max()
        tol = 1e-8 * scale + 16.0 * ULP * np.abs(s_les).max()
        err = np.abs((s_les - s_ns) - inc["spec_radius"]).max()
        print(f"deck {name} {form} block {gb}: spectral radius increment: |diff| {err:.3e} "
              f"tol {tol:.3e} (increment {scale:.3e})")
        assert scale > 0.0 and err <= tol
        # 4. dt * spectral radius = cfl * volume
        dt = les.download("dt", gb)[..., 0]
        vol = fields["volume"][g:-g, g:-g, g:-g, 0]
        assert np.abs(dt * s_les - cfl * vol).max() <= 1e-12 * (cfl * vol).max()
        # 5. turbulentViscosity, viscosityRatio of the function file (output.cpp:284-291)
        got = les.output_pack(gb, ["turbulentViscosity", "viscosityRatio"])
        mu_c = fields["viscosity"][g:-g, g:-g, g:-g, 0]
        want = [ref_les["eddy"] * gas.mu_ref, ref_les["eddy"] / mu_c]
        for q, label in enumerate(("turbulentViscosity", "viscosityRatio")):
            err = np.abs(got[q] - want[q]).max() / np.abs(want[q]).max()
            print(f"deck {name} {form} block {gb}: {label}: {err:.3e} (tol 1e-8)")
            assert want[q].max() > 0.0 and err <= 1e-8
        assert np.all(ns.output_pack(gb, ["turbulentViscosity", "viscosityRatio"]) == 0.0)


FORMS = [("A", "tile"), ("A", "gather"), ("B", "tile"), ("C", "tile"), ("C", "gather"),
         ("E", "tile")]


@pytest.mark.parametrize("name, form", FORMS)
def test_one_residual_against_the_restatement(monkeypatch, name, form):
    """the same state in a largeEddySimulation and a navierStokes context of the same library
    and kernel form, one agx_phase_residual each (on E the library has the gather form only)"""
    les = _solver(monkeypatch, name, les_cases.LES, form)
    ns = _solver(monkeypatch, name, les_cases.NS, form)
    # before the first residual: no eddy viscosity, and the wall ids behave as in navierStokes
    assert np.all(les.output_pack(0, ["turbulentViscosity", "viscosityRatio"]) == 0.0)
    if les.wall_surfaces(0):
        a, b = les.wall_pack(0, ["temperature", "density"]), ns.wall_pack(0, ["temperature", "density"])
        assert all(np.array_equal(x, y) for n in a for x, y in zip(a[n], b[n]))
    cfl = les_ref.residual_once(les)
    assert les_ref.residual_once(ns) == cfl
    _hold_residual_to_restatement(les, ns, name, form, cfl)
    case, g = les.case, les.case.ng
    gas = wall_ref.GasRef(case.gas)

    if les.wall_surfaces(0):
        # 7. the wall payload at the low-Re wall faces
        got = les.wall_pack(0, list(abi.WALL_OUT))
        fields = wall_ref.download_fields(les, 0)
        ref_les = les_ref.operator(fields, gas, case.blocks[0].geom.n, g)
        ref = {n: [] for n in abi.WALL_OUT}
        for surf in les.wall_surfaces(0):
            d, upper = (surf["side"] - 1) // 2, surf["side"] % 2 == 0
            sl = [slice(None)] * 3
            sl[2 - d] = slice(-1, None) if upper else slice(0, 1)
            mut_s = gas.scaling * ref_les["mut"][d][tuple(sl)]
            mu_s = gas.scaling * ref_les["mu_face"][d][tuple(sl)]
            w = wall_ref.wall_vars(fields, surf, gas, g, mut_ratio=mut_s / (mu_s + wall_ref.EPS))
            for n in abi.WALL_OUT:
                ref[n].append(w[n])
        wall_ref.compare(got, ref, names=WALL_NAMES)
        assert max(r.max() for r in ref["viscosityRatio"]) > 0.0
        # 8. the loads integrate that same stress
        loads = les.wall_loads(0, loads_ref.NO_MOMENTS)
        loads_ref.compare(loads, loads_ref.block_reference(les, 0), loads_ref.NO_MOMENTS,
                          what=f"deck {name} {form}")
        assert not np.array_equal(loads["viscousForce_x"],
                                  ns.wall_loads(0, ["viscousForce_x"])["viscousForce_x"])
    les.close(), ns.close()


@pytest.mark.parametrize("name", ["A", "B"])
def test_tile_and_gather_forms_agree_over_time(monkeypatch, name):
    """two RK4 iterations (eight stages) and, in a second pair of contexts, one explicit-Euler
    iteration: state and residual by the measures of tests/parity_utils.py at the suite's 1e-10"""
    for integ, steps in (("rk4", 2), ("explicitEuler", 1)):
        tile = _solver(monkeypatch, name, les_cases.LES, "tile", time_integration=integ)
        gather = _solver(monkeypatch, name, les_cases.LES, "gather", time_integration=integ)
        for nn in range(steps):
            tile.step(nn), gather.step(nn)
        case, g = tile.case, tile.case.ng
        states = _cells(gather, "state")
        got_s = [s[g:-g, g:-g, g:-g] for s in _cells(tile, "state")]
        ref_s = [s[g:-g, g:-g, g:-g] for s in states]
        got_r, ref_r = _cells(tile, "residual"), _cells(gather, "residual")
        print(f"deck {name} {integ}: state rel_err {parity_utils.rel_err(got_s[0], ref_s[0]):.3e} "
              f"residual rel_err {parity_utils.rel_err(got_r[0], ref_r[0]):.3e}")
        assert parity_utils.rel_err(got_s[0], ref_s[0]) < parity_utils.RTOL
        assert parity_utils.rel_err(got_r[0], ref_r[0],
                                    1.0e-3 * parity_utils.flux_scale(case)) < parity_utils.RTOL
        parity_utils.assert_components(case, "state", got_s, ref_s, states)
        parity_utils.assert_components(case, "residual", got_r, ref_r, states)
        assert np.abs(tile.output_pack(0, ["turbulentViscosity"])).max() > 0.0
        tile.close(), gather.close()


def test_two_blocks_cut_inside_a_tile_against_the_one_block(monkeypatch):
    """D against A: residual, spectral radius and eddy viscosity of the two halves within 1e-12
    of each field's largest value: the face at the cut is evaluated once on each side, from the
    same cells.  That holds for every cell but the rim of the cut -- the cells next to it that
    also lie on a j or k boundary: their faces read cells that are face ghost cells of the one
    block and edge ghost cells (another fill, another ghost geometry: SwapGeomSlice's border
    rule, the edge fill) of the two, in the reference as here; the oracle's navierStokes
    residuals of D and A differ there by 8e-8 and are bit-equal everywhere else
    (tests/test_les_ref_host.py).  The rim, like every cell of D, is held to the restatement
    instead, by the checks of test_one_residual_against_the_restatement on both blocks, in the
    gather form, and the tile form to the gather form by the suite's parity measure.  (The
    navierStokes context is a gather-form one because the navierStokes tile kernel takes the
    area vector of the face beyond a block's last i- or j-face from a clamped slot, which across
    a connection on a stretched grid is not that face's: DESIGN section 8.)"""
    one = _solver(monkeypatch, "A", les_cases.LES, "tile")
    two = _solver(monkeypatch, "D", les_cases.LES, "tile")
    two_g = _solver(monkeypatch, "D", les_cases.LES, "gather")
    ns = _solver(monkeypatch, "D", les_cases.NS, "gather")
    cfl = les_ref.residual_once(one)
    assert les_ref.residual_once(two) == cfl and les_ref.residual_once(ns) == cfl
    assert les_ref.residual_once(two_g) == cfl
    rim = les_cases.cut_rim()
    for label, get in (("residual", lambda s, gb: s.download("residual", gb)),
                       ("spec_radius", lambda s, gb: s.download("spec_radius", gb)),
                       ("turbulentViscosity",
                        lambda s, gb: s.output_pack(gb, ["turbulentViscosity"])[0][..., None])):
        whole = get(one, 0)
        halves = np.concatenate([get(two, 0), get(two, 1)], axis=2)
        assert halves.shape == whole.shape
        diff = np.abs(halves - whole).max(-1)
        err = diff[~rim].max() / np.abs(whole).max()
        print(f"D against A, {label}: {err:.3e} (tol 1e-12); in the rim of the cut "
              f"{diff[rim].max() / np.abs(whole).max():.3e}")
        assert err <= 1e-12, label
    assert two.download("residual", 0).shape[2] == les_cases.CUT
    _hold_residual_to_restatement(two_g, ns, "D", "gather", cfl)
    states = _cells(two_g, "state")
    parity_utils.assert_components(two.case, "residual", _cells(two, "residual"),
                                   _cells(two_g, "residual"), states)
    for gb in sorted(two.block_ids):
        a, b = (s.output_pack(gb, ["turbulentViscosity"]) for s in (two, two_g))
        assert np.abs(a - b).max() <= parity_utils.RTOL * np.abs(b).max()
    one.close(), two.close(), two_g.close(), ns.close()


def _refused(name, message, lib=None, deck=(), **kw):
    """deck: attributes set after the case is built (the deck parser refuses them itself; the
    library must refuse them too)"""
    case = les_cases.DECKS[name](**kw)
    for key, val in dict(deck).items():
        setattr(case.deck, key, val)
    with pytest.raises(RuntimeError, match=message):
        Solver(lib or _lib(name), case).close()


@pytest.mark.parametrize("integ", ["implicitEuler", "bdf2", "crankNicholson"])
def test_implicit_les_is_refused_by_name(integ):
    _refused("C", "largeEddySimulation with an implicit time_integration.*no independent "
             "reference.*explicitEuler and rk4 are built", time_integration=integ)


def test_inconsistent_models_are_refused_by_name():
    import aither_amd
    _refused("C", r"largeEddySimulation with turbulence_model 1: it accepts wale only.*"
             r"input\.cpp:965", deck=dict(turbulence_model="sst2003"))
    _refused("C", r"turbulence_model wale with equation_set 1.*input\.cpp:970-978",
             eq=les_cases.NS, deck=dict(turbulence_model="wale"))
    # the 7-equation library goes on refusing everything but rans: by the number of equations,
    # and, told that there are seven, by the equation set
    _refused("C", "built for 7 equations", lib=aither_amd.load(7))
    case = les_cases.deck_c()
    case.n_eq = 7
    with pytest.raises(RuntimeError, match="rans .viscous. only"):
        Solver(aither_amd.load(7), case).close()
