"""The LU-SGS prepare and update kernels move the state and the residual once.

By default k_update_d2 writes the diagonal-ordered (D2) state of the next iteration and
k_lusgs_prepare skips the physical cells (AGX_D2_STATE=update), and k_lusgs_prepare folds the
residual norms so that the update does not read the residual (AGX_RESID_NORMS=prepare).
AGX_D2_STATE=prepare AGX_RESID_NORMS=update is the form in which prepare re-lays the state
every iteration and the update folds the norms.  The two must give the same state, L-inf
record and matrix residual bit for bit; the L2 sums add the same non-negative terms in
another order and may differ by ncells * 2^-52 relative.

Shapes: 37 x 34 x 5 (tiles partial in both directions, more than 32 cells on a diagonal) and
two 20 x 18 x 6 blocks stacked along k.

Run on a real MI355X:  python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

from parity_utils import switches
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import PhasedSolver, Solver

pytestmark = pytest.mark.gpu

WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1),
        2: ("characteristic", 1), 4: ("characteristic", 1)}
FARFIELD = {1: ("characteristic", 1), 2: ("characteristic", 1), 4: ("characteristic", 1)}
# the bench deck (bench.py, workload lusgs)
BENCH = dict(equation_set="navierStokes", face_reconstruction="weno", limiter="none",
             inviscid_flux="ausm", time_integration="implicitEuler", matrix_solver="lusgs",
             matrix_sweeps=1, cfl=10.0)
SINGLE = (37, 34, 5)
STACKED = (20, 18, 6)

NEW = {"AGX_D2_STATE": "update", "AGX_RESID_NORMS": "prepare"}
OLD = {"AGX_D2_STATE": "prepare", "AGX_RESID_NORMS": "update"}


def _single(amplitude=0.05, bcs=WALL, **over):
    return synthetic.single_block_case(SINGLE, stretch=1.2, bcs=bcs, amplitude=amplitude,
                                       **{**BENCH, **over})


def _solver(agx, case, env, cls=Solver, **kw):
    """A solver whose context was created under the given AGX_* switches."""
    with switches(env):
        return cls(agx, case, **kw)


def _iterate(s, case, steps, first=0):
    """`steps` time steps as Solver.step makes them, keeping what agx_iterate returned:
    per nonlinear iteration the raw L2 sums, the L-inf record and the matrix residual."""
    out = []
    for nn in range(first, first + steps):
        s.store_time_n(nn)
        for mm in range(case.deck.nonlinear_iterations):
            l2, linf, mres = s.iterate(mm, case.deck.cfl(nn))
            out.append(dict(l2=l2.copy(), mres=mres,
                            linf=(linf.linf, linf.block, linf.i, linf.j, linf.k, linf.eqn)))
    return out


def _states(s, case):
    g = case.ng
    return [s.download("state", gb)[g:-g, g:-g, g:-g].copy() for gb in sorted(s.block_ids)]


def _run(agx, case, steps, env):
    s = _solver(agx, case, env)
    norms = _iterate(s, case, steps)
    states = _states(s, case)
    s.close()
    return norms, states


def _assert_same(got, ref, case, l2_exact, what):
    """State, L-inf record and matrix residual bit for bit; the L2 sums bit for bit too, or
    within ncells * 2^-52 relative: the bound for reassociating a sum of non-negative terms."""
    (gn, gs), (rn, rs) = got, ref
    tol = case.total_cells * 2.0 ** -52
    assert len(gn) == len(rn)
    for it, (a, b) in enumerate(zip(gn, rn)):
        err = np.abs(a["l2"] - b["l2"]) / b["l2"]
        print(f"{what} it {it}: L2 rel diff {err.max():.3e} (tol {tol:.3e}), "
              f"linf {a['linf']} / {b['linf']}, mres {a['mres']!r} / {b['mres']!r}")
        assert np.all(b["l2"] > 0.0)
        assert a["linf"] == b["linf"], (what, it)
        assert a["mres"] == b["mres"], (what, it)
        if l2_exact:
            assert np.array_equal(a["l2"], b["l2"]), (what, it)
        else:
            assert np.all(err <= tol), (what, it, err)
    for a, b in zip(gs, rs):
        assert np.array_equal(a, b), what


# ---- 1: the bench deck, each switch on its own --------------------------------------------
@pytest.fixture(scope="module")
def bench_ref(agx):
    case = _single()
    return case, _run(agx, case, 4, OLD)


@pytest.mark.parametrize("d2_state,resid_norms", [("update", "prepare"), ("update", "update"),
                                                  ("prepare", "prepare")])
def test_bench_deck_matches_full_form(agx, bench_ref, d2_state, resid_norms):
    """Four iterations of the bench deck on 37 x 34 x 5: every combination of the two switches
    against AGX_D2_STATE=prepare AGX_RESID_NORMS=update.  With the norms left in the update
    everything is bitwise; with the norms folded in prepare the L2 sums are the toleranced
    ones."""
    case, ref = bench_ref
    got = _run(agx, case, 4, {"AGX_D2_STATE": d2_state, "AGX_RESID_NORMS": resid_norms})
    _assert_same(got, ref, case, l2_exact=resid_norms == "update",
                 what=f"D2_STATE={d2_state} RESID_NORMS={resid_norms}")


def test_switch_values_are_checked(agx):
    case = _single()
    for env in ({"AGX_D2_STATE": "sweep"}, {"AGX_RESID_NORMS": "1"}):
        with pytest.raises(RuntimeError):
            _solver(agx, case, env)


# ---- 2: the paths beside the bench deck's ---------------------------------------------------
@pytest.mark.parametrize("name,kw", [
    ("two_sweeps", dict(matrix_sweeps=2)),                       # prepare writes x
    ("euler", dict(equation_set="euler", bcs=FARFIELD)),         # no viscous factor
    ("bdf2", dict(time_integration="bdf2", nonlinear_iterations=2, dt=2.0e-5,
                  dual_time_cfl=100.0)),     # rhs_b reads the state and the time levels
])
def test_variations_match_full_form(agx, name, kw):
    case = _single(**kw)
    steps = 2 if name == "bdf2" else 4          # (bdf2: 2 x 2 nonlinear iterations)
    ref = _run(agx, case, steps, OLD)
    got = _run(agx, case, steps, NEW)
    _assert_same(got, ref, case, l2_exact=False, what=name)


# ---- 3: a state written from outside makes the D2 state stale ------------------------------
@pytest.mark.parametrize("entry", ["state_upload", "field_upload"])
def test_uploaded_state_is_not_taken_for_current(agx, entry):
    """Two iterations, another state through the solver's upload (agx_state_upload) or the
    restart-style field upload (agx_field_upload of AGX_FIELD_STATE), two more: bitwise what
    a fresh context gives that starts from the uploaded state."""
    case, other = _single(), _single(amplitude=0.03)
    new_state = np.ascontiguousarray(other.blocks[0].state, dtype=np.float64)
    assert not np.array_equal(new_state, case.blocks[0].state)
    s = _solver(agx, case, NEW)
    _iterate(s, case, 2)
    if entry == "state_upload":
        s.upload("state", 0, new_state)
    else:
        agx.check(agx.field_upload(s.ctx, s.block_ids[0], abi.FIELD["state"],
                                   new_state.ctypes.data_as(abi.c_dp)), "field_upload")
    got = (_iterate(s, case, 2, first=2), _states(s, case))
    s.close()
    f = _solver(agx, other, NEW)
    ref = (_iterate(f, other, 2, first=2), _states(f, other))
    f.close()
    _assert_same(got, ref, case, l2_exact=True, what=entry)


# ---- 4: ghost positions across a connection keep the full path -----------------------------
def test_stacked_blocks_match_full_form(agx):
    case = synthetic.stacked_blocks_case(n=STACKED, nblocks=2, axis="k", stretch=1.2, bcs=WALL,
                                         amplitude=0.05, **BENCH)
    ref = _run(agx, case, 3, OLD)
    got = _run(agx, case, 3, NEW)
    _assert_same(got, ref, case, l2_exact=False, what="stacked")


# ---- 5: the phases driven by hand -----------------------------------------------------------
def _phased(agx, case, env):
    return _solver(agx, case, env, cls=PhasedSolver, rank=0, exchange=None, alloc=None)


def test_phase_api_returns_the_norms_of_iterate(agx):
    """bc, residual, implicit_begin, sweeps, matrix_residual, implicit_update by hand: the
    matrix residual read back on its own lands in the update's slots of the norm buffer
    between prepare and update, and must not disturb the norms prepare folded."""
    case = _single()
    s = _solver(agx, case, NEW)
    ref = (_iterate(s, case, 4), _states(s, case))
    s.close()
    p = _phased(agx, case, NEW)
    got = (_iterate(p, case, 4), _states(p, case))
    p.close()
    _assert_same(got, ref, case, l2_exact=True, what="phases")


def test_second_residual_before_the_update_supplies_the_norms(agx):
    """agx_phase_residual called again between implicit_begin and the update (on another
    state, so that it is another residual): the update falls back to reading the residual
    planes, and its norms are those of the planes as they are then."""
    case, other = _single(), _single(amplitude=0.03)
    new_state = np.ascontiguousarray(other.blocks[0].state, dtype=np.float64)
    p = _phased(agx, case, NEW)
    first = _iterate(p, case, 2)[-1]
    api, ctx, cfl = agx, p.ctx, case.deck.cfl(2)
    p.store_time_n(2)
    api.check(api.phase_bc_faces(ctx), "bc_faces")
    api.check(api.halo_swap_local(ctx, abi.HALO_STATE), "halo")
    api.check(api.phase_bc_edges(ctx), "bc_edges")
    api.check(api.phase_residual(ctx, 0, cfl), "residual")
    api.check(api.phase_implicit_begin(ctx), "implicit_begin")
    r_first = p.download("residual", 0)
    p.upload("state", 0, new_state)
    api.check(api.phase_bc_faces(ctx), "bc_faces")
    api.check(api.halo_swap_local(ctx, abi.HALO_STATE), "halo")
    api.check(api.phase_bc_edges(ctx), "bc_edges")
    api.check(api.phase_residual(ctx, 0, cfl), "residual")
    r = p.download("residual", 0)
    assert not np.array_equal(r, r_first)
    api.check(api.halo_swap_local(ctx, abi.HALO_UPDATE), "halo")
    api.check(api.phase_relax_forward(ctx, 0), "relax_forward")
    api.check(api.halo_swap_local(ctx, abi.HALO_UPDATE), "halo")
    api.check(api.phase_relax_backward(ctx, 0), "relax_backward")
    api.check(api.halo_swap_local(ctx, abi.HALO_UPDATE), "halo")
    mres = C.c_double(0.0)
    api.check(api.phase_matrix_residual(ctx, C.byref(mres)), "matrix_residual")
    l2 = np.zeros(5)
    linf = abi.Linf()
    api.check(api.phase_implicit_update(ctx, 0, l2.ctypes.data_as(abi.c_dp), C.byref(linf)),
              "implicit_update")
    p.close()
    want = (r * r).sum(axis=(0, 1, 2))
    tol = case.total_cells * 2.0 ** -52
    err = np.abs(l2 - want) / want
    print(f"second residual: L2 rel diff {err.max():.3e} (tol {tol:.3e}); "
          f"first iteration's sums {first['l2']}")
    assert np.all(err <= tol), err
    # the first (k, j, i, equation) of the largest signed residual
    k, j, i, e = np.unravel_index(np.argmax(r), r.shape)
    assert (linf.linf, linf.i, linf.j, linf.k, linf.eqn) == (r[k, j, i, e], i, j, k, e + 1)
    # ... and not those of the residual prepare saw
    assert not np.all(np.abs(l2 - (r_first * r_first).sum(axis=(0, 1, 2))) / want <= tol)
