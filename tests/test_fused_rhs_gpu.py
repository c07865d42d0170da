"""The viscous tile kernel writes the LU-SGS right-hand side where the library can prove it may.

Inside agx_iterate, for a block on the diagonal-ordered (D2) path whose D2 state the last update
left current, k_visc_tile takes its RHS form: it stores b, 1 / a and the aInv_ plane and folds
the residual norms, and agx_phase_implicit_begin launches no k_lusgs_prepare for the block.
AGX_D2_STATE=prepare is the comparison form: the same viscous kernel without the RHS form and
the (full) pass behind it.  Every case compares the default against it: state, L-inf record and
matrix residual bit for bit; the L2 sums add the same squares over other partials (one per wave
of a persistent workgroup instead of one per tile) and may differ by ncells * 2^-52 relative.

Timing group 5 (agx_timing_get) counts the implicit_begin calls that still launched the pass:
the comparisons would pass vacuously if the RHS form never ran, so the counts are asserted.

Shapes: 70 x 13 x 9 -- two viscous column tiles in i (62 + 8 owned cells) and three in j
(6 + 6 + 1), Pi != Pj so that both triangles of the D2 plane and the jlo != 0 branch are
written, few planes so that segments prime often -- and the same block as 9 x 70 x 13.

Run on a real MI355X:  python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

import mg_transfer_cases as mgc
from parity_utils import switches
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import PhasedSolver, Solver

pytestmark = pytest.mark.gpu

# the bench deck and its boundaries (bench.py, workload lusgs)
WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1),
        2: ("characteristic", 1), 4: ("characteristic", 1)}
BENCH = dict(equation_set="navierStokes", face_reconstruction="weno", limiter="none",
             inviscid_flux="ausm", time_integration="implicitEuler", matrix_solver="lusgs",
             matrix_sweeps=1, cfl=10.0)
LONG_I = (70, 13, 9)
LONG_J = (9, 70, 13)
STACKED = (20, 18, 6)

FUSED = {}                                   # the defaults
PASS = {"AGX_D2_STATE": "prepare"}           # the comparison form
G_PREPARE = 5


def _single(n=LONG_I, **over):
    return synthetic.single_block_case(n, stretch=1.2, bcs=WALL, amplitude=0.05,
                                       **{**BENCH, **over})


def _solver(agx, case, env, cls=Solver, **kw):
    """A solver whose context was created under the given AGX_* switches, timing on."""
    with switches(env):
        s = cls(agx, case, **kw)
    agx.check(agx.timing_enable(s.ctx, 1), "timing_enable")
    return s


def _prepare_launches(agx, s):
    """Launches of timing group 5 since the last call, the counter reset."""
    ms, cnt = C.c_double(0.0), C.c_int64(0)
    agx.check(agx.timing_get(s.ctx, G_PREPARE, C.byref(ms), C.byref(cnt)), "timing_get")
    agx.check(agx.timing_reset(s.ctx), "timing_reset")
    return cnt.value


def _iterate(agx, s, case, steps, first=0):
    """`steps` time steps as Solver.step makes them; per agx_iterate call the raw L2 sums, the
    L-inf record, the matrix residual and the launches of the prepare pass."""
    out = []
    for nn in range(first, first + steps):
        s.store_time_n(nn)
        for mm in range(case.deck.nonlinear_iterations):
            l2, linf, mres = s.iterate(mm, case.deck.cfl(nn))
            out.append(dict(l2=l2.copy(), mres=mres, prepare=_prepare_launches(agx, s),
                            linf=(linf.linf, linf.block, linf.i, linf.j, linf.k, linf.eqn)))
    return out


def _states(s, case):
    g = case.ng
    return [s.download("state", gb)[g:-g, g:-g, g:-g].copy() for gb in sorted(s.block_ids)]


def _run(agx, case, steps, env, cls=Solver, **kw):
    s = _solver(agx, case, env, cls=cls, **kw)
    norms = _iterate(agx, s, case, steps)
    states = _states(s, case)
    s.close()
    return norms, states


def _assert_same(got, ref, case, what):
    """State, L-inf record and matrix residual bit for bit; the L2 sums within
    ncells * 2^-52 relative: the bound for reassociating a sum of non-negative terms."""
    (gn, gs), (rn, rs) = got, ref
    tol = case.total_cells * 2.0 ** -52
    assert len(gn) == len(rn)
    for it, (a, b) in enumerate(zip(gn, rn)):
        err = np.abs(a["l2"] - b["l2"]) / b["l2"]
        print(f"{what} it {it}: L2 rel diff {err.max():.3e} (tol {tol:.3e}), "
              f"linf {a['linf']} / {b['linf']}, mres {a['mres']!r} / {b['mres']!r}, "
              f"prepare launches {a['prepare']} / {b['prepare']}")
        assert np.all(b["l2"] > 0.0)
        assert a["linf"] == b["linf"], (what, it)
        assert a["mres"] == b["mres"], (what, it)
        assert np.all(err <= tol), (what, it, err)
    assert len(gs) == len(rs)
    for a, b in zip(gs, rs):
        assert np.array_equal(a, b), what


def _launches(run):
    return [it["prepare"] for it in run[0]]


# ---- 1: the bench deck on the two shapes ----------------------------------------------------
def _bench_run(agx, case, env):
    """Four iterations; the finished diagonal after the second.  The diagonal-ordered path
    refuses the download of AGX_FIELD_DIAGONAL by name (it keeps a_ as 1 / a inside its sweep
    arrays), so the aInv_ plane -- which the RHS form writes in prepare's place -- is read the
    way the library itself reads it: agx_mg_matrix_residual forms A x - b on the planes with
    that plane as the diagonal."""
    s = _solver(agx, case, env)
    norms = _iterate(agx, s, case, 2)
    with pytest.raises(RuntimeError):
        s.download("diagonal", 0)
    ms = C.c_double(0.0)
    agx.check(agx.mg_matrix_residual(s.ctx, C.byref(ms)), "mg_matrix_residual")
    norms += _iterate(agx, s, case, 2, first=2)
    states = _states(s, case)
    s.close()
    return (norms, states), ms.value


@pytest.fixture(scope="module", params=[LONG_I, LONG_J], ids=["70x13x9", "9x70x13"])
def bench_pair(agx, request):
    case = _single(request.param)
    return case, _bench_run(agx, case, FUSED), _bench_run(agx, case, PASS)


def test_bench_deck_matches_the_pass(bench_pair):
    case, (got, gdiag), (ref, rdiag) = bench_pair
    _assert_same(got, ref, case, "bench deck")
    print(f"plane-form matrix residual after iteration 2: {gdiag!r} / {rdiag!r}")
    assert rdiag > 0.0
    assert gdiag == rdiag


def test_the_fused_path_ran(bench_pair):
    """The first iteration takes the full prepare (nothing has left a D2 state yet); from the
    second on the default launches none, the comparison form one per iteration."""
    _, (got, _), (ref, _) = bench_pair
    assert _launches(got) == [1, 0, 0, 0]
    assert _launches(ref) == [1, 1, 1, 1]


# ---- 2: the pass still runs where it must ---------------------------------------------------
def test_stacked_blocks_keep_the_pass(agx):
    """Two blocks with a connection between them (ghost_s): every iteration launches the pass."""
    case = synthetic.stacked_blocks_case(n=STACKED, nblocks=2, axis="k", stretch=1.2, bcs=WALL,
                                         amplitude=0.05, **BENCH)
    got = _run(agx, case, 3, FUSED)
    ref = _run(agx, case, 3, PASS)
    _assert_same(got, ref, case, "stacked")
    assert _launches(got) == [1, 1, 1]


def test_second_nonlinear_iteration_keeps_the_pass(agx):
    """nonlinear_iterations = 2: the mm = 1 call works on a state that is no longer time level
    n (un_is_u = 0), b reads the state and consVarsN, and the pass runs."""
    case = _single(nonlinear_iterations=2)
    got = _run(agx, case, 2, FUSED)
    ref = _run(agx, case, 2, PASS)
    _assert_same(got, ref, case, "nonlinear 2")
    assert _launches(got) == [1, 1, 0, 1]
    assert _launches(ref) == [1, 1, 1, 1]


def test_state_upload_brings_one_full_prepare(agx):
    """agx_state_upload between iterations 2 and 3 clears the block's flags: iteration 3 takes
    the (full) pass, iteration 4 is fused again."""
    case, other = _single(), synthetic.single_block_case(LONG_I, stretch=1.2, bcs=WALL,
                                                         amplitude=0.03, **BENCH)
    new_state = np.ascontiguousarray(other.blocks[0].state, dtype=np.float64)
    assert not np.array_equal(new_state, case.blocks[0].state)
    runs = []
    for env in (FUSED, PASS):
        s = _solver(agx, case, env)
        norms = _iterate(agx, s, case, 2)
        s.upload("state", 0, new_state)
        norms += _iterate(agx, s, case, 2, first=2)
        runs.append((norms, _states(s, case)))
        s.close()
    _assert_same(runs[0], runs[1], case, "state upload")
    assert _launches(runs[0]) == [1, 0, 1, 0]


class _ReadingPhases(PhasedSolver):
    """PhasedSolver.iterate with a residual download between agx_phase_residual and
    agx_phase_implicit_begin (single rank, scalar LU-SGS)."""

    def iterate(self, mm, cfl):
        api, ctx, cfg = self.api, self.ctx, self.cfg
        l2, linf, mres = np.zeros(cfg.n_eq), abi.Linf(), C.c_double(0.0)
        api.check(api.phase_bc_faces(ctx), "phase_bc_faces")
        self._halo(abi.HALO_STATE)
        api.check(api.phase_bc_edges(ctx), "phase_bc_edges")
        api.check(api.phase_residual(ctx, mm, cfl), "phase_residual")
        self.resid = self.download("residual", 0)
        api.check(api.phase_implicit_begin(ctx), "phase_implicit_begin")
        for s in range(cfg.matrix_sweeps):
            self._halo(abi.HALO_UPDATE)
            api.check(api.phase_relax_forward(ctx, s), "relax_forward")
            self._halo(abi.HALO_UPDATE)
            api.check(api.phase_relax_backward(ctx, s), "relax_backward")
        self._halo(abi.HALO_UPDATE)
        api.check(api.phase_matrix_residual(ctx, C.byref(mres)), "matrix_residual")
        api.check(api.phase_implicit_update(ctx, mm, l2.ctypes.data_as(abi.c_dp), C.byref(linf)),
                  "implicit_update")
        return l2, linf, mres.value


def test_phase_api_keeps_the_pass(agx):
    """The same four iterations driven through the phases, the residual read in between: a
    caller may read or change it there, so the pass runs every iteration; the result is
    agx_iterate's."""
    case = _single()
    ref = _run(agx, case, 4, FUSED)
    got = _run(agx, case, 4, FUSED, cls=_ReadingPhases, rank=0, exchange=None, alloc=None)
    _assert_same(got, ref, case, "phases")
    assert _launches(got) == [1, 1, 1, 1]
    assert _launches(ref) == [1, 0, 0, 0]


# ---- 3: a multigrid level with LU-SGS -------------------------------------------------------
def test_multigrid_level_keeps_the_pass(agx):
    """Two levels over the smallest case of tests/mg_transfer_cases.py: the forcing term and
    the coarse level's accumulated diagonal need the pass; two V cycles equal the comparison
    form's."""
    cases, _ = mgc.levels("lusgs5", "split")
    runs = []
    for env in (FUSED, PASS):
        with switches(env):
            m = mgc.open_levels(agx, "lusgs5", "split")
        hist = [m.step(nn) for nn in range(2)]
        g = cases[0].ng
        state = m.download("state", 0)[g:-g, g:-g, g:-g].copy()
        m.close()
        runs.append((hist, state))
    (gh, gs), (rh, rs) = runs
    tol = cases[0].total_cells * 2.0 ** -52
    for a, b in zip(gh, rh):
        # (history holds sqrt(L2 sum): half the relative error of the sum)
        assert np.all(np.abs(a["l2"] - b["l2"]) <= tol * b["l2"])
        assert a["linf"] == b["linf"]
        assert a["matrix"] == b["matrix"]
    assert np.array_equal(gs, rs)
