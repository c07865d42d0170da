"""The multigrid cycle driver (aither_amd.solver.MultigridSolver) against what does not share
its mistakes: on one level the plain iteration (Solver: ora_iterate), bit for bit; on every
level the calls gridLevel::CalcResidual makes.  CPU, on the oracle.

Every other multigrid test compares the library with the oracle under the SAME driver, so a
call the driver leaves out cancels.  gridLevel::CalcResidual (gridLevel.cpp:372-400) ends
with SwapEddyViscAndGradients and, for rans, SwapTurbVars (:386-392); Restriction (:559-563)
calls it on the coarse level: every level makes these swaps."""
import numpy as np
import pytest

from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import MultigridSolver, Solver

WALL = {3: ("viscousWall", 2)}
RANS_WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
             4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
NS = dict(equation_set="navierStokes", bcs=WALL, cfl=20.0, matrix_sweeps=2)
RANS = dict(equation_set="rans", turbulence_model="sst2003", bcs=RANS_WALL, cfl=10.0,
            matrix_sweeps=2)
ROWS = {
    "euler_dplur": dict(matrix_solver="dplur", matrix_sweeps=4, cfl=40.0),
    "ns_lusgs": dict(matrix_solver="lusgs", **NS),
    "ns_blusgs": dict(matrix_solver="blusgs", **NS),
    "ns_bdplur": dict(matrix_solver="bdplur", **NS),
    "rans_lusgs": dict(matrix_solver="lusgs", **RANS),
    "rans_dplur": dict(matrix_solver="dplur", **RANS),
    "rans_blusgs": dict(matrix_solver="blusgs", **RANS),
}
BOX = dict(n=(12, 10, 8), axis="i", stretch=1.15, amplitude=0.05)


def _one_level_equals_plain(oracle, nblocks, iterations=3, **kw):
    cases, trs = synthetic.multigrid_levels(levels=1, nblocks=nblocks, **BOX, **kw)
    assert len(cases) == 1 and trs == []
    m, s = MultigridSolver(oracle, cases, []), Solver(oracle, cases[0])
    try:
        for nn in range(iterations):
            m.step(nn), s.step(nn)
        assert len(m.history) == len(s.history) == iterations * cases[0].deck.nonlinear_iterations
        for hm, hs in zip(m.history, s.history):
            at = (hm["nn"], hm["mm"])
            assert np.array_equal(hm["l2"], hs["l2"]), (at, hm["l2"], hs["l2"])
            assert hm["linf"] == hs["linf"], (at, hm["linf"], hs["linf"])
            assert hm["matrix"] == hs["matrix"], (at, hm["matrix"], hs["matrix"])
        for gb in range(nblocks):
            a, b = m.download("state", gb), s.download("state", gb)
            assert np.array_equal(a, b), (gb, np.abs(a - b).max())
    finally:
        m.close(), s.close()


@pytest.mark.parametrize("nblocks", [1, 2])
@pytest.mark.parametrize("row", sorted(ROWS))
def test_one_level_is_the_plain_iteration(oracle, row, nblocks):
    """MultigridSolver over ONE level against Solver (ora_iterate) on the same case, three
    iterations: the norms, the L-inf record, the matrix residual and every block's state with
    its ghost cells are equal bit for bit.  One block: no connection, nothing to swap.  Two
    blocks joined along i: a driver that leaves out the swap of the velocity gradients
    (viscous block-matrix solvers) or of eddy viscosity, f1, f2 (rans) differs by 2e-10 to
    2e-9 of the state."""
    _one_level_equals_plain(oracle, nblocks, time_integration="implicitEuler", **ROWS[row])


def test_one_level_is_the_plain_iteration_bdf2(oracle):
    """The same with bdf2 and two nonlinear iterations (mm > 0: the right-hand side carries the
    time levels n and n - 1), viscous BLU-SGS on two blocks."""
    _one_level_equals_plain(oracle, 2, iterations=2, time_integration="bdf2",
                            nonlinear_iterations=2, dt=2.0e-5, dual_time_cfl=100.0,
                            **ROWS["ns_blusgs"])


class RecordingApi:
    """Forwards every call to the Api it wraps and logs (name, context, selector): the
    context is the first argument where that is one, the selector the second argument of
    halo_exchange."""

    def __init__(self, api):
        self._api, self.log = api, []

    def __getattr__(self, name):
        target = getattr(self._api, name)
        if name == "check" or not callable(target):
            return target

        def call(*args):
            ctx = args[0].value if args and hasattr(args[0], "value") and \
                isinstance(args[0].value, (int, type(None))) else None
            sel = args[1] if name == "halo_exchange" else None
            self.log.append((name, ctx, sel))
            return target(*args)
        return call


SWAP_CASES = {
    "rans_blusgs": (ROWS["rans_blusgs"], [abi.HALO_VELGRAD_A, abi.HALO_VELGRAD_B, abi.HALO_TURB]),
    "ns_bdplur": (ROWS["ns_bdplur"], [abi.HALO_VELGRAD_A, abi.HALO_VELGRAD_B]),
    "rans_lusgs": (ROWS["rans_lusgs"], [abi.HALO_TURB]),
    # (the library refuses AGX_HALO_VELGRAD_* for the scalar solvers)
    "euler_dplur": (ROWS["euler_dplur"], []),
}


@pytest.mark.parametrize("name", sorted(SWAP_CASES))
def test_every_level_makes_the_swaps_of_calc_residual(oracle, name):
    """A three-level W cycle on two blocks through a recording proxy of the Api: on EVERY
    context, between each phase_residual and the diagonal's inversion that follows it
    (phase_implicit_begin on the finest level, mg_invert_diagonal on a coarse one), the driver
    exchanges the velocity gradients (A then B) exactly when the solver is block-matrix and
    viscous, and eddy viscosity, f1, f2 exactly when there are seven equations
    (gridLevel.cpp:386-392, reached from Restriction :559-563 on the coarse levels) -- and
    nothing else."""
    kw, expected = SWAP_CASES[name]
    cases, trs = synthetic.multigrid_levels(levels=3, cycle="W", nblocks=2, **BOX,
                                            time_integration="implicitEuler", **kw)
    cfg = Solver(oracle, cases[0])
    block = cfg.cfg.matrix_solver in (abi.SOLVER["blusgs"], abi.SOLVER["bdplur"])
    want = ([abi.HALO_VELGRAD_A, abi.HALO_VELGRAD_B] if block and cfg.cfg.is_viscous else []) + \
        ([abi.HALO_TURB] if cfg.cfg.n_eq == 7 else [])
    cfg.close()
    assert want == expected          # (the table above states what the conditions give)
    rec = RecordingApi(oracle)
    m = MultigridSolver(rec, cases, trs)
    start = len(rec.log)
    m.step(0)
    log = rec.log[start:]
    ctxs = [lev.ctx.value for lev in m.levels]
    m.close()
    closers = ("phase_implicit_begin", "mg_invert_diagonal")
    # a W cycle on three levels: the finest level's residual once, the middle level's once,
    # the coarsest level's twice
    for ctx, visits in zip(ctxs, (1, 1, 2)):
        mine = [(n, s) for n, c, s in log if c == ctx]
        opens = [q for q, (n, _) in enumerate(mine) if n == "phase_residual"]
        assert len(opens) == visits, (ctx, len(opens))
        for q in opens:
            rest = mine[q + 1:]
            end = next(p for p, (n, _) in enumerate(rest) if n in closers)
            assert rest[end][0] == (closers[0] if ctx == ctxs[0] else closers[1])
            between = rest[:end]
            assert [n for n, _ in between] == ["halo_exchange"] * len(between), between
            assert [s for _, s in between] == expected, (ctxs.index(ctx), between)
