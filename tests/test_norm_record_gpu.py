"""The L-inf record -- value AND location (block, i, j, k, eqn) -- of the device reductions,
on fields whose maximum is tied bit for bit.

agx_linf's location is formed by the reductions below, each with its own tie-break
(`ov == vmax && ol < vlin`), decoded on the host (update_pass) and merged over blocks and
ranks with a strict `>` (reduce_over_ranks: of equal maxima the lowest rank's).  The decks
are picked from update_pass's branches (tie_fields.PATHS):

  fused        the fused marching stage (one partial per workgroup) + k_norm_final:
               explicit and inviscid (can_fuse) -- rk4, MUSCL + Roe
  k_update     k_update + reduce_norms in the 5-equation build: an explicit stage that is
               not fused -- explicit Euler, navierStokes
  k_update_d2  the update on the diagonal-ordered arrays (agx_lusgs_kernels.hpp) through
               norm_block_fold + reduce_norms: implicit Euler, scalar LU-SGS, 5 equations
  rans         the rans library's implicit update.  The diagonal-ordered path is 5-equation
               only (AGX_FAST), so this is k_update again, in mode 2 and its 7-equation
               build, + reduce_norms

The fields are tie_fields.extruded_state: the same in every plane along one axis, so every
plane holds the maximum (tests/test_parity_measure_host.py checks, on the oracle alone, that
it is tied, off the zero indices of the free directions, and that the oracle names the first
tied cell in the reference's loop order).  A wrong index decode, a tie broken the other way
in a lane, wave, workgroup or block fold, or a rank merge that keeps the wrong record moves
the location.

Box: (70, 36, 6) cells per block for every axis.  Read from the launches: k_update (both
builds) runs 64 x 4 x 1 cells per workgroup (cell_grid, CELL_BLOCK) -- 2 x 9 x 6 workgroups;
k_update_d2 32 x 32 tiles per k-plane -- 3 x 2 x 6; the marching stage 64 lanes x
g_march_tj rows, folded into one partial per persistent workgroup (march_plan) -- several of
them; k_norm_final folds the partials with 256 threads.  So the tied cells of a line along i
lie in different lanes, waves and workgroups, those along j in different rows, tiles and
workgroups, those along k in different workgroups.
"""
import pytest

from parity_utils import RTOL, first_maximum, flux_scale, step_with_residuals, tied_set
from tie_fields import PATHS, assert_tied_record, tie_case
from aither_amd.solver import Solver

pytestmark = pytest.mark.gpu

# paths whose own residual is not tied along an axis (their planes are not computed alike):
# only the own-field rule applies there.  {(path, axis): reason}
TIE_BROKEN = {}


@pytest.fixture(scope="module")
def agx_rans():
    import aither_amd
    return aither_amd.load(7)


@pytest.mark.parametrize("nblocks", [1, 2])
@pytest.mark.parametrize("axis", ["i", "j", "k"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_tied_maximum_names_the_first_cell(agx, agx_rans, oracle, path, axis, nblocks):
    """One time step (rk4: four stages, each an entry).  Two blocks are stacked along the
    extrusion axis: equal maxima in both, the record names block 0."""
    case = tie_case(path, axis, nblocks)
    sg, so = Solver(agx_rans if path == "rans" else agx, case), Solver(oracle, case)
    try:
        sg.step(0)
        step_with_residuals(so, 0)
        rfloor = 1.0e-3 * flux_scale(case)
        assert_tied_record(case, axis, so.history[0]["residual"], so.history[0]["linf"], nblocks)
        own = [sg.download("residual", gb) for gb in sg.block_ids]
        # the library against itself by the reference's rule: the value is the maximum of its
        # own residual bit for bit, the location the first strictly greater entry in loop order
        # (every path keeps the residual of its last iteration; the fused marching stage
        # stores the one it advances with)
        assert first_maximum(own) == tuple(sg.history[-1]["linf"])
        # ... and its maximum is tied bit for bit in the cells the oracle's is
        tied = set(tied_set(own)[0]) == set(tied_set(so.history[-1]["residual"])[0])
        if (path, axis) in TIE_BROKEN:
            return
        assert tied, "the maximum of the library's own residual is not tied as the oracle's is"
        for hg, ho in zip(sg.history, so.history):
            lg, lo = hg["linf"], ho["linf"]
            assert abs(lg[0] - lo[0]) <= RTOL * max(abs(lo[0]), rfloor), (lg, lo)
            assert tuple(lg[1:]) == tuple(lo[1:]), (hg["mm"], lg, lo)
        assert sg.history[0]["linf"][1] == 0
    finally:
        sg.close(), so.close()


def test_two_ranks_return_the_global_record_and_the_tie_goes_to_rank_0(oracle):
    """The two stacked blocks on two ranks (two processes on one GPU, agx_iterate with an
    exchange): every rank returns the merged record, it equals the single-process oracle's in
    value and location, and of the equal maxima of the two blocks rank 0's is kept (MaxLinf,
    resid.cpp:55-79) -- also on rank 1, whose own record is as large."""
    import test_distributed_gpu as dist_tests
    res = dist_tests.two_ranks_on_one_gpu("tie", True)
    case = tie_case("k_update_d2", "k", 2)
    so = Solver(oracle, case)
    step_with_residuals(so, 0)
    assert_tied_record(case, "k", so.history[0]["residual"], so.history[0]["linf"], 2)
    rfloor = 1.0e-3 * flux_scale(case)
    for rank in range(2):
        assert len(res[rank][2]) == len(so.history)
        for lg, ho in zip(res[rank][2], so.history):
            lo = ho["linf"]
            assert abs(lg[0] - lo[0]) <= RTOL * max(abs(lo[0]), rfloor), (rank, lg, lo)
            assert tuple(lg[1:]) == tuple(lo[1:]) and lg[1] == 0, (rank, lg, lo)
    assert res[0][2] == res[1][2]
    so.close()
