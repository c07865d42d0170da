"""Lifetime of what a context owns on the device (csrc/agx_mem.hpp): replacing a block's
boundary surfaces leaves a context that computes what a fresh one does, and contexts that
come and go give their memory back."""

import numpy as np
import pytest

from parity_utils import switches
from aither_amd.case import builder as _b
from aither_amd.case import synthetic
from aither_amd.solver import Solver


def _two_iterations(s):
    s.history.clear()
    for nn in range(2):
        s.step(nn)
    return [(h["l2"].copy(), h["linf"], h["matrix"]) for h in s.history], s.download("state", 0)


# the second way captures the per-block sweep graphs: ni + nj + nk - 2 = 22 >= 8 hyperplanes
@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, dict(AGX_LUSGS="plane", AGX_SWEEP_PIPE="0")],
                         ids=["kp", "plane_graphs"])
def test_set_bcs_again_equals_a_fresh_context(agx, env):
    """agx_block_set_bcs on a block that has run replaces the surface table, the wall table
    and drops the captured sweep graphs; from the same initial state the context then repeats
    its first two iterations bit for bit -- which are those of a context set up once."""
    wall = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
            4: ("characteristic", 1)}
    case = synthetic.single_block_case((10, 8, 6), stretch=1.1, bcs=wall,
                                       equation_set="navierStokes",
                                       time_integration="implicitEuler", matrix_solver="lusgs",
                                       cfl=5.0)
    with switches(**env):
        fresh, again = Solver(agx, case), Solver(agx, case)
    try:
        ref_hist, ref_state = _two_iterations(fresh)
        first_hist, first_state = _two_iterations(again)
        surfs = _b.surface_structs(case, 0)
        agx.check(agx.block_set_bcs(again.ctx, again.block_ids[0], len(surfs), surfs),
                  "block_set_bcs")
        again.upload("state", 0, case.blocks[0].state)
        hist, state = _two_iterations(again)
        assert np.all(np.isfinite(ref_state)) and len(ref_hist) == len(hist) > 0
        for got in ((first_hist, first_state), (hist, state)):
            for (l2, linf, mres), (l2r, linfr, mresr) in zip(got[0], ref_hist):
                assert np.array_equal(l2, l2r) and linf == linfr and mres == mresr
            assert np.array_equal(got[1], ref_state)
    finally:
        fresh.close(), again.close()


@pytest.mark.gpu
def test_context_cycles_return_device_memory(agx):
    """A coarse guard against an owner that never frees or a move that drops a buffer: ten
    cycles of three contexts (D2 LU-SGS, block LU-SGS with the pipelined sweep, node-built
    geometry with DPLUR) may not lower the device's free memory by more than a quarter of one
    cycle's footprint F -- ten leaked cycles would cost 10 F.  (The reading is device-wide.)"""
    import torch
    kw = dict(n=(32, 24, 20), nblocks=2, time_integration="implicitEuler", cfl=5.0)
    cases = [synthetic.stacked_blocks_case(matrix_solver="lusgs", **kw),
             synthetic.stacked_blocks_case(matrix_solver="blusgs", **kw),
             synthetic.stacked_blocks_case(matrix_solver="dplur", geometry="device", **kw)]

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        """the lowest reading while the three contexts live"""
        solvers, low = [], free()
        try:
            for case in cases:
                solvers.append(Solver(agx, case))
                solvers[-1].step(0)
                low = min(low, free())
        finally:
            for s in solvers:
                s.close()
        return low

    before = free()
    footprint = before - cycle()
    cycle()                      # (warm: the runtime's own pools have their size)
    noted = free()
    for _ in range(10):
        cycle()
    after = free()
    print(f"footprint {footprint} B; free before {before}, after two cycles {noted}, "
          f"after ten more {after} B")
    assert footprint > 0
    assert noted - after <= footprint // 4, (footprint, noted, after)
