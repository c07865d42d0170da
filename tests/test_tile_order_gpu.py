"""The order in which the tile kernels' workgroups visit their (column, k) steps.

AGX_TILE_ORDER=column is the (column, k) sequence cut into equal ranges, =step the
(k-chunk, column, k) sequence of aither_amd/csrc/agx_tile_plan.hpp.  Every cell is computed
by the same instructions whichever workgroup owns it, so the two orders must give the same
bits; the step order is held against the oracle as well.  The shapes are the smallest on
which the step order differs from the column order: (131, 15, 9) is 3 x 3 ragged tiles of
both pitches (64 and 62 cells) and takes two chunks of 6 and 3 planes on 8 workgroups,
(65, 7, 20) is 2 x 2 tiles of centralFourth's 60-cell pitch in two chunks of 10
(tests/cpp/tile_plan.cpp holds the plans of exactly these shapes to that).
"""
import gc

import numpy as np
import pytest

from parity_utils import run_pair   # (asserts every field to its RTOL, 1e-10)
from parity_utils import switches
from aither_amd.case import synthetic
from aither_amd.solver import Solver

pytestmark = pytest.mark.gpu

WALL_J = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
          4: ("characteristic", 1)}
VISCOUS = dict(stretch=1.1, bcs=WALL_J, equation_set="navierStokes", face_reconstruction="weno",
               limiter="none", inviscid_flux="ausm", time_integration="implicitEuler",
               matrix_solver="lusgs", cfl=10.0)
RK4 = dict(stretch=1.1, face_reconstruction="thirdOrder", limiter="vanAlbada",
           inviscid_flux="roe", time_integration="rk4", cfl=0.5)


def _run(api, case, steps, order, workgroups):
    with switches(AGX_TILE_ORDER=order, AGX_WORKGROUPS=str(workgroups)):
        s = Solver(api, case)
    try:
        for nn in range(steps):
            s.step(nn)
        out = {f: s.download(f, 0) for f in ("residual", "dt", "state")}
        out["l2"] = np.array([h["l2"] for h in s.history])
        out["linf"] = [h["linf"] for h in s.history]
    finally:
        s.close()
    return out


def _both_orders(api, case, steps, workgroups):
    return [_run(api, case, steps, order, workgroups) for order in ("column", "step")]


def _assert_same_bits(col, stp):
    for f in ("residual", "dt", "state", "l2"):
        assert np.array_equal(col[f], stp[f]), f
    assert col["linf"] == stp["linf"]


@pytest.mark.parametrize("workgroups", [8, 24])
def test_viscous_lusgs_orders_agree_bitwise(agx, workgroups):
    """k_residual_tile (WENO + AUSM) and k_visc_tile<false> under scalar LU-SGS, viscous wall
    on j-min, two steps: residual, dt, state and the norms of the two orders are the same
    bits.  On 8 workgroups the viscous kernel's nine tiles run in two chunks and its ranges
    cross columns; 24 is cut down to 10, where the plan keeps the column order."""
    case = synthetic.single_block_case((131, 15, 9), **VISCOUS)
    _assert_same_bits(*_both_orders(agx, case, 2, workgroups))


@pytest.mark.parametrize("n,workgroups", [((131, 15, 9), 8), ((131, 15, 9), 24),
                                          ((65, 7, 20), 8)])
def test_viscous_central_fourth_orders_agree_bitwise(agx, n, workgroups):
    """The same with viscous_face_reconstruction = centralFourth: k_visc_tile<true>, whose
    priming loads five planes.  With that charge (131, 15, 9) keeps the column order for the
    viscous kernel (the dearest range would cost more than one charge over it); (65, 7, 20)
    takes two chunks of 10 on 8 workgroups."""
    case = synthetic.single_block_case(n, viscous_face_reconstruction="centralFourth", **VISCOUS)
    _assert_same_bits(*_both_orders(agx, case, 2, workgroups))


def test_rk4_fused_orders_agree(agx):
    """The fused stage kernel (k_residual_tile<MUSCL, vanAlbada, Roe, FUSE>), 8 workgroups,
    two steps.  The state is the same bits and the L-inf record the same value at the same
    place; the L2 norms are sums of the workgroups' partial sums, which the step order forms
    over other cells: 1e-13 relative covers the rounding of 5 x 17 685 squares summed in
    another order (about sqrt(n) eps = 3e-14 for a random walk), nothing else may differ."""
    case = synthetic.single_block_case((131, 15, 9), **RK4)
    col, stp = _both_orders(agx, case, 2, 8)
    assert np.array_equal(col["state"], stp["state"])
    assert col["linf"] == stp["linf"]
    err = np.abs(col["l2"] - stp["l2"]) / np.abs(col["l2"])
    print("L2 relative difference between the orders:", err.max())
    assert err.max() <= 1e-13


@pytest.mark.parametrize("n,workgroups", [((65, 5, 3), None), ((131, 15, 9), 8)])
def test_step_order_against_oracle(agx, oracle, n, workgroups):
    """The step order pinned on the oracle, not only on the column order: a viscous LU-SGS
    pair, two steps.  (65, 5, 3) is too small for more than one workgroup; (131, 15, 9) runs
    on 8 workgroups, where its viscous tiles take two chunks."""
    case = synthetic.single_block_case(n, **VISCOUS)
    env = dict(AGX_TILE_ORDER="step")
    if workgroups:
        env["AGX_WORKGROUPS"] = str(workgroups)
    failure = None
    with switches(**env):
        try:
            for s in run_pair(agx, oracle, case, 2):
                s.close()
        except AssertionError as exc:
            failure = repr(exc.args[0] if len(exc.args) == 1 else exc.args)
    if failure is not None:
        gc.collect()
        pytest.fail("HIP (step order) against oracle: " + failure, pytrace=False)
