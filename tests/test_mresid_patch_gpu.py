"""The matrix residual marching along k with a patch of diagonals per workgroup (the default
form, k_matrix_resid_d2m: in-plane neighbours through LDS, the patch's rim from the arrays)
against the form with one plane position per thread (AGX_MRESID=plane): the same sum in the
same order per cell, so the two agree to 1e-12 relative, and two contexts of the default form
give the same bits.  The shapes put ghost neighbours on the rim and inside a patch in every
direction, diagonals on both sides of a run's length, and k on both sides of a chunk (32)."""
import numpy as np
import pytest

from parity_utils import run_pair, switches
from aither_amd.case import synthetic
from aither_amd.solver import Solver

pytestmark = pytest.mark.gpu

WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1),
        2: ("characteristic", 1), 4: ("characteristic", 1)}
VISCOUS = dict(stretch=1.1, bcs=WALL, equation_set="navierStokes",
               time_integration="implicitEuler", matrix_solver="lusgs", matrix_sweeps=2, cfl=5.0)
EULER = dict(stretch=1.1, time_integration="implicitEuler", matrix_solver="lusgs",
             matrix_sweeps=2, cfl=5.0)


def _case(kind, n, kw, axis=None):
    if kind == "single":
        return synthetic.single_block_case(n=n, **kw)
    if kind == "stacked":
        return synthetic.stacked_blocks_case(n=n, nblocks=2, axis=axis, **kw)
    return synthetic.cube_blocks_case(n=n, splits=(2, 2, 2), **kw)


CASES = {
    "thin_j": ("single", (70, 3, 5), VISCOUS, None),
    "thin_i": ("single", (3, 70, 5), VISCOUS, None),
    "long_diagonal": ("single", (68, 66, 3), VISCOUS, None),
    "one_plane_past_a_chunk": ("single", (9, 7, 33), VISCOUS, None),
    "one_plane_past_two_chunks": ("single", (9, 7, 65), VISCOUS, None),
    "single_plane": ("single", (12, 10, 1), VISCOUS, None),
    "euler": ("single", (17, 12, 6), EULER, None),
    "stacked_i": ("stacked", (13, 9, 7), VISCOUS, "i"),
    "stacked_j": ("stacked", (13, 9, 7), VISCOUS, "j"),
    "stacked_k": ("stacked", (13, 9, 7), VISCOUS, "k"),
    "cube": ("cube", (6, 5, 4), VISCOUS, None),
}


def _matrix(agx, case, form):
    with switches(AGX_MRESID=form):
        s = Solver(agx, case)
    s.step(0), s.step(1)
    out = [h["matrix"] for h in s.history]
    s.close()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_patch_form_is_the_plane_form(agx, name):
    kind, n, kw, axis = CASES[name]
    case = _case(kind, n, kw, axis)
    march, again, plane = (_matrix(agx, case, f) for f in ("march", "march", "plane"))
    print(name, "march", march, "plane", plane)
    assert len(march) >= 2 and all(m > 0.0 for m in march)
    assert march == again                      # the same bits from two contexts
    assert np.allclose(march, plane, rtol=1e-12, atol=0.0), (march, plane)


def test_patch_form_against_the_oracle(agx, oracle):
    """Ghost neighbours across a connection in j (lane - 1 and lane + 1 of the waves below and
    above), on the rim and inside a patch.  (Stacked along i the oracle's own residual ties
    its maximum in one entry of two, which run_pair does not take for an L-inf location.)"""
    case = _case("stacked", (13, 9, 7), VISCOUS, "j")
    for s in run_pair(agx, oracle, case, 2):
        s.close()
