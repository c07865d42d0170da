"""The oracle's multigrid transfers (ora_mg_restrict, ora_mg_save_update, ora_mg_prolong) and
its forcing term against the numpy restatement of tests/mg_ref.py, on the CPU.  The same
checks hold the HIP libraries in tests/test_mg_transfers_gpu.py; until now both were held to
each other through whole cycles only, where a convention they share cancels: the forcing term
is summed, not volume weighted; ConvertCellToNode runs without ghost cells, factor 1 at the
corners, 1/2 on the edges, 1/8 elsewhere; a coarse cell may hold a single fine cell."""
import numpy as np
import pytest

import mg_ref
import mg_transfer_cases as T

# one path per equation count is enough here: the oracle keeps x in one place
HOST_PATHS = ("dplur5", "blusgs7")


def test_reference_conventions():
    """mg_ref itself on a 3 x 2 x 1 block by hand: the node factors, the summed and the
    weighted restriction, the interpolation at the corners of a coarse cell."""
    x = np.arange(1.0, 7.0).reshape(1, 2, 3, 1)
    nodes, mag = mg_ref.cell_to_node(x)
    assert nodes.shape == (2, 3, 4, 1) and np.array_equal(nodes, mag)
    assert nodes[0, 0, 0, 0] == 1.0 and nodes[1, 2, 3, 0] == 6.0     # corners: the cell itself
    assert nodes[0, 0, 1, 0] == 0.5 * (1.0 + 2.0)                    # an edge: half the sum
    assert nodes[0, 1, 0, 0] == 0.5 * (1.0 + 4.0)
    assert nodes[0, 1, 1, 0] == 0.125 * (1.0 + 2.0 + 4.0 + 5.0)      # in a face: 1/8 of four
    tc = np.zeros((1, 2, 3, 3), dtype=np.int32)
    tc[..., 0] = [0, 0, 1]
    s, _ = mg_ref.restrict(x, tc, (1, 1, 2))
    assert s[0, 0, :, 0].tolist() == [1.0 + 2.0 + 4.0 + 5.0, 3.0 + 6.0]
    w, _ = mg_ref.restrict(x, tc, (1, 1, 2), np.full((1, 2, 3), 0.25))
    assert w[0, 0, :, 0].tolist() == [3.0, 2.25]
    cf = np.zeros((1, 1, 1, 7))
    one = np.zeros((1, 1, 1, 3), dtype=np.int32)
    n8 = np.arange(8.0).reshape(2, 2, 2, 1)
    assert mg_ref.trilinear(n8, one, cf)[0][0, 0, 0, 0] == 0.0
    cf[..., :4] = 1.0                                                # the upper k face ...
    assert mg_ref.trilinear(n8, one, cf)[0][0, 0, 0, 0] == 4.0
    cf[..., 4:6] = 1.0                                               # ... its upper i edge ...
    assert mg_ref.trilinear(n8, one, cf)[0][0, 0, 0, 0] == 5.0
    cf[..., 6] = 1.0                                                 # ... its upper j corner
    assert mg_ref.trilinear(n8, one, cf)[0][0, 0, 0, 0] == 7.0


@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("path", HOST_PATHS)
def test_restriction_is_the_scatter_add(oracle, path, shape):
    """State and x: ghost cells zero, physical cells within 8 * 2**-52 * sum |w v| of numpy
    -- the oracle adds w * v in the same k, j, i order and is built without contraction
    (oracle/Makefile), so it is equal bit for bit."""
    assert T.check_restriction(oracle, path, shape) == 0.0


@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("path", HOST_PATHS)
def test_prolongation_is_nodes_then_trilinear(oracle, path, shape):
    """Coarse x left as x1 - x0 exactly; fine x within 32 * 2**-52 * (|xf| +
    interp(nodes(|corr|))) of numpy (measured on the oracle: 0.9 to 1.6 of 2**-52 times that
    magnitude, numpy adds the eight cells of a node in another order)."""
    assert T.check_prolongation(oracle, path, shape) <= 1.0


IDENTITY = [(p, s) for p in ("dplur5", "lusgs5", "blusgs5", "blusgs7", "lusgs7") for s in T.SHAPES] + \
    [("bdplur7", "wide"), ("blusgs5", "wide")]


@pytest.mark.parametrize("path,shape", IDENTITY)
def test_coarse_residual_is_the_summed_fine_residual(oracle, path, shape):
    """forcing - (A x - b) with forcing = R(r_fine) + (A x - b) is R(r_fine), summed, for a
    random coarse x of amplitude 1: the mean square of the coarse matrix residual times its
    size (ghost cells counted, as the reference divides) equals sum (R(-residual))**2 to
    rtol 1e-8 (the oracle: 1e-13 at worst on these cases); the fine mean square at x = 0 equals sum residual**2."""
    T.check_forcing_identity(oracle, path, shape)


def test_identity_holds_at_small_amplitude(oracle):
    """... and for a coarse x of amplitude 1e-3."""
    T.check_forcing_identity(oracle, "blusgs5", "wide", amplitude=1.0e-3)
