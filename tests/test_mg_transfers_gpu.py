"""The HIP libraries' multigrid transfers (k_mg_restrict, k_mg_nodes, k_mg_prolong), their
forcing term (k_mg_axmb against the matrix-residual kernels) and the one-level cycle, held to
what does not share their conventions: the numpy restatement of tests/mg_ref.py and the plain
iteration agx_iterate.  The checks are those of tests/test_mg_transfers_host.py (shared in
tests/mg_transfer_cases.py), on every place the libraries keep x in."""
import numpy as np
import pytest

import mg_transfer_cases as T
from parity_utils import rel_err
from aither_amd.case import synthetic
from aither_amd.solver import MultigridSolver, Solver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def agx_rans():
    import aither_amd
    return aither_amd.load(7)


def _lib(agx, agx_rans, path):
    return agx_rans if T.N_EQ(path) == 7 else agx


@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("path", T.TRANSFER_PATHS)
def test_restriction_is_the_scatter_add(agx, agx_rans, path, shape):
    """State and x: every coarse ghost cell exactly 0 (the coarse arrays held other values),
    every physical coarse cell within 8 * 2**-52 * sum |w v| of numpy: at most 8 products and
    7 additions, which the kernel may contract."""
    assert T.check_restriction(_lib(agx, agx_rans, path), path, shape) <= 1.0


@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("path", T.TRANSFER_PATHS)
def test_prolongation_is_nodes_then_trilinear(agx, agx_rans, path, shape):
    """Coarse x left as x1 - x0 exactly, ghost cells included; fine x within 32 * 2**-52 *
    (|xf| + interp(nodes(|corr|))) of numpy."""
    assert T.check_prolongation(_lib(agx, agx_rans, path), path, shape) <= 1.0


IDENTITY = [(p, s) for p in T.TRANSFER_PATHS for s in T.SHAPES] + \
    [("bdplur7", "wide"), ("blusgs5", "wide")]


@pytest.mark.parametrize("path,shape", IDENTITY)
def test_coarse_residual_is_the_summed_fine_residual(agx, agx_rans, path, shape):
    """The coarse matrix residual after a restriction is the summed fine one whatever x the
    coarse level holds (rtol 1e-8 on the sums of squares): k_mg_axmb and the path's
    matrix-residual kernel form the same A x - b, the forcing is summed and carried by the
    path's right-hand side; the fine mean square at x = 0 is that of the residual."""
    T.check_forcing_identity(_lib(agx, agx_rans, path), path, shape)


# ---- one level is the plain iteration --------------------------------------------------------
WALL = T.WALL
RANS_WALL = T.RANS_WALL
# Chosen on the oracle, against the driver as it was before every level made the swaps of
# gridLevel::CalcResidual (gridLevel.cpp:386-392): at the synthetic decks' Reynolds number
# that driver is 2e-10 .. 2e-9 from the plain iteration (the size of the bound below); with
# the reference length shortened -- viscous terms 1e4 .. 1e5 times larger beside the inviscid
# ones -- it is, after three iterations at CFL 200 (rel_err of the state, measured):
ONE_LEVEL = {
    "ns_blusgs": (dict(matrix_solver="blusgs", equation_set="navierStokes", bcs=WALL,
                       l_ref=1.0e-5), 8.7e-5),
    "ns_bdplur": (dict(matrix_solver="bdplur", equation_set="navierStokes", bcs=WALL,
                       l_ref=1.0e-5), 3.5e-5),
    "rans_lusgs": (dict(matrix_solver="lusgs", equation_set="rans", turbulence_model="sst2003",
                        bcs=RANS_WALL, l_ref=1.0e-4), 1.3e-4),
    "rans_dplur": (dict(matrix_solver="dplur", equation_set="rans", turbulence_model="sst2003",
                        bcs=RANS_WALL, l_ref=1.0e-4), 4.9e-6),
    "rans_blusgs": (dict(matrix_solver="blusgs", equation_set="rans", turbulence_model="sst2003",
                         bcs=RANS_WALL, l_ref=1.0e-4), 7.7e-5),
}
ONE_LEVEL_BOX = dict(n=(12, 10, 8), nblocks=2, axis="i", stretch=1.15, amplitude=0.05, levels=1,
                     time_integration="implicitEuler", matrix_sweeps=2, cfl=200.0)


def one_level_pair(api, name):
    """(MultigridSolver over one level, Solver) of a row of ONE_LEVEL after three iterations."""
    cases, trs = synthetic.multigrid_levels(**ONE_LEVEL_BOX, **ONE_LEVEL[name][0])
    m, s = MultigridSolver(api, cases, trs), Solver(api, cases[0])
    for nn in range(3):
        m.step(nn), s.step(nn)
    return m, s


@pytest.mark.parametrize("name", sorted(ONE_LEVEL))
def test_one_level_cycle_is_agx_iterate(agx, agx_rans, name):
    """MultigridSolver over ONE level (the phases, the cycle's relaxation, the plane-form
    matrix residual) against Solver (agx_iterate) in the same library, two blocks joined along
    i, three iterations: rel_err < 1e-9 on the state, rtol 1e-9 on the norms -- the multigrid
    parity tests' own bounds -- and, as measured on the MI355X for all five rows, the physical
    cells of the state equal bit for bit (the phases are the kernels agx_iterate launches).  A
    driver without the gradient and turbulence swaps is 4.9e-6 .. 1.3e-4 away on these decks
    (ONE_LEVEL, measured on the oracle: 4900 .. 130000 times the bound)."""
    m, s = one_level_pair(agx_rans if name.startswith("rans") else agx, name)
    try:
        g = m.case.ng
        for hm, hs in zip(m.history, s.history):
            assert np.allclose(hm["l2"], hs["l2"], rtol=1e-9, atol=0.0), (hm["l2"], hs["l2"])
        for gb in range(2):
            a = m.download("state", gb)[g:-g, g:-g, g:-g]
            b = s.download("state", gb)[g:-g, g:-g, g:-g]
            e = rel_err(a, b)
            print(f"one level {name} block {gb}: rel_err {e:.3e}, bitwise {np.array_equal(a, b)}")
            assert np.all(np.isfinite(a))
            assert e < 1e-9, (gb, e)
            assert np.array_equal(a, b), (gb, e)
    finally:
        m.close(), s.close()
