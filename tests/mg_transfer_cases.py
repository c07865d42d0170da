"""The cases and the checks tests/test_mg_transfers_host.py (the oracle) and
tests/test_mg_transfers_gpu.py (the HIP libraries) share: the multigrid transfers and the
forcing term through the public calls only -- Solver.upload / download of `state`, `update`
and `residual`, mg_restrict, mg_save_update, mg_prolong, mg_matrix_residual -- against the
numpy restatement of tests/mg_ref.py.  Every check returns its worst figure in units of its
bound."""
import ctypes as C
import functools

import numpy as np

import mg_ref
from parity_utils import switches
from aither_amd import abi
from aither_amd.case import builder, multigrid, synthetic
from aither_amd.case.inputfile import Surface
from aither_amd.solver import MultigridSolver

WALL = {3: ("viscousWall", 2)}
RANS_WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
             4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
NS = dict(equation_set="navierStokes", bcs=WALL, cfl=20.0, matrix_sweeps=2)
RANS = dict(equation_set="rans", turbulence_model="sst2003", bcs=RANS_WALL, cfl=10.0,
            matrix_sweeps=2)
# where x lives in the HIP libraries: (deck, environment of the context's creation)
PATHS = {
    "dplur5": (dict(matrix_solver="dplur", matrix_sweeps=4, cfl=40.0), {}),   # planes
    "lusgs5": (dict(matrix_solver="lusgs", **NS), {}),           # diagonal-ordered D2 arrays
    "lusgs5_plane": (dict(matrix_solver="lusgs", **NS), {"AGX_LUSGS": "plane"}),
    "blusgs5": (dict(matrix_solver="blusgs", **NS), {}),         # sweep records
    "blusgs7": (dict(matrix_solver="blusgs", **RANS), {}),
    "lusgs7": (dict(matrix_solver="lusgs", **RANS), {}),
    # (the forcing identity only)
    "bdplur7": (dict(matrix_solver="bdplur", **RANS), {}),
}
TRANSFER_PATHS = ("dplur5", "lusgs5", "lusgs5_plane", "blusgs5", "blusgs7", "lusgs7")
# the smallest shapes that reach the edges
#   split: 11 x 5 x 3 cells, the lower-j side in two surfaces that meet at i = 5: kept nodes
#          i 0,2,4,5,7,9,11  j 0,2,4,5  k 0,2,3 -- a coarse cell of ONE fine cell in every
#          direction, in i in the middle of the block
#   long:  131 x 9 x 2 -> 66 x 5 x 1: the restriction's and the prolongation's grids span two
#          workgroups in i; one cell thick in k
#   two:   two blocks of 11 x 5 x 3 along i (the per-block map cache)
#   wide:  two blocks of 12 x 10 x 4 (the forcing identity's additional cases)
SHAPES = ("split", "long", "two")
N_EQ = lambda path: 7 if path.endswith("7") else 5
STRETCH = 1.15


def _split_surfaces(ni, nj, nk, bcs, splits):
    get = lambda s: bcs.get(s, ("slipWall", 0))
    s = [Surface(get(1)[0], 0, 0, 0, nj, 0, nk, get(1)[1]),
         Surface(get(2)[0], ni, ni, 0, nj, 0, nk, get(2)[1]),
         Surface(get(4)[0], 0, ni, nj, nj, 0, nk, get(4)[1]),
         Surface(get(5)[0], 0, ni, 0, nj, 0, 0, get(5)[1]),
         Surface(get(6)[0], 0, ni, 0, nj, nk, nk, get(6)[1])]
    edges = [0] + list(splits) + [ni]
    for a, b in zip(edges[:-1], edges[1:]):       # the lower j side in patches
        s.append(Surface(get(3)[0], a, b, 0, 0, 0, nk, get(3)[1]))
    s.sort(key=Surface.sort_key)
    return s


@functools.lru_cache(maxsize=None)
def levels(path, shape):
    """(cases, transfers) of two grid levels; shared between the tests and never changed."""
    kw = dict(PATHS[path][0])
    kw["time_integration"] = "implicitEuler"
    if shape == "split":
        bcs = kw.pop("bcs", {})
        deck = synthetic.make_deck(**kw)
        deck.bcs = [_split_surfaces(11, 5, 3, bcs, (5,))]
        deck.multigrid_cycle = "V"
        coords = [synthetic.box_nodes(11, 5, 3, STRETCH)]
        cases, trs = multigrid.build_levels(deck, coords, 2, builder.build_case)
        synthetic.perturbed_state(cases[0], 0.05)
        assert trs[0][0].kept == ([0, 2, 4, 5, 7, 9, 11], [0, 2, 4, 5], [0, 2, 3])
        return cases, trs
    n, nblocks = {"long": ((131, 9, 2), 1), "two": ((11, 5, 3), 2), "wide": ((12, 10, 4), 2)}[shape]
    cases, trs = synthetic.multigrid_levels(n=n, nblocks=nblocks, axis="i", levels=2,
                                            stretch=STRETCH, **kw)
    if shape == "long":
        assert cases[1].blocks[0].geom.n == (66, 5, 1)
    return cases, trs


def open_levels(api, path, shape):
    """A MultigridSolver over the two levels (the AGX_* switches are read when a context is
    created; the environment is restored afterwards)."""
    cases, trs = levels(path, shape)
    with switches(PATHS[path][1]):
        return MultigridSolver(api, cases, trs)


def _core(a, ng):
    return a[ng:-ng, ng:-ng, ng:-ng]


def _ghosts_are_zero(a, ng):
    b = a.copy()
    _core(b, ng)[...] = 0.0
    return not b.any()


def _cells(case, gb):
    ni, nj, nk = case.blocks[gb].geom.n
    return (nk, nj, ni)


def _restrict_call(m, gb, what):
    f, c = m.levels
    t = m.transfers[0][gb]
    vf = None if what == 2 else t["vf"].ctypes.data_as(abi.c_dp)
    m.api.check(m.api.mg_restrict(f.ctx, c.ctx, f.block_ids[gb], what,
                                  t["tc"].ctypes.data_as(C.POINTER(C.c_int32)), vf), "mg_restrict")


def check_restriction(api, path, shape, seed=11):
    """AGX_MG_STATE and AGX_MG_UPDATE: the coarse arrays are filled with non-zero values first,
    ghost cells included; afterwards every coarse ghost cell is exactly 0 and every physical
    coarse cell within RESTRICT_UNITS * 2**-52 * sum |w v| of numpy.  Returns the worst error
    in units of that bound."""
    rng = np.random.default_rng(seed)
    m = open_levels(api, path, shape)
    f, c = m.levels
    ng, worst = f.case.ng, 0.0
    try:
        fine = {}
        for gb in f.block_ids:
            for field in ("state", "update"):
                fine[field, gb] = rng.standard_normal(f._shape(field, gb))
                f.upload(field, gb, fine[field, gb])
                c.upload(field, gb, 3.0 + rng.standard_normal(c._shape(field, gb)))
        for gb in f.block_ids:
            _restrict_call(m, gb, 0)
            _restrict_call(m, gb, 1)
        for gb in f.block_ids:
            t = m.transfers[0][gb]
            for field in ("state", "update"):
                got = c.download(field, gb)
                assert _ghosts_are_zero(got, ng), (field, gb, "coarse ghost cells are not zero")
                ref, mag = mg_ref.restrict(_core(fine[field, gb], ng), t["tc"], _cells(c.case, gb),
                                           t["vf"])
                err = np.abs(_core(got, ng) - ref)
                bound = mg_ref.RESTRICT_UNITS * mg_ref.EPS * mag
                assert mag.min() > 0.0
                units = float((err / bound).max())
                print(f"restriction {path} {shape} block {gb} {field}: {units:.3f} of the bound")
                assert np.all(err <= bound), (field, gb, units)
                worst = max(worst, units)
    finally:
        m.close()
    return worst


def check_prolongation(api, path, shape, seed=12):
    """x0 on the coarse level, mg_save_update; x1 on the coarse level, xf on the fine one,
    mg_prolong of every block: the coarse x is left as x1 - x0 exactly, ghost cells included;
    the fine x is xf + interp(nodes(x1 - x0)) of numpy within PROLONG_UNITS * 2**-52 *
    (|xf| + interp(nodes(|x1 - x0|))), its ghost cells untouched.  Returns the worst error in
    units of that bound."""
    rng = np.random.default_rng(seed)
    m = open_levels(api, path, shape)
    f, c = m.levels
    ng, worst = f.case.ng, 0.0
    try:
        x0 = {gb: rng.standard_normal(c._shape("update", gb)) for gb in c.block_ids}
        x1 = {gb: rng.standard_normal(c._shape("update", gb)) for gb in c.block_ids}
        xf = {gb: rng.standard_normal(f._shape("update", gb)) for gb in f.block_ids}
        for gb in c.block_ids:
            c.upload("update", gb, x0[gb])
        api.check(api.mg_save_update(c.ctx), "mg_save_update")
        for gb in c.block_ids:
            c.upload("update", gb, x1[gb])
            f.upload("update", gb, xf[gb])
        for gb in f.block_ids:
            t = m.transfers[0][gb]
            api.check(api.mg_prolong(c.ctx, f.ctx, f.block_ids[gb],
                                     t["tc"].ctypes.data_as(C.POINTER(C.c_int32)),
                                     t["cf"].ctypes.data_as(abi.c_dp)), "mg_prolong")
        for gb in f.block_ids:
            t = m.transfers[0][gb]
            corr = x1[gb] - x0[gb]
            assert np.array_equal(c.download("update", gb), corr), (gb, "coarse x != x1 - x0")
            got = f.download("update", gb)
            ref, mag = mg_ref.prolong(_core(xf[gb], ng), _core(corr, ng), t["tc"], t["cf"])
            outside = got.copy()
            _core(outside, ng)[...] = _core(xf[gb], ng)
            assert np.array_equal(outside, xf[gb]), (gb, "fine ghost cells changed")
            err = np.abs(_core(got, ng) - ref)
            bound = mg_ref.PROLONG_UNITS * mg_ref.EPS * mag
            units = float((err / bound).max())
            print(f"prolongation {path} {shape} block {gb}: {units:.3f} of the bound")
            assert np.all(err <= bound), (gb, units)
            worst = max(worst, units)
    finally:
        m.close()
    return worst


IDENTITY_RTOL = 1.0e-8     # what the suite allows on the matrix residual


def check_forcing_identity(api, path, shape, seed=13, amplitude=1.0):
    """After a restriction the coarse matrix residual is forcing - (A x - b) with forcing =
    R(r_fine) + (A x - b): the SUMMED fine matrix residual whatever x the coarse level holds
    -- if the kernel that forms the forcing term and the one that forms the matrix residual
    agree on A x - b, and the forcing is summed and carried by the path's right-hand side.
    implicitEuler, mm = 0, fine x = 0: r_fine = b = -residual.  Returns the relative errors
    (coarse identity, fine mean square)."""
    rng = np.random.default_rng(seed)
    m = open_levels(api, path, shape)
    f, c = m.levels
    cfl = f.case.deck.cfl(0)
    n_eq = f.cfg.n_eq
    try:
        for s in m.levels:
            s.store_time_n(0)
        m._boundary_and_residual(f, 0, cfl)
        api.check(api.phase_implicit_begin(f.ctx), "phase_implicit_begin")
        for gb in f.block_ids:
            f.upload("update", gb, np.zeros(f._shape("update", gb)))
        ms = C.c_double(0.0)
        api.check(api.mg_matrix_residual(f.ctx, C.byref(ms)), "mg_matrix_residual")
        fine_ms = ms.value
        resid = [f.download("residual", gb) for gb in f.block_ids]
        m.restriction(0, 0, cfl)
        for gb in c.block_ids:
            c.upload("update", gb, amplitude * rng.standard_normal(c._shape("update", gb)))
        api.check(api.halo_exchange(c.ctx, abi.HALO_UPDATE), "halo_exchange")
        for gb in f.block_ids:
            _restrict_call(m, gb, 2)
        api.check(api.mg_matrix_residual(c.ctx, C.byref(ms)), "mg_matrix_residual")
        coarse_ms = ms.value
    finally:
        m.close()
    size = lambda s: n_eq * sum(int(np.prod(s._shape("update", gb)[:3])) for gb in s.block_ids)
    want_fine = float(sum((r ** 2).sum() for r in resid))
    want = mg_ref.forcing_identity(resid, [t["tc"] for t in m.transfers[0]],
                                   [_cells(c.case, gb) for gb in c.block_ids])
    assert want > 0.0 and want_fine > 0.0
    e_fine = abs(fine_ms * size(f) - want_fine) / want_fine
    e_coarse = abs(coarse_ms * size(c) - want) / want
    print(f"forcing identity {path} {shape}: coarse {e_coarse:.2e}, fine {e_fine:.2e}")
    assert e_fine <= IDENTITY_RTOL, ("fine mean square at x = 0", e_fine)
    assert e_coarse <= IDENTITY_RTOL, ("coarse residual != summed fine residual", e_coarse)
    return e_coarse, e_fine
