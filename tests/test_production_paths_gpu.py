"""The sweep, tile and halo paths that block shape, sweep count, ghost depth and patch
orientation select -- each against the CPU oracle at parity_utils.RTOL.

The formulas are pinned by tests/test_parity_gpu.py on boxes of about 10 x 9 x 8.  What
differs between the library and the oracle is the machinery around them, and which piece of
it runs is a matter of shape: the second chunk of k_lusgs_kp's diagonals, its LDS limit, the
ticket that is taken a second time, the tag that comes round again after four writer
launches, the fused WENO tile kernel, tiles with ragged edges, blocks thinner than the ghost
depth, the eight patch orientations under every halo.  Every case here has the property
that selects its branch; tests/test_host_logic.py::test_production_path_cases_select_their_branch
(no GPU) restates the dispatch conditions on these tables and checks that, so that a later change of a shape cannot silently stop
covering a branch.

Run on a real MI355X:  python -m pytest tests -m gpu
"""
import gc
import os
import resource

import numpy as np
import pytest

from conftest import GOLDEN
from parity_utils import run_pair, rel_err, assert_components, switches, RTOL
from aither_amd import abi
from aither_amd.case import connections as conn_mod
from aither_amd.case import synthetic
from aither_amd.case.builder import build_case
from aither_amd.case.inputfile import parse_input
from aither_amd.solver import Solver

pytestmark = pytest.mark.gpu

FARFIELD = {s: ("characteristic", 1) for s in range(1, 7)}
WALL_J = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
          4: ("characteristic", 1)}
RANS_WALL = dict(FARFIELD)
RANS_WALL[3] = ("viscousWall", 2)

# ---- the dispatch conditions, restated from aither_amd/csrc/agx_api.hip ----------------
KP_CHUNK = 256            # lusgs_kp_variant: CH = 2 when min(ni, nj) > 256
KP_MAX_DIAG = 512         # refused above (block creation)
# k_lusgs_kp runs min(per_cu * num_cu, nk) workgroups of 256 threads.  A CU holds at most 32
# waves = 2048 threads = 8 such workgroups (maxThreadsPerMultiProcessor), the MI355X has 256
# CUs: whatever the occupancy query returns, more than 8 * 256 planes cannot all be resident.
MAX_RESIDENT_WGS = 8 * 256
TILE_I, TILE_J = 64, 6    # owned cells per workgroup of k_residual_tile<.., 6>
VTILE_I = 62              # ... of k_visc_tile (centralFourth: 60)


def kp_chunks(n):
    return 1 if min(n[0], n[1]) <= KP_CHUNK else 2


def tiles(n):
    return (n[0] + TILE_I - 1) // TILE_I, (n[1] + TILE_J - 1) // TILE_J


def ghost_layers(kw):
    return synthetic.make_deck(**kw).num_ghost_layers()


def on_d2_path(kw):
    """use_d2: implicit scalar LU-SGS with the Rusanov Jacobian."""
    return kw.get("time_integration") in ("implicitEuler", "bdf2", "crankNicholson") and \
        kw.get("matrix_solver", "lusgs") == "lusgs" and kw.get("inv_flux_jac", "rusanov") == "rusanov"


def can_fuse(kw):
    """can_fuse: explicit, inviscid, no non-reflecting surface."""
    return kw.get("time_integration", "rk4") in ("rk4", "explicitEuler") and \
        kw.get("equation_set", "euler") == "euler"


def _pair(lib, oracle, case, steps, **kw):
    """run_pair, and both contexts released whatever the outcome: a failed comparison leaves
    the two solvers in the frames of its traceback, and an oracle context that stays alive
    makes the oracle refuse the other equation count for the rest of the session."""
    failure = None
    try:
        for s in run_pair(lib, oracle, case, steps, **kw):
            s.close()
    except AssertionError as exc:
        failure = repr(exc.args[0] if len(exc.args) == 1 else exc.args)
    if failure is not None:
        gc.collect()
        pytest.fail("HIP against oracle: " + failure, pytrace=False)


def _make(spec):
    spec = dict(spec)
    kind = spec.pop("kind", "single")
    if kind == "single":
        return synthetic.single_block_case(**spec)
    if kind == "stacked":
        return synthetic.stacked_blocks_case(**spec)
    return synthetic.cube_blocks_case(**spec)


def _states(api, case, steps):
    s = Solver(api, case)
    for nn in range(steps):
        s.step(nn)
    out = [s.download("state", gb) for gb in s.block_ids]
    s.close()
    return out


@pytest.fixture(scope="module")
def agx_rans():
    import aither_amd
    return aither_amd.load(7)


# ======================= A. k_lusgs_kp ====================================================
KP = dict(stretch=1.1, bcs=WALL_J, equation_set="navierStokes",
          time_integration="implicitEuler", matrix_solver="lusgs", cfl=10.0)

KP_CH2 = {
    # cnt reaches 258: two live lanes in the second chunk
    "edge": dict(kind="single", n=(260, 258, 3), **KP),
    # a well-filled second chunk (44 lanes)
    "filled": dict(kind="single", n=(400, 300, 2), **KP),
    "stacked": dict(kind="stacked", n=(264, 259, 2), nblocks=2, axis="k", **KP),
}
KP_CH2_RUNS = [("edge", 1), ("edge", 2), ("filled", 1), ("filled", 2), ("stacked", 1),
               ("stacked", 3)]


@pytest.mark.parametrize("name,sweeps", KP_CH2_RUNS)
def test_kp_two_chunks(agx, oracle, name, sweeps):
    """k_lusgs_kp<FWD, FULL, CONN, CH = 2>: diagonals of more than 256 cells, the m = 1 half
    of every chunk loop.  One sweep is FULL = false, more are FULL = true; the stacked pair
    is CONN = true -- all four (FULL, CONN) forms of the two-chunk kernel.

    These cases found a bug: before its fix k_lusgs_kp<.., CONN = true, CH = 2> left the
    oracle by 3.4e-2 (one sweep) and 1.8e-1 (three sweeps) of the update after ONE iteration,
    stacked in k and in i alike, and differently from run to run -- the inline-asm stores of x
    lacked the wait states a store of more than 64 bits needs before its data registers are
    written again.  AGX_LUSGS=plane, CH = 1 with connections and CH = 2 without agreed with
    the oracle throughout, which is why nothing else noticed.
    See DESIGN.md section 5."""
    case = _make(dict(KP_CH2[name], matrix_sweeps=sweeps))
    _pair(agx, oracle, case, 2)


KP_LIMIT = dict(kind="single", n=(512, 512, 2), **KP)
KP_OVER = dict(kind="single", n=(513, 513, 2), **KP)


def test_kp_longest_diagonal_runs(agx, oracle):
    """min(ni, nj) = KP_MAX_DIAG = 512 exactly: the launch that asks for 2 * 19 * 8 * 514
    bytes (about 156 KiB) of dynamic LDS through hipFuncSetAttribute works, and both chunks
    are full."""
    _pair(agx, oracle, _make(KP_LIMIT), 2)


def test_kp_diagonal_limit_refused_by_name_and_served_by_the_plane_form(agx, oracle):
    """min(ni, nj) = 513: refused at set-up with the message that names the limit and the way
    out; AGX_LUSGS=plane (the launch-per-hyperplane form) runs the same block."""
    case = _make(KP_OVER)
    with pytest.raises(RuntimeError, match=r"min\(ni, nj\) = 513 exceeds the 512 cells per "
                                           r"diagonal.*AGX_LUSGS=plane"):
        Solver(agx, case)
    with switches(AGX_LUSGS="plane"):
        _pair(agx, oracle, case, 2)


KP_TICKETS = {
    "single": dict(kind="single", n=(6, 5, 2100), **dict(KP, stretch=1.05)),
    "stacked": dict(kind="stacked", n=(6, 5, 2100), nblocks=2, axis="k", **KP),
}


@pytest.mark.parametrize("name,sweeps", [("single", 1), ("single", 2), ("stacked", 2)])
def test_kp_ticket_recycling(agx, oracle, name, sweeps):
    """k_lusgs_kp with more k-planes than workgroups can be resident (nk = 2100 > 8 * 256,
    see MAX_RESIDENT_WGS): a workgroup takes a second ticket and waits on a plane swept by
    another workgroup of the same launch.  Stacked in k: plane 0 of the upper block reads
    connection ghosts instead of a predecessor."""
    case = _make(dict(KP_TICKETS[name], matrix_sweeps=sweeps))
    _pair(agx, oracle, case, 2)


KP_WRAP = {
    "single": dict(kind="single", n=(13, 11, 9), **KP),
    "stacked_i": dict(kind="stacked", n=(9, 8, 7), nblocks=2, axis="i", **KP),
    "stacked_j": dict(kind="stacked", n=(9, 8, 7), nblocks=2, axis="j", **KP),
    "stacked_k": dict(kind="stacked", n=(9, 8, 7), nblocks=2, axis="k", **KP),
    "cube": dict(kind="cube", n=(7, 6, 5), splits=(2, 2, 2),
                 **{k: v for k, v in KP.items() if k != "stretch"}),
}


@pytest.mark.parametrize("sweeps", [3, 4, 5])
@pytest.mark.parametrize("name", sorted(KP_WRAP))
def test_kp_tag_wrap(agx, oracle, name, sweeps):
    """The hand-off tag is epoch & 3: from the third sweep on a half sweep carries the tag of
    an earlier writer launch of the same iteration (prepare, half sweeps; with connections
    the exchange between them scatters into the D2 arrays).  Parity with the oracle, and --
    a stale tag taken for a fresh one is a race that may pass once -- two GPU runs bit for
    bit."""
    spec = dict(KP_WRAP[name], matrix_sweeps=sweeps)
    _pair(agx, oracle, _make(spec), 3)
    a, b = _states(agx, _make(spec), 3), _states(agx, _make(spec), 3)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


KP_WRAP_MG = dict(n=(12, 10, 8), nblocks=2, axis="i", stretch=1.1, levels=3, cycle="W",
                  bcs={3: ("viscousWall", 2)}, equation_set="navierStokes",
                  time_integration="implicitEuler", matrix_solver="lusgs", matrix_sweeps=3,
                  cfl=20.0)


def test_kp_tag_wrap_under_multigrid(agx, oracle):
    """Three LU-SGS sweeps under the multigrid cycle: k_d2_x_copy (x from the planes back into
    the D2 arrays around every transfer) is one more writer launch between the half sweeps.
    States of all three levels and the norms against the oracle, and two GPU runs bit for
    bit."""
    from aither_amd.solver import MultigridSolver

    def run(api):
        s = MultigridSolver(api, *synthetic.multigrid_levels(**KP_WRAP_MG))
        l2, st = [], []
        for nn in range(3):
            l2.append(s.step(nn)["l2"])
            st.append([s.download("state", gb, lev) for lev in range(3) for gb in range(2)])
        s.close()
        return l2, st

    (l2g, sg), (l2o, so), (l2r, sr) = run(agx), run(oracle), run(agx)
    g = synthetic.make_deck(**KP_WRAP_MG).num_ghost_layers()
    fine = synthetic.multigrid_levels(**KP_WRAP_MG)[0][0]
    for nn in range(3):
        e = rel_err(l2g[nn][None, :], l2o[nn][None, :])
        print("mg l2", nn, e)
        assert e < RTOL, (nn, e)
        # (floors: from the finest level's state at the start of the step)
        start = [b.state for b in fine.blocks] if nn == 0 else so[nn - 1][:2]
        assert_components(fine, "l2", l2g[nn][None, :], l2o[nn][None, :], start, (nn,))
        for a, b in zip(sg[nn], so[nn]):
            e = rel_err(a[g:-g, g:-g, g:-g], b[g:-g, g:-g, g:-g])
            print("mg state", nn, e)
            assert e < RTOL, (nn, e)
        for lev in range(3):      # every component on its own scale, per level
            core = lambda x: [a[g:-g, g:-g, g:-g] for a in x[2 * lev:2 * lev + 2]]
            assert_components(fine, "state", core(sg[nn]), core(so[nn]),
                              so[nn][2 * lev:2 * lev + 2], (nn, lev))
        for a, b in zip(sg[nn], sr[nn]):
            assert np.array_equal(a, b)
        assert np.array_equal(l2g[nn], l2r[nn])


# ======================= B. the inviscid tile kernel ======================================
SCHEMES = [("constant", "none"), ("thirdOrder", "none"), ("thirdOrder", "vanAlbada"),
           ("thirdOrder", "minmod"), ("weno", "none"), ("wenoZ", "none")]
FLUXES = ["roe", "ausm"]
TILE_N = (131, 15, 9)      # 3 x 3 tiles of 64 x 6 (and of 62 x 6), ragged in i and j


def tile_kw(recon, lim, flux, **kw):
    return dict(n=TILE_N, stretch=1.1, skew=0.01, face_reconstruction=recon, limiter=lim,
                inviscid_flux=flux, **kw)


FUSED_RUNS = [(r, l, f, "rk4") for r, l in SCHEMES for f in FLUXES] + \
             [(r, "none", f, "explicitEuler") for r in ("weno", "wenoZ") for f in FLUXES]


@pytest.mark.parametrize("recon,lim,flux,ti", FUSED_RUNS)
def test_tile_fused_instances(agx, oracle, recon, lim, flux, ti):
    """k_residual_tile<RECON, LIM, FLUX, FUSE, 6> with FUSE = 2 (stage 0: also forms
    consVarsN) and FUSE = 1 (the later RK4 stages), every (recon, limiter, flux) instance the
    dispatch can reach -- WENO and WENO-Z among them, also as explicitEuler (FUSE = 2 only) --
    on 3 x 3 ragged tiles, a persistent-range plan of 27 workgroups."""
    bcs = FARFIELD if flux == "ausm" else None       # far field / slip walls
    case = synthetic.single_block_case(**tile_kw(recon, lim, flux, bcs=bcs,
                                                 time_integration=ti, cfl=0.4))
    _pair(agx, oracle, case, 2)


@pytest.mark.parametrize("recon,lim", SCHEMES)
@pytest.mark.parametrize("flux", FLUXES)
def test_tile_unfused_instances(agx, oracle, recon, lim, flux):
    """k_residual_tile<RECON, LIM, FLUX, 0, 6> (the residual alone, implicit runs) on the same
    ragged 3 x 3 tiles, followed by k_lusgs_prepare and k_lusgs_kp."""
    case = synthetic.single_block_case(**tile_kw(recon, lim, flux, bcs=FARFIELD,
                                                 time_integration="implicitEuler",
                                                 matrix_solver="lusgs", cfl=10.0))
    _pair(agx, oracle, case, 2)


VISC_TILE_RUNS = [("thirdOrder", "minmod", "roe"), ("wenoZ", "none", "roe"),
                  ("constant", "none", "ausm")]


@pytest.mark.parametrize("recon,lim,flux", VISC_TILE_RUNS)
def test_tile_unfused_instances_viscous(agx, oracle, recon, lim, flux):
    """FUSE = 0 beside k_visc_tile (62 x 6 owned cells: its tile columns differ from the
    inviscid kernel's 64) with a viscous wall, for instances the 88^3 case does not run."""
    case = synthetic.single_block_case(**tile_kw(recon, lim, flux, bcs=WALL_J,
                                                 equation_set="navierStokes",
                                                 time_integration="implicitEuler",
                                                 matrix_solver="lusgs", cfl=10.0))
    _pair(agx, oracle, case, 2)


MARCH_N = (70, 7, 5)       # past one 64-wide tile in i and one 6-row tile in j, a short k-chunk


def test_march_fused_norms_against_the_update_pass(agx):
    """k_residual_march<.., FUSE = true, 6> (AGX_KERNEL=march) folds the residual norms itself;
    with AGX_NO_FUSE=1 the same kernel leaves the stage and the norms to k_update.  An RK4 stage
    is consVarsN - fac * residual, one product and the same fused multiply-add in both kernels,
    so the states are equal bit for bit, both runs form the same residuals, and the L-inf value
    and its location are equal (a maximum with its first location does not depend on the order
    of the fold).  The two passes add the same n = 2450 non-negative squares per equation in two
    orders: each sum is within (n - 1) u of the exact one, relatively, hence the two within
    2 (n - 1) u of each other, u = 2^-53.  Three steps, twelve stages, each compared.
    (explicitEuler is not run here: its stage rho v - fac * residual has two products, the
    fused kernels and k_update round them differently by an ulp)"""
    case = synthetic.single_block_case(n=MARCH_N, stretch=1.1, skew=0.01,
                                       time_integration="rk4", cfl=0.4)
    n = MARCH_N[0] * MARCH_N[1] * MARCH_N[2]
    bound = 2 * (n - 1) * 2.0 ** -53
    runs = []
    for env in ({"AGX_KERNEL": "march"}, {"AGX_KERNEL": "march", "AGX_NO_FUSE": "1"}):
        with switches(env):
            s = Solver(agx, case)
        out = []
        for nn in range(3):
            s.store_time_n(nn)
            for mm in range(case.deck.nonlinear_iterations):
                l2, linf, _ = s.iterate(mm, case.deck.cfl(nn))
                out.append((l2, (linf.linf, linf.block, linf.i, linf.j, linf.k, linf.eqn)))
        g = case.ng        # (ghost cells hold whatever the last ghost fill left there)
        runs.append((out, s.download("state", 0)[g:-g, g:-g, g:-g]))
        s.close()
    (fused, state_f), (plain, state_p) = runs
    assert np.all(np.isfinite(state_f))
    assert np.array_equal(state_f, state_p)
    assert len(fused) == len(plain) == 12
    for it, ((l2f, linf_f), (l2p, linf_p)) in enumerate(zip(fused, plain)):
        assert linf_f == linf_p, (it, linf_f, linf_p)
        assert np.all(l2p > 0.0)
        err = np.abs(l2f - l2p) / l2p
        print("march fused l2", it, err.max())
        assert err.max() <= bound, (it, err, bound)


THIN_SHAPES = [(1, 1, 40), (33, 1, 2), (2, 3, 1), (65, 5, 3)]
_IMPL = dict(time_integration="implicitEuler", cfl=5.0)
_VISC = dict(bcs=WALL_J, equation_set="navierStokes", matrix_solver="lusgs", **_IMPL)
THIN_DECKS = {
    # three ghost layers on blocks one to three cells thick: k_residual_tile<WENO, .., 1 / 2, 6>
    "weno_rk4": dict(face_reconstruction="weno", limiter="none", time_integration="rk4",
                     cfl=0.4),
    # k_lusgs_prepare and k_lusgs_kp with nsteps = ni + nj - 1 = 1, one plane, one sweep ...
    "lusgs1": dict(matrix_solver="lusgs", matrix_sweeps=1, **_IMPL),
    # ... and both triangles
    "lusgs2": dict(matrix_solver="lusgs", matrix_sweeps=2, **_IMPL),
    "dplur": dict(matrix_solver="dplur", matrix_sweeps=3, **_IMPL),
    # k_visc_tile, a wall under a block one cell thick
    "visc_central": dict(**_VISC),
    "visc_central4th": dict(viscous_face_reconstruction="centralFourth", **_VISC),
}
# (no combination is dropped: the oracle alone runs all 24 to finite states,
# tests/test_host_logic.py::test_oracle_runs_the_thin_block_cases)


def thin_case(n, deck):
    return synthetic.single_block_case(n=n, stretch=1.0, **THIN_DECKS[deck])


@pytest.mark.parametrize("deck", sorted(THIN_DECKS))
@pytest.mark.parametrize("n", THIN_SHAPES)
def test_thin_blocks_beyond_muscl_rk4(agx, oracle, n, deck):
    """Blocks thinner than the ghost depth (test_thin_and_ragged_blocks runs them as MUSCL +
    RK4 only) under WENO's three ghost layers, k_lusgs_prepare / k_lusgs_kp, DPLUR and
    k_visc_tile with central and centralFourth face states; see THIN_DECKS."""
    _pair(agx, oracle, thin_case(n, deck), 2)


# ======================= C. all eight orientations ========================================
UNIFORM = os.path.join(GOLDEN, "cases", "uniformFlow", "uniformFlow.inp")
ORIENT_DECKS = {
    # three ghost layers through every orientation
    "weno_lusgs": dict(face_reconstruction="weno", matrix_solver="lusgs", matrix_sweeps=2),
    # x and xold change roles every sweep
    "dplur3": dict(matrix_solver="dplur", matrix_sweeps=3),
    "bdplur": dict(matrix_solver="bdplur", matrix_sweeps=3),
    # velocity-gradient halo in its two five-slot halves, the exchange of x refreshes sw_dyn
    "visc_blusgs2": dict(equation_set="navierStokes", matrix_solver="blusgs", matrix_sweeps=2),
    # the D2 halo maps with the tag coming round (CONN = true)
    "visc_lusgs3": dict(equation_set="navierStokes", matrix_solver="lusgs", matrix_sweeps=3),
    "rans_lusgs": dict(equation_set="rans", turbulence_model="sst2003", matrix_solver="lusgs",
                       matrix_sweeps=2),
    "rans_blusgs": dict(equation_set="rans", turbulence_model="sst2003",
                        matrix_solver="blusgs", matrix_sweeps=2),
}


def uniform_flow_case(**changes):
    """The reference's uniformFlow grid (ten blocks, nine connections, every orientation) under
    a changed deck.  Viscous decks need a wall for the wall distance: the lower j-surface of
    block 0, an outer slip wall, becomes an adiabatic viscousWall."""
    deck = parse_input(UNIFORM)
    for k, v in changes.items():
        assert hasattr(deck, k), k
        setattr(deck, k, v)
    if deck.face_reconstruction in ("weno", "wenoZ"):
        deck.kappa = -2.0         # (what parsing such a deck leaves: kappa belongs to MUSCL)
    if deck.is_viscous():
        (s,) = [s for s in deck.bcs[0] if s.surface_type() == 3]
        assert s.bc_type == "slipWall"
        s.bc_type = "viscousWall"
    case = build_case(UNIFORM, deck=deck)
    synthetic.perturbed_state(case, 0.05)
    return case


@pytest.mark.parametrize("name", sorted(ORIENT_DECKS))
def test_all_orientations_under_every_halo(agx, agx_rans, oracle, name):
    """HALO_STATE with three ghost layers, HALO_UPDATE of DPLUR / BDPLUR (x and xold change
    roles) and of BLU-SGS (halo_planes refreshes sw_dyn), HALO_VELGRAD_A/B, the D2 maps at
    three sweeps and the rans HALO_TURB across all eight patch orientations, lower/lower and
    i<->j / j<->k pairs -- elsewhere they cross orientation 1 only."""
    case = uniform_flow_case(**ORIENT_DECKS[name])
    assert sorted({c.orientation for c in case.connections}) == list(range(1, 9))
    lib = agx_rans if case.n_eq == 7 else agx
    # (L-inf: the ten blocks lie whole periods of the perturbation apart; at step 0 the
    # maxima of several blocks agree to round-off -- one entry of two is undecided)
    _pair(lib, oracle, case, 2, linf_undecided=1 / 2)


@pytest.mark.parametrize("what,field", [(abi.HALO_STATE, "state"), (abi.HALO_UPDATE, "update")])
@pytest.mark.parametrize("solver", ["dplur", "lusgs"])
def test_halo_swap_local_moves_the_cells_of_the_index_maps(agx, what, field, solver):
    """agx_halo_swap_local itself, HALO_STATE and HALO_UPDATE, on the SoA planes (DPLUR) and
    on the diagonal-ordered arrays (LU-SGS: maps dst2 / src2): index-valued arrays in, the
    download equals the numpy restatement of GetSwapLoc (connections.insert_maps) cell for
    cell, all eight orientations.  On the D2 path x carries its writer's tag in the two low
    mantissa bits (kp_tagged): both sides are compared with those two bits cleared.
    (The velocity-gradient and turbulence fields cannot be uploaded through the ABI --
    field_info knows neither -- so HALO_VELGRAD_A/B and HALO_TURB are left to
    test_all_orientations_under_every_halo.)"""
    case = uniform_flow_case(matrix_solver=solver)
    assert on_d2_path(dict(time_integration=case.deck.time_integration,
                           matrix_solver=solver)) == (solver == "lusgs")
    sol = Solver(agx, case)
    ng = case.ng
    probes = []
    for gb, blk in enumerate(case.blocks):
        st = np.arange(blk.state.size, dtype=float).reshape(blk.state.shape) + 1e6 * gb
        sol.upload(field, gb, st)
        probes.append(st.reshape(-1, 5))
    agx.check(agx.halo_swap_local(sol.ctx, what), "halo_swap_local")
    expect = [p.copy() for p in probes]
    for c in case.connections:
        b0, b1 = c.block
        g0, g1 = case.blocks[b0].geom, case.blocks[b1].geom
        d0, s1, _ = conn_mod.insert_maps(c, True, ng, g0.n, g1.n)
        d1, s0, _ = conn_mod.insert_maps(c, False, ng, g1.n, g0.n)
        expect[b0][d0] = probes[b1][s1]
        expect[b1][d1] = probes[b0][s0]

    def untag(a):
        a = np.ascontiguousarray(a)
        return a.view(np.uint64) & ~np.uint64(3)

    for gb in range(len(case.blocks)):
        got = sol.download(field, gb).reshape(-1, 5)
        if field == "update" and solver == "lusgs":
            assert np.array_equal(untag(got), untag(expect[gb])), gb
        else:
            assert np.array_equal(got, expect[gb]), gb
    sol.close()


# ======================= D. full size against the oracle ==================================
def _peak_rss_gib():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2.0 ** 20


CONFIG3 = dict(kind="single", n=(256, 256, 256), stretch=1.2, bcs=WALL_J, amplitude=0.05,
               equation_set="navierStokes", face_reconstruction="weno", limiter="none",
               inviscid_flux="ausm", time_integration="implicitEuler", matrix_solver="lusgs",
               cfl=10.0)
CONFIG4 = dict(kind="cube", n=(128, 128, 128), splits=(2, 2, 2), inviscid_flux="ausm",
               time_integration="implicitEuler", matrix_solver="dplur", matrix_sweeps=4,
               cfl=10.0)


def test_config3_256cubed_against_the_oracle(agx, oracle):
    """BASELINE configs[2] at FULL size against the oracle: one iteration of 256^3, WENO5 +
    AUSMPW+ + viscous, scalar LU-SGS, perturbed state -- k_residual_tile, k_visc_tile,
    k_lusgs_prepare and 256 pipelined planes of k_lusgs_kp with 511 diagonals each (the case
    of test_config3_256cubed_real_scheme_fast_vs_simple_forms, which compares the library
    with itself)."""
    _pair(agx, oracle, _make(CONFIG3), steps=1, fields=("state", "residual"))
    print("peak RSS %.1f GiB" % _peak_rss_gib())


def test_config4_eight_128cubed_blocks_against_the_oracle(agx, oracle):
    """BASELINE configs[3] at FULL size against the oracle: one iteration of 2 x 2 x 2 blocks
    of 128^3, Euler MUSCL + AUSMPW+, DPLUR with four sweeps and twelve connections."""
    _pair(agx, oracle, _make(CONFIG4), steps=1, fields=("state", "residual"))
    print("peak RSS %.1f GiB" % _peak_rss_gib())
