"""Reads between the phases of an iteration leave a run bit-identical or are refused by name
(tests/probe.py) -- CPU, on the oracle; tests/test_probe_gpu.py holds the HIP libraries to the
same and to what the oracle returns at every position.

Before the refusal existed the `ghost` kind -- gradient downloads, gradient variables of
output_pack -- made after phase_bc_faces, after the state halo swap or after phase_bc_edges
changed the three viscous decks below silently: ghosts_for_output ends with the viscous-wall
fill and left it in the ghost cells the inviscid residual then read.  Measured with this
module on the oracle before the refusal, 7 x 6 x 5, two steps, against the unprobed run
(absolute): ns_dplur residual 1.5e-4, dt 4.3e-4, interior state 5.7e-3, x 2.1e-3, L2 1.7e-4,
ns_blusgs the same sizes, ns_lusgs_bdf2 residual 4.9e-10 and L2 2.0e-6, every one named at
phase_bc_faces (the first of the three positions).  Every other position, and the Euler rk4
deck everywhere, was invariant.
"""
import pytest

import probe
from aither_amd.case import synthetic

N = (7, 6, 5)
BOX = dict(stretch=1.2, skew=0.01)
WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
        4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
NS = dict(bcs=WALL, equation_set="navierStokes")


def single(**kw):
    return lambda: synthetic.single_block_case(N, **BOX, **kw)


def stacked(axis, n=N, **kw):
    return lambda: synthetic.stacked_blocks_case(n, nblocks=2, axis=axis, stretch=1.2, **kw)


def two_levels(**kw):
    return lambda: synthetic.multigrid_levels(n=(12, 10, 8), nblocks=1, axis="i", stretch=1.1,
                                              levels=2, cycle="V", **kw)


# name: (make, driver)
DECKS = {
    "euler_rk4": (single(time_integration="rk4", cfl=0.5), "phased"),
    "ns_dplur": (single(time_integration="implicitEuler", matrix_solver="dplur",
                        matrix_sweeps=3, cfl=5.0, **NS), "phased"),
    "ns_blusgs": (single(time_integration="implicitEuler", matrix_solver="blusgs",
                         matrix_sweeps=2, cfl=5.0, **NS), "phased"),
    "ns_lusgs_bdf2": (single(face_reconstruction="weno", limiter="none", inviscid_flux="ausm",
                             time_integration="bdf2", matrix_solver="lusgs",
                             nonlinear_iterations=2, dt=2.0e-6, cfl=-1.0, **NS), "phased"),
    # the same through ora_iterate: positions after store_time_n and after each iterate
    "ns_dplur_iterate": (single(time_integration="implicitEuler", matrix_solver="dplur",
                                matrix_sweeps=3, cfl=5.0, **NS), "solver"),
    "ns_lusgs_bdf2_iterate": (single(face_reconstruction="weno", limiter="none",
                                     inviscid_flux="ausm", time_integration="bdf2",
                                     matrix_solver="lusgs", nonlinear_iterations=2, dt=2.0e-6,
                                     cfl=-1.0, **NS), "solver"),
    # a connection: the local halo swaps between the phases
    "ns_bdplur_stacked_k": (stacked("k", time_integration="implicitEuler",
                                    matrix_solver="bdplur", matrix_sweeps=2, cfl=5.0, **NS),
                            "phased"),
    "rans_lusgs_stacked_i": (stacked("i", n=(9, 8, 7), time_integration="implicitEuler",
                                     matrix_solver="lusgs", matrix_sweeps=2, cfl=10.0,
                                     bcs=WALL, equation_set="rans",
                                     turbulence_model="sst2003"), "phased"),
    # a V cycle on two levels: every mg_* entry, reads on both levels
    "mg_ns_lusgs": (two_levels(time_integration="implicitEuler", matrix_solver="lusgs",
                               matrix_sweeps=2, cfl=20.0, bcs={3: ("viscousWall", 2)},
                               equation_set="navierStokes"), "multigrid"),
}
# what the oracle does not hold at all, per kind (probe.NOT_HELD): it gives no geometry back
# and forms neither node nor wall payloads; inviscid runs keep no viscosity_
ORACLE_LACKS = {"plain": {(f, "plain", "oracle") for f in probe.abi.GEOM_FIELDS},
                "aux": set(),
                "ghost": {("node_vars", "ghost", "oracle"), ("wall_vars", "ghost", "oracle")}}


@pytest.fixture(scope="module")
def unprobed(oracle):
    """The unprobed run of every deck, made once."""
    return {name: probe.run(oracle, make, driver)[0] for name, (make, driver) in DECKS.items()}


@pytest.mark.parametrize("kind", probe.KINDS)
@pytest.mark.parametrize("name", sorted(DECKS))
def test_reads_at_every_position_leave_the_run_bit_identical(oracle, unprobed, name, kind):
    """Two time steps probed after EVERY hooked entry against the unprobed run: interior state
    and update, residual, dt, cons_n, cons_nm1 of every block (and level) and every history
    entry (L2, the L-inf value and location, the matrix residual) with np.array_equal.  The
    refusals are exactly probe.REFUSED_AT's rows for the entries the run reaches (the ghost
    kind from phase_bc_faces to phase_residual), plus what the oracle does not hold."""
    make, driver = DECKS[name]
    p = probe.assert_invariant(oracle, make, driver, kind, base=unprobed[name])
    assert len(p.seen) == len(p.labels) > 0
    lacks = set(ORACLE_LACKS[kind])
    viscous = make()[0][0].deck.is_viscous() if driver == "multigrid" else make().deck.is_viscous()
    if not viscous:
        # (the wall payload is not asked for; the oracle's viscosity download of an inviscid
        # run returns its zeros, the HIP libraries refuse it by name)
        lacks.discard(("wall_vars", "ghost", "oracle"))
    assert {r for r in p.refused if r[2] != "fill_open"} == lacks
    if kind == "ghost" and driver != "solver":
        assert {(e, k) for e, k, why in p.refused if why == "fill_open"} == \
            {(e, "ghost") for e in ("phase_bc_faces", "phase_bc_edges")} | \
            ({("halo_swap_local[state]", "ghost")} if driver == "phased" else set())


def test_every_driver_reaches_its_entries(oracle):
    """The positions of the three drivers: PhasedSolver every phase of the header's order and
    the local swaps between them, Solver store_time_n and iterate, MultigridSolver every mg_*
    entry it calls."""
    def labels(name):
        make, driver = DECKS[name]
        return set(probe.run(oracle, make, driver, "aux")[1].labels)
    implicit = {"phase_bc_faces", "halo_swap_local[state]", "phase_bc_edges", "phase_residual",
                "phase_implicit_begin", "halo_swap_local[update]", "phase_relax_forward",
                "phase_matrix_residual", "phase_implicit_update", "store_time_n"}
    assert labels("ns_dplur") == implicit
    assert labels("ns_lusgs_bdf2") == implicit | {"phase_relax_backward"}
    assert labels("ns_bdplur_stacked_k") == implicit | {"halo_swap_local[velgrad_a]",
                                                        "halo_swap_local[velgrad_b]"}
    assert labels("rans_lusgs_stacked_i") == implicit | {"phase_relax_backward",
                                                         "halo_swap_local[turb]"}
    assert labels("euler_rk4") == {"store_time_n", "phase_bc_faces", "halo_swap_local[state]",
                                   "phase_bc_edges", "phase_residual", "phase_explicit_update"}
    assert labels("ns_dplur_iterate") == {"store_time_n", "iterate"}
    mg = labels("mg_ns_lusgs")
    assert set(probe.MG) <= mg and {"phase_bc_faces", "phase_residual", "phase_relax_forward",
                                    "phase_relax_backward", "phase_implicit_update"} <= mg


def test_a_refused_read_leaves_the_run_alone_and_names_where_it_is_legal(oracle):
    """The refusal itself: after phase_bc_faces a gradient download fails with the message that
    says why and where the call is legal; after phase_residual the same call succeeds; and the
    fill of ora_iterate does not arm it."""
    from aither_amd.solver import Solver
    s = Solver(oracle, DECKS["ns_dplur"][0]())
    try:
        s.download("vel_grad", 0)
        oracle.check(oracle.phase_bc_faces(s.ctx), "phase_bc_faces")
        for call in (lambda: s.download("press_grad", 0),
                     lambda: s.output_pack(0, ["density", "velGrad_ux"])):
            with pytest.raises(RuntimeError, match=r"ghost cells, which are being filled for the "
                                                   r"coming residual.*legal from "
                                                   r"agx_phase_residual to the next "
                                                   r"agx_phase_bc_faces and between agx_iterate"):
                call()
        s.output_pack(0, ["density", "resid_energy"])          # (no gradients: not refused)
        oracle.check(oracle.halo_swap_local(s.ctx, 0), "halo_swap_local")
        oracle.check(oracle.phase_bc_edges(s.ctx), "phase_bc_edges")
        oracle.check(oracle.phase_residual(s.ctx, 0, 5.0), "phase_residual")
        s.download("press_grad", 0)
        s.step(0)
        s.download("press_grad", 0)
    finally:
        s.close()
