"""Reads between the phases of an iteration, on the four HIP libraries (tests/probe.py).

(a) Every deck below selects one piece of the state the library defers across its entries
("reads between phases").  A run read by one probe kind after EVERY hooked
entry ends bit for bit where the unread run ends, and the reads that are refused are exactly
probe.REFUSED_AT's.  tests/test_host_logic.py::test_probe_decks_select_their_piece asserts
without a GPU that each deck has the property that selects its piece, and
::test_probe_census that every entry is reached in every library.

(b) What the reads return is held to the CPU oracle driven through the same proxy, position
by position: x to 1e-9 of the oracle's largest |x| at that position (the project's figure
for x, test_multigrid_seven_equations_parity), everything else to parity_utils.RTOL with
rel_err and, for n_eq-component data, per component.  The node and wall payloads, which the
oracle does not form, and the geometry, which it does not give back, are held by (a) and by
their own modules.

Run on a real MI355X:  python -m pytest tests/test_probe_gpu.py -m gpu
"""
import gc

import numpy as np
import pytest

import probe
import tp_cases
from parity_utils import RTOL, assert_components, component_err, flux_scale, rel_err
from aither_amd.case import synthetic
from test_production_paths_gpu import on_d2_path

pytestmark = pytest.mark.gpu

N = (7, 6, 5)
N_RANS = tp_cases.RANS_BASE["n"]
FAR = {s: ("characteristic", 1) for s in range(1, 7)}
WALL = dict(FAR)
WALL[3] = ("viscousWall", 2)
WALL_LAW_TAG = 4
assert (WALL_LAW_TAG, "lusgs") in tp_cases.WALL_LAW
WALL_LAW = dict(WALL)
WALL_LAW[3] = ("viscousWall", WALL_LAW_TAG)
NS = dict(bcs=WALL, equation_set="navierStokes", time_integration="implicitEuler", cfl=5.0)
RANS = dict(bcs=WALL, equation_set="rans", turbulence_model="sst2003",
            time_integration="implicitEuler", cfl=10.0)
BDF2 = dict(NS, time_integration="bdf2", nonlinear_iterations=2, dt=2.0e-6, cfl=-1.0,
            face_reconstruction="weno", limiter="none", inviscid_flux="ausm")
MG = dict(n=(12, 10, 8), nblocks=1, axis="i", stretch=1.1, levels=2, cycle="V",
          time_integration="implicitEuler", matrix_sweeps=2)

# All decks on stretch = 1.2; the single blocks skewed by 0.01 as well (the stacked form has
# no skew: its blocks must meet face to face).
# name: (library, form, deck keywords).  form: "single" / "stacked" (two blocks; axis in the
# keywords) / "mg" (synthetic.multigrid_levels) / a callable returning the case.
# library: (n_eq, thermodynamic model) of aither_amd.load
CP5, CP7, TP5, TP7 = (5, tp_cases.CP), (7, tp_cases.CP), (5, tp_cases.TP), (7, tp_cases.TP)
DECKS = {
    # fused stage: fused_pending, the state / state2 swap, halo_set[STATE]
    "euler_rk4": (CP5, "single", dict(time_integration="rk4", cfl=0.5)),
    "euler_rk4_stacked_i": (CP5, "stacked", dict(axis="i", time_integration="rk4", cfl=0.5)),
    # the FUSE form of the other explicit scheme
    "euler_explicit_weno": (CP5, "single", dict(time_integration="explicitEuler", cfl=0.4,
                                                face_reconstruction="weno", limiter="none")),
    # D2 arrays, x_planes_current, the tag epoch; stacked: the CONN form
    "ns_lusgs2": (CP5, "single", dict(matrix_solver="lusgs", matrix_sweeps=2, **NS)),
    "ns_lusgs2_stacked_k": (CP5, "stacked", dict(axis="k", matrix_solver="lusgs",
                                                 matrix_sweeps=2, **NS)),
    # consn_pending, state_is_time_n
    "ns_lusgs2_bdf2": (CP5, "single", dict(matrix_solver="lusgs", matrix_sweeps=2, **BDF2)),
    "ns_lusgs2_bdf2_stacked_k": (CP5, "stacked", dict(axis="k", matrix_solver="lusgs",
                                                      matrix_sweeps=2, **BDF2)),
    # the hyperplane form with its captured graphs, all blocks of a half sweep side by side
    "euler_lusgs_roe_stacked_i": (CP5, "stacked", dict(
        axis="i", time_integration="implicitEuler", matrix_solver="lusgs", matrix_sweeps=2,
        inv_flux_jac="approximateRoe", bcs=FAR, cfl=5.0)),
    # x / xold change roles, halo_set[UPDATE], the xold[0] scratch of the aux reads
    "ns_dplur3_stacked_j": (CP5, "stacked", dict(axis="j", matrix_solver="dplur",
                                                 matrix_sweeps=3, **NS)),
    # velocity-gradient halo, sweep records, the pipelined record sweep
    "ns_bdplur_stacked_i": (CP5, "stacked", dict(axis="i", matrix_solver="bdplur",
                                                 matrix_sweeps=2, **NS)),
    "ns_blusgs_c4_stacked_k": (CP5, "stacked", dict(
        axis="k", matrix_solver="blusgs", matrix_sweeps=2,
        viscous_face_reconstruction="centralFourth", **NS)),
    # k_lusgs_pipe tickets and progress, the shared rans_rec, viscosity_ of the last update
    "rans_lusgs_stacked_i": (CP7, "stacked", dict(n=N_RANS, axis="i", matrix_solver="lusgs",
                                                  matrix_sweeps=2, **RANS)),
    "rans_blusgs_stacked_i": (CP7, "stacked", dict(n=N_RANS, axis="i", matrix_solver="blusgs",
                                                   matrix_sweeps=2, **RANS)),
    # have_wall_data, the stored wall data under bc_pass mode 2
    "rans_wall_law": (CP7, "single", dict(n=N_RANS, matrix_solver="lusgs",
                                          wall_treatment="wallLaw",
                                          **dict(RANS, bcs=WALL_LAW))),
    # eager ghost fill with nonreflecting surfaces: have_time_n, k_nr_grads
    # (the keywords of a callable row restate its deck for the dispatch conditions)
    "stagnation_nonreflecting": (CP5, lambda: tp_cases.stagnation_case(tp_cases.CP),
                                 dict(time_integration="implicitEuler", matrix_solver="lusgs")),
    # mg_x_to_planes / mg_x_from_planes, mg_coarse, agx_mg_save_update
    "mg_euler_lusgs": (CP5, "mg", dict(MG, matrix_solver="lusgs", cfl=40.0)),
    "mg_rans_blusgs": (CP7, "mg", dict(MG, matrix_solver="blusgs", cfl=10.0, bcs=WALL,
                                       equation_set="rans", turbulence_model="sst2003")),
    # Newton temperature in the aux and output kernels
    "tp_weno_ausm_visc_lusgs": (TP5, lambda: tp_cases.hot_single(
        **dict(tp_cases.FIVE["weno_ausm_visc_lusgs"], n=N)), {}),
    "tp_rans_sst_blusgs": (TP7, lambda: tp_cases.rans_case("sst_blusgs"), {}),
    # ... and the transfers of the cycle on the hot state
    "tp_mg_euler_lusgs": (TP5, lambda: tp_cases.hot_multigrid(
        **dict(MG, matrix_solver="lusgs", cfl=40.0)), {}),
    "tp_mg_rans_blusgs": (TP7, lambda: tp_cases.hot_multigrid(
        **dict(MG, matrix_solver="blusgs", cfl=10.0, bcs=WALL, equation_set="rans",
               turbulence_model="sst2003")), {}),
}
MULTIGRID = ("mg_euler_lusgs", "mg_rans_blusgs", "tp_mg_euler_lusgs", "tp_mg_rans_blusgs")

# the drivers of every deck: PhasedSolver (every phase position) and Solver (after
# store_time_n and after each iterate: the only place the eager prefill is live); the
# multigrid decks run through MultigridSolver
RUNS = [(name, drv) for name in sorted(DECKS)
        for drv in (("multigrid",) if name in MULTIGRID else ("phased", "solver"))]
TIMED = "ns_dplur3_stacked_j"        # the deck that runs with agx_timing_enable on


def deck_kw(name):
    """The deck keywords of a table row (for the dispatch conditions, no case is built)."""
    return DECKS[name][2]


def maker(name):
    lib, form, kw = DECKS[name]
    kw = dict(kw)
    if callable(form):
        return form
    if form == "single":
        n = kw.pop("n", N)
        return lambda: synthetic.single_block_case(n, stretch=1.2, skew=0.01, **kw)
    if form == "stacked":
        n = kw.pop("n", N)
        return lambda: synthetic.stacked_blocks_case(n, nblocks=2, stretch=1.2, **kw)
    return lambda: synthetic.multigrid_levels(**kw)


def library(name):
    import aither_amd
    return aither_amd.load(*DECKS[name][0])


# ---- (b): what the reads return, against the oracle -------------------------------------------
GHOSTED = ("state", "update", "temperature", "viscosity")
ONLY_HIP = set(probe.abi.GEOM_FIELDS) | {"node_vars", "wall_vars"}
TAGGED_ZERO = 3 * 2.0 ** -1074      # x of the D2 path carries its writer's tag in two mantissa bits
AUX_VAR = {"temperature": "temperature", "viscosity": "viscosity"}   # field -> cell variable


def per_variable(a, b, floor=0.0):
    """rel_err of a payload [nvar, ...], every variable on its own scale."""
    return max(rel_err(x.reshape(-1, 1), y.reshape(-1, 1), floor) for x, y in zip(a, b))


def gradient_floors(case, states):
    """Round-off floors of the cell-centre gradients, in the manner of parity_utils.flux_scale:
    a Green-Gauss gradient is a sum of face values times face areas over a volume, so below
    1e-3 x (largest |field|) x (largest face area / smallest volume) it is the round-off of
    those terms -- the temperature gradient of the initial state, whose density and pressure
    carry the same perturbation, is 1e-16 of T A / V.  states: the oracle's state per block
    at the position.  Returns the 24 floors of probe.GRAD_VARS' order (velocity 9, T, rho, p,
    tke, omega 3 each), nondimensional, and their dimensional factors (output.cpp:235-407)."""
    g, gas = case.ng, case.gas
    vmin = min(float(np.abs(b.geom.vol.a[g:-g, g:-g, g:-g]).min()) for b in case.blocks)
    geo = 1.0e-3 * flux_scale(case) / vmin
    core = [np.asarray(s)[g:-g, g:-g, g:-g] for s in states]
    top = lambda f: max(float(np.abs(f(c)).max()) for c in core)
    n_eq = core[0].shape[-1]
    mags = [top(lambda c: np.sqrt((c[..., 1:4] ** 2).sum(axis=-1)))] * 9 + \
        [top(lambda c: c[..., 4] / (c[..., 0] * gas.gas_constant))] * 3 + \
        [top(lambda c: c[..., 0])] * 3 + [top(lambda c: c[..., 4])] * 3 + \
        ([top(lambda c: c[..., 5])] * 3 + [top(lambda c: c[..., 6])] * 3 if n_eq == 7 else [0.0] * 6)
    rr, ar, lr, tr = gas.rho_ref, gas.a_ref, gas.l_ref, gas.t_ref
    mur = gas.visc_c1 * tr ** 1.5 / (tr + gas.visc_s)
    dims = [ar / lr] * 9 + [tr / lr] * 3 + [rr / lr] * 3 + [rr * ar * ar / lr] * 3 + \
        [ar * ar / lr] * 3 + [ar * ar * rr / (mur * lr)] * 3
    return geo * np.array(mags), np.array(dims)


GRAD_SLOT = {"vel_grad": 0, "temp_grad": 9, "dens_grad": 12, "press_grad": 15}


def aux_windows(prober, nlev):
    """Per position and level: do the oracle's temperature_ / viscosity_ arrays belong to the
    state it holds?  They are those of its last residual (UpdateAuxillaryVariables, the
    reference's members), the library forms them on demand from the state it holds
    (test_temperature_viscosity_fields): the two are the same quantity from a level's
    phase_residual up to the entry that next changes its state -- its update, or a restriction
    into it.  Outside that window the library's field is held to the oracle's OUTPUT variable
    of the same position instead, which the oracle also forms from the state it holds."""
    open_ = [False] * nlev
    out = []
    for label, levs in zip(prober.labels, prober.levels):
        if label == "phase_residual":
            open_[levs[0]] = True
        elif label in ("phase_explicit_update", "phase_implicit_update"):
            open_[levs[0]] = False
        elif label == "mg_restrict":
            open_[levs[1]] = False
        elif label == "iterate":
            open_[levs[0]] = False
        out.append(tuple(open_))
    return out


def compare_position(cases, pos, label, og, oo, inviscid, bad, window, plain):
    """Everything the probes of one position returned, library (og) against oracle (oo).
    window: aux_windows of this position; plain: the oracle's plain reads of this position.
    Mismatches are appended to bad as (position, label, key, figure, bound)."""
    only_g = {k[-1] for k in set(og) - set(oo)}
    only_o = {k[-1] for k in set(oo) - set(og)}
    assert only_g <= ONLY_HIP, (pos, label, only_g)
    assert only_o <= ({"viscosity"} if inviscid else set()) | {"diagonal"}, (pos, label, only_o)

    def core(lev, key, x):
        g = cases[lev].ng
        return x[g:-g, g:-g, g:-g] if key in GHOSTED else x

    for lev, case in enumerate(cases):
        keys = sorted(k for k in og if k in oo and k[0] == lev and k[2] != "halo_count")
        rfloor = 1.0e-3 * flux_scale(case)
        blocks = sorted({k[1] for k in keys})
        for name in sorted({k[2] for k in keys}):
            got = [core(lev, name, og[(lev, gb, name)]) for gb in blocks]
            ref = [core(lev, name, oo[(lev, gb, name)]) for gb in blocks]
            if name == "update":
                scale = max(np.abs(r).max() for r in ref)
                err = max(np.abs(a - r).max() for a, r in zip(got, ref))
                bound = 1.0e-9 * scale if scale > 0.0 else TAGGED_ZERO
                if not err <= bound:
                    bad.append((pos, label, (lev, name), err, bound))
                continue
            if name == "viscosity" and inviscid:
                continue      # (the oracle's zeros; the libraries refuse the call by name)
            if name in AUX_VAR and not window[lev]:
                # the oracle's output variable of this position (dimensional) instead
                gas = case.gas
                mu_ref = gas.visc_c1 * gas.t_ref ** 1.5 / (gas.t_ref + gas.visc_s)
                unit = gas.t_ref if name == "temperature" else mu_ref
                names = [n for n in probe.CELL_VARS if n != "viscosity" or not inviscid]
                ref = [plain[(lev, gb, "cell_vars")][names.index(AUX_VAR[name])][..., None] / unit
                       for gb in blocks]
            if name == "grad_vars" or name in GRAD_SLOT:
                fl, dims = gradient_floors(case, [plain[(lev, gb, "state")] for gb in blocks])
            if name == "grad_vars":
                err = max(rel_err(a[v].reshape(-1, 1), r[v].reshape(-1, 1), fl[v] * dims[v])
                          for a, r in zip(got, ref) for v in range(len(probe.GRAD_VARS)))
            elif name in GRAD_SLOT:
                err = max(rel_err(a, r, fl[GRAD_SLOT[name]]) for a, r in zip(got, ref))
            elif name == "cell_vars":
                err = max(per_variable(a, r) for a, r in zip(got, ref))
            else:
                err = max(rel_err(a, r, rfloor if name == "residual" else 0.0)
                          for a, r in zip(got, ref))
            if not err < RTOL:
                bad.append((pos, label, (lev, name), err, RTOL))
            if name in ("state", "residual", "cons_n", "cons_nm1"):
                states = [oo[(lev, gb, "state")] for gb in blocks]
                try:
                    if name in ("state", "residual"):
                        assert_components(case, name, got, ref, states)
                    else:
                        ce = component_err(got, ref, np.zeros(got[0].shape[-1]))
                        assert ce.max() < RTOL, (name, "per component", ce)
                except AssertionError as exc:
                    bad.append((pos, label, (lev, name), exc.args[0], RTOL))
        for k in og:
            if k[2] == "halo_count":
                assert np.array_equal(og[k], oo[k]), (pos, label, k)


@pytest.mark.parametrize("name,driver", RUNS)
def test_reads_between_phases(oracle, name, driver):
    """One (library, deck, driver): the unread run and one run per probe kind on the library
    (bitwise, part a), one run per probe kind on the oracle (part b)."""
    lib, make = library(name), maker(name)
    timing = name == TIMED
    made = make()
    cases = made[0] if driver == "multigrid" else [made]
    inviscid = not cases[0].deck.is_viscous()
    d2 = DECKS[name][0] == CP5 and on_d2_path(deck_kw(name))
    failure = None
    try:
        base = probe.run(lib, make, driver, timing=timing)[0]
        bad = []
        plain = None
        for kind in probe.KINDS:
            pg = probe.assert_invariant(lib, make, driver, kind, timing=timing, base=base)
            po = probe.assert_invariant(oracle, make, driver, kind)
            assert pg.labels == po.labels and len(pg.seen) == len(pg.labels)
            assert pg.levels == po.levels
            if kind == "plain":
                plain = po.seen
            # refusals: by position the same in both; otherwise what the library does not
            # hold -- viscosity_ of an inviscid run, wall-law data before the first residual,
            # the scalar diagonal on the diagonal-ordered LU-SGS path
            want = set()
            if inviscid and kind == "aux":
                want.add(("viscosity", "aux", "inviscid"))
            if d2 and kind == "plain":
                want.add(("diagonal", "plain", "d2_diagonal"))
            if deck_kw(name).get("wall_treatment") == "wallLaw" and kind == "ghost":
                want.add(("wall_vars", "ghost", "no_wall_data"))
            got = {r for r in pg.refused if r[2] != "fill_open"}
            assert got == want, (kind, sorted(got), sorted(want))
            windows = aux_windows(po, len(cases))
            for pos, label in enumerate(pg.labels):
                compare_position(cases, pos, label, pg.seen[pos], po.seen[pos], inviscid, bad,
                                 windows[pos], plain[pos])
        for row in bad[:400]:
            print("PROBE-PARITY", name, driver, row)
        assert not bad, (len(bad), bad[:6])
    except AssertionError as exc:
        failure = repr(exc.args[0] if len(exc.args) == 1 else exc.args)
    if failure is not None:
        gc.collect()      # (a live oracle context refuses the other equation count)
        pytest.fail(failure, pytrace=False)
