"""Shared helpers for the parity tests (HIP path vs CPU oracle)."""
import contextlib
import os

import numpy as np

from aither_amd.solver import Solver

# fp64 tolerance stated by BASELINE.json north_star: residuals and updated
# state within 1e-10 relative of the CPU reference.
RTOL = 1.0e-10
MATRIX_RTOL = 1.0e-6   # cap of the bound run_pair DERIVES per case (matrix_tolerance:
                       # 5e-9 .. 1e-7 for the synthetic decks, cancellation factors 12 .. 270)
MATRIX_FLOOR = 1.0e-14  # below this the matrix residual of a converged / uniform state
                        # is the round-off of O(1) operands


@contextlib.contextmanager
def switches(env=None, **more):
    """The AGX_* switches `env` (a dict, and / or keywords) in os.environ for the body -- they
    are read when a context is created -- and the environment as it was afterwards."""
    env = dict(env or {}, **more)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def matrix_tolerance(so):
    """Relative tolerance of the matrix residual, derived: f - (A x - b) is what is LEFT
    after its operands A x, the off-diagonal terms and b cancel, so its error is the 1e-10
    parity of those operands (x, state, residual: asserted field by field in run_pair)
    amplified by |operands| / |remainder|.  The oracle reports both sums of squares of its
    last matrix residual (ora_debug_matrix_operands, a test hook); a factor 4 covers the
    three operands and the square root.  Returns (tolerance, cancellation factor)."""
    import ctypes as C
    fn = so.api.lib.ora_debug_matrix_operands
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    ops, res = C.c_double(0.0), C.c_double(0.0)
    so.api.check(fn(so.ctx, C.byref(ops), C.byref(res)), "debug_matrix_operands")
    if res.value <= 0.0:
        return MATRIX_RTOL, float("inf")
    amp = (ops.value / res.value) ** 0.5
    return 4.0 * RTOL * amp, amp


def rel_err(got, ref, floor=0.0):
    """max |got-ref| per last-axis component, relative to the largest of
      * that component's max |ref|,
      * 10 % of the whole field's max |ref|  (components that are physically
        zero, e.g. the w-momentum residual of a 2-D case, are pure round-off),
      * `floor`: an absolute scale below which the quantity is round-off of
        the terms it is built from (see flux_scale)."""
    got = np.asarray(got, dtype=float)
    ref = np.asarray(ref, dtype=float)
    comp_axes = tuple(range(ref.ndim - 1))
    gmax = np.abs(ref).max()
    scale = np.maximum(np.abs(ref).max(axis=comp_axes), max(0.1 * gmax, floor))
    scale = np.where(scale > 0, scale, 1.0)
    return (np.abs(got - ref).max(axis=comp_axes) / scale).max()


def flux_scale(case):
    """Magnitude of one face flux: largest face area times rho*c^2 ~ O(1) in the
    reference's nondimensionalisation.  A residual is the sum of six such
    fluxes, so its round-off floor is ~1e-16 * flux_scale; residuals smaller
    than 1e-3 * flux_scale (e.g. the exactly-zero residual of a uniform flow
    at iteration 0) are compared on that scale."""
    amax = 0.0
    for blk in case.blocks:
        g = blk.geom
        for d in "ijk":
            amax = max(amax, float(g.farea[d].a[..., 3].max()))
    return amax


# ---- per-component measure -------------------------------------------------------------
# rel_err holds every component against 10 % of the LARGEST component's maximum: in a
# 7-equation case tke, the mean-flow residuals and their norms are held only relative to
# omega.  component_err holds each component against its own maximum over the whole case,
# or -- where that maximum is the round-off of cancelling fluxes -- against a floor formed
# from the reference's state and geometry alone (state_floors, residual_floors).  The
# floors are neither fitted to the code under test nor too low: the oracle's own answer to
# a 1e-13 perturbation of its input bounds them (tests/test_parity_measure_host.py).
VECTOR = (1, 2, 3)      # velocity in the state, momentum in the residual and the norms


def _blocks(x):
    if isinstance(x, (list, tuple)):
        return [np.asarray(a, dtype=float) for a in x]
    return [np.asarray(x, dtype=float)]


def _old_scale(ref, floor):
    """The scale rel_err(., ref, floor) divides by, per component."""
    axes = tuple(range(ref.ndim - 1))
    return np.maximum(np.abs(ref).max(axis=axes), max(0.1 * np.abs(ref).max(), floor))


def component_scales(ref, floors, old_floor=0.0):
    """Per block, the scale of every last-axis component: the component's max |ref| over
    ALL blocks (the three components of a vector share the largest of theirs), or its floor
    if that is larger -- capped, in every block, by the scale rel_err gives the component
    there, so that the measure can only be stricter than rel_err.  The cap is needed: a
    shared vector scale exceeds rel_err's scale of the smaller components, and the energy
    floor rho (|V| + c) H is about three times rel_err's flux floor."""
    ref = _blocks(ref)
    n = ref[0].shape[-1]
    own = np.zeros(n)
    for r in ref:
        own = np.maximum(own, np.abs(r).max(axis=tuple(range(r.ndim - 1))))
    if n > max(VECTOR):
        own[list(VECTOR)] = own[list(VECTOR)].max()
    new = np.maximum(own, np.asarray(floors, dtype=float))
    out = []
    for r in ref:
        old = _old_scale(r, old_floor)
        scale = np.minimum(new, old)
        out.append(np.where(scale > 0, scale, 1.0))
    return out


def component_err(got, ref, floors, old_floor=0.0):
    """max |got - ref| / max(max |ref_e|, floors[e]) for each last-axis component e.
    got, ref: one array or a list with one array per block; max |ref_e| is over all blocks
    (a block whose mass residual is 6e-20 does not set its own scale) and shared by the
    components of a vector.  old_floor: the floor the callers give rel_err for this field;
    the scale of a component in a block is capped by rel_err's (see component_scales)."""
    got, ref = _blocks(got), _blocks(ref)
    err = np.zeros(ref[0].shape[-1])
    for g, r, scale in zip(got, ref, component_scales(ref, floors, old_floor)):
        err = np.maximum(err, np.abs(g - r).max(axis=tuple(range(r.ndim - 1))) / scale)
    return err


def _interior(case, states):
    g = case.ng
    return [np.asarray(s)[g:-g, g:-g, g:-g] for s in states]


def state_floors(case, states):
    """No floor for rho, p, tke, omega; the velocity vector is held against the largest |V|
    (states: the reference's state per block, ghost cells included)."""
    n = states[0].shape[-1]
    fl = np.zeros(n)
    fl[list(VECTOR)] = max(np.sqrt((s[..., 1:4] ** 2).sum(axis=-1)).max()
                           for s in _interior(case, states))
    return fl


def residual_floors(case, states):
    """flux_scale per equation: 1e-3 x the largest face area x the magnitude of that
    equation's face flux in the reference's state -- rho (|V| + c) for mass,
    rho (|V| + c) |V| + p for momentum, rho (|V| + c) H for energy, the mass flux times the
    largest tke / omega for the turbulence equations.  A residual is the sum of six such
    fluxes; below this floor it is their round-off.  (c and H with the frozen gamma.)"""
    gam = case.gas.gamma
    n = states[0].shape[-1]
    mag = np.zeros(n)
    for s in _interior(case, states):
        rho, p = s[..., 0], s[..., 4]
        v = np.sqrt((s[..., 1:4] ** 2).sum(axis=-1))
        m = rho * (v + np.sqrt(gam * p / rho))
        h = gam / (gam - 1.0) * p / rho + 0.5 * v * v
        cur = [m.max(), (m * v + p).max(), (m * v + p).max(), (m * v + p).max(), (m * h).max()]
        if n == 7:
            cur += [m.max() * np.abs(s[..., 5]).max(), m.max() * np.abs(s[..., 6]).max()]
        mag = np.maximum(mag, cur)
    return 1.0e-3 * flux_scale(case) * mag


def norm_floors(case, states):
    """The floors of the L2 norms: residual_floors x sqrt(total_cells), as nfloor."""
    return residual_floors(case, states) * np.sqrt(case.total_cells)


def assert_components(case, kind, got, ref, states, msg=()):
    """component_err < RTOL for a field of the whole case.  kind: "state" (got, ref: the
    physical cells per block), "residual" (per block) or "l2" (the norms, [1, neq]);
    states: the reference's state per block, ghost cells included (the floors' input)."""
    rfloor = 1.0e-3 * flux_scale(case)
    floors, old = {"state": (state_floors, 0.0), "residual": (residual_floors, rfloor),
                   "l2": (norm_floors, rfloor * np.sqrt(case.total_cells))}[kind]
    ce = component_err(got, ref, floors(case, states), old)
    assert ce.max() < RTOL, (kind, "per component", ce) + tuple(msg)
    return ce


# ---- the L-inf record --------------------------------------------------------------------
def first_maximum(fields, parents=None):
    """The reference's record of a residual (procBlock.cpp:863-866, main.cpp:254): the first
    entry strictly greater than everything before it in loop order -- block, k, j, i,
    equation -- starting from 0.  fields: [nk, nj, ni, neq] per block.  Returns
    (value, block, i, j, k, eqn) with eqn counted from 1, all zero if nothing is positive."""
    best = (0.0, 0, 0, 0, 0, 0)
    for n, f in enumerate(fields):
        f = np.asarray(f)
        lin = int(np.argmax(f))            # the first of equal maxima in C order
        k, j, i, e = np.unravel_index(lin, f.shape)
        if f[k, j, i, e] > best[0]:
            best = (float(f[k, j, i, e]), n if parents is None else parents[n],
                    int(i), int(j), int(k), int(e) + 1)
    return best


def tied_set(fields, parents=None):
    """(locations of the entries that equal the global maximum bitwise, the distance from
    that maximum down to the largest value outside the set)."""
    vmax = max(float(np.max(f)) for f in fields)
    locs, rest = [], -np.inf
    for n, f in enumerate(fields):
        f = np.asarray(f)
        hit = f == vmax
        for k, j, i, e in zip(*np.nonzero(hit)):
            locs.append((n if parents is None else parents[n], int(i), int(j), int(k),
                         int(e) + 1))
        if not hit.all():
            rest = max(rest, float(f[~hit].max()))
    return locs, vmax - rest


LINF_MARGIN = 10.0 * RTOL     # the oracle's maximum must stand out by this much (relative)
LINF_MAX_SKIPPED = 0.25       # of the history entries of a run_pair call


def step_with_residuals(sol, nn):
    """Solver.step(nn), keeping the residual of every block after every nonlinear iteration
    (history entry "residual": the field that iteration's norms were formed from).  A
    restatement of aither_amd/solver.py Solver.step with that one key added;
    tests/test_parity_measure_host.py::test_step_with_residuals_is_solver_step holds the
    two together."""
    d = sol.case.deck
    cfl = d.cfl(nn)
    sol.store_time_n(nn)
    for mm in range(d.nonlinear_iterations):
        l2, linf, mres = sol.iterate(mm, cfl)
        mres = (mres / (sol.case.total_cells * sol.cfg.n_eq)) ** 0.5
        sol.history.append(dict(
            nn=nn, mm=mm, l2=np.sqrt(l2), norm=sol.normalized(l2, nn, mm),
            linf=(linf.linf, linf.block, linf.i, linf.j, linf.k, linf.eqn), matrix=mres,
            residual=[sol.download("residual", gb) for gb in sol.block_ids]))
    return sol.history[-1]


SYNC_FIELDS = ("state", "cons_n", "cons_nm1", "update")


def run_pair(agx, oracle, case, steps, fields=("state", "residual", "dt"),
             resync=True, check_from=0, linf_undecided=LINF_MAX_SKIPPED):
    """Advance `steps` time steps with both backends and compare everything
    that crosses the boundary after every step.

    resync=True (default) measures parity "on identical inputs" (BASELINE.json
    north_star): before each step after the first, the oracle's state, time
    levels and update are uploaded into the HIP solver, so each comparison is
    one time step (all its nonlinear iterations) from bit-identical inputs.
    A residual is a small difference of large fluxes, so without the resync
    its error relative to its own (shrinking) magnitude grows like
    |flux| / |residual| times the state error although the state itself stays
    within 1e-13 (see test_free_running_drift).

    check_from: first time step that is compared (earlier ones run, resynchronised
    as usual, but are not asserted on) -- for cases whose first step is
    ill-conditioned in the reference's own formulas, see the caller.

    Every comparison is made twice: with rel_err (10 % of the field's largest component)
    and with component_err (every component on its own scale or its flux floor).

    The L-inf record of EVERY history entry: the value as before; the location
    (block, i, j, k, eqn) against the oracle's wherever the oracle's own residual separates
    its maximum from the largest value outside the bitwise-tied set by more than LINF_MARGIN
    (a location inside the tied set where that set has several members; which member is the
    own-field rule's business) -- at most LINF_MAX_SKIPPED of the entries may fail that
    condition (LINF_MARGIN is relative to max(maximum, flux floor), the scale the value is
    held on; entries whose maximum is itself under that margin -- the round-off residual of
    a uniform stream -- have no location to hold and are not counted; a caller whose case exceeds the quarter
    names its exact share in linf_undecided and says why); and after the last nonlinear iteration of a step, where the library's
    `residual` is the field the norm was formed from (every path keeps it: the fused
    marching stage stores the residual it advances with), the library against itself by the
    reference's rule: the value is the maximum of its own residual bit for bit, the
    location the first strictly greater entry in loop order."""
    sg, so = Solver(agx, case), Solver(oracle, case)
    ng = case.ng
    n_hist = 0
    rfloor = 1.0e-3 * flux_scale(case)
    nfloor = rfloor * np.sqrt(case.total_cells)
    gbs = list(sg.block_ids)
    n_entries = n_skipped = 0
    for nn in range(steps):
        if resync and nn > 0:
            for gb in gbs:
                for f in SYNC_FIELDS:
                    sg.upload(f, gb, so.download(f, gb))
                # (a state upload re-derives what the library keeps from the state at
                # start-up -- the rans viscosity_ of AuxillaryAndWidths, main.cpp:169 --
                # so the oracle gets the same call)
                so.upload("state", gb, so.download("state", gb))
            sg.l2_first = None if so.l2_first is None else so.l2_first.copy()
        # the floors of this step: from the state the oracle starts it with
        start = [so.download("state", gb) for gb in gbs]
        cfloor, cnfloor = residual_floors(case, start), norm_floors(case, start)
        sg.step(nn), step_with_residuals(so, nn)
        assert len(sg.history) == len(so.history)
        if nn < check_from:
            n_hist = len(so.history)
            continue
        for hg, ho in zip(sg.history[n_hist:], so.history[n_hist:]):
            e = rel_err(hg["l2"][None, :], ho["l2"][None, :], nfloor)
            assert e < RTOL, ("L2 residual norm", hg["nn"], hg["mm"], e,
                              hg["l2"], ho["l2"])
            ce = component_err(hg["l2"][None, :], ho["l2"][None, :], cnfloor, nfloor)
            assert ce.max() < RTOL, ("L2 residual norm, per component", hg["nn"], hg["mm"],
                                     ce, hg["l2"], ho["l2"])
            if ho["matrix"] > 0:
                # the last nonlinear iteration of the step against the DERIVED bound (the
                # hook describes the oracle's last matrix residual), the earlier ones
                # against its cap
                last = ho is so.history[-1]
                tol, amp = matrix_tolerance(so) if last else (MATRIX_RTOL, None)
                tol = min(tol, MATRIX_RTOL)
                assert abs(hg["matrix"] - ho["matrix"]) <= tol * ho["matrix"] + MATRIX_FLOOR, \
                    ("matrix residual", hg["matrix"], ho["matrix"], tol, amp)
            # the L-inf record of this entry
            lg, lo = hg["linf"], ho["linf"]
            assert abs(lg[0] - lo[0]) <= RTOL * max(abs(lo[0]), rfloor), (lg, lo)
            assert first_maximum(ho["residual"], gbs) == tuple(lo), \
                ("the oracle's record is not the first maximum of its residual", lo)
            tied, gap = tied_set(ho["residual"], gbs)
            # the residual is held to RTOL of max(|r|, rfloor): a maximum that stands out
            # by ten times that is the same cell in both
            margin = LINF_MARGIN * max(lo[0], rfloor)
            if lo[0] <= margin:
                continue      # the whole field is under the margin (a uniform stream)
            n_entries += 1
            if gap > margin:
                assert tuple(lg[1:]) in tied, ("L-inf location", hg["nn"], hg["mm"], lg, lo)
                if len(tied) == 1:
                    assert tuple(lg[1:]) == tuple(lo[1:])
            else:
                n_skipped += 1
        n_hist = len(so.history)
        lg, lo = sg.history[-1]["linf"], so.history[-1]["linf"]
        assert abs(lg[0] - lo[0]) <= RTOL * max(abs(lo[0]), rfloor), (lg, lo)
        if "residual" in fields:
            own = [sg.download("residual", gb) for gb in gbs]
            assert first_maximum(own, gbs) == tuple(lg), \
                ("L-inf record against the library's own residual", nn, lg,
                 first_maximum(own, gbs))
        for gb in gbs:
            for f in fields:
                a, b = sg.download(f, gb), so.download(f, gb)
                if f == "state":      # corners are never assigned by either
                    a = a[ng:-ng, ng:-ng, ng:-ng]
                    b = b[ng:-ng, ng:-ng, ng:-ng]
                e = rel_err(a, b, rfloor if f == "residual" else 0.0)
                assert e < RTOL, (f, gb, nn, e)
        # ... and every component on its own scale over all blocks
        core = lambda a: a[ng:-ng, ng:-ng, ng:-ng]
        if "state" in fields:
            b = [so.download("state", gb) for gb in gbs]
            ce = component_err([core(sg.download("state", gb)) for gb in gbs],
                               [core(x) for x in b], state_floors(case, b))
            assert ce.max() < RTOL, ("state, per component", nn, ce)
        if "residual" in fields:
            ce = component_err([sg.download("residual", gb) for gb in gbs],
                               so.history[-1]["residual"], cfloor, rfloor)
            assert ce.max() < RTOL, ("residual, per component", nn, ce)
        for h in so.history:          # (kept per entry only until compared)
            h.pop("residual", None)
    assert n_skipped <= linf_undecided * n_entries + 1.0e-9, \
        ("L-inf location: the oracle's maximum is not separated in too many entries",
         n_skipped, n_entries)
    return sg, so
