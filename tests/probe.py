"""Reads between the phases of an iteration: a probing proxy of abi.Api and what it asks for.

The C-ABI lets a caller who drives the phases himself download a field or pack an output
payload between any two calls.  The library defers a good deal of state across those calls
("reads between phases"), and a read has to respect all of it: a run that
is read at every position must end bit for bit where the unread run ends, or the read must
be refused by name.

ProbingApi forwards every call to the Api it wraps and calls hook(label, args) after each
SUCCESSFUL call of a hooked entry (HOOKED).  The drivers -- Solver, PhasedSolver on one rank,
MultigridSolver -- run on it unchanged.  The label is the entry's name; the halo
entries carry their selector ("halo_swap_local[state]"), because the same entry stands at
positions with different rules.

Three kinds of probe (Prober):
  plain  the stored fields, the nine geometry fields, both restart payloads, the cell
         variables without gradients, halo_count, sync, timing_get
  aux    temperature and viscosity (formed on demand into a scratch plane)
  ghost  what refills the ghost cells of the state: the four gradient fields, the gradient
         variables of output_pack, the node payload, the wall payload

A refused call is recorded with its reason; REFUSED_AT is the table of (label, kind) pairs
that are refused because of WHERE they stand, and NOT_HELD what a configuration or a
library does not hold at all.  Nothing else may fail.
"""
import ctypes as C
import re

import numpy as np

from aither_amd import abi
from aither_amd.solver import MultigridSolver, PhasedSolver, Solver

HALO_NAMES = {abi.HALO_STATE: "state", abi.HALO_UPDATE: "update",
              abi.HALO_VELGRAD_A: "velgrad_a", abi.HALO_VELGRAD_B: "velgrad_b",
              abi.HALO_TURB: "turb"}
PHASES = tuple(n for n in abi.SYMBOLS if n.startswith("phase_"))
MG = tuple(n for n in abi.SYMBOLS if n.startswith("mg_"))
HALO = ("halo_swap_local", "halo_pack", "halo_unpack")
HOOKED = ("store_time_n", "iterate") + PHASES + HALO + MG
KINDS = ("plain", "aux", "ghost")

PLAIN_FIELDS = ("state", "residual", "dt", "spec_radius", "cons_n", "update", "diagonal",
                "cons_nm1")
AUX_FIELDS = ("temperature", "viscosity")
GRAD_FIELDS = ("vel_grad", "temp_grad", "dens_grad", "press_grad")
assert set(PLAIN_FIELDS + AUX_FIELDS + GRAD_FIELDS) | set(abi.GEOM_FIELDS) == set(abi.FIELD)
GRAD_VARS = tuple(n for n, v in sorted(abi.OUT.items(), key=lambda kv: kv[1])
                  if abi.OUT["velGrad_ux"] <= v < abi.OUT["resid_mass"])
CELL_VARS = tuple(n for n, v in sorted(abi.OUT.items(), key=lambda kv: kv[1])
                  if n not in GRAD_VARS)
# (the library forms no viscosityRatio, turbulentViscosity, f1, f2 at nodes, by name)
NODE_VARS = ("density", "vel_x", "vel_y", "vel_z", "pressure", "temperature", "mach",
             "velGrad_uy", "tempGrad_y", "pressGrad_x")
WALL_VARS = ("yplus", "shearStress", "heatFlux", "frictionVelocity", "temperature",
             "shearStress_x")
TIMING_GROUPS = 7

# ---- refusals -----------------------------------------------------------------------------
# Refused because of the position: from the caller's phase_bc_faces to the phase_residual that
# follows it the ghost cells are being filled for that residual (include/aither_gfx950.h,
# "reads between phases"); the `ghost` kind would leave its viscous-wall fill in them.
REFUSED_AT = {
    ("phase_bc_faces", "ghost"),
    ("halo_swap_local[state]", "ghost"),
    ("halo_pack[state]", "ghost"),
    ("halo_unpack[state]", "ghost"),
    ("phase_bc_edges", "ghost"),
}
FILL_OPEN = re.compile(r"being filled for the coming residual.*legal from agx_phase_residual")
# Not held at all, whatever the position: (reason, pattern of the message)
NOT_HELD = {
    "inviscid": re.compile(r"viscosity_ is only kept for viscous runs"),
    # the oracle forms no node payload and no wall payload, and gives no geometry back
    "oracle": re.compile(r"ora_\w+ failed \(1\): (unknown output variable (64|128)|"
                         r"unknown field (1[4-9]|2[0-2]))$"),
    # the diagonal-ordered LU-SGS path keeps a_ inside its sweep arrays only
    "d2_diagonal": re.compile(r"keeps the scalar diagonal a_ only as 1 / a inside its sweep arrays"),
    # wall-law surfaces before the first residual has stored their wall data
    "no_wall_data": re.compile(r"hold no wall data before the first residual"),
}


def expected_refusals(labels):
    """The rows of REFUSED_AT whose label a run has reached."""
    return {(e, k) for e, k in REFUSED_AT if e in set(labels)}


class ProbingApi:
    """Forwards every call to the Api it wraps; after a successful call of a hooked entry
    (HOOKED) it calls hook(label, args)."""

    def __init__(self, api, hook=None):
        self._api, self.hook = api, hook

    def __getattr__(self, name):
        target = getattr(self._api, name)
        if name not in HOOKED:
            return target

        def call(*args):
            rc = target(*args)
            if rc == 0 and self.hook is not None:
                label = name
                if name in HALO:
                    label = "%s[%s]" % (name, HALO_NAMES[args[2] if name != "halo_swap_local"
                                                         else args[1]])
                self.hook(label, args)
            return rc
        return call


class Prober:
    """The hook: at every position (only=None) or at position `only` alone it makes the reads
    of `kind` on every solver it was given (the levels of a multigrid run) and keeps what they
    returned: seen[position] = {key: array}, refused = {(label or key, kind, reason)}."""

    def __init__(self, kind, only=None):
        self.kind, self.only = kind, only
        self.solvers, self.labels, self.seen, self.refused = [], [], {}, set()
        self.restricted = set()
        self.levels = []      # per position: the levels whose contexts the entry was given

    def __call__(self, label, args=()):
        pos = len(self.labels)
        self.labels.append(label)
        ctxs = [a.value for a in args[:2] if isinstance(a, C.c_void_p)]
        self.levels.append(tuple(lev for lev, s in enumerate(self.solvers)
                                 if s.ctx.value in ctxs))
        if label == "mg_restrict":       # (fine, coarse, ...): the coarse level has a state now
            self.restricted.add(args[1].value)
        if self.kind is None or not self.solvers or (self.only is not None and pos != self.only):
            return
        obs = {}
        for lev, s in enumerate(self.solvers):
            # every level of a multigrid run, a coarse one from its first restriction on
            # (before it, its state is the zeros of its allocation)
            if lev == 0 or s.ctx.value in self.restricted:
                getattr(self, "_" + self.kind)(s, lev, label, obs)
        self.seen[pos] = obs

    def _try(self, label, obs, key, fn):
        try:
            obs[key] = fn()
        except RuntimeError as exc:
            msg = str(exc)
            if FILL_OPEN.search(msg):
                assert (label, self.kind) in REFUSED_AT, (label, self.kind, msg)
                self.refused.add((label, self.kind, "fill_open"))
                return
            for reason, pat in NOT_HELD.items():
                if pat.search(msg):
                    self.refused.add((key[-1], self.kind, reason))
                    return
            raise

    def _plain(self, s, lev, label, obs):
        api = s.api
        names = [n for n in CELL_VARS if n != "viscosity" or s.cfg.is_viscous]
        for gb in s.block_ids:
            for f in PLAIN_FIELDS + tuple(abi.GEOM_FIELDS):
                self._try(label, obs, (lev, gb, f), lambda: s.download(f, gb))
            for which in (0, 1):
                self._try(label, obs, (lev, gb, "restart%d" % which),
                          lambda: s.restart_pack(gb, which))
            self._try(label, obs, (lev, gb, "cell_vars"), lambda: s.output_pack(gb, names))
        for cid in s.conn_ids:
            if cid >= 0:
                obs[(lev, cid, "halo_count")] = np.array(
                    [api.halo_count(s.ctx, cid, w) for w in (abi.HALO_STATE, abi.HALO_UPDATE)])
        api.check(api.sync(s.ctx), "sync")
        ms, n = C.c_double(0.0), C.c_int64(0)
        for grp in range(TIMING_GROUPS):
            api.check(api.timing_get(s.ctx, grp, C.byref(ms), C.byref(n)), "timing_get")

    def _aux(self, s, lev, label, obs):
        for gb in s.block_ids:
            for f in AUX_FIELDS:
                self._try(label, obs, (lev, gb, f), lambda: s.download(f, gb))

    def _ghost(self, s, lev, label, obs):
        for gb in s.block_ids:
            for f in GRAD_FIELDS:
                self._try(label, obs, (lev, gb, f), lambda: s.download(f, gb))
            self._try(label, obs, (lev, gb, "grad_vars"),
                      lambda: s.output_pack(gb, list(GRAD_VARS)))
            self._try(label, obs, (lev, gb, "node_vars"),
                      lambda: s.node_pack(gb, list(NODE_VARS)))
            if s.cfg.is_viscous and s.wall_surfaces(gb):
                self._try(label, obs, (lev, gb, "wall_vars"),
                          lambda: np.concatenate([r.ravel() for rows in s.wall_pack(
                              gb, list(WALL_VARS)).values() for r in rows]))


# ---- runs -----------------------------------------------------------------------------------
DRIVERS = ("solver", "phased", "multigrid")


def run(api, make, driver, kind=None, only=None, steps=2, timing=False):
    """One run of `steps` time steps of make()'s case on `api` under the proxy.  Returns
    (final, prober): final holds what has to be bit-identical between a probed and an unprobed
    run -- per level and block the interior state and update, residual, dt, cons_n, cons_nm1,
    and every history entry."""
    prober = Prober(kind, only)
    proxy = ProbingApi(api, prober)
    made = make()
    if driver == "solver":
        top = Solver(proxy, made)
        levels = [top]
    elif driver == "phased":
        top = PhasedSolver(proxy, made, 0, None, None)
        levels = [top]
    else:
        top = MultigridSolver(proxy, *made)
        levels = top.levels
    try:
        if timing:
            for s in levels:
                api.check(api.timing_enable(s.ctx, 1), "timing_enable")
        prober.solvers = levels
        for nn in range(steps):
            top.step(nn)
        prober.solvers = []
        final = {}
        for lev, s in enumerate(levels):
            g = s.case.ng
            for gb in s.block_ids:
                for f in ("state", "update"):
                    final[(lev, gb, f)] = s.download(f, gb)[g:-g, g:-g, g:-g]
                for f in ("residual", "dt", "cons_n", "cons_nm1"):
                    final[(lev, gb, f)] = s.download(f, gb)
        for q, h in enumerate(top.history):
            final[("history", q, "l2")] = np.array(h["l2"])
            final[("history", q, "linf")] = np.array(h["linf"], dtype=float)
            final[("history", q, "matrix")] = np.array(h["matrix"])
    finally:
        top.close()
    return final, prober


def differences(a, b):
    """{key: largest |a - b|} over the keys whose arrays are not bit-identical."""
    assert a.keys() == b.keys()
    return {k: float(np.abs(a[k] - b[k]).max()) for k in a if not np.array_equal(a[k], b[k])}


def assert_invariant(api, make, driver, kind, steps=2, timing=False, base=None):
    """The run probed by `kind` at EVERY position ends bit for bit where the unprobed run
    (`base`, or made here) ends; only when it does not, the run is repeated probed at one
    position at a time, and the failure names the first (label, kind) that disturbs it.  The
    refusals by position equal the rows of REFUSED_AT the run reaches.  Returns the probed
    run's Prober."""
    if base is None:
        base = run(api, make, driver, steps=steps, timing=timing)[0]
    final, prober = run(api, make, driver, kind, steps=steps, timing=timing)
    diff = differences(base, final)
    if diff:
        for pos, label in enumerate(prober.labels):
            one = differences(base, run(api, make, driver, kind, only=pos, steps=steps,
                                        timing=timing)[0])
            if one:
                raise AssertionError(
                    "a %s read after %s (position %d of %d, %s driver) changes the run: %r"
                    % (kind, label, pos, len(prober.labels), driver, one))
        raise AssertionError("the %s reads change the run only together (%s driver): %r"
                             % (kind, driver, diff))
    by_position = {(e, k) for e, k, why in prober.refused if why == "fill_open"}
    want = expected_refusals(prober.labels) if kind == "ghost" else set()
    assert by_position == want, (sorted(by_position), sorted(want))
    return prober
