"""Time statistics on the device: running means, Reynolds stresses and wall means.

The reference samples are what the pinned evaluators return at each sample time --
output_pack of density, vel_*, pressure, temperature, turbulentViscosity, tke, sdr, and
wall_pack -- fed through tests/stats_ref.py (the extended-precision two-pass form, with the
bound and the constants the host test measures).  Nothing of the new code is its own reference.
"""
import ctypes as C
import re

import numpy as np
import pytest

import flow_fields
import les_cases
import probe
import stats_ref
import tp_cases
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import PhasedSolver, Solver

pytestmark = pytest.mark.gpu

W5 = stats_ref.WEIGHTS
CELL = ("density", "vel_x", "vel_y", "vel_z", "pressure", "temperature")
MOM = ("mom_x", "mom_y", "mom_z")
COV = {"cov_uu": ("vel_x", "vel_x"), "cov_uv": ("vel_x", "vel_y"), "cov_uw": ("vel_x", "vel_z"),
       "cov_vv": ("vel_y", "vel_y"), "cov_vw": ("vel_y", "vel_z"), "cov_ww": ("vel_z", "vel_z"),
       "var_density": ("density", "density"), "var_pressure": ("pressure", "pressure"),
       "var_temperature": ("temperature", "temperature")}
WCOV = {"var_" + n: (n, n) for n in ("pressure", "shearStress_x", "shearStress_y",
                                      "shearStress_z")}
WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("pressureOutlet", 3),
        4: ("characteristic", 1)}
# five different fields of tests/flow_fields.py: (axis, sign, swing, dp)
FIELDS = (("i", 1, 0.35, 0.08), ("j", -1, 0.25, 0.05), ("k", 1, 0.30, 0.03),
          ("i", -1, 0.15, 0.06), ("k", -1, 0.20, 0.02))


def _lib(case):
    import aither_amd
    return aither_amd.load(case.n_eq, case.gas.thermodynamic_model)


def _extras(s):
    seven = s.cfg.n_eq == 7
    eddy = seven or s.cfg.equation_set == abi.EQN["largeEddySimulation"]
    return (("turbulentViscosity",) if eddy else ()) + (("tke", "sdr") if seven else ())


def _has_wall(s, gb):
    return bool(s.cfg.is_viscous and s.wall_surfaces(gb))


def cell_sample(s, gb):
    names = list(CELL + _extras(s))
    x = dict(zip(names, s.output_pack(gb, names)))
    for c, n in zip("xyz", MOM):
        x[n] = x["density"] * x["vel_" + c]
    return x


def wall_names(s):
    return [n for n in abi.WALL_OUT if s.cfg.n_eq == 7 or n not in ("tke", "sdr")]


def wall_sample(s, gb):
    names = wall_names(s)
    got = s.wall_pack(gb, names)
    return {n: np.concatenate([r.ravel() for r in got[n]]) for n in names}


def _flat(rows):
    return np.concatenate([r.ravel() for r in rows])


def hold_to_reference(s, gb, cells, walls, weights, what):
    """Every id of both ranges that this library and context keep, against the two-pass
    reference of the samples, within the bound of stats_ref.  Returns the largest co-moment of
    the velocities."""
    means = list(cells[0])
    names = ["mean_" + n for n in means] + list(COV)
    got = dict(zip(names, s.stats_pack(gb, names)))
    worst = _hold(got, cells, weights, means, COV, what + " cells")
    if walls:
        wmeans = list(walls[0])
        wn = ["mean_" + n for n in wmeans] + list(WCOV)
        wgot = {n: _flat(r) for n, r in s.wall_stats_pack(gb, wn).items()}
        _hold(wgot, walls, weights, wmeans, WCOV, what + " wall faces")
    return worst


def _hold(got, samples, weights, means, covs, what):
    rmean, rcov, _ = stats_ref.two_pass(samples, weights, list(covs.values()))
    big, dev = stats_ref.scales(samples, weights)
    n = len(samples)
    wm = wc = big_uu = 0.0
    for m in means:
        bound = stats_ref.C1 * n * stats_ref.ULP * big[m]
        err = float(np.abs(got["mean_" + m] - rmean[m]).max())
        wm = max(wm, err / bound if bound else err)
        assert err <= bound, (what, m, err, bound)
    for name, (a, b) in covs.items():
        bound = stats_ref.C2 * n * stats_ref.ULP * (big[a] * dev[b] + big[b] * dev[a])
        err = float(np.abs(got[name] - rcov[(a, b)]).max())
        wc = max(wc, err / bound if bound else err)
        assert err <= bound, (what, name, err, bound)
        if name.startswith("cov_"):
            big_uu = max(big_uu, float(np.abs(got[name]).max()))
    print("%s: worst mean error %.3g, worst second-moment error %.3g of the bound"
          % (what, wm, wc))
    return big_uu


def sample_and_record(s, weight, cells, walls):
    for gb in sorted(s.block_ids):
        cells.setdefault(gb, []).append(cell_sample(s, gb))
        if _has_wall(s, gb):
            walls.setdefault(gb, []).append(wall_sample(s, gb))
    s.stats_sample(weight)


# ---- 1. a sampled run against the reference ----------------------------------------------------
RUNS = {
    "les_A": lambda: les_cases.deck_a(),
    "les_C_walls": lambda: les_cases.deck_c(),
    "tp_navier_stokes": lambda: tp_cases.hot_single(**tp_cases.FIVE["weno_ausm_visc_lusgs"]),
    "rans_wall": lambda: synthetic.single_block_case(**tp_cases.RANS_BASE),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_sampled_run_against_the_reference(name):
    case = RUNS[name]()
    s = Solver(_lib(case), case)
    cells, walls = {}, {}
    for nn, w in enumerate(W5):
        s.step(nn)
        sample_and_record(s, w, cells, walls)
    assert (name != "les_A") == bool(walls)
    for gb in sorted(s.block_ids):
        uu = hold_to_reference(s, gb, cells[gb], walls.get(gb), W5, name)
        assert uu > 0.0, "the velocity co-moments are zero everywhere"
        assert s.stats_weight(gb) == (sum(W5), 5)
    s.close()


# ---- 2. shapes -----------------------------------------------------------------------------------
def _set_field(s, case, q):
    axis, sign, swing, dp = FIELDS[q]
    # (transonic_state takes its base state from the case's first cell: every field is formed
    # on the state the case was built with, whatever was set before)
    if not hasattr(case, "stats_base"):
        case.stats_base = [blk.state.copy() for blk in case.blocks]
    for blk, base in zip(case.blocks, case.stats_base):
        blk.state[...] = base
    flow_fields.transonic_state(case, axis, sign, swing=swing, dp=dp)
    for gb in sorted(s.block_ids):
        s.upload("state", gb, case.blocks[gb].state)


SHAPES = {
    # a row crossing a 64-lane wave, odd strides, an odd cell count (the pad of the pitch)
    "67x3x2_two_ghosts": lambda: synthetic.single_block_case((67, 3, 2), amplitude=0.0),
    # three ghost layers, a viscous wall, an even cell count
    "5x4x3_weno_wall": lambda: synthetic.single_block_case(
        (5, 4, 3), amplitude=0.0, stretch=1.1, bcs=WALL, equation_set="navierStokes",
        face_reconstruction="weno", limiter="none"),
    "3x3x3_odd": lambda: synthetic.single_block_case((3, 3, 3), amplitude=0.0),
    "les_D_two_blocks": lambda: les_cases.deck_d(),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    case = SHAPES[name]()
    assert case.ng == (3 if "weno" in name else 2)
    s = Solver(_lib(case), case)
    cells, walls = {}, {}
    for q, w in enumerate(W5):
        _set_field(s, case, q)
        sample_and_record(s, w, cells, walls)
    for gb in sorted(s.block_ids):
        assert hold_to_reference(s, gb, cells[gb], walls.get(gb), W5, "%s block %d" % (name, gb)) > 0
    if len(s.block_ids) > 1:
        # each block's accumulators are its own
        assert case.blocks[0].geom.n != case.blocks[1].geom.n
        before = s.stats_download(1)
        s._stat_weight(0, 0.5)
        assert np.array_equal(s.stats_download(1), before)
        assert s.stats_weight(0) == (sum(W5) + 0.5, 6) and s.stats_weight(1) == (sum(W5), 5)
    s.close()


# ---- 3. exactness ----------------------------------------------------------------------------------
def _ulps(a, exact):
    exact = np.asarray(exact, dtype=np.longdouble)
    return float((np.abs(np.asarray(a, dtype=np.longdouble) - exact) /
                  np.spacing(np.abs(exact.astype(np.float64)))).max())


@pytest.mark.parametrize("name", ["les_C_walls", "tp_navier_stokes", "rans_wall"])
def test_identical_samples_are_exact(name):
    """Three identical samples: means bit-equal to output_pack / wall_pack of the variable,
    second moments exactly 0; mean_mom within 2 ulp of the product rho u (the exact product
    of the sampled state, made dimensional; measured on the card: the figure is printed);
    doubling all weights changes no bit."""
    case = RUNS[name]()
    s = Solver(_lib(case), case)
    s.step(0)
    payloads = []
    for scale in (1.0, 2.0):
        s.stats_reset()
        for w in W5[:3]:
            s.stats_sample(scale * w)
        x = cell_sample(s, 0)
        means = [n for n in x if n not in MOM]
        got = dict(zip(means, s.stats_pack(0, ["mean_" + n for n in means])))
        for n in means:
            assert np.array_equal(got[n], x[n]), n
        assert not s.stats_pack(0, list(COV)).any()
        wx = wall_sample(s, 0)
        wgot = s.wall_stats_pack(0, ["mean_" + n for n in wx] + list(WCOV))
        for n in wx:
            assert np.array_equal(_flat(wgot["mean_" + n]), wx[n]), n
        for n in WCOV:
            assert not _flat(wgot[n]).any(), n
        payloads.append((s.stats_pack(0, list(abi.STAT_OUT)[:9] + list(COV)),
                         s.wall_stats_pack(0, ["mean_" + n for n in wx] + list(WCOV))))
    assert np.array_equal(payloads[0][0], payloads[1][0])
    for n in payloads[0][1]:
        assert np.array_equal(_flat(payloads[0][1][n]), _flat(payloads[1][1][n])), n
    # rho u_i against the exact product
    g = case.ng
    st = s.download("state", 0)[g:-g, g:-g, g:-g].astype(np.longdouble)
    fac = np.longdouble(s.cfg.gas.rho_ref) * np.longdouble(s.cfg.gas.a_ref)
    mom = s.stats_pack(0, ["mean_mom_x", "mean_mom_y", "mean_mom_z"])
    worst = max(_ulps(mom[c], st[..., 0] * st[..., 1 + c] * fac) for c in range(3))
    print("%s: mean_mom against the exact product: %.3g ulp" % (name, worst))
    assert worst <= 2.0
    s.close()


# ---- 4. resume, 6. determinism ------------------------------------------------------------------
def _sampled(case, lo, hi, start=None):
    s = Solver(_lib(case), case)
    if start is not None:
        s.stats_upload(0, start)
    for q in range(lo, hi):
        _set_field(s, case, q)
        s.stats_sample(W5[q])
    return s


def _all_stats(s):
    names = [n for n in abi.STAT_OUT if n not in ("mean_turbulentViscosity", "mean_tke",
                                                  "mean_sdr")]
    wn = [n for n in abi.WALL_STAT_OUT if n not in ("mean_tke", "mean_sdr")]
    return s.stats_pack(0, names), np.stack([_flat(r) for r in
                                             s.wall_stats_pack(0, wn).values()])


def test_resume_and_determinism():
    make = SHAPES["5x4x3_weno_wall"]
    whole = _sampled(make(), 0, 5)
    again = _sampled(make(), 0, 5)
    assert np.array_equal(whole.stats_download(0), again.stats_download(0))   # determinism
    again.close()
    first = _sampled(make(), 0, 3)
    saved = first.stats_download(0)
    first.close()
    case = make()
    rest = _sampled(case, 3, 5, start=saved.copy())
    payload = rest.stats_download(0)
    assert np.array_equal(payload, whole.stats_download(0))
    assert payload[0] == 18 and payload[1] == 18 and payload.size == 4 + 18 * 60 + 18 * 15
    assert rest.stats_weight(0) == (sum(W5), 5)
    for a, b in zip(_all_stats(rest), _all_stats(whole)):
        assert np.array_equal(a, b)
    # the payload round trip
    rest.stats_upload(0, saved)
    assert np.array_equal(rest.stats_download(0), saved)
    # a zero-weight sample starts the average anew: as a fresh context's first sample
    rest.stats_sample(0.0)
    with pytest.raises(RuntimeError, match="no sample has been taken"):
        rest.stats_download(0)
    _set_field(rest, case, 1)
    rest.stats_sample(0.5)
    fresh = _sampled(make(), 1, 2)      # (W5[1] is 0.5)
    assert np.array_equal(rest.stats_download(0), fresh.stats_download(0))
    for s in (whole, rest, fresh):
        s.close()


# ---- 5. the run is untouched ---------------------------------------------------------------------
def _final(s):
    g = s.case.ng
    out = {"state": s.download("state", 0)[g:-g, g:-g, g:-g], "residual": s.download("residual", 0)}
    for q, h in enumerate(s.history):
        out["l2", q] = np.array(h["l2"])
        out["linf", q] = np.array(h["linf"], dtype=float)
        out["matrix", q] = np.array(h["matrix"])
    return out


UNTOUCHED = {
    # bdf2 + LU-SGS on the diagonal-ordered path (dual time stepping)
    "bdf2_lusgs": lambda: synthetic.single_block_case(**tp_cases.FIVE["wenoz_roe_bdf2_dual"]),
    "rk4_walls": lambda: synthetic.single_block_case((9, 8, 7), stretch=1.15, bcs=WALL,
                                                     equation_set="navierStokes",
                                                     time_integration="rk4", cfl=0.5),
}


@pytest.mark.parametrize("name", list(UNTOUCHED))
def test_sampling_leaves_the_run_bit_identical(name):
    finals = []
    for sampled in (False, True):
        case = UNTOUCHED[name]()
        s = Solver(_lib(case), case)
        for nn in range(3):
            s.step(nn)
            if sampled:
                s.stats_sample(1.0 + nn)
        if sampled:
            assert s.stats_weight(0) == (6.0, 3)
        finals.append(_final(s))
        s.close()
    assert finals[0].keys() == finals[1].keys()
    for k in finals[0]:
        assert np.array_equal(finals[0][k], finals[1][k]), k


def _phased(case, sample):
    """Two steps of a one-rank PhasedSolver; sample=True: a sample after every phase and halo
    call.  Returns (final, {label: refused?})."""
    seen = {}
    holder = []

    def hook(label, args):
        if not sample or not holder:
            return
        try:
            holder[0].stats_sample(1.0)
            seen.setdefault(label, set()).add(False)
        except RuntimeError as exc:
            assert probe.FILL_OPEN.search(str(exc)), str(exc)
            seen.setdefault(label, set()).add(True)

    s = PhasedSolver(probe.ProbingApi(_lib(case), hook), case, 0, None, None)
    holder.append(s)
    for nn in range(2):
        s.step(nn)
    holder.clear()
    final = _final(s)
    s.close()
    return final, seen


def test_sample_between_phases():
    """A viscous block with a wall: refused from phase_bc_faces up to phase_residual with the
    text of the ghost-refilling reads, legal from phase_residual on -- and the run sampled at
    every legal position is the unsampled run.  An euler deck: legal everywhere."""
    base, _ = _phased(UNTOUCHED["rk4_walls"](), False)
    final, seen = _phased(UNTOUCHED["rk4_walls"](), True)
    closed = {lab for lab, r in seen.items() if r == {True}}
    assert closed == {"phase_bc_faces", "halo_swap_local[state]", "phase_bc_edges"}, seen
    assert seen["phase_residual"] == {False} and seen["phase_explicit_update"] == {False}
    for k in base:
        assert np.array_equal(base[k], final[k]), k
    euler = lambda: synthetic.single_block_case((9, 8, 7), stretch=1.15, time_integration="rk4")
    base, _ = _phased(euler(), False)
    final, seen = _phased(euler(), True)
    assert {"phase_bc_faces", "phase_bc_edges", "phase_residual"} <= set(seen)
    assert all(r == {False} for r in seen.values()), seen
    for k in base:
        assert np.array_equal(base[k], final[k]), k


# ---- 7. refusals -------------------------------------------------------------------------------
def _raw_pack(s, ids):
    arr = (C.c_int32 * len(ids))(*ids)
    out = np.empty(1 << 16)
    s.api.check(s.api.output_pack(s.ctx, s.block_ids[0], len(ids), arr,
                                  out.ctypes.data_as(abi.c_dp)), "output_pack")


def _raw_upload(s, field, values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    s.api.check(s.api.field_upload(s.ctx, s.block_ids[0], abi.FIELD[field],
                                   a.ctypes.data_as(abi.c_dp)), "field_upload")


def test_refusals_by_their_text():
    ns_case = SHAPES["5x4x3_weno_wall"]()
    ns = Solver(_lib(ns_case), ns_case)
    none = "no sample has been taken"
    with pytest.raises(RuntimeError, match=none):
        ns.stats_pack(0, ["mean_density"])
    with pytest.raises(RuntimeError, match=none):
        ns.wall_stats_pack(0, ["mean_pressure"])
    with pytest.raises(RuntimeError, match=none):
        ns.stats_download(0)
    for w, text in ((-1.0, "negative or not finite"), (float("nan"), "negative or not finite"),
                    (float("inf"), "negative or not finite")):
        with pytest.raises(RuntimeError, match=text):
            ns.stats_sample(w)
    ns.stats_sample(1.0)
    base, wbase = abi.STAT_BASE, abi.WSTAT_BASE
    for ids, text in (([base, 0], "cell and statistics variables in one call"),
                      ([wbase, base], "statistics and wall statistics variables in one call"),
                      ([wbase, 64], "wall and wall statistics variables in one call"),
                      ([base, 128], "node and statistics variables in one call"),
                      ([base, 256], "load and statistics variables in one call"),
                      ([base] * 22, "nvar 22 out of range"),
                      ([wbase] * 19, "nvar 19 out of range"),
                      ([533], "unknown output variable 533"),
                      ([594], "unknown output variable 594"),
                      ([575], "unknown output variable 575")):
        with pytest.raises(RuntimeError, match=re.escape(text)):
            _raw_pack(ns, ids)
    _raw_pack(ns, [base] * 21)
    _raw_pack(ns, [wbase] * 18)
    with pytest.raises(RuntimeError, match="not kept by the 5-equation libraries"):
        ns.stats_pack(0, ["mean_tke"])
    with pytest.raises(RuntimeError, match="not kept by the 5-equation libraries"):
        ns.wall_stats_pack(0, ["mean_sdr"])
    with pytest.raises(RuntimeError, match="this context has no eddy viscosity"):
        ns.stats_pack(0, ["mean_turbulentViscosity"])
    with pytest.raises(RuntimeError, match="AGX_FIELD_STAT_SAMPLE is upload only"):
        out = np.empty(8)
        ns.api.check(ns.api.field_download(ns.ctx, 0, abi.FIELD["stat_sample"],
                                           out.ctypes.data_as(abi.c_dp)), "field_download")
    payload = ns.stats_download(0)
    for slot, value, text in ((0, 19.0, "19 cell planes"), (1, 0.0, "0 wall values per face"),
                              (2, -1.0, "negative or not finite"),
                              (3, float("nan"), "negative or not finite")):
        bad = payload.copy()
        bad[slot] = value
        with pytest.raises(RuntimeError, match=text):
            _raw_upload(ns, "stat_accum", bad)
    assert np.array_equal(ns.stats_download(0), payload)      # a refused upload changed nothing
    ns.close()
    # an inviscid context; a viscous block without a viscousWall surface
    eu_case = SHAPES["3x3x3_odd"]()
    eu = Solver(_lib(eu_case), eu_case)
    eu.stats_sample(1.0)
    with pytest.raises(RuntimeError, match="wall statistics need a viscous context"):
        _raw_pack(eu, [wbase])
    assert eu.stats_download(0)[1] == 0
    eu.close()
    les_case = les_cases.deck_a()
    les = Solver(_lib(les_case), les_case)
    les.stats_sample(1.0)
    with pytest.raises(RuntimeError, match="has no viscousWall surface"):
        _raw_pack(les, [wbase])
    assert les.stats_pack(0, ["mean_turbulentViscosity"]).shape == (1, 6, 9, 66)
    assert les.stats_download(0)[0] == 19
    les.close()
