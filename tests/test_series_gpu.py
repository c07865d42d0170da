"""Time series at chosen cells and wall faces, recorded on the device.

The reference of a sampled row is what the pinned evaluators return at the same moment --
output_pack and wall_pack -- at the planned points: the same evaluator on the same operands,
so the expectation is equality bit for bit.  The reference of the nearest-cell search is
tests/series_ref.py on the downloaded centres.
"""
import numpy as np
import pytest

import les_cases
import probe
import series_ref
import tp_cases
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import PhasedSolver, Solver, pool_series

pytestmark = pytest.mark.gpu

N = (7, 5, 3)
WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("pressureOutlet", 3),
        4: ("characteristic", 1)}
RANS_ONLY = ("tke", "sdr", "f1", "f2", "tkeGrad_x", "tkeGrad_y", "tkeGrad_z", "omegaGrad_x",
             "omegaGrad_y", "omegaGrad_z", "resid_tke", "resid_sdr")
PLAIN = ["pressure", "vel_x", "vel_y", "vel_z", "density"]
VELGRAD = [n for n in abi.OUT if n.startswith("velGrad_")]

DECKS = {
    # the 5-equation library, navierStokes, a low-Re wall at j-min
    "navier_stokes": lambda: synthetic.single_block_case(
        N, stretch=1.15, skew=0.01, bcs=WALL, equation_set="navierStokes",
        time_integration="rk4", cfl=0.5),
    # largeEddySimulation: turbulentViscosity is the WALE eddy viscosity (7 x 5 x 9, two walls)
    "les": lambda: les_cases.deck_c(),
    # the thermally perfect library, vibrational mode excited: cp, cv, energy of T
    "tp_hot": lambda: tp_cases.hot_single(n=N, stretch=1.15, skew=0.01, bcs=WALL,
                                          equation_set="navierStokes", time_integration="rk4",
                                          cfl=0.5),
    # the rans library with wall functions: tke, sdr, f1, f2, the stored wall data
    "rans_wall_law": lambda: synthetic.single_block_case(
        **dict(tp_cases.RANS_BASE, matrix_solver="lusgs", wall_treatment="wallLaw")),
}


def _lib(case):
    import aither_amd
    return aither_amd.load(case.n_eq, case.gas.thermodynamic_model)


def cell_names(s):
    """every cell variable this library and context keep"""
    return [n for n in abi.OUT
            if (s.cfg.n_eq == 7 or n not in RANS_ONLY) and (s.cfg.is_viscous or n != "viscosity")]


def wall_names(s):
    return [n for n in abi.WALL_OUT if s.cfg.n_eq == 7 or n not in ("tke", "sdr")]


def points_67(n, seed=3):
    """67 cells of a block of n cells: the two corners whose gradients reach into the ghost
    cells, one cell twice in a row, the rest drawn with repetition"""
    ni, nj, nk = n
    rng = np.random.default_rng(seed)
    pts = [(0, 0, 0), (ni - 1, nj - 1, nk - 1), (3, 2, 1), (3, 2, 1)]
    while len(pts) < 67:
        pts.append((int(rng.integers(ni)), int(rng.integers(nj)), int(rng.integers(nk))))
    return np.array(pts)


def at_cells(pack, pts):
    return pack[:, pts[:, 2], pts[:, 1], pts[:, 0]]


def wall_flat(s, gb, names):
    got = s.wall_pack(gb, names)
    return np.stack([np.concatenate([r.ravel() for r in got[n]]) for n in names])


def cp_operations(case):
    """cp of the thermally perfect library is the one variable whose bits may differ: it is
    cv + R with cv = R (n + cvv), which the compiler contracts into one fma where cv itself is
    not asked for by the same thread (k_series_cells: one variable per thread) and leaves as a
    product and a sum where it is (k_output_pack: every variable per thread).  Floating-point
    operations between the loaded state and the result, counted in the evaluator
    (k_series_cells, out_point, cv_of, vib_terms, out_value): T = p / (rho R): 2; 1 / T: 1; per
    vibrational mode x = theta / T, exp, expm1 with its sign, r = em / om, x x r / om (3) and
    the sum: 8; cv = R (n + cvv): 2; cp = cv + R: 1; cp aR aR / tR: 3.  On the card the two
    differ by one unit in the last place, 0.05 of the bound (printed)."""
    return 2 + 1 + 8 * case.gas.n_vib + 2 + 1 + 3


def hold_bits(names, got, ref, what, bounded=None):
    """got, ref: [V, P].  Equality bit for bit, variable by variable; every difference is
    printed before the assertion.  bounded: {name: (n, largest magnitude of the variable over
    the block)} for a variable held to n x 2^-52 x that magnitude instead."""
    bad = []
    for n, a, b in zip(names, got, ref):
        if bounded and n in bounded:
            ops, big = bounded[n]
            err = float(np.abs(a - b).max())
            print("%s: %s held to %d x 2^-52 x %.6g: worst error %.3g of the bound"
                  % (what, n, ops, big, err / (ops * 2.0 ** -52 * big)))
            if err > ops * 2.0 ** -52 * big:
                bad.append(n)
        elif not np.array_equal(a, b):
            bad.append(n)
            print("%s: %s differs: max |diff| %.3g, max |ref| %.3g"
                  % (what, n, float(np.abs(a - b).max()), float(np.abs(b).max())))
    assert not bad, (what, bad)


def sample_cells(s, gb, names, pts, t=0.0):
    s.series_plan(gb, names, pts, 2)
    s.series_sample(t)
    tt, vals = s.series_rows(gb)
    assert tt.tolist() == [t] and vals.shape == (1, len(names), len(pts))
    return vals[0]


# ---- 1. the values are the pack's --------------------------------------------------------------
@pytest.mark.parametrize("name", list(DECKS))
def test_values_are_the_packs(name):
    case = DECKS[name]()
    s = Solver(_lib(case), case)
    for nn in range(3):
        s.step(nn)
    n = case.blocks[0].geom.n
    names, pts = cell_names(s), points_67(n)
    assert set(VELGRAD) <= set(names) and "resid_energy" in names
    if name == "les":
        assert "turbulentViscosity" in names
    if name == "rans_wall_law":
        assert {"tke", "sdr", "f1", "resid_sdr", "omegaGrad_z"} <= set(names)
    got = sample_cells(s, 0, names, pts, t=1.5)
    pack = s.output_pack(0, names)
    ref = at_cells(pack, pts)
    assert np.abs(ref[names.index("velGrad_vx")]).max() > 0.0
    if name in ("les", "rans_wall_law"):
        assert np.abs(ref[names.index("turbulentViscosity")]).max() > 0.0
    bounded = None
    if name == "tp_hot":
        assert case.gas.n_vib >= 1
        bounded = {"cp": (cp_operations(case), float(np.abs(pack[names.index("cp")]).max()))}
    hold_bits(names, got, ref, name + " cells", bounded)
    # the wall faces: every face of every wall surface, and one face twice
    wn = wall_names(s)
    faces = sum(int(np.prod(w["shape"])) for w in s.wall_surfaces(0))
    assert faces > 1
    fpts = np.array(list(range(faces)) + [faces // 2])
    s.series_plan(0, wn, fpts, 2, kind="wall")
    s.series_sample(2.5)
    tt, vals = s.series_rows(0)
    assert tt.tolist() == [2.5]
    ref = wall_flat(s, 0, wn)[:, fpts]
    assert np.abs(ref[wn.index("shearStress")]).max() > 0.0
    hold_bits(wn, vals[0], ref, name + " wall faces")
    s.close()


# ---- 2. shapes ---------------------------------------------------------------------------------
def test_shapes_one_point_and_a_wave_crossing_plan():
    case = DECKS["navier_stokes"]()
    assert case.ng == 2
    s = Solver(_lib(case), case)
    s.step(0)
    pack = s.output_pack(0, PLAIN + VELGRAD)
    # P = 1, V = 1
    got = sample_cells(s, 0, ["velGrad_wy"], np.array([(6, 4, 2)]))
    assert got.shape == (1, 1) and got[0, 0] == pack[5 + VELGRAD.index("velGrad_wy"), 2, 4, 6]
    # P = 67, V = 5: 335 threads, across waves and a workgroup
    pts = points_67(N)
    got = sample_cells(s, 0, PLAIN, pts)
    hold_bits(PLAIN, got, at_cells(pack[:5], pts), "67 x 5")
    assert np.array_equal(got[:, 2], got[:, 3])                  # the same cell twice
    # the gradients of the two corners reach into the ghost cells
    got = sample_cells(s, 0, VELGRAD, pts[:2])
    hold_bits(VELGRAD, got, at_cells(pack[5:], pts[:2]), "corner gradients")
    s.close()


def test_two_blocks_with_plans_of_different_kinds():
    case = synthetic.stacked_blocks_case(N, nblocks=2, axis="k", stretch=1.15, bcs=WALL,
                                         equation_set="navierStokes", time_integration="rk4",
                                         cfl=0.5)
    s = Solver(_lib(case), case)
    s.step(0)
    pts = points_67(N, seed=5)[:9]
    wn = wall_names(s)
    faces = sum(int(np.prod(w["shape"])) for w in s.wall_surfaces(1))
    fpts = np.arange(faces)[::-1]
    s.series_plan(0, PLAIN + VELGRAD, pts, 4)
    s.series_plan(1, wn, fpts, 3, kind="wall")
    for t in (0.25, 0.5):
        s.series_sample(t)
    t0, v0 = s.series_rows(0)
    t1, v1 = s.series_rows(1)
    assert t0.tolist() == t1.tolist() == [0.25, 0.5]
    assert np.array_equal(v0[0], v0[1]) and np.array_equal(v1[0], v1[1])   # nothing moved
    hold_bits(PLAIN + VELGRAD, v0[1], at_cells(s.output_pack(0, PLAIN + VELGRAD), pts), "block 0")
    hold_bits(wn, v1[1], wall_flat(s, 1, wn)[:, fpts], "block 1")
    # each block's record is its own
    s.series_drop(0)
    assert s.series_rows(0)[0].size == 0 and s.series_rows(1)[0].size == 2
    s.series_clear()
    with pytest.raises(RuntimeError, match="has no plan"):
        s.series_rows(1)
    s.close()


# ---- 3. the ring -------------------------------------------------------------------------------
def test_the_ring_wraps_and_refuses_when_full():
    case = DECKS["navier_stokes"]()
    s = Solver(_lib(case), case)
    pts = points_67(N)[:5]
    s.series_plan(0, PLAIN, pts, 3)
    ring, rows = series_ref.Ring(3), {}

    def sample(t):
        s.step(len(rows))
        rows[t] = at_cells(s.output_pack(0, PLAIN), pts)
        s.series_sample(t)
        ring.sample(t)

    def check():
        tt, vals = s.series_rows(0)
        assert tt.tolist() == ring.rows
        for t, v in zip(tt, vals):
            assert np.array_equal(v, rows[t]), t

    for t in (0.0, 1.0, 2.0):
        sample(t)
    check()
    with pytest.raises(RuntimeError, match="is full .*collect the rows first"):
        s.series_sample(3.0)
    check()                                              # nothing was overwritten
    with pytest.raises(RuntimeError, match="cannot drop 4 rows"):
        s.series_drop(0, 4)
    s.series_drop(0, 2)
    ring.drop(2)
    check()
    sample(3.0), sample(4.0)                             # the record has wrapped
    assert ring.rows == [2.0, 3.0, 4.0]
    check()
    with pytest.raises(RuntimeError, match="is full"):
        s.series_sample(5.0)
    # a plan upload clears the rows
    s.series_plan(0, PLAIN, pts, 3)
    assert s.series_rows(0)[0].size == 0
    s.series_sample(6.0)
    assert s.series_rows(0)[0].tolist() == [6.0]
    # the plan comes back as uploaded
    back = s._series_down(0, "series_plan", 4 + 5 + 15, "series_plan")
    assert np.array_equal(back, abi.series_plan(PLAIN, pts, 3))
    # P = 0 frees; a sample then refuses
    s.series_plan(0, PLAIN, [], 3)
    with pytest.raises(RuntimeError, match="AGX_FIELD_SERIES_SAMPLE: block 0 has no plan"):
        s._series_up(0, "series_sample", np.array([7.0]), "series_sample")
    s.series_sample(7.0)                                 # (no block has a plan: nothing to do)
    s.close()


# ---- 4. determinism, 5. a sample is a read ----------------------------------------------------
def _plan_all(s):
    """every cell variable the context keeps, gradients included, on every block"""
    for gb in sorted(s.block_ids):
        n = s.case.blocks[gb].geom.n
        s.series_plan(gb, cell_names(s), points_67(n)[:12], 8)


def _final(s):
    g = s.case.ng
    out = {"state": s.download("state", 0)[g:-g, g:-g, g:-g], "residual": s.download("residual", 0)}
    for q, h in enumerate(s.history):
        out["l2", q] = np.array(h["l2"])
        out["linf", q] = np.array(h["linf"], dtype=float)
        out["matrix", q] = np.array(h["matrix"])
    return out


def _run(name, sampled, kind="cells"):
    case = DECKS[name]()
    s = Solver(_lib(case), case)
    records = []
    for nn in range(3):
        s.step(nn)
        if not sampled:
            continue
        if nn == 0:
            if kind == "cells":
                _plan_all(s)
            else:
                faces = sum(int(np.prod(w["shape"])) for w in s.wall_surfaces(0))
                s.series_plan(0, wall_names(s), np.arange(faces), 8, kind="wall")
        s.series_sample(float(nn))
    if sampled:
        records = s.series_rows(0)
        assert records[0].tolist() == [0.0, 1.0, 2.0]
    final = _final(s)
    s.close()
    return final, records


@pytest.mark.parametrize("name", list(DECKS))
def test_sampling_leaves_the_run_bit_identical_and_is_deterministic(name):
    base, _ = _run(name, False)
    for kind in ("cells", "wall"):
        first, rows1 = _run(name, True, kind)
        assert base.keys() == first.keys()
        for k in base:
            assert np.array_equal(base[k], first[k]), (kind, k)
        _, rows2 = _run(name, True, kind)
        assert np.array_equal(rows1[1], rows2[1]), kind
        assert not np.array_equal(rows1[1][0], rows1[1][2])      # the signal moves


PHASED = lambda: synthetic.single_block_case((9, 8, 7), stretch=1.15, bcs=WALL,
                                             equation_set="navierStokes",
                                             time_integration="rk4", cfl=0.5)


def _phased(plan):
    """Two steps of a one-rank PhasedSolver; plan: None, or (names, points, kind) sampled after
    every phase and halo call.  Returns (final, {label: {refused?}}); a sample that is taken is
    held against the pack at that position."""
    seen, holder = {}, []

    def hook(label, args):
        if plan is None or not holder:
            return
        s = holder[0]
        names, pts, kind = plan
        try:
            s.series_sample(1.0)
        except RuntimeError as exc:
            assert probe.FILL_OPEN.search(str(exc)), str(exc)
            seen.setdefault(label, set()).add(True)
            return
        seen.setdefault(label, set()).add(False)
        vals = s.series_rows(0)[1]
        s.series_drop(0)
        assert vals.shape[0] == 1
        if kind == "cells" and not set(names) & set(VELGRAD):
            hold_bits(names, vals[0], at_cells(s.output_pack(0, names), pts), label)

    case = PHASED()
    s = PhasedSolver(probe.ProbingApi(_lib(case), hook), case, 0, None, None)
    if plan is not None:
        s.series_plan(0, plan[0], plan[1], 2, kind=plan[2])
    holder.append(s)
    for nn in range(2):
        s.step(nn)
    holder.clear()
    final = _final(s)
    s.close()
    return final, seen


def test_sample_between_phases():
    """A plan with gradient ids and a wall plan: refused exactly between phase_bc_faces and
    phase_residual, with the text of the ghost-refilling reads.  A plan of plain cell variables:
    accepted there too, delivering what output_pack delivers there.  Every sampled run is the
    unsampled run bit for bit."""
    base, _ = _phased(None)
    pts = points_67((9, 8, 7))[:10]
    closed = {"phase_bc_faces", "halo_swap_local[state]", "phase_bc_edges"}
    for plan in ((PLAIN + VELGRAD, pts, "cells"), (["shearStress_x", "pressure"],
                                                   np.arange(9 * 7), "wall")):
        final, seen = _phased(plan)
        assert {lab for lab, r in seen.items() if r == {True}} == closed, seen
        assert seen["phase_residual"] == {False} and seen["phase_explicit_update"] == {False}
        for k in base:
            assert np.array_equal(base[k], final[k]), (plan[2], k)
    final, seen = _phased((PLAIN + ["temperature", "resid_energy", "dt"], pts, "cells"))
    assert closed | {"phase_residual"} <= set(seen)
    assert all(r == {False} for r in seen.values()), seen
    for k in base:
        assert np.array_equal(base[k], final[k]), k


# ---- 6. locate ---------------------------------------------------------------------------------
def _centres(s, gb):
    g = s.case.ng
    return s.download("center", gb)[g:-g, g:-g, g:-g]


def hold_located(got, ref, what):
    """indices exactly; d2 to 4 x 2^-52 relative: three products and two sums, contracted or
    not"""
    assert np.array_equal(got[:, :3], ref[:, :3]), what
    err = np.abs(got[:, 3] - ref[:, 3])
    print("%s: worst d2 error %.3g of the bound" %
          (what, float((err / (4 * 2.0 ** -52 * ref[:, 3] + 1e-300)).max())))
    assert (err <= 4 * 2.0 ** -52 * ref[:, 3]).all(), what


def _cloud(center, count, seed):
    """points inside the block's box, drawn from a generator (no two cells are equally near but
    by accident: the reference would tell), and a few far outside"""
    rng = np.random.default_rng(seed)
    lo, hi = center.reshape(-1, 3).min(0), center.reshape(-1, 3).max(0)
    pts = lo + (hi - lo) * rng.random((count, 3))
    if count >= 8:
        pts[-4:] = lo + (hi - lo) * np.array([(40.0, -30.0, 2.0), (-1e6, 0.5, 0.5),
                                              (0.5, 3e9, -2e9), (-7.0, -8.0, -9.0)])
    return pts


def _no_near_ties(center, pts):
    """keeps the points whose two smallest distances are apart by more than the bound on d2:
    there a contracted and an uncontracted sum pick the same cell"""
    flat = center.reshape(-1, 3)
    keep = []
    for x in pts:
        d2 = np.sort(((flat - x) ** 2).sum(axis=1))
        keep.append(d2[1] - d2[0] > 64 * 2.0 ** -52 * d2[1])
    return pts[np.array(keep)]


@pytest.mark.parametrize("n", [(7, 5, 3), (9, 8, 7)])
def test_locate_against_the_reference(n):
    assert int(np.prod(n)) in (105, 504)
    case = synthetic.single_block_case(n, stretch=1.3, skew=0.05)
    s = Solver(_lib(case), case)
    center = _centres(s, 0)
    for count, seed in ((1, 1), (300, 2)):
        pts = _no_near_ties(center, _cloud(center, count, seed))
        assert len(pts) >= max(1, count - 2)
        got = s.series_locate(pts)
        assert got.shape == (len(pts), 5) and not got[:, 0].any()
        hold_located(got[:, 1:], series_ref.nearest(center, pts), "%s, %d points" % (n, count))
    # the located cells, fed to a plan, sample what output_pack holds there
    s.step(0)
    s.series_plan_located(got, PLAIN, 2)
    s.series_sample(0.0)
    cells = got[:, 1:4].astype(int)
    hold_bits(PLAIN, s.series_rows(0)[1][0], at_cells(s.output_pack(0, PLAIN), cells), "located")
    s.close()


def _power_of_two_box(nblocks=1):
    """series_ref.tie_box as blocks: 4 x 3 x 2 cells of spacing 0.5 each, stacked along k (not
    connected: nothing iterates here)"""
    from aither_amd.case import builder
    ni, nj, nk = 4, 3, 2
    deck = synthetic.make_deck()
    deck.bcs = [synthetic.box_surfaces(ni, nj, nk) for _ in range(nblocks)]
    coords = [synthetic.box_nodes(ni, nj, nk, lengths=(2.0, 1.5, 1.0), origin=(0.0, 0.0, 1.0 * b))
              for b in range(nblocks)]
    return builder.build_case(None, deck=deck, coords=coords)


def test_locate_exact_ties():
    """the tie cases of the host test: points on the face midpoints, edge midpoints and corners
    of the cells of a box whose spacing is a power of two; d2 is exact with or without
    contraction, so indices and d2 are held exactly"""
    case = _power_of_two_box()
    s = Solver(_lib(case), case)
    center = _centres(s, 0)
    ref_center, pts = series_ref.tie_box()
    assert np.array_equal(center, ref_center)
    assert len(pts) == 9 * 7 * 5
    got = s.series_locate(pts)
    assert np.array_equal(got[:, 1:], series_ref.nearest(center, pts))
    s.close()


def test_locate_over_two_blocks_picks_the_lower_on_the_shared_plane():
    case = _power_of_two_box(2)
    s = Solver(_lib(case), case)
    c0, c1 = _centres(s, 0), _centres(s, 1)
    top, bottom = c0[-1, 1, 2], c1[0, 1, 2]
    assert np.array_equal(top[:2], bottom[:2])
    zmid = 0.5 * (top[2] + bottom[2])
    assert zmid - top[2] == bottom[2] - zmid                     # exactly on the shared plane
    pts = np.array([(top[0], top[1], zmid), tuple(bottom), tuple(top)])
    got = s.series_locate(pts)
    ref = series_ref.join({0: series_ref.nearest(c0, pts), 1: series_ref.nearest(c1, pts)})
    assert np.array_equal(got, ref)
    assert got[:, 0].tolist() == [0.0, 1.0, 0.0] and got[1, 4] == 0.0 and got[0, 4] > 0.0
    # pool_series is the same join
    one = [np.column_stack([np.full(3, float(gb)), series_ref.nearest(c, pts)])
           for gb, c in ((1, c1), (0, c0))]
    assert np.array_equal(pool_series(one), ref)
    s.close()


# ---- 7. refusals -------------------------------------------------------------------------------
def _refused(s, field, payload, text, gb=0):
    with pytest.raises(RuntimeError, match=text):
        s._series_up(gb, field, np.asarray(payload, dtype=float), field)


def test_refusals_by_their_text():
    ns_case = DECKS["navier_stokes"]()
    ns = Solver(_lib(ns_case), ns_case)
    no_plan = "has no plan"
    _refused(ns, "series_sample", [0.0], no_plan)
    _refused(ns, "series_rows", [0.0], no_plan)
    for field in ("series_plan", "series_rows"):
        with pytest.raises(RuntimeError, match=no_plan):
            ns._series_down(0, field, 64, field)
    with pytest.raises(RuntimeError, match="has located no points"):
        ns._series_down(0, "series_locate", 64, "series_locate")
    with pytest.raises(RuntimeError, match="AGX_FIELD_SERIES_SAMPLE is upload only"):
        ns._series_down(0, "series_sample", 64, "series_sample")
    good = abi.series_plan(["pressure"], [(1, 1, 1)], 2)
    cases = (
        (0, 2.0, r"entry 0 \(kind"), (1, -1.0, r"entry 1 \(P"), (1, 1.5, r"entry 1 \(P"),
        (2, 55.0, r"entry 2 \(V.*is 55"), (2, 0.0, r"entry 2 \(V"),
        (3, 0.0, r"entry 3 \(capacity"), (3, float("nan"), r"entry 3 \(capacity"),
        (4, 54.0, "entry 4: unknown output variable 54"),
        (4, 64.0, "entry 4: unknown output variable 64"),
        (4, float(abi.OUT["tke"]), "not kept by the 5-equation libraries"),
        (4, float(abi.OUT["resid_sdr"]), "not kept by the 5-equation libraries"),
        (5, 7.0, r"entry 5 \(i of a cell\) is 7"), (6, -1.0, r"entry 6 \(j of a cell\)"),
        (7, float("inf"), r"entry 7 \(k of a cell\)"), (7, 3.0, r"entry 7 \(k of a cell\) is 3"))
    for slot, value, text in cases:
        bad = good.copy()
        bad[slot] = value
        _refused(ns, "series_plan", bad, text)
    wall = abi.series_plan(["pressure"], [0], 2, kind="wall")
    for slot, value, text in ((4, 0.0, "entry 4: unknown output variable 0"),
                              (4, 78.0, "entry 4: unknown output variable 78"),
                              (4, 73.0, r"wall variable 73 \(tke, sdr\) is not kept"),
                              (5, 21.0, r"entry 5 \(a face of the wall payload\) is 21")):
        bad = wall.copy()
        bad[slot] = value
        _refused(ns, "series_plan", bad, text)
    # a refused upload left no plan behind; an accepted one is replaced only by an accepted one
    _refused(ns, "series_sample", [0.0], no_plan)
    ns._series_up(0, "series_plan", good, "series_plan")
    bad = good.copy()
    bad[3] = 0.0
    _refused(ns, "series_plan", bad, "capacity")
    assert np.array_equal(ns._series_down(0, "series_plan", good.size, "series_plan"), good)
    _refused(ns, "series_sample", [float("nan")], "is not finite")
    _refused(ns, "series_rows", [1.0], "cannot drop 1 rows")
    _refused(ns, "series_rows", [0.5], "cannot drop 0.5 rows")
    _refused(ns, "series_locate", [0.0, 1, 2, 3], r"entry 0 \(P")
    _refused(ns, "series_locate", [2.0, 1, 2, 3, 4, float("nan"), 6],
             r"entry 5 \(coordinate 1 of point 1\)")
    _refused(ns, "series_locate", [1.0, 1e151, 2, 3], r"entry 1 \(coordinate 0 of point 0\)")
    # the wall surfaces of the block are set again: a wall plan is of the payload it was made for
    ns.series_plan(0, ["pressure"], [0, 20], 2, kind="wall")
    ns.series_sample(0.0)
    from aither_amd.case import builder
    surfs = builder.surface_structs(ns_case, 0)
    ns.api.check(ns.api.block_set_bcs(ns.ctx, 0, len(surfs), surfs), "block_set_bcs")
    _refused(ns, "series_sample", [1.0], "wall surfaces of block 0 changed since its plan")
    ns.series_plan(0, ["pressure"], [0, 20], 2, kind="wall")
    ns.series_sample(1.0)
    ns.close()
    # an inviscid context: no viscosity, no wall variables
    eu_case = synthetic.single_block_case(N, amplitude=0.02)
    eu = Solver(_lib(eu_case), eu_case)
    _refused(eu, "series_plan", abi.series_plan(["viscosity"], [(0, 0, 0)], 1),
             "only kept for viscous runs")
    _refused(eu, "series_plan", wall, "wall variables need a viscous context")
    eu.close()
    # a viscous block without a viscousWall surface
    les_case = les_cases.deck_a()
    les = Solver(_lib(les_case), les_case)
    _refused(les, "series_plan", wall, "block 0 has no viscousWall surface")
    les.close()
    # wall-law surfaces before the first residual
    wl_case = DECKS["rans_wall_law"]()
    wl = Solver(_lib(wl_case), wl_case)
    wl.series_plan(0, ["yplus"], [0], 2, kind="wall")
    _refused(wl, "series_sample", [0.0], "hold no wall data before the first residual")
    wl.step(0)
    wl.series_sample(0.0)
    wl.close()
