"""Time statistics collapsed along index directions on the device (AGX_CSTAT_BASE,
Solver.stats_collapse).

The reference is tests/collapse_ref.two_pass (np.longdouble) over what the pinned per-cell
evaluators return -- stats_pack of every id and AGX_FIELD_VOLUME x l_ref^3 -- with the bound and
the constants the host test measures.  Nothing of the new code is its own reference.
"""
import ctypes as C
import re

import numpy as np
import pytest

import collapse_ref as cr
import les_cases
import stats_ref
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import Solver, pool_bins

pytestmark = pytest.mark.gpu

W5 = stats_ref.WEIGHTS
OVER = {1: "i", 2: "j", 3: "ij", 4: "k", 5: "ik", 6: "jk", 7: "ijk"}
WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("pressureOutlet", 3),
        4: ("characteristic", 1)}
RANS_BCS = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
            4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}


def _lib(case):
    import aither_amd
    return aither_amd.load(case.n_eq, case.gas.thermodynamic_model)


def _names(s):
    """The ids this library and context keep."""
    seven = s.cfg.n_eq == 7
    eddy = seven or s.cfg.equation_set == abi.EQN["largeEddySimulation"]
    gone = (() if eddy else ("mean_turbulentViscosity",)) + (() if seven else ("mean_tke",
                                                                               "mean_sdr"))
    return [n for n in abi.STAT_OUT if n not in gone]


def _cells(s, gb):
    """Per cell, dimensional: ({name: [nk, nj, ni]} of every id, the volumes)."""
    names = _names(s)
    cell = dict(zip(names, s.stats_pack(gb, names)))
    g = s.case.blocks[gb].geom.ng
    vol = s.download("volume", gb)[g:-g, g:-g, g:-g, 0] * s.cfg.gas.l_ref ** 3
    return cell, vol


def _split(values):
    means = {n: v for n, v in values.items() if n.startswith("mean_")}
    coms = {abi.STAT_PAIRS[n]: v for n, v in values.items() if n in abi.STAT_PAIRS}
    return means, coms


def hold_to_reference(s, gb, mask, what, cells=None):
    """stats_collapse of every id and the volume over `mask` against two_pass of the per-cell
    values, within the bound of collapse_ref; the reached fractions are printed."""
    cell, vol = cells or _cells(s, gb)
    names = list(cell)
    got = dict(zip(names + ["volume"], s.stats_collapse(gb, names + ["volume"], OVER[mask])))
    means, coms = _split({n: cr.to_bins(a, mask) for n, a in cell.items()})
    gm, gc = _split({n: got[n] for n in names})
    vb = cr.to_bins(vol, mask)
    assert got["volume"].shape == vb.shape[:-1]
    wm, wc = cr.reached((got["volume"], gm, gc), vb, means, coms)
    # 5. the volume: the sum of the cells' within N ulp
    n = vb.shape[-1]
    ref_v = vb.astype(np.longdouble).sum(axis=-1)
    wv = float((np.abs(got["volume"] - ref_v) / (n * cr.ULP * ref_v)).max())
    print("%s mask %d (%d bins of %d cells): means %.3g, second moments %.3g of the bound, "
          "volume %.3g of N ulp" % (what, mask, vb[..., 0].size, n, wm, wc, wv))
    assert wm <= 1.0 and wc <= 1.0 and wv <= 1.0, (what, mask, wm, wc, wv)
    return got


# ---- 1. sampled runs against the reference ---------------------------------------------------------
def _ns_67():
    return synthetic.single_block_case((67, 3, 3), stretch=1.1, bcs=WALL,
                                       equation_set="navierStokes", time_integration="rk4",
                                       cfl=0.5)


def _rans_smoke():
    return synthetic.single_block_case((12, 10, 8), stretch=1.2, bcs=RANS_BCS,
                                       equation_set="rans", turbulence_model="sst2003",
                                       time_integration="implicitEuler", cfl=10.0)


RUNS = {"les_A": (les_cases.deck_a, 5, (1, 2, 3, 4, 5, 6, 7), 19),
        "ns_67x3x3": (_ns_67, 5, (1, 4, 5, 7), 18),
        "rans_12x10x8": (_rans_smoke, 3, (2, 7), 21)}


def _sampled(make, steps):
    case = make()
    s = Solver(_lib(case), case)
    for nn in range(steps):
        s.step(nn)
        s.stats_sample(W5[nn])
    return s


@pytest.mark.parametrize("name", list(RUNS))
def test_sampled_run_against_the_reference(name):
    make, steps, masks, planes = RUNS[name]
    s = _sampled(make, steps)
    cells = _cells(s, 0)
    assert len(cells[0]) == planes
    ni, nj, nk = s.case.blocks[0].geom.n
    for mask in masks:
        got = hold_to_reference(s, 0, mask, name, cells)
        rest = tuple(n for bit, n in ((4, nk), (2, nj), (1, ni)) if not mask & bit)
        assert got["cov_uu"].shape == rest
        assert (got["cov_uu"] > 0.0).all() and (got["var_pressure"] > 0.0).all()
    s.close()


# ---- 2. uploaded accumulators ------------------------------------------------------------------------
def _uploaded(n, planes_of):
    """A euler block of n cells whose accumulators are planes_of(rng, shape [18, nk, nj, ni])."""
    case = synthetic.single_block_case(n, amplitude=0.0, stretch=1.15)
    s = Solver(_lib(case), case)
    s.stats_sample(1.0)
    payload = s.stats_download(0)
    ni, nj, nk = n
    assert payload[0] == 18 and payload[1] == 0 and payload.size == 4 + 18 * ni * nj * nk
    rng = np.random.default_rng(ni * nj * nk)
    payload[4:] = planes_of(rng, (18, nk, nj, ni)).ravel()
    payload[2], payload[3] = 3.75, 5.0
    s.stats_upload(0, payload)
    return s


def _replicated(mask):
    def planes(rng, shape):
        a = rng.uniform(-1.0, 1.0, shape)
        a[0] += 2.0                     # (density, pressure and temperature away from 0)
        a[4] += 2.0
        a[5] += 2.0
        for ax, bit in enumerate(cr.AXIS_BIT):
            if mask & bit:
                a = np.repeat(np.take(a, [0], axis=1 + ax), shape[1 + ax], axis=1 + ax)
        return a
    return planes


@pytest.mark.parametrize("mask", list(OVER))
def test_cells_identical_along_the_collapsed_directions_are_exact(mask):
    """Planes replicated along the collapsed directions of a stretched block: the bin's value
    is, bit for bit, what stats_pack gives for a cell of the bin."""
    s = _uploaded((67, 5, 3), _replicated(mask))
    names = _names(s)
    vol = _cells(s, 0)[1]
    assert np.ptp(cr.to_bins(vol, mask), axis=-1).min() > 0.0      # the volumes do differ
    cell = s.stats_pack(0, names)
    got = s.stats_collapse(0, names, OVER[mask])
    first = tuple(0 if mask & bit else slice(None) for bit in cr.AXIS_BIT)
    for q, n in enumerate(names):
        assert np.array_equal(got[q], cell[q][first]), n
    s.close()


def test_small_fluctuations_stay_within_the_bound():
    """Means of 1 + 1e-8 noise, co-moments of 1e-16: the family sums of squares lose."""
    def planes(rng, shape):
        a = 1.0 + 1e-8 * rng.uniform(-1.0, 1.0, shape)
        a[9:] = 1e-16 * rng.uniform(0.0, 1.0, (9,) + shape[1:])
        return a
    s = _uploaded((67, 5, 3), planes)
    cells = _cells(s, 0)
    for mask in OVER:
        hold_to_reference(s, 0, mask, "1 + 1e-8 noise", cells)
    s.close()


# ---- 3. a bin that crosses the chunk -----------------------------------------------------------------
def test_a_bin_larger_than_the_chunk():
    """130 x 20 x 15: over "jk" a bin marches 300 (j, k) positions, four chunks of
    abi.CSTAT_CHUNK = 64 and one of 44; over "ijk" the 300 rows of 130 cells (two cells per lane
    and a short third)."""
    assert abi.CSTAT_CHUNK == 64 and 20 * 15 > abi.CSTAT_CHUNK and (20 * 15) % abi.CSTAT_CHUNK
    def planes(rng, shape):
        a = rng.uniform(-1.0, 1.0, shape)
        a[0] += 2.0
        a[4] += 2.0
        a[5] += 2.0
        a[9:] = rng.uniform(0.0, 1.0, (9,) + shape[1:])
        return a
    s = _uploaded((130, 20, 15), planes)
    cells = _cells(s, 0)
    for mask in (6, 7, 2, 5):
        hold_to_reference(s, 0, mask, "130x20x15", cells)
    s.close()


# ---- 4. determinism, and the run is untouched --------------------------------------------------------
def test_determinism_subsets_and_the_run():
    finals = []
    for collapse in (False, True):
        case = les_cases.deck_a()
        s = Solver(_lib(case), case)
        for nn in range(5):
            s.step(nn)
            s.stats_sample(W5[nn])
            if collapse:
                for mask in (1, 6, 7):
                    s.stats_collapse(0, _names(s) + ["volume"], OVER[mask])
        finals.append(dict(state=s.download("state", 0), residual=s.download("residual", 0),
                           stats=s.stats_download(0),
                           l2=np.array([h["l2"] for h in s.history])))
        if not collapse:
            s.close()
    for k in finals[0]:
        assert np.array_equal(finals[0][k], finals[1][k]), k
    names = _names(s) + ["volume"]
    for mask in OVER:
        over = OVER[mask]
        whole = s.stats_collapse(0, names, over)
        assert np.array_equal(whole, s.stats_collapse(0, names, over))
        back = s.stats_collapse(0, names[::-1], over)
        assert np.array_equal(back[::-1], whole)
        pick = [names.index(n) for n in ("cov_uv", "mean_pressure", "cov_uv", "volume",
                                         "var_temperature")]
        some = s.stats_collapse(0, [names[q] for q in pick], over)
        assert np.array_equal(some, whole[pick])
        for q in (0, 12, len(names) - 1):
            assert np.array_equal(s.stats_collapse(0, [names[q]], over)[0], whole[q])
    s.close()


# ---- 6. two blocks -------------------------------------------------------------------------------------
def test_two_blocks_joined_by_pool_bins():
    """Deck D is deck A cut at i = 31.  A's accumulators after five sampled steps, cut there and
    uploaded into D's blocks, collapsed over "i" block by block and joined by pool_bins,
    against A's own collapse and against the reference of A's cells."""
    a = _sampled(les_cases.deck_a, 5)
    payload = a.stats_download(0)
    ni, nj, nk = les_cases.N_A
    planes = payload[4:].reshape(19, nk, nj, ni)
    case = les_cases.deck_d()
    d = Solver(_lib(case), case)
    d.stats_sample(1.0)
    cut = les_cases.CUT
    for gb, sl in enumerate((slice(0, cut), slice(cut, ni))):
        d.stats_upload(gb, np.concatenate([payload[:4], planes[..., sl].ravel()]))
    names = _names(a)
    parts = []
    for gb in range(2):
        got = dict(zip(names + ["volume"], d.stats_collapse(gb, names + ["volume"], "i")))
        assert got["volume"].shape == (nk, nj)
        means = {n: got[n] for n in names if n.startswith("mean_")}
        covs = {n: got[n] for n in names if n in abi.STAT_PAIRS}
        parts.append((got["volume"], means, covs))
    vol, means, covs = pool_bins(parts)
    cell, cvol = _cells(a, 0)
    cm, cc = _split({n: cr.to_bins(x, 1) for n, x in cell.items()})
    pooled = (vol, means, {abi.STAT_PAIRS[n]: c for n, c in covs.items()})
    wm, wc = cr.reached(pooled, cr.to_bins(cvol, 1), cm, cc)
    print("two blocks joined: means %.3g, second moments %.3g of the bound" % (wm, wc))
    assert wm <= 1.0 and wc <= 1.0
    # ... and against A's own collapse
    own = dict(zip(names + ["volume"], a.stats_collapse(0, names + ["volume"], "i")))
    bm, bc = cr.bounds(cr.to_bins(cvol, 1), cm, cc)
    assert np.allclose(vol, own["volume"], rtol=ni * cr.ULP, atol=0.0)
    for n in means:
        assert (np.abs(means[n] - own[n]) <= bm[n]).all(), n
    for n in covs:
        assert (np.abs(covs[n] - own[n]) <= bc[abi.STAT_PAIRS[n]]).all(), n
    a.close()
    d.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------
def _raw_pack(s, ids, out=None):
    arr = (C.c_int32 * len(ids))(*ids)
    out = np.empty(1 << 12) if out is None else out
    s.api.check(s.api.output_pack(s.ctx, s.block_ids[0], len(ids), arr,
                                  out.ctypes.data_as(abi.c_dp)), "output_pack")
    return out


def test_refusals_by_their_text():
    case = synthetic.single_block_case((5, 4, 3), amplitude=0.0, stretch=1.1, bcs=WALL,
                                       equation_set="navierStokes")
    s = Solver(_lib(case), case)
    cid = abi.cstat_id
    with pytest.raises(RuntimeError, match="no sample has been taken"):
        s.stats_collapse(0, ["mean_density"], "k")
    s.stats_sample(1.0)
    one = cid(1, "mean_density")
    refused = (
        ([abi.CSTAT_BASE + 3], "mask 0"),
        ([abi.CSTAT_BASE + 32 * 8], "mask 8"),
        ([abi.CSTAT_BASE + 32 * 31 + 21], "mask 31"),
        ([abi.CSTAT_BASE + 32 * 3 + 22], "n = 22"),
        ([abi.CSTAT_BASE + 32 * 7 + 31], "n = 31"),
        ([one, cid(2, "mean_density")], "masks 1 and 2 in one call"),
        ([one, abi.OUT["density"]], "cell and collapsed statistics variables in one call"),
        ([abi.WALL_OUT["density"], one], "wall and collapsed statistics variables in one call"),
        ([one, abi.NODE_OUT["density"]], "node and collapsed statistics variables in one call"),
        ([one, abi.LOAD_OUT["area"]], "load and collapsed statistics variables in one call"),
        ([one, abi.STAT_BASE], "statistics and collapsed statistics variables in one call"),
        ([abi.WSTAT_BASE, one],
         "wall statistics and collapsed statistics variables in one call"),
        ([one] * 23, "nvar 23 out of range"),
        ([cid(4, "mean_turbulentViscosity")], "this context has no eddy viscosity"),
        ([cid(4, "mean_tke")], "not kept by the 5-equation libraries"),
        ([cid(7, "mean_density"), cid(7, "mean_sdr")], "not kept by the 5-equation libraries"),
        ([abi.CSTAT_BASE + 32 * 32], "unknown output variable 2048"),
        ([abi.CSTAT_BASE - 1], "unknown output variable 1023"),
    )
    for ids, text in refused:
        out = np.full(1 << 12, np.nan)
        with pytest.raises(RuntimeError, match=re.escape(text)):
            _raw_pack(s, ids, out)
        assert np.isnan(out).all(), text          # nothing written
    assert not np.isnan(_raw_pack(s, [one] * 22)[:22 * 12]).any()
    with pytest.raises(ValueError, match="collapsed directions"):
        s.stats_collapse(0, ["mean_density"], "x")
    assert s.stats_collapse(0, ["volume"], "ijk").shape == (1,)
    assert s.stats_collapse(0, ["volume", "cov_uu"], "j").shape == (2, 3, 5)
    # the statistics go, and the call is refused again
    s.stats_reset()
    with pytest.raises(RuntimeError, match="no sample has been taken"):
        s.stats_collapse(0, ["volume"], "ijk")
    s.close()
