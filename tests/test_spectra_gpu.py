"""Spectra along homogeneous directions, accumulated on the device.

The reference is tests/spectra_ref.py::reference -- the definition in longdouble, the mean
subtracted in longdouble -- of what output_pack returns at each sample time; the bound is
spectra_ref.bound with the constant measured on the float64 restatement (never on the device).
Every test prints the share of the bound the device reaches.

What output_pack returns is taken before its dimensional factor is multiplied in (read()):
the nondimensional variables of the state the device holds, which read() holds against
output_pack bit for bit (pack == x * factor in float64), and the factors go onto the
longdouble reference.  The pack itself carries the rounding of that one product in every cell,
2^-53 |x| of noise that is not the device's: on a line whose mean is 500 times its
fluctuation (a velocity of 9 varying by 0.02 across three cells of the navierStokes deck)
the spectrum of the rounded pack sits 86 bounds from the spectrum of the data, the bound
being in terms of the fluctuation A', as it must be to have teeth on pressure-like data.
"""
import numpy as np
import pytest

import les_cases
import probe
import spectra_ref as sr
import tp_cases
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import PhasedSolver, Solver, pool_spectra

pytestmark = pytest.mark.gpu

SIX = list(abi.SPECTRA_NAMES)
UVW = ["vel_x", "vel_y", "vel_z"]
W5 = (1.0, 0.5, 2.0, 0.25, 1.0)


def _lib(case):
    import aither_amd
    return aither_amd.load(case.n_eq, case.gas.thermodynamic_model)


def legal_overs(along):
    a, b = [d for d in "ijk" if d != along]
    return ["", a, b, a + b]


def lines_of(n, over):
    return int(np.prod([n["ijk".index(d)] for d in over] or [1]))


def factors(s, names):
    g = s.case.gas
    one = {"density": g.rho_ref, "pressure": g.rho_ref * g.a_ref * g.a_ref,
           "temperature": g.t_ref}
    return np.array([one.get(n, g.a_ref) for n in names])


def read(s, gb, names):
    """x[nvar, nk, nj, ni]: the variables of `names` as output_pack forms them from the state
    the device holds now, before the dimensional factor -- held against output_pack bit for
    bit, so this is a read of output_pack at this position."""
    g, gas = s.case.ng, s.case.gas
    st = s.download("state", gb)[g:-g, g:-g, g:-g]
    x = {"density": st[..., 0], "vel_x": st[..., 1], "vel_y": st[..., 2], "vel_z": st[..., 3],
         "pressure": st[..., 4], "temperature": st[..., 4] / (st[..., 0] * gas.gas_constant)}
    pack = s.output_pack(gb, names)
    dim = {"density": lambda v: v * gas.rho_ref, "pressure": lambda v: v * gas.rho_ref
           * gas.a_ref * gas.a_ref, "temperature": lambda v: v * gas.t_ref}
    for n, p in zip(names, pack):
        assert np.array_equal(dim.get(n, lambda v: v * gas.a_ref)(x[n]), p), n
    return np.array([x[n] for n in names])


def scaled(s, names, idx, ref, a1, mu):
    """The reference of nondimensional samples made dimensional in longdouble."""
    f = factors(s, names).astype(sr.LD)
    fs = np.array([f[v] * f[v] for v in range(len(names))] + [f[a] * f[b] for a, b in idx])
    tail = (1,) * (ref.ndim - 1)
    f64 = f.astype(np.float64).reshape((-1,) + (1,) * (a1.ndim - 1))
    return ref * fs.reshape((-1,) + tail), a1 * f64, mu * f64


def product_means(s, names, idx, packs, weights, along, over):
    """[nspec, *remaining extents (k, j, i)]: the weighted mean over the samples of the mean of
    x_a x_b over `along` and the pooled directions, dimensional, in longdouble; no transform."""
    f = factors(s, names).astype(sr.LD)
    axes = tuple(sorted({"i": 2, "j": 1, "k": 0}[d] for d in along + over))
    ab = [(v, v) for v in range(len(names))] + list(idx)
    out, big_w = 0, sr.LD(0)
    for x, w in zip(packs, weights):
        x = np.asarray(x, dtype=sr.LD)
        one = np.array([(x[a] * f[a] * x[b] * f[b]).mean(axis=axes) for a, b in ab])
        out, big_w = out + sr.LD(w) * one, big_w + sr.LD(w)
    return out / big_w


def hold(s, gb, names, pairs, along, over, packs, weights, what):
    """The block's spectra against the longdouble reference of the samples `packs` (read()),
    within the bound; Parseval: the sum over the modes against the mean of the product.
    Returns the values."""
    got, big_w, samples = s.spectra(gb)
    assert samples == len(packs) and big_w == float(sum(weights))
    idx = [(names.index(a) if isinstance(a, str) else a, names.index(b) if isinstance(b, str)
            else b) for a, b in pairs]
    ref, a1, mu = scaled(s, names, idx, *sr.reference(packs, weights, idx, along, over))
    n = s.case.blocks[gb].geom.n
    nn, lines = n["ijk".index(along)], lines_of(n, over)
    assert got.shape == ref.shape == (len(names) + len(pairs),) + \
        abi.spectra_shape(n, along, over)[0] + (nn // 2 + 1,)
    lim = sr.bound(a1, mu, idx, nn, lines, len(packs))
    share = sr.reached(got, ref, lim)
    # Parseval against the mean of the product formed directly, with no transform: the mean
    # of x_a x_b over the cells of the bin's lines and the samples, in longdouble
    direct = product_means(s, names, idx, packs, weights, along, over)
    total = np.abs(got.sum(axis=-1).astype(sr.LD) - direct).astype(np.float64)
    pshare = float(np.max(total / lim.sum(axis=-1)))
    print("%s along %s over %r: %.3f of the bound, Parseval %.3f" % (what, along, over, share,
                                                                      pshare))
    assert share <= 1.0, (what, along, over, share)
    assert pshare <= 1.0, (what, along, over, pshare)
    return got


# ---- 1. harmonics, uploaded state ----------------------------------------------------------------
@pytest.mark.parametrize("n", [(8, 7, 5), (67, 3, 2), (2, 3, 130)])
def test_harmonics(n):
    case = synthetic.single_block_case(n, stretch=1.1, time_integration="rk4")
    s = Solver(_lib(case), case)
    g, gas = case.ng, case.gas
    base = s.download("state", 0)
    names, pairs = ["vel_x", "vel_y"], [("vel_y", "vel_x")]
    au, av, mu_u, mu_v, pu, pv = 0.25, 0.5, 0.3, -0.2, 0.4, 1.3
    for along in "ijk":
        big_n = n["ijk".index(along)]
        for m0 in sorted({1, big_n // 2}):
            nyq = 2 * m0 == big_n
            ph_u, ph_v = (0.0, 0.0) if nyq else (pu, pv)
            st = base.copy()
            k = np.arange(big_n).reshape([-1 if d == along else 1 for d in "kji"])
            phys = st[g:-g, g:-g, g:-g]
            phys[..., 1] = mu_u + au * np.cos(2 * np.pi * m0 * k / big_n + ph_u)
            phys[..., 2] = mu_v + av * np.cos(2 * np.pi * m0 * k / big_n + ph_v)
            s.upload("state", 0, st)
            pack = read(s, 0, names)
            for over in legal_overs(along):
                s.spectra_plan(0, names, pairs, along, over)
                s.spectra_sample(1.0)
                got = hold(s, 0, names, pairs, along, over, [pack], [1.0], "harmonic %s m0 %d"
                           % (n, m0))
                a2 = gas.a_ref ** 2
                want = np.zeros((3, big_n // 2 + 1))
                want[:, 0] = [mu_u ** 2, mu_v ** 2, mu_u * mu_v]
                if big_n == 2 or nyq:
                    want[:, m0] = [au ** 2, av ** 2, au * av]
                else:
                    want[:, m0] = [au ** 2 / 2, av ** 2 / 2, au * av / 2 * np.cos(pv - pu)]
                flat = got.reshape(3, -1, big_n // 2 + 1)
                assert np.abs(flat - want[:, None, :] * a2).max() <= 1e-13 * a2
    s.close()


# ---- 2. runs against the longdouble reference ------------------------------------------------------
RUNS = {
    "les_a": (lambda: les_cases.deck_a(), "i", "jk"),
    "navier_stokes": (lambda: synthetic.single_block_case(
        (67, 3, 3), stretch=1.15, skew=0.01, equation_set="navierStokes",
        time_integration="rk4", cfl=0.5), "i", "k"),
    "rans": (lambda: synthetic.single_block_case(
        (12, 10, 8), stretch=1.2, equation_set="rans", turbulence_model="sst2003",
        bcs={3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
             4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)},
        time_integration="implicitEuler", cfl=10.0), "k", "i"),
    "tp_hot": (lambda: tp_cases.hot_single(n=(7, 5, 9), stretch=1.15, skew=0.01,
                                           equation_set="navierStokes", time_integration="rk4",
                                           cfl=0.5), "k", "ij"),
}
PAIRS = [("vel_x", "vel_y"), ("vel_z", "vel_x"), ("pressure", "density"),
         ("temperature", "vel_y")]


@pytest.mark.parametrize("name", list(RUNS))
def test_runs_hold_the_reference(name):
    make, along, over = RUNS[name]
    case = make()
    s = Solver(_lib(case), case)
    s.spectra_plan(0, SIX, PAIRS, along, over)
    packs = []
    for nn, w in enumerate(W5):
        s.step(nn)
        s.spectra_sample(w)
        packs.append(read(s, 0, SIX))
    assert np.abs(packs[-1] - packs[0]).max() > 0.0
    hold(s, 0, SIX, PAIRS, along, over, packs, W5, name)
    # the same samples along another direction, unpooled: a plan replaces a plan
    other = "j" if along != "j" else "i"
    s.spectra_plan(0, UVW, [(0, 1)], other, "")
    s.spectra_sample(2.0)
    hold(s, 0, UVW, [(0, 1)], other, "", [packs[-1][1:4]], [2.0], name + " replaced")
    s.close()


# ---- 3. exactness and determinism ------------------------------------------------------------------
def _vortical(n=(8, 7, 5)):
    case = synthetic.single_block_case(n, stretch=1.1, time_integration="rk4")
    return les_cases.vortical_state(case)


def test_exactness_and_determinism():
    case = _vortical()
    s = Solver(_lib(case), case)
    plan = (["vel_x", "pressure", "vel_z"], [("vel_x", "vel_z"), (1, 0)])
    for along, over in (("i", "jk"), ("j", "i"), ("k", "")):
        s.spectra_plan(0, *plan, along, over)
        s.spectra_sample(1.0)
        one = s.spectra(0)[0]
        for w in (3.0, 0.5):
            s.spectra_sample(w)
        assert np.array_equal(s.spectra(0)[0], one), "identical samples"
        raw = s.spectra_download(0)
        # doubled weights; and a reset starts again
        s.spectra_reset()
        assert s.spectra(0)[1:] == (0.0, 0.0)
        for w in (2.0, 6.0, 1.0):
            s.spectra_sample(w)
        twice = s.spectra_download(0)
        assert np.array_equal(abi.spectra_accum_split(raw)[3], abi.spectra_accum_split(twice)[3])
        # a second context: the same bits; a subset and a reordered plan: what they share
        t = Solver(_lib(case), case)
        t.spectra_plan(0, *plan, along, over)
        t.spectra_sample(1.0)
        assert np.array_equal(t.spectra(0)[0], one), "two runs"
        t.spectra_plan(0, ["pressure"], [], along, over)
        t.spectra_sample(1.0)
        assert np.array_equal(t.spectra(0)[0][0], one[1]), "subset"
        t.spectra_plan(0, ["vel_z", "density", "vel_x", "pressure"], [(2, 3), (0, 2)], along, over)
        t.spectra_sample(1.0)
        again = t.spectra(0)[0]
        for mine, theirs in ((0, 2), (2, 0), (3, 1), (4, 4), (5, 3)):
            assert np.array_equal(again[mine], one[theirs]), ("reordered", mine)
        t.close()
    # lines identical along the pooled direction: one line's bits
    g = case.ng
    st = s.download("state", 0)
    st[:] = st[:, g:g + 1, :, :]          # (every j-row is the first)
    s.upload("state", 0, st)
    s.spectra_plan(0, *plan, "i", "")
    s.spectra_sample(1.0)
    single = s.spectra(0)[0]
    s.spectra_plan(0, *plan, "i", "j")
    s.spectra_sample(1.0)
    pooled = s.spectra(0)[0]
    assert np.array_equal(pooled, single[:, :, 0, :])
    for j in range(1, single.shape[2]):
        assert np.array_equal(single[:, :, j, :], single[:, :, 0, :])
    s.close()


def test_subset_and_superset_where_the_lds_limits_the_tile():
    """130 x 16 x 2 along i pooled over j: the LDS, not the row, limits the tile (12 lines for
    a plan of six variables, and so for every plan), and the tile is cut (12 + 4).  Plans of
    1, 3 and 6 variables return the same bits for what they share."""
    case = _vortical((130, 16, 2))
    s = Solver(_lib(case), case)
    assert sr.shape((130, 16, 2), 0, 2, 1)["tl"] == sr.shape((130, 16, 2), 0, 2, 6)["tl"] == 12
    for over in ("j", "jk"):
        s.spectra_plan(0, SIX, [("vel_x", "vel_y"), ("pressure", "vel_z")], "i", over)
        s.spectra_sample(1.0)
        six = hold(s, 0, SIX, [("vel_x", "vel_y"), ("pressure", "vel_z")], "i", over,
                   [read(s, 0, SIX)], [1.0], "six variables")
        s.spectra_plan(0, ["vel_y", "pressure", "vel_x"], [(2, 0)], "i", over)
        s.spectra_sample(1.0)
        three = s.spectra(0)[0]
        for mine, theirs in ((0, 2), (1, 4), (2, 1), (3, 6)):
            assert np.array_equal(three[mine], six[theirs]), ("three of six", over, mine)
        s.spectra_plan(0, ["vel_z"], [], "i", over)
        s.spectra_sample(1.0)
        assert np.array_equal(s.spectra(0)[0][0], six[3]), ("one of six", over)
    s.close()


# ---- 4. the run is untouched -----------------------------------------------------------------------
def _final(s):
    g = s.case.ng
    out = {"state": s.download("state", 0)[g:-g, g:-g, g:-g], "residual": s.download("residual", 0)}
    for q, h in enumerate(s.history):
        out["l2", q] = np.array(h["l2"])
        out["norm", q] = np.array(h["norm"])
        out["linf", q] = np.array(h["linf"], dtype=float)
        out["matrix", q] = np.array(h["matrix"])
    return out


UNTOUCHED = {
    # the fused explicit path (two state buffers)
    "rk4_fused": lambda: synthetic.single_block_case((9, 8, 7), stretch=1.15,
                                                     time_integration="rk4", cfl=0.5),
    # scalar LU-SGS, dual time stepping
    "bdf2_lusgs": lambda: synthetic.single_block_case(**tp_cases.FIVE["wenoz_roe_bdf2_dual"]),
}


@pytest.mark.parametrize("name", list(UNTOUCHED))
def test_sampling_leaves_the_run_bit_identical(name):
    finals = []
    for sampled in (False, True):
        case = UNTOUCHED[name]()
        s = Solver(_lib(case), case)
        packs = []
        if sampled:
            s.spectra_plan(0, UVW, [(0, 1)], "j", "k")
        for nn in range(5):
            s.step(nn)
            if sampled:
                s.spectra_sample(1.0 + nn)
                packs.append(read(s, 0, UVW))
        if sampled:
            hold(s, 0, UVW, [(0, 1)], "j", "k", packs, [1.0 + nn for nn in range(5)], name)
        finals.append(_final(s))
        s.close()
    assert finals[0].keys() == finals[1].keys()
    for k in finals[0]:
        assert np.array_equal(finals[0][k], finals[1][k]), k


def _phased(case, sample):
    """Two steps of a one-rank PhasedSolver; sample=True: after every phase and halo call the
    spectrum of one sample is taken and compared with that of output_pack read there."""
    holder, seen = [], []

    def hook(label, args):
        if not sample or not holder:
            return
        s = holder[0]
        s.spectra_reset()
        s.spectra_sample(1.0)
        got = s.spectra(0)[0]
        pack = read(s, 0, SIX)
        ref, a1, mu = scaled(s, SIX, [(1, 2)], *sr.reference([pack], [1.0], [(1, 2)], "i", "j"))
        n = s.case.blocks[0].geom.n
        lim = sr.bound(a1, mu, [(1, 2)], n[0], n[1], 1)
        seen.append((label, sr.reached(got, ref, lim)))

    s = PhasedSolver(probe.ProbingApi(_lib(case), hook), case, 0, None, None)
    if sample:
        s.spectra_plan(0, SIX, [(1, 2)], "i", "j")
    holder.append(s)
    for nn in range(2):
        s.step(nn)
    holder.clear()
    final = _final(s)
    s.close()
    return final, seen


@pytest.mark.parametrize("name", list(UNTOUCHED))
def test_sample_between_phases(name):
    base, _ = _phased(UNTOUCHED[name](), False)
    final, seen = _phased(UNTOUCHED[name](), True)
    labels = {lab for lab, _ in seen}
    assert {"phase_bc_faces", "phase_bc_edges", "phase_residual"} <= labels, labels
    worst = max(seen, key=lambda e: e[1])
    print("%s: %d positions, at most %.3f of the bound (%s)" % (name, len(seen), worst[1],
                                                                 worst[0]))
    assert worst[1] <= 1.0, worst
    for k in base:
        assert np.array_equal(base[k], final[k]), k


# ---- 5. carrying an average on ---------------------------------------------------------------------
def test_carrying_on():
    def run(first, last, payload=None, scale=1.0):
        case = UNTOUCHED["rk4_fused"]()
        s = Solver(_lib(case), case)
        s.spectra_plan(0, UVW, [(2, 0)], "k", "i")
        if payload is not None:
            s.spectra_upload(0, payload)
        for nn in range(5):
            s.step(nn)
            if first <= nn < last:
                s.spectra_sample(scale * W5[nn])
        out = s.spectra_download(0), s.spectra(0)
        s.close()
        return out

    whole, (vals, big_w, samples) = run(0, 5)
    assert (big_w, samples) == (sum(W5), 5)
    part, _ = run(0, 3)
    assert abi.spectra_accum_split(part)[1:3] == (sum(W5[:3]), 3.0)
    rest, (vals2, _, _) = run(3, 5, part)
    assert np.array_equal(rest, whole) and np.array_equal(vals, vals2)
    # five different samples with every weight doubled: W doubles, no bit of S changes
    twice, (vals3, big_w3, _) = run(0, 5, scale=2.0)
    assert big_w3 == 2 * sum(W5) and np.array_equal(vals3, vals)
    assert np.array_equal(abi.spectra_accum_split(twice)[3], abi.spectra_accum_split(whole)[3])


# ---- 6. pool_spectra -------------------------------------------------------------------------------
def test_pool_spectra_joins_the_blocks_of_a_cut():
    """Deck D is deck A cut in i: the spectra along j pooled over i (and k) of its two blocks,
    joined by pool_spectra, against the reference of deck A's whole block."""
    a, d = les_cases.deck_a(), les_cases.deck_d()
    sa, sd = Solver(_lib(a), a), Solver(_lib(d), d)
    for over in ("i", "ik"):
        pack = read(sa, 0, UVW)
        ref, a1, mu = scaled(sa, UVW, [(0, 1)], *sr.reference([pack], [1.0], [(0, 1)], "j", over))
        parts = []
        for gb in (0, 1):
            assert np.array_equal(read(sd, gb, UVW), pack[..., :les_cases.CUT] if gb == 0
                                  else pack[..., les_cases.CUT:])
            sd.spectra_plan(gb, UVW, [(0, 1)], "j", over)
        sd.spectra_sample(1.0)
        for gb in (0, 1):
            vals, big_w, _ = sd.spectra(gb)
            parts.append((vals, big_w, sd.spectra_lines(gb)))
        got, weight = pool_spectra(parts)
        n = a.blocks[0].geom.n
        lines = lines_of(n, over)
        assert weight == float(lines)
        lim = sr.bound(a1, mu, [(0, 1)], n[1], lines, 1)
        share = sr.reached(got, ref, lim)
        print("pooled over %r: %.3f of the bound" % (over, share))
        assert share <= 1.0
    sa.close(), sd.close()


# ---- 7. refusals -----------------------------------------------------------------------------------
def test_refusals():
    case = _vortical((8, 7, 1))
    s = Solver(_lib(case), case)
    up = lambda field, payload: s._series_up(0, field, np.asarray(payload, dtype=float), field)
    for call in (lambda: up("spectra_sample", [1.0]), lambda: s.spectra_download(0),
                 lambda: s.spectra(0), lambda: up("spectra_accum", np.zeros(16))):
        with pytest.raises(RuntimeError, match=r"block 0 has no plan \(upload "
                                               r"AGX_FIELD_SPECTRA_PLAN first\)"):
            call()
    out = abi.OUT
    u, v = out["vel_x"], out["vel_y"]
    refused = [
        ([0, 0, 1, 0, out["mach"]], "is not one of density, vel_x, vel_y, vel_z, pressure, "
                                    "temperature"),
        ([0, 0, 2, 0, u, u], "variable %d is repeated" % u),
        ([0, 0, 2, 1, u, v, 0, 2], r"entry 7 \(a variable of a pair.*an integer from 0 to 1"),
        ([0, 0, 2, 2, u, v, 0, 1, 0, 1], r"pair 1, \(0, 1\), is repeated"),
        ([0, 0, 2, 2, u, v, 0, 1, 1, 0], r"pair 1, \(1, 0\), is repeated"),
        ([0, 0, 2, 1, u, v, 1, 1], "the auto-spectrum of a variable is kept already"),
        ([0, 0, 7, 0, 0, 1, 2, 3, 4, 8, 5], "nvar = 7: a plan holds at most 6 variables"),
        ([0, 1, 1, 0, u], r"over \(mask 1\) contains along \(0\)"),
        ([1, 5, 1, 0, u], None),       # (legal: along j over i and k)
        ([2, 0, 1, 0, u], "N = 1 cells along direction 2: a spectrum needs N >= 2"),
        ([3, 0, 1, 0, u], r"entry 0 \(along: 0 i, 1 j, 2 k\) is 3"),
        ([0, 0, 1.5, 0, u], r"entry 2 \(nvar, the variables\) is 1.5"),
    ]
    for payload, text in refused:
        if text is None:
            up("spectra_plan", payload)
            continue
        with pytest.raises(RuntimeError, match=text):
            up("spectra_plan", payload)
    # the plan that stood is still there, untouched by the refused uploads
    s.spectra_plan(0, ["vel_x", "vel_y"], [(0, 1)], "i", "j")
    s.spectra_sample(1.0)
    before = s.spectra_download(0)
    for w, text in ((-1.0, "the weight -1 is negative or not finite"),
                    (float("nan"), "the weight nan is negative or not finite"),
                    (float("inf"), "the weight inf is negative or not finite")):
        with pytest.raises(RuntimeError, match=text):
            s.spectra_sample(w)
    bad = before.copy()
    bad[1] = 0.0                   # (another over)
    with pytest.raises(RuntimeError, match="entry 1 of the payload's plan is 0, the plan of "
                                           "block 0 holds 2"):
        s.spectra_upload(0, bad)
    bad = before.copy()
    bad[10] = 3.0                  # nbin
    with pytest.raises(RuntimeError, match="the payload holds 3 bins of 5 modes, the plan of "
                                           "block 0 gives 1 of 5"):
        s.spectra_upload(0, bad)
    bad = before.copy()
    bad[8] = -1.0                  # W
    with pytest.raises(RuntimeError, match="the sum of weights -1 or the sample count 1 is "
                                           "negative or not finite"):
        s.spectra_upload(0, bad)
    with pytest.raises(RuntimeError, match="AGX_FIELD_SPECTRA_VALUES is download only"):
        up("spectra_values", [0.0])
    assert np.array_equal(s.spectra_download(0), before)
    s.spectra_clear()
    with pytest.raises(RuntimeError, match="block 0 has no plan"):
        s.spectra(0)
    s.close()


def test_the_longest_line_and_one_beyond():
    """N = AGX_SPECTRA_MAX_N with six variables fills the line kernel's LDS; one more cell is
    refused by name.  (Three cells in j: with two, cos(2 pi y) of the vortical state is 6e-17
    and the density an exact constant along every line, whose bound is 0; the serial sum of
    1024 equal values rounds, so the device's line is a constant 1e-16 and its spectrum 1e-60,
    not 0.)"""
    case = synthetic.single_block_case((abi.SPECTRA_MAX_N, 3, 2), time_integration="rk4")
    case = les_cases.vortical_state(case)
    s = Solver(_lib(case), case)
    s.spectra_plan(0, SIX, [(1, 2)], "i", "j")
    s.spectra_sample(1.0)
    hold(s, 0, SIX, [(1, 2)], "i", "j", [read(s, 0, SIX)], [1.0], "N = 1024")
    s.close()
    case = synthetic.single_block_case((abi.SPECTRA_MAX_N + 1, 3, 2), time_integration="rk4")
    s = Solver(_lib(case), case)
    with pytest.raises(RuntimeError, match="N = 1025 cells along direction 0: the line kernel "
                                           "holds lines of at most AGX_SPECTRA_MAX_N = 1024"):
        s.spectra_plan(0, ["vel_x"], [], "i", "")
    s.close()
