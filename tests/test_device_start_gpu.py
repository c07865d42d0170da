"""Start and resume on the device: agx_state_fill, agx_state_from_cloud, agx_restart_unpack.

Every check is a bit-for-bit comparison with an array the host code already makes and the
existing uploads: after each call a block must be exactly as if the caller had uploaded the
ghost-padded array (zero ghost cells) through agx_state_upload, or consVarsNm1 through
agx_field_upload.  The references: build_case(initial="host")'s arrays, numpy's argmin of the
brute-force squared distances, and tests/restart_ref.py for the restart readers.

Cloud cases carry a condition on their inputs, asserted on the CPU: for every cell the nearest
and the second-nearest squared distance differ by more than 1e-9 of the larger, so that a
contracted dot product on the device cannot change the winner.  Exact ties are a case of
their own (the lowest index wins).
"""
import ctypes as C
import os

import numpy as np
import pytest

import aither_amd
import restart_ref
from aither_amd import abi
from aither_amd.case import builder, synthetic
from aither_amd.case.builder import build_case
from aither_amd.solver import Solver
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

VORTEX = os.path.join(GOLDEN, "cases", "convectingVortex", "convectingVortex.inp")
WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1),
        2: ("characteristic", 1), 4: ("characteristic", 1)}
RANS_WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
             4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
LIB_KW = {
    "5eq": dict(equation_set="navierStokes", bcs=WALL),
    "7eq": dict(equation_set="rans", turbulence_model="sst2003", bcs=RANS_WALL),
    "5eq_tp": dict(equation_set="navierStokes", bcs=WALL, thermodynamic_model="thermallyPerfect",
                   temperature_factor=7.0),
}
RECON = {1: "constant", 2: "thirdOrder", 3: "weno"}
ULP = 2.0 ** -52


def _lib(case):
    return aither_amd.load(case.n_eq, case.gas.thermodynamic_model)


def _advance(s, case, steps, first=0):
    """`steps` time steps as Solver.step makes them: what agx_iterate returned per nonlinear
    iteration (raw L2 sums, L-inf record, matrix residual)."""
    out = []
    for nn in range(first, first + steps):
        s.store_time_n(nn)
        for mm in range(case.deck.nonlinear_iterations):
            l2, linf, mres = s.iterate(mm, case.deck.cfl(nn))
            out.append((l2.copy(), (linf.linf, linf.block, linf.i, linf.j, linf.k, linf.eqn),
                        mres))
    return out


def _states(s):
    return [s.download("state", gb) for gb in sorted(s.block_ids)]


def _assert_same_run(got, ref, what):
    (gn, gs), (rn, rs) = got, ref
    assert len(gn) == len(rn) and len(gn) > 0
    for it, (a, b) in enumerate(zip(gn, rn)):
        assert np.all(np.isfinite(b[0])) and np.all(b[0] > 0.0), (what, it)
        assert np.array_equal(a[0], b[0]), (what, it, a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2], (what, it)
    for a, b in zip(gs, rs):
        assert np.array_equal(a, b), what


def _d2(cen, pts):
    d = cen[:, None, :] - pts[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _assert_gap(d2):
    """the condition on the inputs: nearest and second nearest differ by > 1e-9 of the larger"""
    if d2.shape[1] < 2:
        return 1.0
    two = np.partition(d2, 1, axis=1)[:, :2]
    gap = (two[:, 1] - two[:, 0]) / two[:, 1]
    assert np.all(gap > 1e-9), gap.min()
    return float(gap.min())


def _cloud(seed, npts, n_eq):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-0.05, 1.05, size=(npts, 3))
    st = rng.uniform(0.5, 1.5, size=(npts, n_eq))
    st[:, 1:4] -= 1.0
    return pts, st


# ---- 1: fill ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ng", [1, 2, 3])
@pytest.mark.parametrize("lib", list(LIB_KW))
def test_fill_is_the_upload_of_the_host_array(lib, ng):
    kw = dict(stretch=1.1, face_reconstruction=RECON[ng], limiter="none",
              time_integration="implicitEuler", cfl=5.0, **LIB_KW[lib])
    host = synthetic.single_block_case((7, 5, 3), amplitude=0.0, **kw)
    dev = synthetic.single_block_case((7, 5, 3), initial="device", **kw)
    assert host.ng == ng and dev.blocks[0].state.kind == "uniform"
    ref = host.blocks[0].state
    assert np.all(ref[:ng] == 0.0) and np.all(ref[ng:-ng, ng:-ng, ng:-ng, 0] > 0.0)
    sd, sh = Solver(_lib(dev), dev), Solver(_lib(host), host)
    try:
        assert np.array_equal(sd.download("state", 0), ref)
        assert np.array_equal(sh.download("state", 0), ref)
        got = (_advance(sd, dev, 2), _states(sd))
        want = (_advance(sh, host, 2), _states(sh))
        _assert_same_run(got, want, (lib, ng))
        # ... and over a state that is there: the ghost cells the iterations filled go to zero
        assert not np.all(sd.download("state", 0)[:ng] == 0.0)
        sd.state_fill(0, dev.blocks[0].state.prim)
        assert np.array_equal(sd.download("state", 0), ref)
    finally:
        sd.close(), sh.close()


# ---- 2: cloud ---------------------------------------------------------------------------------
def test_cloud_golden_vortex_matches_the_host_path():
    host = build_case(VORTEX)
    dev = build_case(VORTEX, initial="device")
    g = host.ng
    cen = host.blocks[0].geom.center.a[g:-g, g:-g, g:-g].reshape(-1, 3)
    gap = _assert_gap(_d2(cen, dev.blocks[0].state.pts))
    print(f"convectingVortex: smallest relative gap {gap:.6f}")
    sd, sh = Solver(_lib(dev), dev), Solver(_lib(host), host)
    try:
        assert np.array_equal(sd.download("state", 0), host.blocks[0].state)
        got = (_advance(sd, dev, 3), _states(sd))
        want = (_advance(sh, host, 3), _states(sh))
        _assert_same_run(got, want, "convectingVortex")
    finally:
        sd.close(), sh.close()


@pytest.mark.parametrize("geometry,lib", [("host", "5eq"), ("device", "5eq"), ("host", "7eq")])
def test_cloud_is_the_argmin_of_the_brute_force_distances(geometry, lib):
    """9 x 6 x 5, stretched and skewed, array-built and node-built; clouds of 1, 257 and 700
    points: one point, one past an LDS tile, a ragged third tile."""
    kw = dict(LIB_KW[lib], time_integration="implicitEuler", cfl=5.0)
    case = synthetic.single_block_case((9, 6, 5), stretch=1.3, skew=0.03, amplitude=0.0,
                                       geometry=geometry, **kw)
    g, n_eq = case.ng, case.n_eq
    s = Solver(_lib(case), case)
    try:
        # (the centres the kernel reads; a node-built block has them on the device alone)
        cen = s.geometry("center", 0)[g:-g, g:-g, g:-g].reshape(-1, 3)
        assert cen.shape == (9 * 6 * 5, 3)
        for seed, npts in ((11, 1), (12, 257), (13, 700)):
            pts, st = _cloud(seed, npts, n_eq)
            d2 = _d2(cen, pts)
            _assert_gap(d2)
            idx = np.argmin(d2, axis=1)
            if npts > 256:
                assert idx.max() >= 256          # (winners beyond the first tile)
            far = s.state_from_cloud(0, pts, st)
            ref = builder.padded_state(case.blocks[0].geom, st[idx].reshape(5, 6, 9, n_eq))
            assert np.array_equal(s.download("state", 0), ref), npts
            want = float(np.sqrt(d2[np.arange(len(idx)), idx]).max())
            print(f"{geometry} {lib} npts={npts}: max_dist {far!r} numpy {want!r} "
                  f"rel {abs(far - want) / want:.3e}")
            assert abs(far - want) <= 8.0 * 2.0 ** -53 * want, (npts, far, want)
    finally:
        s.close()


@pytest.mark.parametrize("order", ["appended", "interleaved"])
def test_cloud_ties_go_to_the_lowest_index(order):
    """Every point twice, with another state: the copy with the lower index wins.  The points
    are the cell centres themselves, so max_dist is exactly 0 (numpy's is)."""
    case = synthetic.single_block_case((9, 6, 5), stretch=1.3, skew=0.03, amplitude=0.0)
    g = case.ng
    s = Solver(_lib(case), case)
    try:
        cen = s.geometry("center", 0)[g:-g, g:-g, g:-g].reshape(-1, 3)
        _assert_gap(_d2(cen, cen))
        _, st = _cloud(21, len(cen), 5)
        perm = np.random.default_rng(22).permutation(len(cen))
        pts, st = cen[perm], st[perm]
        if order == "appended":        # copies 270 apart: another LDS tile
            pts2, st2 = np.concatenate([pts, pts]), np.concatenate([st, st + 1.0])
            low = np.arange(len(pts))
        else:                          # copies side by side
            pts2, st2 = np.repeat(pts, 2, axis=0), np.repeat(st, 2, axis=0)
            st2[1::2] += 1.0
            low = 2 * np.arange(len(pts))
        d2 = _d2(cen, pts2)
        idx = np.argmin(d2, axis=1)                 # (numpy: the first of equal minima)
        assert np.all(np.isin(idx, low)) and np.all(d2[np.arange(len(idx)), idx] == 0.0)
        far = s.state_from_cloud(0, pts2, st2)
        ref = builder.padded_state(case.blocks[0].geom, st2[idx].reshape(5, 6, 9, 5))
        assert np.array_equal(s.download("state", 0), ref)
        assert far == 0.0
    finally:
        s.close()


# ---- 3: restart -------------------------------------------------------------------------------
BDF2 = dict(time_integration="bdf2", nonlinear_iterations=2, dt=2.0e-6, cfl=-1.0)
RESTART_DECKS = {
    "bdf2_lusgs": lambda: synthetic.single_block_case(
        (10, 8, 6), stretch=1.2, skew=0.01, matrix_solver="lusgs", **BDF2, **LIB_KW["5eq"]),
    "rans_blusgs": lambda: synthetic.single_block_case(
        (9, 7, 5), stretch=1.15, matrix_solver="blusgs", **BDF2, **LIB_KW["7eq"]),
    "tp": lambda: synthetic.single_block_case(
        (10, 8, 6), stretch=1.2, matrix_solver="lusgs", **BDF2, **LIB_KW["5eq_tp"]),
}


@pytest.mark.parametrize("deck", list(RESTART_DECKS))
def test_restart_unpack_is_the_reference_reader(deck):
    case = RESTART_DECKS[deck]()
    lib, g = _lib(case), case.ng
    a = Solver(lib, case)
    _advance(a, case, 3)
    pay = [a.restart_pack(0, which) for which in (0, 1)]
    a.close()
    gas = builder.config_struct(case).gas            # (the agx_gas the library got)
    ref_state = restart_ref.padded(restart_ref.unpack(pay[0], gas, 0), g)
    ref_nm1 = restart_ref.unpack(pay[1], gas, 1)
    assert np.all(ref_state[g:-g, g:-g, g:-g, 0] > 0.0) and np.all(ref_nm1[..., 0] > 0.0)
    b, c = Solver(lib, case), Solver(lib, case)
    try:
        b.restart_unpack(0, pay[0], 0)
        b.restart_unpack(0, pay[1], 1)
        assert np.array_equal(b.download("state", 0), ref_state)
        assert np.array_equal(b.download("cons_nm1", 0), ref_nm1)
        for which in (0, 1):
            back = b.restart_pack(0, which)
            err = np.abs(back - pay[which])
            print(f"{deck} which={which}: pack(unpack) worst "
                  f"{(err[pay[which] != 0] / np.abs(pay[which][pay[which] != 0])).max() / ULP:.3f}"
                  " x 2^-52")
            assert np.all(err <= 2.0 * ULP * np.abs(pay[which])), (deck, which)
        c.upload("state", 0, ref_state)
        c.upload("cons_nm1", 0, ref_nm1)
        got = (_advance(b, case, 3, first=3), _states(b))
        want = (_advance(c, case, 3, first=3), _states(c))
        _assert_same_run(got, want, deck)
    finally:
        b.close(), c.close()


# ---- 4: a state written mid-run makes the derived data stale ----------------------------------
BENCH = dict(equation_set="navierStokes", face_reconstruction="weno", limiter="none",
             inviscid_flux="ausm", time_integration="implicitEuler", matrix_solver="lusgs",
             matrix_sweeps=1, cfl=10.0)


@pytest.mark.parametrize("entry", ["restart_unpack", "state_fill", "state_from_cloud"])
def test_state_written_mid_run_is_not_taken_for_current(agx, entry):
    """The default LU-SGS path on 34 x 33 x 4 (two prepare tiles in i and in j; the lean D2
    state is current after the first update): two iterations, the entry, two more -- bitwise
    the same sequence with agx_state_upload of the equivalent array in the middle."""
    make = lambda: synthetic.single_block_case((34, 33, 4), stretch=1.2, bcs=WALL, **BENCH)
    case = make()
    geom, g = case.blocks[0].geom, case.ng
    prim = builder.initial_primitive(case.deck, case.gas, 0)
    if entry == "state_fill":
        call = lambda s: s.state_fill(0, 1.05 * prim)
        equivalent = builder.padded_state(geom, 1.05 * prim)
    elif entry == "state_from_cloud":
        pts, st = _cloud(31, 300, 5)
        st = prim * (1.0 + 0.05 * (st - np.array([1.0, 0.0, 0.0, 0.0, 1.0])))
        d2 = _d2(geom.center.a[g:-g, g:-g, g:-g].reshape(-1, 3), pts)
        _assert_gap(d2)
        call = lambda s: s.state_from_cloud(0, pts, st)
        equivalent = builder.padded_state(geom, st[np.argmin(d2, axis=1)].reshape(4, 33, 34, 5))
    else:
        other = synthetic.single_block_case((34, 33, 4), stretch=1.2, bcs=WALL, amplitude=0.03,
                                            **BENCH).blocks[0].state[g:-g, g:-g, g:-g]
        gas = builder.config_struct(case).gas
        payload = np.ones(other.shape[:3] + (6,))
        payload[..., :5] = other * np.array(restart_ref.divisors(gas, 0)[:5])
        call = lambda s: s.restart_unpack(0, payload, 0)
        equivalent = restart_ref.padded(restart_ref.unpack(payload, gas, 0), g)
    assert not np.array_equal(equivalent, case.blocks[0].state)
    runs = []
    for middle in (call, lambda s: s.upload("state", 0, equivalent)):
        s = Solver(agx, case)
        try:
            _advance(s, case, 2)
            middle(s)
            assert np.array_equal(s.download("state", 0), equivalent)
            runs.append((_advance(s, case, 2, first=2), _states(s)))
        finally:
            s.close()
    _assert_same_run(runs[0], runs[1], entry)


# ---- 5: refusals ------------------------------------------------------------------------------
def _refused(api, rc, match):
    with pytest.raises(RuntimeError, match=match):
        api.check(rc, "call")


def test_refusals_name_their_reason_and_leave_the_state(agx):
    """(which = 1 is refused where agx_field_upload refuses AGX_FIELD_CONS_NM1, through the same
    table and in its words; no configuration makes it refuse that field today.)"""
    case = synthetic.single_block_case((7, 5, 3), stretch=1.1)
    s = Solver(agx, case)
    p = lambda a: a.ctypes.data_as(abi.c_dp)
    try:
        before = s.download("state", 0)
        prim = builder.initial_primitive(case.deck, case.gas, 0)
        pts, st = _cloud(41, 5, 5)
        pay = s.restart_pack(0, 0)
        ctx, bid = s.ctx, s.block_ids[0]
        # a bad block id
        for bad in (-1, 1, 99):
            _refused(agx, agx.state_fill(ctx, bad, p(prim)), f"bad block id {bad}")
            _refused(agx, agx.state_from_cloud(ctx, bad, 5, p(pts), p(st), None),
                     f"bad block id {bad}")
            _refused(agx, agx.restart_unpack(ctx, bad, 0, p(pay)), f"bad block id {bad}")
        # null pointers
        _refused(agx, agx.state_fill(ctx, bid, None), "agx_state_fill: null pointer")
        _refused(agx, agx.state_from_cloud(ctx, bid, 5, None, p(st), None),
                 "agx_state_from_cloud: null pointer")
        _refused(agx, agx.state_from_cloud(ctx, bid, 5, p(pts), None, None),
                 "agx_state_from_cloud: null pointer")
        _refused(agx, agx.restart_unpack(ctx, bid, 0, None), "agx_restart_unpack: null pointer")
        # which, npts
        for which in (-1, 2):
            _refused(agx, agx.restart_unpack(ctx, bid, which, p(pay)),
                     r"agx_restart_unpack: which is 0 \(state\) or 1 \(consVarsNm1\)")
        for npts in (0, -3):
            _refused(agx, agx.state_from_cloud(ctx, bid, npts, p(pts), p(st), None),
                     f"agx_state_from_cloud: npts {npts} < 1")
        # nonphysical or non-finite values, in the fill's state and in the cloud's last row
        for e, value, why in ((0, 0.0, "nonphysical density"), (0, -1.0, "nonphysical density"),
                              (4, 0.0, "nonphysical pressure"), (4, -2.0, "nonphysical pressure"),
                              (2, np.nan, "non-finite value"), (4, np.inf, "non-finite value"),
                              (0, np.nan, "non-finite value")):
            bad = prim.copy()
            bad[e] = value
            _refused(agx, agx.state_fill(ctx, bid, p(bad)), "agx_state_fill: " + why)
            bst = st.copy()
            bst[-1, e] = value
            _refused(agx, agx.state_from_cloud(ctx, bid, 5, p(pts), p(bst), None),
                     "agx_state_from_cloud: " + why + r" \(cloud state 4\)")
        assert np.array_equal(s.download("state", 0), before)
    finally:
        s.close()
    # before agx_setup_finalize
    ctx = C.c_void_p()
    agx.check(agx.ctx_create(0, 0, C.byref(ctx)), "ctx_create")
    try:
        _refused(agx, agx.state_fill(ctx, 0, p(prim)),
                 "agx_state_fill: agx_setup_finalize has not been called")
        _refused(agx, agx.state_from_cloud(ctx, 0, 5, p(pts), p(st), None),
                 "agx_state_from_cloud: agx_setup_finalize has not been called")
        _refused(agx, agx.restart_unpack(ctx, 0, 0, p(pay)),
                 "agx_restart_unpack: agx_setup_finalize has not been called")
    finally:
        agx.ctx_destroy(ctx)
