"""Integrated wall loads on the device (agx_output_pack with AGX_LOAD_*, k_wall_loads): force,
moment and heat load per load surface against the numpy reference of tests/loads_ref.py, fed
with the library's own wall payload, the downloaded face areas and face centres formed from the
case's nodes.  The bound is the one loads_ref derives: (N + 16) 2^-52 S for the summation plus
the per-face tolerances of tests/test_wall_pack_gpu.py times the surface's area;
tests/test_wall_loads_host.py shows on every case used here that a missing face or a flipped
side exceeds it."""
import ctypes as C

import numpy as np
import pytest

import loads_ref
import probe
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import Solver

pytestmark = pytest.mark.gpu

ALL = loads_ref.NAMES
ELEVEN = loads_ref.NO_MOMENTS


def _lib(n_eq=5, model="caloricallyPerfect"):
    import aither_amd
    return aither_amd.load(n_eq, model)


def _hold(sol, names=ELEVEN, nodes=None, what=""):
    """every load surface of every block against the reference"""
    got_all = {}
    for gb in sorted(sol.block_ids):
        if not sol.load_surfaces(gb):
            continue
        got = sol.wall_loads(gb, names)
        ref = loads_ref.block_reference(sol, gb, nodes=nodes)
        assert all(got[n].shape == (len(ref),) for n in names)
        loads_ref.compare(got, ref, names, what=f"{what} block {gb}")
        got_all[gb] = got
    return got_all


# ---- against the library's own wall payload ---------------------------------------------------
@pytest.mark.parametrize("name,lib", [("laminar_central", (5,)), ("laminar_fourth", (5,)),
                                      ("stacked_k", (5,)), ("hot_tp", (5, "thermallyPerfect")),
                                      ("rans_low_re", (7,))])
def test_loads_are_the_sums_of_the_wall_payload(name, lib):
    sol = Solver(_lib(*lib), loads_ref.CASES[name]())
    sol.step(0), sol.step(1)
    got = _hold(sol, what=name)
    assert len(got) == len(sol.block_ids)
    if name.startswith("laminar"):
        assert [s["side"] for s in sol.load_surfaces(0)] == [1, 3, 4]
        # isothermal and constant-heat-flux walls exchange heat, all three are dragged
        assert np.all(got[0]["heatLoad"][1:] != 0.0)
        assert np.all(np.abs(got[0]["viscousForce_x"]) > 0.0)
    sol.close()


def test_wall_law_surfaces_sum_the_stored_wall_data():
    sol = Solver(_lib(7), loads_ref.CASES["wall_law"]())
    with pytest.raises(RuntimeError, match="no wall data before the first residual"):
        for gb in sorted(sol.block_ids):
            if sol.wall_surfaces(gb):
                sol.wall_loads(gb, ["area"])
    sol.step(0), sol.step(1)
    got = _hold(sol, what="wallLaw")
    assert got
    sol.close()


# ---- reduction boundaries -----------------------------------------------------------------------
def test_surfaces_around_the_wave_and_chunk_sizes():
    """1, 63, 64, 65, 255, 256, 257 faces (and 2): several surfaces per side, lower side viscous,
    upper side slip; no iteration, the perturbed initial state"""
    sol = Solver(_lib(), loads_ref.CASES["strip"]())
    surfs = sol.load_surfaces(0)
    faces = [int(np.prod(s["shape"])) for s in surfs]
    assert sorted(faces) == [1, 1, 2, 63, 64, 64, 65, 255, 256, 257]
    assert {s["side"] for s in surfs} == {3, 4}
    _hold(sol, what="strip")
    sol.close()


def test_surface_of_more_than_64_chunks():
    sol = Solver(_lib(), loads_ref.CASES["big"]())
    faces = [int(np.prod(s["shape"])) for s in sol.load_surfaces(0)]
    assert faces == [256, 256, 258, 258, 16512, 16512]
    _hold(sol, what="big")
    sol.close()


# ---- absolute signs -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box_euler", "box_laminar"])
def test_closed_box_at_rest(name):
    """all six sides walls, gas at rest at uniform p: every side is pushed outwards with p A,
    and the six forces cancel within the bound"""
    case = loads_ref.CASES[name]()
    sol = Solver(_lib(), case)
    surfs = sol.load_surfaces(0)
    assert [s["side"] for s in surfs] == [1, 2, 3, 4, 5, 6]
    got = _hold(sol, what=name)[0]
    ref = loads_ref.block_reference(sol, 0)
    p = 101325.0                              # synthetic.make_deck
    total, bound = np.zeros(3), np.zeros(3)
    for q, s in enumerate(surfs):
        d = (s["side"] - 1) // 2
        area = ref[q]["area"][0]
        assert abs(area - 1.0) <= 1e-12       # a unit box
        for c, x in enumerate("xyz"):
            want = -loads_ref.sigma(s["side"]) * p * area if c == d else 0.0
            f, bd = got["pressureForce_" + x][q], ref[q]["pressureForce_" + x][1]
            print(f"{name} side {s['side']} pressureForce_{x}: {f:.17g} analytic {want:.17g} "
                  f"bound {bd:.3e}")
            assert abs(f - want) <= bd + 4.0 * 2.0 ** -52 * abs(want)
            total[c] += f
            bound[c] += bd
    print(f"{name} total pressure force {total} bound {bound}")
    assert np.all(np.abs(total) <= bound)
    assert got["pressureForce_x"][0] < 0.0 < got["pressureForce_x"][1]      # i-min towards -x
    sol.close()


def test_uploaded_shear_flow_drags_the_walls():
    """u = a y (a > 0), uniform T: the j-min wall is dragged towards +x with mu(T) a A, the
    j-max wall, which moves with the gas next to it, towards -x.  Each wall is three surfaces
    along k; the middle ones read no ghost cell of the k sides.  (The ghost cells of the i
    sides -- slip walls -- hold v = w = 0 like the field, and d u / d x of their cells enters
    the normal stress only, not the x component on a j-face.)"""
    case = loads_ref.CASES["couette"]()
    sol = Solver(_lib(), case)
    surfs = sol.load_surfaces(0)
    walls = [q for q, s in enumerate(surfs) if s["bc_type"] == "viscousWall"]
    assert len(walls) == 6
    got = sol.wall_loads(0, ELEVEN)
    ref = loads_ref.block_reference(sol, 0)
    loads_ref.compare(got, ref, ELEVEN, what="couette")
    gas = case.gas
    state = case.blocks[0].state
    g = case.ng
    t_dim = state[g, g, g, 4] / (state[g, g, g, 0] * gas.gas_constant) * gas.t_ref
    mu = gas.visc_c1 * t_dim ** 1.5 / (t_dim + gas.visc_s)
    checked = 0
    for q in walls:
        s = surfs[q]
        if s["range"][4] == 0 or s["range"][5] == loads_ref.COUETTE_N[2]:
            continue
        area = ref[q]["area"][0]
        want = loads_ref.sigma(s["side"]) * mu * loads_ref.COUETTE_A * area
        f, bd = got["viscousForce_x"][q], ref[q]["viscousForce_x"][1]
        print(f"couette side {s['side']} viscousForce_x {f:.17g} analytic {want:.17g} "
              f"bound {bd:.3e}")
        assert abs(f - want) <= bd
        checked += 1
    assert checked == 2
    j_min = [q for q in walls if surfs[q]["side"] == 3]
    assert all(got["viscousForce_x"][q] > 0.0 for q in j_min)
    sol.close()


# ---- moments ------------------------------------------------------------------------------------
def _moment_solver(geometry):
    host = loads_ref.CASES["moments"]()
    if geometry == "host":
        return Solver(_lib(), host)
    case = synthetic.single_block_case(loads_ref.MOMENT_N, bcs=loads_ref.MOMENT_BCS,
                                       geometry="device", **loads_ref.MOMENT_KW,
                                       **loads_ref.LAMINAR)
    case.blocks[0].state[...] = host.blocks[0].state       # (the perturbed state)
    return Solver(_lib(), case)


def test_moments_on_device_geometry_and_their_refusal_on_host_geometry():
    nodes = synthetic.box_nodes(*loads_ref.MOMENT_N, loads_ref.MOMENT_KW["stretch"],
                                skew=loads_ref.MOMENT_KW["skew"])
    dev = _moment_solver("device")
    assert dev.load_names(0) == ALL
    got = _hold(dev, ALL, nodes=nodes, what="moments")[0]
    assert [s["bc_type"] for s in dev.load_surfaces(0)] == \
        ["viscousWall", "slipWall", "viscousWall", "viscousWall", "slipWall"]
    # the shift to another reference point: M - r x F, against the reference about it
    about = np.array([0.7, -0.4, 1.9])                       # metres
    shifted = dev.wall_loads(0, loads_ref.MOMENTS, about=about)
    ref0 = loads_ref.block_reference(dev, 0, nodes=nodes - about / dev.case.gas.l_ref)
    ref = loads_ref.block_reference(dev, 0, nodes=nodes)
    for q in range(len(ref)):
        for kind in ("pressure", "viscous"):
            fb = [ref[q][f"{kind}Force_{c}"][1] for c in "xyz"]
            for c, x in enumerate("xyz"):
                c1, c2 = (c + 1) % 3, (c + 2) % 3
                ex, bd = ref0[q][f"{kind}Moment_{x}"]
                bd = bd + ref[q][f"{kind}Moment_{x}"][1] + abs(about[c1]) * fb[c2] + \
                    abs(about[c2]) * fb[c1]
                assert abs(shifted[f"{kind}Moment_{x}"][q] - ex) <= bd, (q, kind, x)
    total = dev.total_loads()
    for n in ALL:
        assert abs(total[n] - sum(float(v) for v in got[n])) <= 1e-15 * sum(abs(v) for v in got[n])
    host = _moment_solver("host")
    assert host.load_names(0) == ELEVEN
    for n in loads_ref.MOMENTS:
        with pytest.raises(RuntimeError, match=r"is a moment.*agx_block_geom carries no face "
                                               r"centres.*nodes"):
            host.wall_loads(0, [n])
    _hold(host, ELEVEN, what="moments, host geometry")
    mine = host.wall_loads(0)
    for q, r in enumerate(ref):
        for n in ELEVEN:
            # both runs within their bounds of references that differ by the geometry's roundings
            assert abs(mine[n][q] - got[n][q]) <= 2.0 * r[n][1] + 64 * 2.0 ** -52 * abs(got[n][q]), n
    dev.close(), host.close()


# ---- determinism and the id rules -----------------------------------------------------------------
def _raw(sol, gb, ids, n=None, size=4096):
    arr = (C.c_int32 * len(ids))(*ids)
    out = np.zeros(size)
    sol.api.check(sol.api.output_pack(sol.ctx, sol.block_ids[gb], len(ids) if n is None else n,
                                      arr, out.ctypes.data_as(abi.c_dp)), "output_pack")
    return out


def test_contract_determinism_id_rules_and_no_side_effects():
    def make():
        s = Solver(_lib(), loads_ref.CASES["contract"]())
        s.step(0), s.step(1)
        return s
    sol, plain = make(), make()
    nsurf = len(sol.load_surfaces(0))
    ids = [abi.LOAD_OUT[n] for n in ELEVEN]
    full = _raw(sol, 0, ids)[:11 * nsurf].reshape(11, nsurf)
    assert np.array_equal(full, _raw(sol, 0, ids)[:11 * nsurf].reshape(11, nsurf))
    assert np.all(full[0] > 0.0)
    # a subset, a reordering and a repetition are rows of the full call, bit for bit
    pick = ["heatLoad", "area", "viscousForce_z", "heatLoad", "pressureForce_y"]
    raw = _raw(sol, 0, [abi.LOAD_OUT[n] for n in pick])[:5 * nsurf].reshape(5, nsurf)
    for row, n in zip(raw, pick):
        assert np.array_equal(row, full[ELEVEN.index(n)]), n
    rows = _raw(sol, 0, [abi.LOAD_OUT["area_x"]] * 17)[:17 * nsurf].reshape(17, nsurf)
    assert all(np.array_equal(r, full[ELEVEN.index("area_x")]) for r in rows)
    # refusals, by their message
    load = abi.LOAD_OUT["area"]
    with pytest.raises(RuntimeError, match="cell and load variables in one call"):
        _raw(sol, 0, [abi.OUT["density"], load])
    with pytest.raises(RuntimeError, match="wall and load variables in one call"):
        _raw(sol, 0, [load, abi.WALL_OUT["yplus"]])
    with pytest.raises(RuntimeError, match="node and load variables in one call"):
        _raw(sol, 0, [abi.NODE_OUT["density"], load])
    with pytest.raises(RuntimeError, match="nvar 18 out of range"):
        _raw(sol, 0, [load] * 18)
    for bad in (255, 273, 182, 127):
        with pytest.raises(RuntimeError, match="unknown output variable"):
            _raw(sol, 0, [bad])
    far = synthetic.single_block_case((8, 6, 5), bcs={s: ("characteristic", 1) for s in range(1, 7)},
                                      **loads_ref.NS)
    s2 = Solver(_lib(), far)
    with pytest.raises(RuntimeError, match="has no viscousWall or slipWall surface"):
        _raw(s2, 0, [load])
    s2.close()
    # an euler block with slip walls: the wall payload is refused, the loads are there
    euler = synthetic.single_block_case((8, 6, 5), **loads_ref.EULER)
    s3 = Solver(_lib(), euler)
    with pytest.raises(RuntimeError, match="need a viscous context"):
        _raw(s3, 0, [abi.WALL_OUT["yplus"]])
    _hold(s3, what="euler slip walls")
    s3.close()
    # the cell payload is the same before and after a load call, bit for bit
    names = ["density", "velGrad_vx", "tempGrad_y", "resid_energy", "pressure"]
    before = plain.output_pack(0, names)
    assert np.array_equal(sol.output_pack(0, names), before)
    sol.wall_loads(0)
    assert np.array_equal(sol.output_pack(0, names), before)
    # ... and one more step gives the run without the load calls
    a, b = sol.step(2), plain.step(2)
    assert np.array_equal(a["l2"], b["l2"]) and a["linf"] == b["linf"]
    assert np.array_equal(sol.download("state", 0), plain.download("state", 0))
    sol.close(), plain.close()


# ---- reads between phases ---------------------------------------------------------------------------
class _LoadProber(probe.Prober):
    """probe.Prober with a kind of its own: a load call on every block after every hooked
    entry; a refusal must carry the FILL_OPEN message"""

    def __init__(self):
        super().__init__("loads")
        self.refused_at = set()

    def _loads(self, s, lev, label, obs):
        for gb in s.block_ids:
            if not s.load_surfaces(gb):
                continue
            try:
                obs[(lev, gb, "loads")] = np.stack(list(s.wall_loads(gb, ELEVEN).values()))
            except RuntimeError as exc:
                assert probe.FILL_OPEN.search(str(exc)), str(exc)
                self.refused_at.add(label)


def _probed(make, lib):
    base = probe.run(lib, make, "phased")[0]
    prober = _LoadProber()
    proxy = probe.ProbingApi(lib, prober)
    top = probe.PhasedSolver(proxy, make(), 0, None, None)
    final = {}
    try:
        prober.solvers = [top]
        for nn in range(2):
            top.step(nn)
        prober.solvers = []
        g = top.case.ng
        for gb in top.block_ids:
            for f in ("state", "update"):
                final[(0, gb, f)] = top.download(f, gb)[g:-g, g:-g, g:-g]
            for f in ("residual", "dt", "cons_n", "cons_nm1"):
                final[(0, gb, f)] = top.download(f, gb)
        for q, h in enumerate(top.history):
            final[("history", q, "l2")] = np.array(h["l2"])
            final[("history", q, "linf")] = np.array(h["linf"], dtype=float)
            final[("history", q, "matrix")] = np.array(h["matrix"])
    finally:
        top.close()
    assert probe.differences(base, final) == {}
    return prober


def test_load_calls_between_the_phases_of_a_laminar_run():
    make = lambda: synthetic.single_block_case((7, 6, 5), stretch=1.2, skew=0.01,
                                               bcs=loads_ref.WALLS, matrix_solver="lusgs",
                                               matrix_sweeps=2, **loads_ref.NS)
    prober = _probed(make, _lib())
    want = {label for label, kind in probe.expected_refusals(prober.labels)}
    assert want and prober.refused_at == want, (sorted(prober.refused_at), sorted(want))
    assert len(prober.seen) == len(prober.labels)
    answered = [pos for pos, obs in prober.seen.items() if obs]
    assert len(answered) == sum(1 for label in prober.labels if label not in want)


def test_load_calls_between_the_phases_of_an_euler_run():
    make = lambda: synthetic.single_block_case((7, 6, 5), stretch=1.2, skew=0.01,
                                               time_integration="rk4", cfl=0.5)
    prober = _probed(make, _lib())
    assert prober.refused_at == set()
    assert prober.labels and all(prober.seen[pos] for pos in range(len(prober.labels)))
