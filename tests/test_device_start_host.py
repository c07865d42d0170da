"""Start and resume on the device, the parts that need no GPU: the C-ABI tables carry the three
entries (agx_state_fill, agx_state_from_cloud, agx_restart_unpack), a state recipe realised on
the host is the array build_case(initial="host") builds, and the numpy restatement of the
reference's restart readers (tests/restart_ref.py) inverts the oracle's restart pack.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import aither_amd
import restart_ref
from aither_amd import abi
from aither_amd.case import builder, synthetic
from aither_amd.case.builder import build_case
from aither_amd.solver import Solver
from conftest import GOLDEN, ROOT

ENTRIES = ("state_fill", "state_from_cloud", "restart_unpack")
VORTEX = os.path.join(GOLDEN, "cases", "convectingVortex", "convectingVortex.inp")
WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("pressureOutlet", 3)}
ULP = 2.0 ** -52


def test_abi_tables_carry_the_three_entries():
    header = open(os.path.join(ROOT, "include", "aither_gfx950.h")).read()
    wrappers = open(os.path.join(ROOT, "include", "aither_gfx950.hpp")).read()
    for name in ENTRIES:
        assert name in abi.SYMBOLS, name
        assert re.search(r"\bint agx_%s\s*\(agx_ctx \*ctx, int block," % name, header), name
        assert "AGX_SYM(%s)(ctx_, block," % name in wrappers, name
    assert abi.SYMBOLS["state_fill"][1] == [ctypes.c_void_p, ctypes.c_int, abi.c_dp]
    assert abi.SYMBOLS["state_from_cloud"][1] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                                  abi.c_dp, abi.c_dp, abi.c_dp]
    assert abi.SYMBOLS["restart_unpack"][1] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                abi.c_dp]
    # all four libraries export them (load only: no GPU call)
    for path in (aither_amd.LIB_PATH, aither_amd.RANS_LIB_PATH, aither_amd.TP_LIB_PATH,
                 aither_amd.RANS_TP_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in ENTRIES:
            assert hasattr(lib, "agx_" + name), (path, name)


def test_device_only_entries_refuse_by_name_where_a_library_lacks_them(oracle):
    """The CPU oracle has no device to form a state on: its bound names refuse when called;
    the product library must export them."""
    assert set(abi.DEVICE_ONLY) == set(ENTRIES)
    for name in ENTRIES:
        with pytest.raises(NotImplementedError, match="ora_" + name):
            getattr(oracle, name)(None, 0, None)

    class Empty:
        pass
    with pytest.raises(AttributeError):
        abi.Api(Empty(), "agx_")


def _same_blocks(host, dev):
    assert len(host.blocks) == len(dev.blocks)
    for bh, bd in zip(host.blocks, dev.blocks):
        assert isinstance(bd.state, builder.StateRecipe) and isinstance(bh.state, np.ndarray)
        got = builder.realise(bd.state, bd.geom)
        assert got.shape == bh.state.shape and np.array_equal(got, bh.state)
    return [b.state.kind for b in dev.blocks]


def test_realise_of_a_cloud_recipe_is_the_host_array():
    for geometry in ("host", "device"):
        host = build_case(VORTEX, geometry=geometry)
        dev = build_case(VORTEX, geometry=geometry, initial="device")
        assert _same_blocks(host, dev) == ["cloud"]
        r = dev.blocks[0].state
        assert r.pts.shape == (1521, 3) and r.st.shape == (1521, 5)
        g = host.ng
        assert np.all(host.blocks[0].state[g:-g, g:-g, g:-g, 0] > 0.0)


@pytest.mark.parametrize("kw", [
    dict(),
    dict(bcs={3: ("viscousWall", 2)}, equation_set="rans", turbulence_model="sst2003",
         time_integration="implicitEuler", cfl=5.0, turbulence=(0.02, 5.0)),
    dict(face_reconstruction="weno", limiter="none"),            # three ghost layers
])
def test_realise_of_a_uniform_recipe_is_the_host_array(kw):
    host = synthetic.single_block_case((7, 5, 3), stretch=1.1, amplitude=0.0, **kw)
    dev = synthetic.single_block_case((7, 5, 3), stretch=1.1, initial="device", **kw)
    assert _same_blocks(host, dev) == ["uniform"]
    assert dev.blocks[0].state.prim.shape == (dev.n_eq,)
    g = host.ng
    assert np.all(host.blocks[0].state[:g] == 0.0) and np.all(host.blocks[0].state[g:-g, g:-g, g:-g] != 0.0)


def test_initial_device_is_refused_with_multigrid_and_bad_values():
    deck = synthetic.make_deck(time_integration="implicitEuler")
    deck.bcs = [synthetic.box_surfaces(8, 8, 8)]
    deck.multigrid_levels = 2
    coords = [synthetic.box_nodes(8, 8, 8)]
    with pytest.raises(NotImplementedError, match="initial='device' with multigridLevels"):
        build_case(None, deck=deck, coords=coords, initial="device")
    deck.multigrid_levels = 1
    with pytest.raises(ValueError, match="initial='nowhere'"):
        build_case(None, deck=deck, coords=coords, initial="nowhere")
    with pytest.raises(ValueError, match="kind 'other'"):
        builder.realise(builder.StateRecipe("other"), None)


def _bdf2_case(kind):
    if kind == "rans":
        return synthetic.single_block_case((9, 7, 5), stretch=1.15, bcs=WALL, equation_set="rans",
                                           turbulence_model="sst2003", time_integration="bdf2",
                                           matrix_solver="lusgs", nonlinear_iterations=2,
                                           dt=2.0e-6, cfl=-1.0)
    return synthetic.single_block_case((10, 8, 6), stretch=1.2, skew=0.01, bcs=WALL,
                                       equation_set="navierStokes", time_integration="bdf2",
                                       matrix_solver="lusgs", nonlinear_iterations=2, dt=2.0e-6,
                                       cfl=-1.0)


@pytest.mark.parametrize("kind", ["laminar", "rans"])
def test_restart_ref_inverts_the_oracle_pack(kind, oracle):
    """(x s) / s: two roundings, so restart_ref.unpack of the oracle's payload is within
    2 units of 2^-52 relative of the oracle's own state and consVarsNm1."""
    case = _bdf2_case(kind)
    s = Solver(oracle, case)
    for nn in range(3):
        s.step(nn)
    g = case.ng
    gas = s.cfg.gas
    for which, ref in ((0, s.download("state", 0)[g:-g, g:-g, g:-g]),
                       (1, s.download("cons_nm1", 0))):
        payload = s.restart_pack(0, which)
        assert payload.shape == ref.shape[:3] + (case.n_eq + 1,)
        got = restart_ref.unpack(payload, gas, which)
        assert got.shape == ref.shape
        nz = ref != 0.0
        worst = float((np.abs(got - ref)[nz] / np.abs(ref)[nz]).max())
        print(f"{kind} which={which}: worst relative difference {worst / ULP:.3f} x 2^-52")
        assert np.all(np.abs(got - ref) <= 2.0 * ULP * np.abs(ref)), (kind, which, worst / ULP)
        # the divisors are those of the library's pack, in the reference's order
        d = restart_ref.divisors(gas, which)
        assert d[4] == gas.rho_ref * gas.a_ref * gas.a_ref
    pad = restart_ref.padded(got, g)
    assert pad.shape == s.download("state", 0).shape and np.all(pad[:g] == 0.0)
    s.close()
