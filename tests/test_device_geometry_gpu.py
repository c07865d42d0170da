"""A block's whole geometry built on the device from its nodes (agx_block_geom.nodes) against
the host pipeline fed with the same device metrics (build_case(setup=DeviceSetup)).

After the metrics every set-up step is a copy, a sign flip or a single add / subtract, so
volume, centre and the face areas must agree bit for bit at every entry, corners included;
widths and wall distance hold the sqrt of a dot product the device compiler may contract and
are held to rtol = 1e-14 (the bound test_setup_device.py uses for the wall search)."""
import ctypes as C
import os

import numpy as np
import pytest

import aither_amd
from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.case.builder import build_case
from aither_amd.solver import DeviceSetup, Solver
from conftest import GOLDEN
from parity_utils import RTOL, rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
EXACT = ("volume", "center", "farea_i", "farea_j", "farea_k")
CLOSE = ("width_i", "width_j", "width_k", "wall_dist")
WALL = {3: ("viscousWall", 2)}
CUBE_KW = dict(bcs=WALL, equation_set="navierStokes", time_integration="implicitEuler",
               cfl=5.0)


def _golden(name):
    return os.path.join(GOLDEN, "cases", name, name + ".inp")


def _tp_path():
    return os.path.join(HERE, "golden", "thermallyPerfect", "thermallyPerfect.inp")


# name -> builder(**build_case keywords)
CASES = {
    "uniformFlow": lambda **kw: build_case(_golden("uniformFlow"), **kw),
    "wallLaw": lambda **kw: build_case(_golden("wallLaw"), **kw),
    "rae2822": lambda **kw: build_case(_golden("rae2822"), **kw),
    "shockTube": lambda **kw: build_case(_golden("shockTube"), **kw),
    "thermallyPerfect": lambda **kw: build_case(_tp_path(), **kw),
    "couette": lambda **kw: build_case(_golden("couette"), **kw),
    "cube222": lambda **kw: synthetic.cube_blocks_case((6, 5, 4), (2, 2, 2), **CUBE_KW, **kw),
    "cube321": lambda **kw: synthetic.cube_blocks_case((6, 5, 4), (3, 2, 1), **CUBE_KW, **kw),
}


def _lib(case):
    return aither_amd.load(case.n_eq, case.gas.thermodynamic_model)


def _pair(name, **deck_kw):
    """(host pipeline on device metrics, device-built twin with the same state, library)"""
    make = CASES[name]
    probe = make(geometry="device", **deck_kw)
    lib = _lib(probe)
    setup = DeviceSetup(lib)
    host = make(setup=setup, **deck_kw)
    setup.close()
    for bh, bd in zip(host.blocks, probe.blocks):
        bd.state = bh.state.copy()
    return host, probe, lib


def _host_array(geom, name):
    if name == "volume":
        return geom.vol.a
    if name == "center":
        return geom.center.a
    if name == "wall_dist":
        return geom.wall_dist.a
    kind, d = name.split("_")
    return (geom.farea if kind == "farea" else geom.width)[d].a


def test_every_branch_is_covered_by_the_cases():
    """What the list of cases is there for (checked on the host code)."""
    host = CASES["uniformFlow"]()
    assert len(host.blocks) == 10 and len(host.connections) == 9
    assert {c.orientation for c in host.connections} == set(range(1, 9))
    assert CASES["shockTube"](geometry="device").ng == 3
    assert CASES["thermallyPerfect"](geometry="device").ng == 1
    rae = CASES["rae2822"](geometry="device")
    assert any(c.block[0] == c.block[1] for c in rae.connections)
    cou = CASES["couette"](geometry="device")
    assert any(not c.is_interblock for c in cou.connections)
    for name, nconn, nchanged in (("cube222", 12, 9), ("cube321", 7, 4)):
        h, d = CASES[name](), CASES[name](geometry="device")
        assert len(h.connections) == nconn
        assert sum(a.border != b.border for a, b in zip(h.connections, d.connections)) == nchanged


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_geometry_equals_host_pipeline(name):
    host, dev, lib = _pair(name)
    s = Solver(lib, dev)
    worst = {}
    try:
        for gb, blk in enumerate(host.blocks):
            for f in EXACT + CLOSE:
                got, ref = s.geometry(f, gb), _host_array(blk.geom, f)
                assert got.shape == ref.shape, (f, gb)
                if f in EXACT:
                    diff = got.view(np.uint64) != ref.view(np.uint64)
                    worst[f] = max(worst.get(f, 0), int(diff.sum()))
                else:
                    scale = np.where(ref != 0.0, np.abs(ref), 1.0)
                    worst[f] = max(worst.get(f, 0.0), float((np.abs(got - ref) / scale).max()))
        print(f"{name}: entries that differ in bits / largest relative difference: {worst}")
        for gb, blk in enumerate(host.blocks):
            for f in EXACT:
                got, ref = s.geometry(f, gb), _host_array(blk.geom, f)
                bad = np.argwhere(got.view(np.uint64) != ref.view(np.uint64))
                assert bad.size == 0, (name, f, gb, len(bad), bad[:5].tolist())
            for f in CLOSE:
                np.testing.assert_allclose(s.geometry(f, gb), _host_array(blk.geom, f),
                                           rtol=1e-14, atol=0.0, err_msg=f"{name} {f} {gb}")
    finally:
        s.close()


def _run_both(host, dev, lib, steps=3):
    sh, sd = Solver(lib, host), Solver(lib, dev)
    try:
        for nn in range(steps):
            sh.step(nn), sd.step(nn)
        assert len(sh.history) == len(sd.history) > 0
        for a, b in zip(sd.history, sh.history):
            e = rel_err(a["l2"][None, :], b["l2"][None, :])
            print(f"step {b['nn']}.{b['mm']}: L2 rel err {e:.2e}")
            assert e < RTOL, (b["nn"], b["mm"], e, a["l2"], b["l2"])
        for gb in sh.block_ids:
            a, b = sd.download("state", gb), sh.download("state", gb)
            assert np.all(np.isfinite(b))
            e = rel_err(a, b)
            print(f"block {gb}: state rel err {e:.2e}")
            assert e < RTOL, (gb, e)
    finally:
        sh.close(), sd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,deck_kw", [
    ("cube222", dict(matrix_solver="lusgs")),
    ("cube222", dict(matrix_solver="blusgs")),
    ("uniformFlow", {}),
    ("wallLaw", {}),
])
def test_borders_reach_the_halo_maps(name, deck_kw):
    """Same state, three implicit iterations: a halo map built from borders SwapGeomSlice did
    not update copies ghost cells the host-built solver leaves alone."""
    host, dev, lib = _pair(name, **deck_kw)
    if deck_kw:
        assert host.deck.matrix_solver == deck_kw["matrix_solver"] and host.deck.is_viscous()
    assert host.deck.is_implicit()
    _run_both(host, dev, lib)


@pytest.mark.gpu
def test_geometry_round_trip_of_an_array_built_block():
    host, _, lib = _pair("wallLaw")
    s = Solver(lib, host)
    try:
        for gb, blk in enumerate(host.blocks):
            for f in EXACT + CLOSE:
                got, ref = s.geometry(f, gb), np.ascontiguousarray(_host_array(blk.geom, f))
                assert got.shape == ref.shape
                assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (f, gb)
        # ... and they cannot be uploaded
        a = np.ascontiguousarray(host.blocks[0].geom.vol.a)
        rc = lib.field_upload(s.ctx, s.block_ids[0], abi.FIELD["volume"],
                              a.ctypes.data_as(abi.c_dp))
        assert rc != 0 and b"cannot be uploaded" in lib.last_error()
    finally:
        s.close()


def _ctx(lib, case):
    from aither_amd.case import builder
    ctx = C.c_void_p()
    lib.check(lib.ctx_create(0, 0, C.byref(ctx)), "ctx_create")
    cfg = builder.config_struct(case)
    lib.check(lib.config_set(ctx, C.byref(cfg)), "config_set")
    return ctx


def _node_geom(x, ng):
    x = np.ascontiguousarray(x, dtype=np.float64)
    bg = abi.BlockGeom()
    bg.nk, bg.nj, bg.ni = (n - 1 for n in x.shape[:3])
    bg.ng = ng
    bg.nodes = x.ctypes.data_as(abi.c_dp)
    return bg, x


@pytest.mark.gpu
def test_refusals():
    lib = aither_amd.load()
    kw = dict(time_integration="implicitEuler")
    host = synthetic.single_block_case((6, 5, 4), **kw)
    g = host.blocks[0].geom
    bid = C.c_int(-1)

    # nodes together with an array: named
    ctx = _ctx(lib, host)
    bg, keep = _node_geom(g.nodes, g.ng)
    vol = np.ascontiguousarray(g.vol.a)
    bg.vol = vol.ctypes.data_as(abi.c_dp)
    assert lib.block_create(ctx, C.byref(bg), C.byref(bid)) != 0
    assert b"nodes given together with vol" in lib.last_error()
    # a block turned inside out: the message of the host metrics
    bg, keep = _node_geom(g.nodes[:, :, ::-1], g.ng)
    assert lib.block_create(ctx, C.byref(bg), C.byref(bid)) != 0
    assert b"negative volume" in lib.last_error()
    lib.ctx_destroy(ctx)

    # node-built and array-built blocks in one context, either order
    ctx = _ctx(lib, host)
    bg, keep = _node_geom(g.nodes, g.ng)
    lib.check(lib.block_create(ctx, C.byref(bg), C.byref(bid)), "block_create")
    s_host = Solver(lib, host)             # (an array-built block is fine in its own context)
    s_host.close()
    ab = abi.BlockGeom()
    ab.ni, ab.nj, ab.nk, ab.ng = g.ni, g.nj, g.nk, g.ng
    arrs = [np.ascontiguousarray(a) for a in (
        g.farea["i"].a, g.farea["j"].a, g.farea["k"].a, g.vol.a, g.center.a, g.width["i"].a,
        g.width["j"].a, g.width["k"].a, g.wall_dist.a)]
    for nm, a in zip(("farea_i", "farea_j", "farea_k", "vol", "center", "width_i", "width_j",
                      "width_k", "wall_dist"), arrs):
        setattr(ab, nm, a.ctypes.data_as(abi.c_dp))
    assert lib.block_create(ctx, C.byref(ab), C.byref(bid)) != 0
    assert b"not both" in lib.last_error()
    lib.ctx_destroy(ctx)
    ctx = _ctx(lib, host)
    lib.check(lib.block_create(ctx, C.byref(ab), C.byref(bid)), "block_create")
    assert lib.block_create(ctx, C.byref(bg), C.byref(bid)) != 0
    assert b"not both" in lib.last_error()
    lib.ctx_destroy(ctx)

    # a connection whose partner lives on another rank
    dev = synthetic.stacked_blocks_case((6, 5, 4), nblocks=2, geometry="device", **kw)
    dev.blocks[1].rank = 1
    for c in dev.connections:
        c.rank = [0, 1]
    with pytest.raises(RuntimeError, match="another rank"):
        Solver(lib, dev, rank=0)
