"""A block's geometry built on the device from its nodes (agx_block_geom.nodes), CPU side:
the header, abi.py and the host layers that hand the nodes over.  The device code itself is
held to the host pipeline in test_device_geometry_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, GOLDEN
from aither_amd import abi
from aither_amd.case import connections, geometry, synthetic
from aither_amd.case.builder import build_case

GEOM_NAMES = ("volume", "center", "farea_i", "farea_j", "farea_k", "width_i", "width_j",
              "width_k", "wall_dist")
METRIC_ATTRS = ("vol", "center", "farea", "fcen", "width", "wall_dist")
WALL = {3: ("viscousWall", 2)}


def _header():
    return open(os.path.join(ROOT, "include", "aither_gfx950.h")).read()


def test_nodes_is_the_last_field_of_the_block_descriptor():
    body = re.search(r"typedef struct agx_block_geom \{(.*?)\} agx_block_geom;", _header(),
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls[-1] == "const double *nodes"
    names = [n for n, _ in abi.BlockGeom._fields_]
    assert names[-1] == "nodes" and names[-2] == "wall_dist"
    # appended only: every earlier field sits where it sat (6 ints, 9 pointers)
    assert abi.BlockGeom.nodes.offset == 24 + 9 * ctypes.sizeof(ctypes.c_void_p)
    assert abi.BlockGeom.wall_dist.offset == 24 + 8 * ctypes.sizeof(ctypes.c_void_p)
    assert not abi.BlockGeom().nodes              # zero-initialised: the array path


def test_geometry_field_ids_match_the_header():
    ids = {m.group(1).lower(): int(m.group(2))
           for m in re.finditer(r"AGX_FIELD_(\w+)\s*=\s*(\d+)", _header())}
    for name in GEOM_NAMES:
        assert abi.FIELD[name] == ids[name], name
        assert name in abi.GEOM_FIELDS
    assert sorted(abi.FIELD[n] for n in GEOM_NAMES) == list(range(14, 23))
    assert len(set(abi.FIELD.values())) == len(abi.FIELD)


def _cases():
    path = lambda name: os.path.join(GOLDEN, "cases", name, name + ".inp")
    yield "uniformFlow", lambda **kw: build_case(path("uniformFlow"), **kw)
    yield "wallLaw", lambda **kw: build_case(path("wallLaw"), **kw)
    yield "cube", lambda **kw: synthetic.cube_blocks_case(
        (6, 5, 4), (2, 2, 2), bcs=WALL, equation_set="navierStokes",
        time_integration="implicitEuler", **kw)


@pytest.mark.parametrize("name", ["uniformFlow", "wallLaw", "cube"])
def test_device_case_has_the_host_case_minus_its_metrics(name):
    make = dict(_cases())[name]
    host, dev = make(), make(geometry="device")
    assert len(host.blocks) == len(dev.blocks) and host.total_cells == dev.total_cells
    assert host.n_eq == dev.n_eq and host.ng == dev.ng
    for bh, bd in zip(host.blocks, dev.blocks):
        assert isinstance(bd.geom, geometry.NodeGeometry)
        assert bd.geom.n == bh.geom.n and bd.geom.ng == bh.geom.ng
        for attr in METRIC_ATTRS:
            assert not hasattr(bd.geom, attr), attr
        assert bd.geom.nodes.flags["C_CONTIGUOUS"] and bd.geom.nodes.dtype == np.float64
        np.testing.assert_array_equal(bd.geom.nodes, bh.geom.nodes)
        assert bd.state.shape == bh.state.shape
        assert bd.surfaces == bh.surfaces
        assert (bd.parent, bd.global_pos, bd.rank, bd.local_pos) == \
            (bh.parent, bh.global_pos, bh.rank, bh.local_pos)
    # the connections as found, before SwapGeomSlice's border update (which the host build
    # has applied to its own and the library applies to its stored copy)
    coords = [b.geom.nodes for b in host.blocks]
    found = connections.find_connections(host.deck.bcs, coords, host.deck)
    assert len(dev.connections) == len(found) == len(host.connections)
    for cd, cf, ch in zip(dev.connections, found, host.connections):
        assert cd == cf
        for f in ("rank", "block", "local_block", "boundary", "d1s", "d1e", "d2s", "d2e",
                  "const_surf", "orientation", "is_interblock"):
            assert getattr(cd, f) == getattr(ch, f), f
        assert all(h or not d for d, h in zip(cd.border, ch.border))   # borders only get set


def test_cube_host_build_changes_borders_the_device_case_does_not_hold():
    """The case the GPU test relies on: the T-intersection rule fires on the host."""
    make = dict(_cases())["cube"]
    host, dev = make(), make(geometry="device")
    changed = sum(ch.border != cd.border for ch, cd in zip(host.connections, dev.connections))
    assert changed == 9 and len(host.connections) == 12


def test_device_geometry_is_refused_across_ranks_and_bad_values():
    with pytest.raises(NotImplementedError, match="several ranks"):
        synthetic.stacked_blocks_case((4, 4, 4), nblocks=2, ranks=[0, 1], geometry="device")
    with pytest.raises(ValueError, match="geometry"):
        synthetic.single_block_case((4, 4, 4), geometry="gpu")


def test_oracle_takes_the_longer_descriptor(oracle):
    """The oracle's descriptor ends before `nodes`; a host-built case still runs on it."""
    from aither_amd.solver import Solver
    case = synthetic.single_block_case((6, 5, 4), time_integration="implicitEuler")
    s = Solver(oracle, case)
    out = s.step(0)
    assert np.all(np.isfinite(out["l2"]))
    s.close()
