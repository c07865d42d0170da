"""Integrated wall loads, host side: the ids of the header against abi.LOAD_OUT, the numpy
reference of tests/loads_ref.py on cases with closed-form answers, and the proof that the bound
of loads_ref has teeth on every case tests/test_wall_loads_gpu.py uses -- leaving out any single
face, or flipping sigma on any surface, moves `area` or `pressureForce` beyond it."""
import os
import re

import numpy as np
import pytest

import loads_ref
from aither_amd import abi
from aither_amd.case import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "aither_gfx950.h")) as fh:
        return fh.read()


def _load_enum():
    body = re.search(r"enum \{ (AGX_LOAD_BASE = (\d+),.*?AGX_LOAD_END) \};", _header(), re.S)
    assert body, "the header has no AGX_LOAD_* enum"
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    enum, nxt = {}, 0
    for item in (t.strip() for t in text.split(",")):
        if "=" in item:
            name, val = (t.strip() for t in item.split("="))
            nxt = enum[val] if val in enum else int(val)
        else:
            name = item
        enum[name] = nxt
        nxt += 1
    return enum


HEADER_NAMES = {"area": "AREA", "heatLoad": "HEAT"}
for _k, _h in (("area", "AREA"), ("pressureForce", "PRESSURE_FORCE"),
               ("viscousForce", "VISCOUS_FORCE"), ("pressureMoment", "PRESSURE_MOMENT"),
               ("viscousMoment", "VISCOUS_MOMENT")):
    for _c in "xyz":
        HEADER_NAMES[f"{_k}_{_c}"] = f"{_h}_{_c.upper()}"


def test_load_ids_match_the_header():
    enum = _load_enum()
    assert enum["AGX_LOAD_BASE"] == 256 == abi.LOAD_BASE
    assert enum["AGX_LOAD_END"] == 256 + 17 and len(abi.LOAD_OUT) == 17
    assert set(HEADER_NAMES) == set(abi.LOAD_OUT)
    for name, h in HEADER_NAMES.items():
        assert abi.LOAD_OUT[name] == enum["AGX_LOAD_" + h], name
    # the order of the issue's table
    order = ["area", "area_x", "area_y", "area_z", "pressureForce_x", "pressureForce_y",
             "pressureForce_z", "viscousForce_x", "viscousForce_y", "viscousForce_z", "heatLoad",
             "pressureMoment_x", "pressureMoment_y", "pressureMoment_z", "viscousMoment_x",
             "viscousMoment_y", "viscousMoment_z"]
    assert [abi.LOAD_OUT[n] for n in order] == list(range(256, 273))
    assert list(abi.LOAD_MOMENTS) == order[11:]


def test_the_four_id_ranges_do_not_overlap():
    text = _header()
    count = int(re.search(r"AGX_OUT_COUNT = (\d+)", text).group(1))
    ranges = [set(range(0, count)), set(abi.WALL_OUT.values()),
              set(range(abi.NODE_BASE, abi.NODE_BASE + count)), set(abi.LOAD_OUT.values())]
    assert set(abi.OUT.values()) <= ranges[0] and set(abi.NODE_OUT.values()) <= ranges[2]
    for a in range(4):
        for b in range(a + 1, 4):
            assert not ranges[a] & ranges[b], (a, b)
    # the ids existing tests expect to be refused stay in no range
    for bad in (-1, 54, 63, 78, 99, 127, 182, 255):
        assert not any(bad in r for r in ranges), bad


# ---- the reference alone ------------------------------------------------------------------
def _box(n=(5, 4, 3), lengths=(1.0, 2.0, 0.5), stretch=1.3):
    """a Cartesian box: padded face areas per direction [k, j, i, 4] (no ghost cells), its
    nodes and the six whole-side surfaces"""
    from aither_amd.case import geometry
    ni, nj, nk = n
    nodes = synthetic.box_nodes(ni, nj, nk, stretch, lengths=lengths)
    m = geometry.interior_metrics(nodes)
    farea = {0: m["farea_i"], 1: m["farea_j"], 2: m["farea_k"]}
    rng = {1: (0, 0, 0, nj, 0, nk), 2: (ni, ni, 0, nj, 0, nk), 3: (0, ni, 0, 0, 0, nk),
           4: (0, ni, nj, nj, 0, nk), 5: (0, ni, 0, nj, 0, 0), 6: (0, ni, 0, nj, nk, nk)}
    surfs = []
    for side, r in rng.items():
        d = (side - 1) // 2
        cnt = [r[1] - r[0], r[3] - r[2], r[5] - r[4]]
        cnt[d] = 1
        surfs.append(dict(side=side, range=r, shape=(cnt[2], cnt[1], cnt[0])))
    return nodes, farea, surfs


def _uniform(surf, value):
    return np.full(surf["shape"], value)


def test_box_with_uniform_pressure():
    nodes, farea, surfs = _box()
    p, l_ref = 101325.0, 1.0
    size = {0: 2.0 * 0.5, 1: 1.0 * 0.5, 2: 1.0 * 2.0}
    total_f, total_a, total_bound = np.zeros(3), np.zeros(3), np.zeros(3)
    for surf in surfs:
        d = (surf["side"] - 1) // 2
        z = _uniform(surf, 0.0)
        ref = loads_ref.surface_reference(surf, _uniform(surf, p), [z, z, z], z, farea[d], 0,
                                          l_ref)
        sg = loads_ref.sigma(surf["side"])
        assert abs(ref["area"][0] - size[d]) <= 1e-14
        for c, x in enumerate("xyz"):
            want = -sg * p * size[d] if c == d else 0.0
            ex, bd = ref["pressureForce_" + x]
            assert abs(ex - want) <= 1e-12 * p * size[d], (surf["side"], x)
            total_f[c] += ex
            total_bound[c] += bd
            total_a[c] += ref["area_" + x][0]
    assert np.all(np.abs(total_a) <= 1e-15)
    assert np.all(np.abs(total_f) <= total_bound), (total_f, total_bound)


def test_couette_face_values_give_mu_a_area():
    nodes, farea, surfs = _box(lengths=(1.0, 1.0, 1.0), stretch=1.0)
    mu, a = 1.8e-5, 20.0
    for surf in surfs:
        if surf["side"] not in (3, 4):
            continue
        z = _uniform(surf, 0.0)
        # tau . n on the stored area vector (+y on both sides) of u = a y
        tau = [_uniform(surf, mu * a), z, z]
        ref = loads_ref.surface_reference(surf, _uniform(surf, 1.0e5), tau, z, farea[1], 0, 1.0)
        want = loads_ref.sigma(surf["side"]) * mu * a * 1.0
        ex, bd = ref["viscousForce_x"]
        assert abs(ex - want) <= bd and bd < 1e-6 * abs(want)
        assert ref["viscousForce_y"][0] == 0.0 and ref["viscousForce_z"][0] == 0.0
        # ... and the wall is pushed along its outward normal
        assert np.sign(ref["pressureForce_y"][0]) == -loads_ref.sigma(surf["side"])


def test_reference_point_shift():
    """M about r0 formed from shifted face centres equals M - r0 x F"""
    nodes, farea, surfs = _box()
    skewed = synthetic.box_nodes(5, 4, 3, 1.3, lengths=(1.0, 2.0, 0.5), skew=0.02)
    r0 = np.array([0.3, -1.1, 2.5])
    fc = loads_ref.face_centres(skewed)
    fc0 = loads_ref.face_centres(skewed - r0)
    rng = np.random.default_rng(7)
    for surf in surfs:
        d = (surf["side"] - 1) // 2
        p = 1.0e5 * (1.0 + 0.1 * rng.random(surf["shape"]))
        tau = [rng.standard_normal(surf["shape"]) for _ in range(3)]
        q = rng.standard_normal(surf["shape"])
        a = loads_ref.surface_reference(surf, p, tau, q, farea[d], 0, 1.0, fc[d])
        b = loads_ref.surface_reference(surf, p, tau, q, farea[d], 0, 1.0, fc0[d])
        for kind in ("pressure", "viscous"):
            f = np.array([a[f"{kind}Force_{c}"][0] for c in "xyz"])
            m = np.array([a[f"{kind}Moment_{c}"][0] for c in "xyz"])
            m0 = np.array([b[f"{kind}Moment_{c}"][0] for c in "xyz"])
            scale = np.abs(m).max() + np.abs(np.cross(r0, f)).max()
            assert np.abs(m - np.cross(r0, f) - m0).max() <= 1e-13 * scale, kind


def test_face_centres_are_the_package_metrics():
    from aither_amd.case import geometry
    nodes = synthetic.box_nodes(5, 4, 3, 1.3, skew=0.02)
    m = geometry.interior_metrics(nodes)
    fc = loads_ref.face_centres(nodes)
    for d, name in enumerate("ijk"):
        assert np.abs(fc[d] - m["fcen_" + name]).max() <= 4e-16


# ---- the bound has teeth on every case the GPU tests use ------------------------------------
@pytest.mark.parametrize("name", sorted(loads_ref.CASES))
def test_bound_notices_a_missing_face_and_a_flipped_side(name):
    case = loads_ref.CASES[name]()
    ng, gas = case.ng, case.gas
    p_sc = gas.rho_ref * gas.a_ref * gas.a_ref
    seen = 0
    for gb, blk in enumerate(case.blocks):
        g = blk.geom
        p_cells = blk.state[ng:ng + g.nk, ng:ng + g.nj, ng:ng + g.ni, 4] * p_sc
        for surf in loads_ref.host_load_surfaces(case, gb):
            d = (surf["side"] - 1) // 2
            p = loads_ref.adjacent_cells(surf, p_cells)
            z = np.zeros_like(p)
            farea = np.asarray(g.farea["ijk"[d]].a)
            terms = loads_ref.surface_terms(surf, p, [z, z, z], z, farea, ng, gas.l_ref)
            ref = loads_ref.surface_reference(surf, p, [z, z, z], z, farea, ng, gas.l_ref)
            # leaving out any single face moves `area` beyond its bound
            assert terms["area"][0].min() > ref["area"][1], (name, gb, surf)
            # flipping sigma changes every force component by twice its value
            moved = [2.0 * abs(ref["pressureForce_" + c][0]) > ref["pressureForce_" + c][1]
                     for c in "xyz"]
            assert any(moved), (name, gb, surf)
            seen += 1
    assert seen > 0
