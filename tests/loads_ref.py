"""The integrated wall loads (agx_output_pack with AGX_LOAD_*), restated in numpy.

The seventeen sums of a load surface from per-face values, face areas, face centres and the
side's sign -- and the bound a device sum has to meet, derived here and nowhere measured.

    area                 sum |A|
    area_c               sum m_c |A|                     m = sigma n, sigma = +1 on lower sides
    pressureForce_c      - sum p m_c |A|                 (1, 3, 5), -1 on upper sides (2, 4, 6)
    viscousForce_c       sum (tau . m)_c |A|             (the wall payload's shear vector is
    heatLoad             sum (k + kt) grad T . m |A|      tau . n, its heat flux grad T . n)
    pressureMoment, viscousMoment      sum r_f x (force term), about the origin

Every sum comes back as (exact, S, N): math.fsum of the terms, the sum of their magnitudes
(for a moment both products of the cross-product component count) and the number of faces.

The bound: |got - exact| <= (N + 16) 2^-52 S + A_s tol_face.  The first part covers any
summation order of N terms plus up to sixteen roundings per term (the factors applied per
face here and per sum on the device, the face-centre mean, the products).  The second part is
the per-face tolerance the project already uses for the same quantities (tests/wall_ref.py
compare): 1e-10 of the surface's largest |p| for what is formed from the state alone, 1e-8 of
its largest |tau| or heat flux for what is formed from gradients, times the surface's area
A_s; for moments times the largest |r_f| as well.  Areas carry no per-face tolerance.
"""
import math

import numpy as np

from aither_amd import abi
from aither_amd.case import builder as _b
from aither_amd.case import synthetic
from aither_amd.case.inputfile import Surface

NAMES = list(abi.LOAD_OUT)
MOMENTS = [n for n in NAMES if "Moment" in n]
NO_MOMENTS = [n for n in NAMES if n not in MOMENTS]
WALL_NAMES = ["pressure", "shearStress_x", "shearStress_y", "shearStress_z", "heatFlux"]
EPS52 = 2.0 ** -52


def sigma(side):
    return 1.0 if side % 2 == 1 else -1.0


def face_centres(nodes):
    """FaceCenterI/J/K (plot3d.cpp:150-331, what k_plot3d_metrics implements): a quarter of the
    four nodes of the face, added in the order (0,0), (1,0), (0,1), (1,1) of its two running
    directions, the lower one first.  nodes [nk+1, nj+1, ni+1, 3] -> {d: [k, j, i, 3]}."""
    x = np.asarray(nodes, dtype=np.float64)
    nk, nj, ni = (s - 1 for s in x.shape[:3])
    out = {}
    n = lambda dj, dk: x[dk:nk + dk, dj:nj + dj, :]
    out[0] = 0.25 * (((n(0, 0) + n(1, 0)) + n(0, 1)) + n(1, 1))
    n = lambda di, dk: x[dk:nk + dk, :, di:ni + di]
    out[1] = 0.25 * (((n(0, 0) + n(1, 0)) + n(0, 1)) + n(1, 1))
    n = lambda di, dj: x[:, dj:nj + dj, di:ni + di]
    out[2] = 0.25 * (((n(0, 0) + n(1, 0)) + n(0, 1)) + n(1, 1))
    return out


def _window(surf, pad):
    """index of the surface's faces in a [k, j, i, c] face array padded by `pad` cells"""
    r = surf["range"]
    d = (surf["side"] - 1) // 2
    lo, hi = [r[0], r[2], r[4]], [r[1], r[3], r[5]]
    hi[d] = lo[d] + 1
    return tuple(slice(lo[q] + pad, hi[q] + pad) for q in (2, 1, 0))


def adjacent_cells(surf, cells):
    """the wall-adjacent physical cells of a surface from a [nk, nj, ni] cell array"""
    r = surf["range"]
    d = (surf["side"] - 1) // 2
    lo, hi = [r[0], r[2], r[4]], [r[1], r[3], r[5]]
    if surf["side"] % 2 == 0:
        lo[d] -= 1
    hi[d] = lo[d] + 1
    return cells[tuple(slice(lo[q], hi[q]) for q in (2, 1, 0))]


def surface_terms(surf, p, tau, q, farea, ng, l_ref, fcen=None):
    """The terms of the seventeen sums of one surface: {name: [arrays of terms]} (a moment has
    two arrays: the two products of its cross-product component).  p, q: (nk, nj, ni) of the
    surface, tau: three such arrays (tau . n), dimensional; farea: the padded [k, j, i, 4]
    area array of the surface's direction as downloaded; fcen: face_centres()[d] or None."""
    sg = sigma(surf["side"])
    fa = farea[_window(surf, ng)]
    assert fa.shape[:3] == tuple(surf["shape"]), (fa.shape, surf["shape"])
    area = fa[..., 3] * (l_ref * l_ref)
    m = [sg * fa[..., c] for c in range(3)]
    t = {"area": [area], "heatLoad": [sg * q * area]}
    fp, fv = [], []
    for c, x in enumerate("xyz"):
        t["area_" + x] = [m[c] * area]
        fp.append(-(p * m[c] * area))
        fv.append(sg * tau[c] * area)
        t["pressureForce_" + x], t["viscousForce_" + x] = [fp[c]], [fv[c]]
    if fcen is not None:
        r = fcen[_window(surf, 0)] * l_ref
        for c, x in enumerate("xyz"):
            c1, c2 = (c + 1) % 3, (c + 2) % 3
            t["pressureMoment_" + x] = [r[..., c1] * fp[c2], -(r[..., c2] * fp[c1])]
            t["viscousMoment_" + x] = [r[..., c1] * fv[c2], -(r[..., c2] * fv[c1])]
    return t


def sums(terms):
    """{name: (exact, S, N)}"""
    out = {}
    for name, arrs in terms.items():
        flat = np.concatenate([a.ravel() for a in arrs])
        out[name] = (math.fsum(flat), math.fsum(np.abs(flat)), arrs[0].size)
    return out


def tol_face(name, p, tau, q, rmax):
    if name.startswith("area"):
        return 0.0
    mag = np.sqrt(tau[0] ** 2 + tau[1] ** 2 + tau[2] ** 2).max()
    t = {"pressure": 1e-10 * np.abs(p).max(), "viscous": 1e-8 * mag,
         "heatLoad": 1e-8 * np.abs(q).max()}[name.split("_")[0].replace("Force", "")
                                             .replace("Moment", "")]
    return t * (rmax if "Moment" in name else 1.0)


def bound(n, s, area, tol):
    return (n + 16) * EPS52 * s + area * tol


def surface_reference(surf, p, tau, q, farea, ng, l_ref, fcen=None):
    """{name: (exact, bound)} of one surface"""
    ref = sums(surface_terms(surf, p, tau, q, farea, ng, l_ref, fcen))
    area = ref["area"][0]
    rmax = 0.0
    if fcen is not None:
        r = fcen[_window(surf, 0)] * l_ref
        rmax = float(np.sqrt((r ** 2).sum(-1)).max())
    return {name: (ex, bound(n, s, area, tol_face(name, p, tau, q, rmax)))
            for name, (ex, s, n) in ref.items()}


def block_reference(sol, gb, nodes=None):
    """[{name: (exact, bound)} per load surface] of block gb from the library's own wall
    payload (viscousWall surfaces of a viscous context), the cell pressure (all others), the
    downloaded face areas and -- for the moments -- face centres from `nodes`."""
    case = sol.case
    ng, l_ref = case.ng, case.gas.l_ref
    surfs = sol.load_surfaces(gb)
    viscous = bool(sol.cfg.is_viscous)
    wall = sol.wall_pack(gb, WALL_NAMES) if viscous and sol.wall_surfaces(gb) else None
    pcell = sol.output_pack(gb, ["pressure"])[0]
    farea = {d: sol.geometry("farea_" + "ijk"[d], gb) for d in range(3)}
    fcen = face_centres(nodes) if nodes is not None else None
    out, w = [], 0
    for surf in surfs:
        d = (surf["side"] - 1) // 2
        if viscous and surf["bc_type"] == "viscousWall":
            p, q = wall["pressure"][w], wall["heatFlux"][w]
            tau = [wall["shearStress_" + c][w] for c in "xyz"]
            w += 1
        else:
            p = adjacent_cells(surf, pcell)
            q = np.zeros_like(p)
            tau = [q, q, q]
        out.append(surface_reference(surf, p, tau, q, farea[d], ng, l_ref,
                                     fcen[d] if fcen is not None else None))
    return out


def compare(got, ref, names=None, log=print, what=""):
    """got: {name: ndarray[nsurf]} (Solver.wall_loads); ref: block_reference's list.  Prints
    each figure before it asserts."""
    names = names or [n for n in NAMES if n in got and n in ref[0]]
    bad = []
    for s, r in enumerate(ref):
        for n in names:
            ex, bd = r[n]
            err = abs(float(got[n][s]) - ex)
            log(f"wall_loads {what} surface {s} {n}: got {got[n][s]:.17g} exact {ex:.17g} "
                f"|diff| {err:.3e} bound {bd:.3e}")
            if not err <= bd:
                bad.append((s, n, err, bd))
    assert not bad, bad


# ---- cases of the GPU tests (tests/test_wall_loads_gpu.py), built here so that the host file
# can show on each that the bound has teeth ------------------------------------------------
WALLS = {3: ("viscousWall", 4), 4: ("viscousWall", 5), 1: ("viscousWall", 2),
         2: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
LAMINAR = dict(equation_set="navierStokes", face_reconstruction="weno", limiter="none",
               inviscid_flux="ausm", time_integration="implicitEuler", matrix_solver="lusgs",
               cfl=5.0)
NS = dict(equation_set="navierStokes", time_integration="implicitEuler", cfl=5.0)
EULER = dict(equation_set="euler", time_integration="implicitEuler", cfl=5.0)
STACKED_BCS = {3: ("viscousWall", 4), 1: ("viscousWall", 2), 2: ("characteristic", 1),
               4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
# a skewed, stretched box with walls of both kinds on lower and upper sides
MOMENT_BCS = {1: ("viscousWall", 2), 2: ("slipWall", 0), 3: ("viscousWall", 4),
              4: ("viscousWall", 5), 5: ("slipWall", 0), 6: ("characteristic", 1)}
MOMENT_N, MOMENT_KW = (9, 8, 6), dict(stretch=1.2, skew=0.01, l_ref=2.0)
ALL_WALLS = lambda name, tag: {s: (name, tag) for s in range(1, 7)}


def split_case(n, surfaces, stretch=1.0, skew=0.0, amplitude=0.05, geometry="host",
               states=(), **deck_kw):
    """synthetic.single_block_case with the block's surfaces given one by one (several
    rectangular surfaces per side) and further BC states"""
    ni, nj, nk = n
    deck = synthetic.make_deck(**deck_kw)
    deck.bc_states = list(deck.bc_states) + list(states)
    deck.bcs = [sorted(surfaces, key=Surface.sort_key)]
    coords = [synthetic.box_nodes(ni, nj, nk, stretch, skew=skew)]
    case = _b.build_case(None, deck=deck, coords=coords, geometry=geometry)
    if amplitude and geometry == "host":
        synthetic.perturbed_state(case, amplitude)
    return case


def strip_surfaces():
    """block (257, 3, 2): j-min in viscousWall surfaces of 257, 1, 63, 64, 65 and 64 faces,
    j-max in slipWall surfaces of 255, 2, 256 and 1 faces; the other sides farfield"""
    ni, nj, nk = STRIP_N
    s = [Surface("viscousWall", 0, ni, 0, 0, 0, 1, 2)]
    lo = 0
    for cnt in (1, 63, 64, 65, 64):
        s.append(Surface("viscousWall", lo, lo + cnt, 0, 0, 1, 2, 2))
        lo += cnt
    assert lo == ni
    s += [Surface("slipWall", 0, 255, nj, nj, 0, 1, 0), Surface("slipWall", 255, ni, nj, nj, 0, 1, 0),
          Surface("slipWall", 0, 256, nj, nj, 1, 2, 0), Surface("slipWall", 256, ni, nj, nj, 1, 2, 0)]
    s += [Surface("characteristic", 0, 0, 0, nj, 0, nk, 1),
          Surface("characteristic", ni, ni, 0, nj, 0, nk, 1),
          Surface("characteristic", 0, ni, 0, nj, 0, 0, 1),
          Surface("characteristic", 0, ni, 0, nj, nk, nk, 1)]
    return s


STRIP_N = (257, 3, 2)
BIG_N = (129, 128, 2)         # its k sides: 16 512 faces, 65 chunks of 256
COUETTE_N, COUETTE_A, COUETTE_TAG = (6, 5, 6), 20.0, 11


def couette_case():
    """u = a y, uniform p and T, between a j-min wall at rest and a j-max wall moving at
    a * 1 m; each wall in three surfaces along k; the i and k sides slip walls"""
    from aither_amd.case.inputfile import State
    ni, nj, nk = COUETTE_N
    s = []
    for k0, k1 in ((0, 2), (2, 4), (4, nk)):
        s.append(Surface("viscousWall", 0, ni, 0, 0, k0, k1, 2))
        s.append(Surface("viscousWall", 0, ni, nj, nj, k0, k1, COUETTE_TAG))
    s += [Surface("slipWall", 0, 0, 0, nj, 0, nk, 0), Surface("slipWall", ni, ni, 0, nj, 0, nk, 0),
          Surface("slipWall", 0, ni, 0, nj, 0, 0, 0), Surface("slipWall", 0, ni, 0, nj, nk, nk, 0)]
    moving = State("viscousWall", dict(tag=COUETTE_TAG, velocity=[COUETTE_A, 0.0, 0.0]))
    case = split_case(COUETTE_N, s, amplitude=0.0, states=[moving], velocity=[0.0, 0.0, 0.0],
                      **NS)
    blk = case.blocks[0]
    y = blk.geom.center.a[..., 1] * case.gas.l_ref
    blk.state[..., 1] = COUETTE_A * y / case.gas.a_ref
    return case


def rans_case():
    from test_output_pack import _case
    return _case("rans")


def hot_case():
    import tp_cases
    return tp_cases.hot_single(n=(10, 9, 7), stretch=1.2, skew=0.01, bcs=WALLS, **LAMINAR)


def wall_law_case():
    from conftest import golden_case
    return golden_case("wallLaw")


# name -> maker of the case as the host sees it (host geometry: the same nodes)
CASES = {
    "laminar_central": lambda: synthetic.single_block_case(
        (12, 9, 7), stretch=1.2, skew=0.01, bcs=WALLS, viscous_face_reconstruction="central",
        **LAMINAR),
    "laminar_fourth": lambda: synthetic.single_block_case(
        (12, 9, 7), stretch=1.2, skew=0.01, bcs=WALLS,
        viscous_face_reconstruction="centralFourth", **LAMINAR),
    "stacked_k": lambda: synthetic.stacked_blocks_case(
        (8, 7, 6), nblocks=2, axis="k", stretch=1.15, bcs=STACKED_BCS, **LAMINAR),
    "hot_tp": hot_case,
    "rans_low_re": rans_case,
    "wall_law": wall_law_case,
    "strip": lambda: split_case(STRIP_N, strip_surfaces(), **NS),
    "big": lambda: synthetic.single_block_case(BIG_N, **EULER),
    "box_euler": lambda: synthetic.single_block_case(
        (6, 5, 4), stretch=1.2, amplitude=0.0, velocity=[0.0, 0.0, 0.0], **EULER),
    "box_laminar": lambda: synthetic.single_block_case(
        (6, 5, 4), stretch=1.2, amplitude=0.0, velocity=[0.0, 0.0, 0.0],
        bcs=ALL_WALLS("viscousWall", 2), **NS),
    "couette": couette_case,
    "moments": lambda: synthetic.single_block_case(MOMENT_N, bcs=MOMENT_BCS, **MOMENT_KW, **LAMINAR),
    "contract": lambda: synthetic.single_block_case((10, 8, 6), stretch=1.2, skew=0.01,
                                                    bcs=WALLS, **LAMINAR),
}


def host_load_surfaces(case, gb):
    """Solver.load_surfaces without a solver"""
    out = []
    for s in case.blocks[gb].surfaces:
        if s.bc_type not in ("viscousWall", "slipWall"):
            continue
        side = s.surface_type()
        d = (side - 1) // 2
        n = [s.imax - s.imin, s.jmax - s.jmin, s.kmax - s.kmin]
        n[d] = 1
        out.append(dict(side=side, tag=s.tag, bc_type=s.bc_type,
                        range=(s.imin, s.imax, s.jmin, s.jmax, s.kmin, s.kmax),
                        shape=(n[2], n[1], n[0])))
    return out
