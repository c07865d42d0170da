"""The decks of the large-eddy-simulation (WALE) tests and their vortical, sign-changing field.

The shapes are the smallest that cross what the viscous tile kernel can get wrong: it owns
62 x 6 cells per workgroup and step (60 x 6 with centralFourth) and cuts the (column, k)
sequence into ranges.

  A  66 x 9 x 6, stretched and sheared, characteristic boundaries, central: two tiles in i and
     in j, a few workgroups, a range that starts mid-column
  B  A with centralFourth: the 60-wide i tiles and the centralFourth k window
  C  7 x 5 x 9, isothermal viscousWall at j-min, adiabatic one at i-max, the rest
     characteristic: one partial tile, overhang threads, low-Re wall faces
  D  A split into two blocks at i = 31, inside a tile: the block connection
  E  C on the thermally perfect library, vibrational mode excited (tests/tp_cases.py)

Every deck comes in any equation set (`equation_set=`) with the same grid and the same state,
so a largeEddySimulation context and a navierStokes context can be held side by side.
"""
import math

import numpy as np

from aither_amd.case import builder, synthetic

CHAR = {s: ("characteristic", 1) for s in range(1, 7)}
WALLS = dict(CHAR)
WALLS[3] = ("viscousWall", 4)       # isothermal (and moving), j-min
WALLS[2] = ("viscousWall", 2)       # adiabatic, i-max
N_A, N_C, CUT = (66, 9, 6), (7, 5, 9), 31
LES = dict(equation_set="largeEddySimulation", turbulence_model="wale")
NS = dict(equation_set="navierStokes", turbulence_model="none")
EULER = dict(equation_set="euler", turbulence_model="none")


def vortical_state(case):
    """Velocity gradients of order 1 to 3 on cells about 0.1 wide, every velocity component
    changing sign, density and pressure 5 % off their free-stream values: by
    mut = (Cw length)^2 a^1.5 / (b^2.5 + a^1.25) that is an eddy viscosity of some 1e-3 to
    1e-2 of the molecular one (nondimensional mu is 1 at the reference temperature).  Physical
    cells only; the ghost cells are the boundary conditions'."""
    two_pi = 2.0 * math.pi
    for blk in case.blocks:
        g = blk.geom.ng
        ni, nj, nk = blk.geom.n
        c = blk.geom.center.a
        x, y, z = c[..., 0], c[..., 1], c[..., 2]
        base = blk.state[g, g, g, :].copy()
        new = np.zeros(c.shape[:3] + (blk.state.shape[-1],))
        new[..., 0] = base[0] * (1.0 + 0.05 * np.sin(two_pi * x) * np.cos(two_pi * y))
        new[..., 1] = 0.30 * np.sin(two_pi * x) * np.cos(two_pi * y) * np.cos(math.pi * z) + 0.04
        new[..., 2] = -0.28 * np.cos(two_pi * x) * np.sin(two_pi * y + 0.3) * np.cos(math.pi * z)
        new[..., 3] = 0.22 * np.sin(two_pi * x + 0.5) * np.sin(two_pi * y) * np.sin(two_pi * z)
        new[..., 4] = base[4] * (1.0 + 0.05 * np.cos(two_pi * x) * np.sin(two_pi * z))
        blk.state[...] = 0.0
        blk.state[g:g + nk, g:g + nj, g:g + ni, :] = new[g:g + nk, g:g + nj, g:g + ni, :]
    return case


def _deck(recon, eq, time_integration, **kw):
    opts = dict(face_reconstruction="thirdOrder", limiter="vanAlbada", inviscid_flux="roe",
                viscous_face_reconstruction=recon, time_integration=time_integration, cfl=0.4)
    opts.update(eq)
    opts.update(kw)
    return synthetic.make_deck(**opts)


def _nodes_a():
    # (three units long: the i-cells are about 0.05 wide, so the i-faces' molecular flux does
    # not bury the eddy terms of the other directions)
    return synthetic.box_nodes(*N_A, stretch=1.15, lengths=(3.0, 1.0, 1.0), skew=0.02)


def deck_a(eq=LES, recon="central", time_integration="rk4", **kw):
    """A (recon="centralFourth": B)"""
    deck = _deck(recon, eq, time_integration, **kw)
    deck.bcs = [synthetic.box_surfaces(*N_A, CHAR)]
    return vortical_state(builder.build_case(None, deck=deck, coords=[_nodes_a()]))


def deck_d(eq=LES, time_integration="rk4", **kw):
    """A's nodes cut at i = CUT into two blocks joined by an interblock connection"""
    deck = _deck("central", eq, time_integration, **kw)
    x = _nodes_a()
    ni, nj, nk = N_A
    lo, hi = dict(CHAR), dict(CHAR)
    lo[2] = ("interblock", 1000 * 1 + 1)
    hi[1] = ("interblock", 1000 * 2 + 0)
    deck.bcs = [synthetic.box_surfaces(CUT, nj, nk, lo),
                synthetic.box_surfaces(ni - CUT, nj, nk, hi)]
    coords = [x[:, :, :CUT + 1].copy(), x[:, :, CUT:].copy()]
    return vortical_state(builder.build_case(None, deck=deck, coords=coords))


def deck_c(eq=LES, time_integration="rk4", **kw):
    deck = _deck("central", eq, time_integration, **kw)
    deck.bcs = [synthetic.box_surfaces(*N_C, WALLS)]
    coords = [synthetic.box_nodes(*N_C, stretch=1.2, skew=0.01)]
    return vortical_state(builder.build_case(None, deck=deck, coords=coords))


def deck_e(eq=LES, time_integration="rk4", **kw):
    """C with the hot settings of tests/tp_cases.py (thermally perfect, 7 x 288 K)"""
    import tp_cases
    deck = _deck("central", eq, time_integration, thermodynamic_model=tp_cases.TP,
                 temperature_factor=tp_cases.HOT, **kw)
    deck.bcs = [synthetic.box_surfaces(*N_C, WALLS)]
    coords = [synthetic.box_nodes(*N_C, stretch=1.2, skew=0.01)]
    return tp_cases.excited(vortical_state(builder.build_case(None, deck=deck, coords=coords)))


def cut_rim():
    """[k, j, i] mask over A's cells: the two cells next to D's cut that also lie on a j or k
    boundary.  Their viscous faces read cells (i beyond the cut, j or k beyond the boundary)
    that are face ghost cells of the one block and edge ghost cells of the two."""
    ni, nj, nk = N_A
    rim = np.zeros((nk, nj, ni), dtype=bool)
    rim[:, :, CUT - 1:CUT + 1] = True
    rim[1:-1, 1:-1, :] = False
    return rim


DECKS = {"A": lambda **kw: deck_a(**kw),
         "B": lambda **kw: deck_a(recon="centralFourth", **kw),
         "C": deck_c, "D": deck_d, "E": deck_e}
FOURTH = {"A": False, "B": True, "C": False, "D": False, "E": False}
