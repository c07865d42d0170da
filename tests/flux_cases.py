"""The cases of the boundary-flux tests (tests/test_surface_flux_host.py, _gpu.py): the
smallest shapes at which the surface kernels can go wrong.

  F1  one block of 20 x 15 x 6 cells, stretched and skewed, with the transonic, sign-changing
      field of tests/flow_fields.py (the stream along +i).  Every side another kind of
      boundary: inlet (i-min), pressureOutlet (i-max), supersonicInflow (j-max),
      characteristic (k-min), an isothermal moving viscousWall (k-max), and j-min split at
      i = 9 into a slipWall patch and an adiabatic viscousWall patch -- two surfaces on one
      side.  The k-surfaces have 300 faces: two chunks of 256, the second padded; every other
      surface is one partial chunk.  (The far field lies on k-min: on j-max the second ghost
      layer of a characteristic boundary leaves this field with a negative pressure, which
      the centralFourth face values read.)
  F2  F1's nodes cut at i = 9 (where the two patches of j-min meet) into two blocks joined by
      a local interblock connection.
  F3  deck C of tests/les_cases.py, 7 x 5 x 9, an isothermal moving wall and an adiabatic wall:
      as navierStokes, as largeEddySimulation, and on the thermally perfect library (deck E).
  F4  loads_ref.rans_case() and loads_ref.wall_law_case() on the 7-equation library.
"""
import flow_fields
import les_cases
import loads_ref
from aither_amd.case import builder, synthetic
from aither_amd.case.inputfile import Surface

N1, CUT = (20, 15, 6), 9
AXIS, SIGN = "i", +1
NODES = dict(stretch=1.15, skew=0.02)

EULER = dict(equation_set="euler", time_integration="rk4", cfl=0.4)
NS = dict(equation_set="navierStokes", time_integration="rk4", cfl=0.3)
# (reconstruction, limiter, flux) of the inviscid decks; "constant" is first order
SCHEMES = {
    "constant_roe": dict(face_reconstruction="constant", limiter="none", inviscid_flux="roe"),
    "constant_ausm": dict(face_reconstruction="constant", limiter="none", inviscid_flux="ausm"),
    "muscl_vanalbada_roe": dict(face_reconstruction="thirdOrder", limiter="vanAlbada",
                                inviscid_flux="roe"),
    "muscl_vanalbada_ausm": dict(face_reconstruction="thirdOrder", limiter="vanAlbada",
                                 inviscid_flux="ausm"),
    "muscl_minmod_roe": dict(face_reconstruction="thirdOrder", limiter="minmod",
                             inviscid_flux="roe"),
    "muscl_minmod_ausm": dict(face_reconstruction="thirdOrder", limiter="minmod",
                              inviscid_flux="ausm"),
    "weno_ausm": dict(face_reconstruction="weno", limiter="none", inviscid_flux="ausm"),
}


def f1_surfaces(ni=N1[0], i0=0, lo=None, hi=None):
    """the surfaces of F1, or of the part i0 .. i0 + ni of it (F2): lo / hi replace the
    boundary at i-min / i-max by an interblock surface with that tag"""
    _, nj, nk = N1
    s = [Surface("interblock" if lo else "inlet", 0, 0, 0, nj, 0, nk, lo or 10),
         Surface("interblock" if hi else "pressureOutlet", ni, ni, 0, nj, 0, nk, hi or 3)]
    # j-min: slipWall up to the cut, an adiabatic viscousWall beyond it
    a, b = max(0, 0 - i0), min(ni, CUT - i0)
    if b > a:
        s.append(Surface("slipWall", a, b, 0, 0, 0, nk, 0))
    a, b = max(0, CUT - i0), min(ni, N1[0] - i0)
    if b > a:
        s.append(Surface("viscousWall", a, b, 0, 0, 0, nk, 2))
    s += [Surface("supersonicInflow", 0, ni, nj, nj, 0, nk, 8),
          Surface("characteristic", 0, ni, 0, nj, 0, 0, 1),
          Surface("viscousWall", 0, ni, 0, nj, nk, nk, 4)]
    return sorted(s, key=Surface.sort_key)


def _deck(**kw):
    kw["velocity"] = flow_fields.free_stream_velocity(AXIS, SIGN)
    return synthetic.make_deck(**kw)


def f1(**kw):
    deck = _deck(**kw)
    deck.bcs = [f1_surfaces()]
    case = builder.build_case(None, deck=deck, coords=[synthetic.box_nodes(*N1, **NODES)])
    flow_fields.transonic_state(case, AXIS, SIGN)
    return case


def f2(**kw):
    """(the tag of an interblock surface: 1000 x the partner's surface type + its block)"""
    deck = _deck(**kw)
    ni = N1[0]
    deck.bcs = [f1_surfaces(CUT, 0, hi=1000 * 1 + 1), f1_surfaces(ni - CUT, CUT, lo=1000 * 2 + 0)]
    x = synthetic.box_nodes(*N1, **NODES)
    case = builder.build_case(None, deck=deck,
                              coords=[x[:, :, :CUT + 1].copy(), x[:, :, CUT:].copy()])
    flow_fields.transonic_state(case, AXIS, SIGN)
    return case


# which surfaces of F2's blocks make up each surface of F1, as (block, index in its list)
def f2_parts(f1_surfs, f2_surfs):
    """per F1 surface the F2 surfaces that tile it (same side and BC type, not connections)"""
    out = []
    for s in f1_surfs:
        parts = [(gb, q) for gb, surfs in enumerate(f2_surfs) for q, t in enumerate(surfs)
                 if t["side"] == s["side"] and t["bc_type"] == s["bc_type"] and
                 t["tag"] == s["tag"]]
        out.append(parts)
    return out


F3 = {
    "ns": (lambda **kw: les_cases.deck_c(eq=les_cases.NS, **kw), (5,)),
    "les": (lambda **kw: les_cases.deck_c(eq=les_cases.LES, **kw), (5,)),
    "tp": (lambda **kw: les_cases.deck_e(eq=les_cases.LES, **kw), (5, "thermallyPerfect")),
}
F4 = {"rans": loads_ref.rans_case, "wall_law": loads_ref.wall_law_case}
