"""The transonic decks shared by tests/test_flow_branches_host.py (oracle only) and
tests/test_flow_branches_gpu.py (HIP vs oracle): every scheme family of the synthetic parity
decks on the field of tests/flow_fields.py, whose flow selects the branches the Mach-0.16
stream of synthetic.perturbed_state never does.

A case: lib (5 | 7 equations), tp (thermally perfect at tp_cases.HOT), axis / sign of the fast
velocity, kind (single | stacked), deck (keywords of the synthetic builders), steps, and
`claims`: the census keys (tests/branch_census.py) the case is there for.  The host module
asserts that each claimed arm holds >= MIN_FACES faces before every compared step, that the
oracle stays physical, and that the claims of all cases together cover REQUIRED.
"""
from branch_census import AUSM, CHARACTERISTIC, ROE
import flow_fields

MIN_FACES = 8
MARGIN = 1.0e-6
HOT = 7.0                # tp_cases.HOT (x 288.15 K)
TP = "thermallyPerfect"

N5, N7 = (12, 11, 10), (9, 8, 7)
FARFIELD = {s: ("characteristic", 1) for s in range(1, 7)}
# pressure outlets on the three high faces, far field on the low ones
OUTLETS = {1: ("characteristic", 1), 2: ("pressureOutlet", 3), 3: ("characteristic", 1),
           4: ("pressureOutlet", 3), 5: ("characteristic", 1), 6: ("pressureOutlet", 3)}
# a viscous wall on a face the fast axis does not cross
WALL_K = {5: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
          3: ("characteristic", 1), 4: ("characteristic", 1), 6: ("characteristic", 1)}
WALL_J = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
          4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}
# inlet (tag 10: the deck's free stream), pressure outlet across the fast axis i; supersonic
# in/outflow and the far field on the transverse faces.  The stream enters at i-min (sign +)
# or at i-max (sign -).
BOX_PLUS = {1: ("inlet", 10), 2: ("pressureOutlet", 3), 3: ("supersonicInflow", 8),
            4: ("supersonicOutflow", 9), 5: ("characteristic", 1), 6: ("characteristic", 1)}
BOX_MINUS = {2: ("inlet", 10), 1: ("pressureOutlet", 3), 3: ("supersonicInflow", 8),
             4: ("supersonicOutflow", 9), 5: ("characteristic", 1), 6: ("characteristic", 1)}
# the hold arm of extrap_hold: far field all round, the density of the three layers next to
# j-min (a transverse face: subsonic in- and outflow mixed) ramped to 2.6 x
RAMP = (3, 2.6)

BOX5 = dict(n=N5, stretch=1.1, skew=0.01)
RANS = dict(n=N7, stretch=1.2, bcs=WALL_J, equation_set="rans", turbulence_model="sst2003",
            time_integration="implicitEuler", cfl=10.0)


def _fast(flux, axis, sign):
    """the arms only the fast axis can select, by the sign of the stream"""
    if flux == "ausm":
        names = ("vel>0", "vnL>cS", "vnR>cS", "ml>1", "mr>1") if sign > 0 else \
            ("vel<0", "ml<-1", "mr<-1", "mavg<0")
        return [f"ausm:{axis}:{n}" for n in names]
    return [f"roe:{axis}:" + ("|vn-a|<0.1" if sign > 0 else "|vn+a|<0.1")] + \
        ([f"roe:{axis}:vn<0"] if sign < 0 else [])


def _cross(flux, axis):
    """both signs of the normal velocity across the fast axis"""
    others = [d for d in "ijk" if d != axis]
    if flux == "ausm":
        return [f"ausm:{d}:{n}" for d in others for n in ("vel<0", "vel>0", "mavg<0")]
    return [f"roe:{d}:vn<0" for d in others] + [f"!roe:{d}:vn<0" for d in others]


def _ends(axis, sign):
    """characteristic faces across the fast axis: all four arms, inflow on the face the stream
    enters by"""
    lo = 2 * "ijk".index(axis) + 1
    inn, out = (lo, lo + 1) if sign > 0 else (lo + 1, lo)
    return [f"bc:{inn}:characteristic:supIn", f"bc:{inn}:characteristic:subIn",
            f"bc:{out}:characteristic:supOut", f"bc:{out}:characteristic:subOut"]


def _case(lib, axis, sign, claims, tp=False, kind="single", steps=3, ramp=None, **deck):
    return dict(lib=lib, axis=axis, sign=sign, tp=tp, kind=kind, steps=steps, ramp=ramp,
                deck=deck, claims=claims)


VAN_ALBADA = ["muscl:vanAlbada:lim=0", "muscl:vanAlbada:den*sq<=0"]
MINMOD = ["muscl:minmod:clip0", "muscl:minmod:clip1"]

CASES = {
    # ---- 5-equation library ----------------------------------------------------------
    "ausm_muscl_rk4_i_plus": _case(
        5, "i", +1, _fast("ausm", "i", +1) + _cross("ausm", "i") + _ends("i", +1) + VAN_ALBADA,
        **BOX5, bcs=FARFIELD, inviscid_flux="ausm", time_integration="rk4", cfl=0.5),
    "ausm_muscl_rk4_k_minus": _case(
        5, "k", -1, _fast("ausm", "k", -1) + _cross("ausm", "k") + _ends("k", -1) + VAN_ALBADA,
        **BOX5, bcs=FARFIELD, inviscid_flux="ausm", time_integration="rk4", cfl=0.5),
    "roe_minmod_rk4_j_minus": _case(
        5, "j", -1, _fast("roe", "j", -1) + _cross("roe", "j") + MINMOD +
        ["bc:4:pressureOutlet:regular", "bc:3:characteristic:supOut",
         "bc:3:characteristic:subOut"],
        **BOX5, bcs=OUTLETS, limiter="minmod", time_integration="rk4", cfl=0.5),
    "roe_minmod_rk4_i_plus": _case(
        5, "i", +1, _fast("roe", "i", +1) + _cross("roe", "i") + MINMOD +
        ["bc:2:pressureOutlet:fallback", "bc:2:pressureOutlet:regular",
         "bc:1:characteristic:supIn", "bc:1:characteristic:subIn"],
        **BOX5, bcs=OUTLETS, limiter="minmod", time_integration="rk4", cfl=0.5),
    "weno_ausm_lusgs2_i_minus": _case(
        5, "i", -1, _fast("ausm", "i", -1) + _cross("ausm", "i") + _ends("i", -1),
        **BOX5, bcs=FARFIELD, face_reconstruction="weno", limiter="none", inviscid_flux="ausm",
        time_integration="implicitEuler", matrix_solver="lusgs", matrix_sweeps=2, cfl=10.0),
    "wenoz_roe_bdf2_k_plus": _case(
        5, "k", +1, _fast("roe", "k", +1) + _cross("roe", "k") + _ends("k", +1),
        **BOX5, bcs=FARFIELD, face_reconstruction="wenoZ", limiter="none",
        time_integration="bdf2", nonlinear_iterations=3, dt=2.0e-5, dual_time_cfl=100.0,
        matrix_sweeps=2),
    "roe_jacobian_lusgs2_j_plus": _case(
        5, "j", +1, _fast("roe", "j", +1) + _cross("roe", "j") + _ends("j", +1),
        **BOX5, bcs=FARFIELD, inv_flux_jac="approximateRoe", time_integration="implicitEuler",
        matrix_solver="lusgs", matrix_sweeps=2, cfl=10.0),
    "roe_jacobian_dplur3_i_minus": _case(
        5, "i", -1, _fast("roe", "i", -1) + _cross("roe", "i") + _ends("i", -1),
        **BOX5, bcs=FARFIELD, inv_flux_jac="approximateRoe", time_integration="implicitEuler",
        matrix_solver="dplur", matrix_sweeps=3, cfl=5.0),
    # (the implicit decks run at CFL 2: the field is no steady state, and at CFL 10 the second
    # ghost layer of the far field goes to negative pressures within three steps)
    "blusgs_ausm_j_plus": _case(
        5, "j", +1, _fast("ausm", "j", +1) + _cross("ausm", "j") + _ends("j", +1),
        **BOX5, bcs=FARFIELD, inviscid_flux="ausm", time_integration="implicitEuler",
        matrix_solver="blusgs", matrix_sweeps=2, cfl=2.0),
    "bdplur_ausm_i_minus": _case(
        5, "i", -1, _fast("ausm", "i", -1) + _cross("ausm", "i") + _ends("i", -1),
        **BOX5, bcs=FARFIELD, inviscid_flux="ausm", time_integration="implicitEuler",
        matrix_solver="bdplur", matrix_sweeps=3, cfl=2.0),
    "visc_ausm_lusgs_j_plus": _case(
        5, "j", +1, _fast("ausm", "j", +1) + _ends("j", +1),
        **BOX5, bcs=WALL_K, equation_set="navierStokes", inviscid_flux="ausm",
        time_integration="implicitEuler", matrix_solver="lusgs", cfl=2.0),
    "visc_central4th_ausm_rk4_i_minus": _case(
        5, "i", -1, _fast("ausm", "i", -1) + _ends("i", -1),
        **BOX5, bcs=WALL_J, equation_set="navierStokes", inviscid_flux="ausm",
        viscous_face_reconstruction="centralFourth", time_integration="rk4", cfl=0.3),
    "ausm_minmod_rk4_k_plus": _case(
        5, "k", +1, _fast("ausm", "k", +1) + _cross("ausm", "k") + _ends("k", +1) + MINMOD,
        **BOX5, bcs=FARFIELD, inviscid_flux="ausm", limiter="minmod", time_integration="rk4",
        cfl=0.5),
    "ausm_upwind_rk4_j_minus": _case(
        5, "j", -1, _fast("ausm", "j", -1) + _cross("ausm", "j") + _ends("j", -1),
        **BOX5, bcs=FARFIELD, inviscid_flux="ausm", face_reconstruction="upwind",
        limiter="none", time_integration="rk4", cfl=0.5),
    "boundary_box_i_plus": _case(
        5, "i", +1, ["bc:1:inlet:sup", "bc:1:inlet:sub", "bc:2:pressureOutlet:fallback",
                     "bc:2:pressureOutlet:regular"],
        **BOX5, bcs=BOX_PLUS, time_integration="implicitEuler", matrix_solver="lusgs", cfl=5.0),
    "boundary_box_i_minus": _case(
        5, "i", -1, ["bc:2:inlet:sup", "bc:2:inlet:sub", "bc:1:pressureOutlet:fallback",
                     "bc:1:pressureOutlet:regular"],
        **BOX5, bcs=BOX_MINUS, inviscid_flux="ausm", time_integration="implicitEuler",
        matrix_solver="lusgs", cfl=5.0),
    "hold_arm_ramp_i_plus": _case(
        5, "i", +1, ["bc:3:extrap:held", "bc:3:extrap:extrapolated"], ramp=RAMP,
        **BOX5, bcs=FARFIELD, time_integration="rk4", cfl=0.5),
    "stacked_ausm_dplur_i_minus": _case(
        5, "i", -1, _fast("ausm", "i", -1) + _ends("i", -1), kind="stacked",
        n=(8, 7, 6), nblocks=2, stretch=1.1, bcs=FARFIELD, inviscid_flux="ausm",
        limiter="none", time_integration="implicitEuler", matrix_solver="dplur",
        matrix_sweeps=4, cfl=20.0),
    # ---- 7-equation library: the turbulence waves of roe_flux under |vnR|, far-field
    # turbulence on the supersonic-inflow arm -------------------------------------------------
    "sst_roe_lusgs_i_plus": _case(
        7, "i", +1, _fast("roe", "i", +1) + _ends("i", +1),
        **RANS, matrix_solver="lusgs", matrix_sweeps=2),
    "sst_roe_lusgs_k_minus": _case(
        7, "k", -1, _fast("roe", "k", -1) + _ends("k", -1),
        **RANS, matrix_solver="lusgs", matrix_sweeps=2),
    "sst_ausm_blusgs_i_plus": _case(
        7, "i", +1, _fast("ausm", "i", +1) + _ends("i", +1),
        **RANS, inviscid_flux="ausm", matrix_solver="blusgs", matrix_sweeps=2),
    "sst_ausm_blusgs_k_minus": _case(
        7, "k", -1, _fast("ausm", "k", -1) + _ends("k", -1),
        **RANS, inviscid_flux="ausm", matrix_solver="blusgs", matrix_sweeps=2),
    # ---- thermally perfect libraries, at ~2000 K ---------------------------------------------
    "tp_ausm_muscl_rk4_j_plus": _case(
        5, "j", +1, _fast("ausm", "j", +1) + _ends("j", +1), tp=True,
        **BOX5, bcs=FARFIELD, inviscid_flux="ausm", time_integration="rk4", cfl=0.5),
    "tp_sst_roe_lusgs_i_minus": _case(
        7, "i", -1, _fast("roe", "i", -1) + _ends("i", -1), tp=True,
        **RANS, matrix_solver="lusgs", matrix_sweeps=2),
}

# ---- kernel forms (GPU module; the host module checks that their fields stay physical) ----
FORMS = {
    # inviscid tile / march / gather: AUSM + WENO, ragged tile edges in i and j
    "kernel": _case(
        5, "i", -1, _fast("ausm", "i", -1) + _cross("ausm", "i"),
        n=(70, 13, 9), stretch=1.15, skew=0.01, bcs=FARFIELD, face_reconstruction="weno",
        limiter="none", inviscid_flux="ausm", time_integration="rk4", cfl=0.5),
    # viscous tile / march / gather
    "visc": _case(
        5, "i", -1, _fast("roe", "i", -1) + _cross("roe", "i"),
        n=(70, 15, 9), stretch=1.1, skew=0.01, bcs=WALL_J, equation_set="navierStokes",
        time_integration="rk4", cfl=0.3),
    # LU-SGS kp / plane, two sweeps (both triangles)
    "lusgs": _case(
        5, "j", +1, _fast("ausm", "j", +1) + _cross("ausm", "j"),
        n=(21, 19, 17), stretch=1.1, bcs=WALL_K, equation_set="navierStokes",
        inviscid_flux="ausm", time_integration="implicitEuler", matrix_solver="lusgs",
        matrix_sweeps=2, cfl=2.0),
}


def build(spec):
    deck = dict(spec["deck"])
    if spec["tp"]:
        deck["thermodynamic_model"] = TP
    return flow_fields.transonic_case(spec["axis"], spec["sign"], kind=spec["kind"],
                                      temperature_factor=HOT if spec["tp"] else 1.0,
                                      ramp=spec["ramp"], **deck)


def reconstruction(spec):
    return "weno" if spec["deck"].get("face_reconstruction", "").startswith("weno") else "muscl"


def flux(spec):
    return spec["deck"].get("inviscid_flux", "roe")


# ---- what the table as a whole has to cover (test_every_branch_is_covered_by_the_cases) ----
REQUIRED = (
    [f"ausm:{d}:{n}" for d in "ijk" for n in AUSM] +
    [f"roe:{d}:{n}" for d in "ijk" for n in ROE] +
    VAN_ALBADA + MINMOD +
    ["characteristic:low:" + a for a in CHARACTERISTIC] +
    ["characteristic:high:" + a for a in CHARACTERISTIC] +
    ["inlet:sup", "inlet:sub", "pressureOutlet:fallback", "pressureOutlet:regular",
     "extrap:held", "extrap:extrapolated"])


def arm(key):
    """a claimed census key as an entry of REQUIRED (boundary arms: without the surface
    number, characteristic ones by low / high surface)"""
    if not key.startswith("bc:"):
        return key
    _, side, kind, name = key.split(":")
    if kind == "characteristic":
        return f"characteristic:{'low' if int(side) % 2 else 'high'}:{name}"
    return f"{kind}:{name}"
