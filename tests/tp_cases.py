"""Hot synthetic cases for the thermally perfect gas (shared by the CPU and the GPU tests).

The synthetic decks sit at 288 K, where the vibrational part of cv is ~1e-3 of cv; here they
are built with temperature_factor = HOT (~2000 K, theta / T ~ 1.5 for air), and every helper
that hands out a case asserts on its initial state that the mode is excited: in every physical
cell (cv(T) - n R) / cv(T) >= MIN_VIB_SHARE.  That is a condition on the inputs (numpy model,
aither_amd.case.fluid), not a measured number; at HOT the share is ~0.25, so the 5 % perturbed
field stays well inside, and T -- hence gamma, cp, Pr -- differs between the two sides of
every face.

Each case names the rows of DESIGN section 8's device-site table it reaches.
"""
import numpy as np

from aither_amd.case import fluid, synthetic
from aither_amd.case.builder import build_case
from aither_amd.case.inputfile import State
from test_parity_gpu import CASES, RANS_WALL, WALL_J

TP, CP = "thermallyPerfect", "caloricallyPerfect"
HOT = 7.0                # x 288.15 K
MIN_VIB_SHARE = 0.10


def vibrational_share(case):
    """smallest (cv(T) - n R) / cv(T) over the physical cells of the case's initial state"""
    gas, g = case.gas, case.ng
    low = np.inf
    for blk in case.blocks:
        s = blk.state[g:-g, g:-g, g:-g]
        t = s[..., 4] / (s[..., 0] * gas.gas_constant)
        cv = fluid.cv(gas, t)
        low = min(low, float(((cv - gas.n * gas.gas_constant) / cv).min()))
    return low


def excited(case):
    assert case.gas.thermodynamic_model == TP and case.gas.n_vib > 0
    share = vibrational_share(case)
    assert share >= MIN_VIB_SHARE, share
    return case


def hot_single(model=TP, **kw):
    kw.setdefault("amplitude", 0.05)
    case = synthetic.single_block_case(thermodynamic_model=model, temperature_factor=HOT, **kw)
    return excited(case) if model == TP else case


def hot_stacked(**kw):
    kw.setdefault("amplitude", 0.05)
    return excited(synthetic.stacked_blocks_case(thermodynamic_model=TP,
                                                 temperature_factor=HOT, **kw))


def hot_multigrid(**kw):
    kw.setdefault("amplitude", 0.05)
    cases, transfers = synthetic.multigrid_levels(thermodynamic_model=TP,
                                                  temperature_factor=HOT, **kw)
    excited(cases[0])
    return cases, transfers


def stagnation_case(model, factor=1.0):
    """stagnation inlet (i-min) and nonreflecting pressure outlet (i-max), slip walls; the
    stagnation state scaled with the deck's temperature factor"""
    n = (10, 9, 8)
    deck = synthetic.make_deck(thermodynamic_model=model, time_integration="implicitEuler",
                               matrix_solver="lusgs", cfl=5.0, temperature_factor=factor)
    deck.bc_states.append(State("stagnationInlet", dict(tag=11, p0=103300.0 * factor,
                                                        t0=289.7 * factor,
                                                        direction=[1.0, 0.0, 0.0])))
    deck.bcs = [synthetic.box_surfaces(*n, {1: ("stagnationInlet", 11),
                                            2: ("pressureOutlet", 7)})]
    case = build_case(None, deck=deck, coords=[synthetic.box_nodes(*n, 1.1)])
    synthetic.perturbed_state(case)
    return case


# ---- 5-equation library (libaither_gfx950_tp.so) ------------------------------------------
FIVE = {
    # fluxes and reconstruction
    # roe_flux (T_roe, h, a); rho_energy / cons_to_prim of the fused explicit stage; skewed grid
    "muscl_roe_rk4_skew": CASES["cfg2_muscl_roe_rk4"],
    # ausm_flux (gamma of each side), sound_speed of the far field all round, k_update
    "minmod_ausm_euler": CASES["minmod_ausm_euler"],
    # ausm_flux on WENO states; visc_max_term / visc_term / off_diagonal (gamma, Pr of the
    # cell's T); update_prim_with_cons of the off-diagonals; adiabatic wall, pressure outlet
    "weno_ausm_visc_lusgs": CASES["cfg3_weno_ausm_visc_lusgs"],
    # roe_flux on WENO-Z states; bdf2: rho_energy of store_time_n, the state at time n
    "wenoz_roe_bdf2_dual": CASES["wenoz_roe_bdf2_dual"],
    # implicit solvers and Jacobians
    # DPLUR, 4 sweeps (off_diagonal through update_prim_with_cons), far field all round
    "dplur_4sweeps": CASES["dplur_muscl_ausm"],
    # inv_flux_jacobian gamma(T), tsl_jacobian gamma(T) (laminar: mu_t cp = 0), BLU-SGS
    "blusgs_visc_2sweeps": CASES["blusgs_weno_ausm_visc_2sweeps"],
    # the same Jacobians in BDPLUR; isothermal moving wall (ghost density of the wall T)
    "bdplur_visc_iso_wall": CASES["bdplur_visc_iso_wall"],
    # approximateRoe: roe_flux of the updated state in the off-diagonals, LU-SGS 2 sweeps
    "roe_jacobian_lusgs2": CASES["roe_jacobian_lusgs2"],
    # Crank-Nicholson, viscous: state at time n through rho_energy / temperature_from_energy
    "visc_iso_crank_lusgs": CASES["visc_iso_crank_lusgs"],
    # centralFourth viscous faces (temperature of the four-cell face state)
    "visc_central4th_lusgs": CASES["visc_central4th_lusgs"],
    # ghost states
    # nonreflecting inlet / outlet with bdf2: gamma(T_n), sound_speed of the state at time n,
    # cons_to_prim of the state at time n
    "nonreflecting_bdf2_lusgs": CASES["nonreflecting_bdf2_lusgs"],
    # constant-heat-flux wall (low-Re), pressure outlet
    "visc_heatflux_wall_lusgs": CASES["visc_heatflux_wall_lusgs"],
}

# ---- 7-equation library (libaither_gfx950_rans_tp.so) --------------------------------------
RANS_BASE = dict(n=(9, 8, 7), stretch=1.2, bcs=RANS_WALL, equation_set="rans",
                 turbulence_model="sst2003", time_integration="implicitEuler", cfl=10.0)
RANS = {
    # tsl_jacobian mu_t cp(T) / Pr_t, rans_cell_direction (gamma, Pr of the cell's T), rans
    # viscous flux mu_t cp(T_face) / Pr_t; BLU-SGS
    "sst_blusgs": dict(matrix_solver="blusgs", matrix_sweeps=2),
    # the same with ausm_flux and BDPLUR
    "sst_bdplur_ausm": dict(matrix_solver="bdplur", matrix_sweeps=3, inviscid_flux="ausm"),
    # Wilcox 2006 (Pr_t = 8 / 9 in mu_t cp(T) / Pr_t), scalar LU-SGS: visc_term, off_diagonal
    "wilcox2006_lusgs": dict(turbulence_model="kOmegaWilcox2006", matrix_solver="lusgs",
                             matrix_sweeps=2),
    # SST-DES, scalar LU-SGS
    "sstdes_lusgs": dict(turbulence_model="sstdes", matrix_solver="lusgs", matrix_sweeps=2,
                         turbulence=(0.2, 2.4e4)),
}
# supersonic inflow / outflow, subsonic inlet, pressure outlet (sound_speed in the inlet /
# outlet ghosts), beside a viscous wall and a characteristic far field: Mach ~0.06 and ~1.3
# at ~2000 K (a ~ 870 m/s)
RANS_BOX_BCS = {1: ("supersonicInflow", 8), 2: ("supersonicOutflow", 9), 3: ("viscousWall", 2),
                4: ("characteristic", 1), 5: ("inlet", 10), 6: ("pressureOutlet", 3)}
RANS_BOX_VELOCITIES = [(50.0, 20.0, 10.0), (1100.0, 20.0, 10.0)]
# wall law: Pr and cp of the interior T (of the wall T for the isothermal wall's recovery
# factor), cp(T_wall) in UpdateGamma, the wall-law ghost's kappa with cp(T_wall)
WALL_LAW = [(2, "lusgs"), (4, "lusgs"), (5, "lusgs"), (4, "blusgs")]


def rans_case(name):
    deck = dict(RANS_BASE)
    deck.update(RANS[name])
    return hot_single(**deck)


def rans_box_case(vel):
    return hot_single(n=(9, 8, 7), stretch=1.2, bcs=RANS_BOX_BCS, equation_set="rans",
                      turbulence_model="sst2003", velocity=list(vel),
                      time_integration="implicitEuler", cfl=5.0)


def wall_law_case(tag, solver):
    wall = dict(RANS_WALL)
    wall[3] = ("viscousWall", tag)
    return hot_single(n=(9, 8, 7), stretch=1.2, bcs=wall, equation_set="rans",
                      turbulence_model="sst2003", matrix_solver=solver,
                      time_integration="implicitEuler", cfl=10.0, wall_treatment="wallLaw")


# connections: the ghost cells of the off-diagonals come from the neighbour block
def stacked_five():
    return hot_stacked(n=(7, 8, 6), nblocks=2, axis="i", stretch=1.15, bcs=WALL_J,
                       equation_set="navierStokes", time_integration="implicitEuler",
                       matrix_solver="blusgs", matrix_sweeps=3, cfl=10.0)


def stacked_rans():
    return hot_stacked(n=(7, 8, 6), nblocks=2, axis="i", stretch=1.15, bcs=RANS_WALL,
                       equation_set="rans", turbulence_model="sst2003",
                       time_integration="implicitEuler", matrix_solver="lusgs",
                       matrix_sweeps=2, cfl=10.0)


# multigrid, W cycle, three levels, two blocks: k_mg_restrict / k_mg_prolong with
# prim_to_cons / cons_to_prim, the forcing term
def multigrid_five():
    return hot_multigrid(n=(12, 10, 8), nblocks=2, axis="i", stretch=1.1, levels=3, cycle="W",
                         time_integration="implicitEuler", matrix_solver="dplur",
                         matrix_sweeps=4, cfl=40.0)


def multigrid_rans():
    return hot_multigrid(n=(12, 10, 8), nblocks=2, axis="i", stretch=1.15, levels=3, cycle="W",
                         bcs=RANS_WALL, equation_set="rans", turbulence_model="sst2003",
                         time_integration="implicitEuler", matrix_solver="blusgs",
                         matrix_sweeps=2, cfl=10.0)
