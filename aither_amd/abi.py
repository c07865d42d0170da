"""ctypes mirror of include/aither_gfx950.h (plumbing only).

`bind(lib, prefix)` attaches argument/return types to every entry point the
header declares, for either the product library (prefix "agx_") or the CPU
oracle used by the tests (prefix "ora_", same signatures).
"""
import ctypes as C

import numpy as np

RECON = {"constant": 0, "muscl": 1, "weno": 2, "wenoZ": 3}
LIMITER = {"none": 0, "vanAlbada": 1, "minmod": 2}
FLUX = {"roe": 0, "ausm": 1}
TIME = {"explicitEuler": 0, "rk4": 1, "implicitEuler": 2,
        "crankNicholson": 3, "bdf2": 4}
SOLVER = {"lusgs": 0, "dplur": 1, "blusgs": 2, "bdplur": 3}
EQN = {"euler": 0, "navierStokes": 1, "rans": 2, "largeEddySimulation": 3}
JACOBIAN = {"rusanov": 0, "approximateRoe": 1}
VISC_RECON = {"central": 0, "centralFourth": 1}
TURB = {"none": 0, "sst2003": 1, "kOmegaWilcox2006": 2, "sstdes": 3, "wale": 4}
BC = {"slipWall": 0, "viscousWall": 1, "characteristic": 2, "inlet": 3,
      "supersonicInflow": 4, "supersonicOutflow": 5, "stagnationInlet": 6,
      "pressureOutlet": 7, "interblock": 8, "periodic": 9}
FIELD = {"state": 0, "residual": 1, "dt": 2, "spec_radius": 3, "cons_n": 4,
         "update": 5, "diagonal": 6, "temperature": 7, "viscosity": 8,
         "cons_nm1": 9, "vel_grad": 10, "temp_grad": 11, "dens_grad": 12,
         "press_grad": 13,
         # the geometry the device holds (download only), ghost cells included
         "volume": 14, "center": 15, "farea_i": 16, "farea_j": 17, "farea_k": 18,
         "width_i": 19, "width_j": 20, "width_k": 21, "wall_dist": 22}
# time statistics: one weight (upload only) / the raw accumulators of a block.  Payloads of
# their own layout, not arrays over the block's cells: FIELD resolves their names
# (FIELD["stat_sample"]), but iterating FIELD gives the block-shaped fields only -- the ones
# Solver.upload / download move (Solver.stats_* move these two).  Only FIELD[name] sees the two
# names: `name in FIELD`, FIELD.get(name), len and iteration do NOT (tests/probe.py holds the
# iterated set to the block-shaped fields); ask STAT_FIELD for those.
STAT_FIELD = {"stat_sample": 23, "stat_accum": 24}
# time series at chosen cells and wall faces (AGX_FIELD_SERIES_*): the plan, one sample (upload
# only), the recorded rows, the nearest-cell search.  Payloads of their own layout like the two
# above, and resolved the same way: FIELD["series_plan"] works, iteration does not see them.
SERIES_FIELD = {"series_plan": 25, "series_sample": 26, "series_rows": 27, "series_locate": 28}
SERIES_KIND = {"cells": 0, "wall": 1}
# spectra along a homogeneous direction (AGX_FIELD_SPECTRA_*): the plan, one sample (upload of
# a weight), the raw accumulators, the dimensional values.  Resolved like the series ids.
SPECTRA_FIELD = {"spectra_plan": 29, "spectra_sample": 30, "spectra_accum": 31,
                 "spectra_values": 32}
SPECTRA_NAMES = ("density", "vel_x", "vel_y", "vel_z", "pressure", "temperature")
SPECTRA_MAX_N = 1024


class _Fields(dict):
    def __missing__(self, name):
        if name in SERIES_FIELD:
            return SERIES_FIELD[name]
        if name in SPECTRA_FIELD:
            return SPECTRA_FIELD[name]
        return STAT_FIELD[name]


FIELD = _Fields(FIELD)
# geometry fields: (components, direction with one more entry or None)
GEOM_FIELDS = {"volume": (1, None), "center": (3, None), "farea_i": (4, "i"),
               "farea_j": (4, "j"), "farea_k": (4, "k"), "width_i": (1, None),
               "width_j": (1, None), "width_k": (1, None), "wall_dist": (1, None)}
HALO_STATE, HALO_UPDATE, HALO_VELGRAD_A, HALO_VELGRAD_B, HALO_TURB = 0, 1, 2, 3, 4
# variables of a function file (AGX_OUT_*), under the reference's names (output.cpp:235-407)
OUT = {"density": 0, "vel_x": 1, "vel_y": 2, "vel_z": 3, "pressure": 4, "mach": 5, "sos": 6,
       "dt": 7, "temperature": 8, "energy": 9, "enthalpy": 10, "cp": 11, "cv": 12, "rank": 13,
       "globalPosition": 14, "viscosityRatio": 15, "turbulentViscosity": 16, "viscosity": 17,
       "tke": 18, "sdr": 19, "f1": 20, "f2": 21, "wallDistance": 22}
for _n, _base in (("velGrad", 23),):
    for _q, _c in enumerate(("ux", "vx", "wx", "uy", "vy", "wy", "uz", "vz", "wz")):
        OUT[f"{_n}_{_c}"] = _base + _q
for _n, _base in (("tempGrad", 32), ("densityGrad", 35), ("pressGrad", 38), ("tkeGrad", 41),
                  ("omegaGrad", 44)):
    for _q, _c in enumerate("xyz"):
        OUT[f"{_n}_{_c}"] = _base + _q
for _q, _c in enumerate(("mass", "mom_x", "mom_y", "mom_z", "energy", "tke", "sdr")):
    OUT[f"resid_{_c}"] = 47 + _q
# variables of the wall function file (AGX_WALL_*), under the reference's names
# (output.cpp:519-553); shearStress_x/y/z: the components, an extension
WALL_OUT = {"yplus": 64, "shearStress": 65, "viscosityRatio": 66, "heatFlux": 67,
            "frictionVelocity": 68, "density": 69, "pressure": 70, "temperature": 71,
            "viscosity": 72, "tke": 73, "sdr": 74,
            "shearStress_x": 75, "shearStress_y": 76, "shearStress_z": 77}
# variables of the nodal function file (AGX_NODE_BASE + AGX_OUT_*): the names of OUT
NODE_BASE = 128
NODE_OUT = {_n: NODE_BASE + _v for _n, _v in OUT.items()}
# integrated wall loads (AGX_LOAD_*): one value per load surface (viscousWall, slipWall)
LOAD_BASE = 256
LOAD_OUT = {"area": LOAD_BASE}
for _n, _base in (("area", 1), ("pressureForce", 4), ("viscousForce", 7)):
    for _q, _c in enumerate("xyz"):
        LOAD_OUT[f"{_n}_{_c}"] = LOAD_BASE + _base + _q
LOAD_OUT["heatLoad"] = LOAD_BASE + 10
for _n, _base in (("pressureMoment", 11), ("viscousMoment", 14)):
    for _q, _c in enumerate("xyz"):
        LOAD_OUT[f"{_n}_{_c}"] = LOAD_BASE + _base + _q
LOAD_MOMENTS = tuple(_n for _n in LOAD_OUT if "Moment" in _n)
# boundary fluxes (AGX_FLUX_*): one value per flux surface, positive out of the block; and the
# block balance (AGX_BUDGET_*): one value per id.  EQUATIONS: the library's equations in order.
EQUATIONS = ("mass", "mom_x", "mom_y", "mom_z", "energy", "tke", "sdr")
FLUX_BASE, FLUX_END, BUDGET_BASE, BUDGET_END = 384, 399, 448, 463
FLUX_OUT = {"area": FLUX_BASE}
BUDGET_OUT = {"volume": BUDGET_BASE}
for _q, _c in enumerate(EQUATIONS):
    FLUX_OUT[f"inviscid_{_c}"] = FLUX_BASE + 1 + _q
    BUDGET_OUT[f"total_{_c}"] = BUDGET_BASE + 1 + _q
for _q, _c in enumerate(EQUATIONS):
    FLUX_OUT[f"viscous_{_c}"] = FLUX_BASE + 8 + _q
    BUDGET_OUT[f"residual_{_c}"] = BUDGET_BASE + 8 + _q
# time statistics of the cells (AGX_STAT_BASE + n): means, velocity co-moments, variances
STAT_BASE, STAT_END = 512, 533
STAT_OUT = {_n: STAT_BASE + _q for _q, _n in enumerate(
    ["mean_density", "mean_vel_x", "mean_vel_y", "mean_vel_z", "mean_pressure",
     "mean_temperature", "mean_mom_x", "mean_mom_y", "mean_mom_z", "mean_turbulentViscosity",
     "mean_tke", "mean_sdr", "cov_uu", "cov_uv", "cov_uw", "cov_vv", "cov_vw", "cov_ww",
     "var_density", "var_pressure", "var_temperature"])}
# ... and of the viscousWall faces (AGX_WSTAT_BASE + n): the mean of every wall variable, then
# the variances of the wall pressure and the shear components
WSTAT_BASE, WSTAT_END = 576, 594
WALL_STAT_OUT = {"mean_" + _n: WSTAT_BASE + _v - 64 for _n, _v in WALL_OUT.items()}
for _q, _n in enumerate(("pressure", "shearStress_x", "shearStress_y", "shearStress_z")):
    WALL_STAT_OUT["var_" + _n] = WSTAT_BASE + len(WALL_OUT) + _q
# ... and of the cells collapsed along index directions (AGX_CSTAT_BASE + 32 * mask + n):
# n in the order of STAT_OUT, then the bin's volume; mask bit 0 = i, bit 1 = j, bit 2 = k.
# CSTAT_CHUNK: the collapsed (j, k) positions of a bin are pooled in chunks of this many.
CSTAT_BASE, CSTAT_COUNT, CSTAT_CHUNK = 1024, 22, 64
CSTAT_NAMES = tuple(STAT_OUT) + ("volume",)
# the two means of each second moment
STAT_PAIRS = {"cov_uu": ("mean_vel_x", "mean_vel_x"), "cov_uv": ("mean_vel_x", "mean_vel_y"),
              "cov_uw": ("mean_vel_x", "mean_vel_z"), "cov_vv": ("mean_vel_y", "mean_vel_y"),
              "cov_vw": ("mean_vel_y", "mean_vel_z"), "cov_ww": ("mean_vel_z", "mean_vel_z"),
              "var_density": ("mean_density", "mean_density"),
              "var_pressure": ("mean_pressure", "mean_pressure"),
              "var_temperature": ("mean_temperature", "mean_temperature")}


def cstat_mask(over):
    """The mask of a string out of "i", "j", "k" (e.g. "ik" -> 5)."""
    over = str(over)
    if not over or any(c not in "ijk" for c in over) or len(set(over)) != len(over):
        raise ValueError(f"collapsed directions {over!r}: a non-empty string out of 'i', 'j', "
                         "'k', each at most once")
    return sum(1 << "ijk".index(c) for c in over)


def cstat_id(mask, name):
    """The id of statistics variable `name` (CSTAT_NAMES) collapsed over `mask`."""
    return CSTAT_BASE + 32 * int(mask) + CSTAT_NAMES.index(name)


def series_plan(names, points, capacity, kind="cells"):
    """The payload of AGX_FIELD_SERIES_PLAN: {kind, P, V, capacity, V ids, P points} as
    float64.  kind "cells": names of OUT, points[P, 3] = (i, j, k) of physical cells; kind
    "wall": names of WALL_OUT, points[P] = indices into the block's wall payload.  No points:
    the payload that discards the block's plan."""
    table = OUT if SERIES_KIND[kind] == 0 else WALL_OUT
    per = 3 if SERIES_KIND[kind] == 0 else 1
    pts = np.asarray(points, dtype=np.float64).reshape(-1, per)
    ids = [float(table[n]) for n in names]
    head = [float(SERIES_KIND[kind]), float(len(pts)), float(len(ids)), float(capacity)]
    return np.concatenate([np.array(head + ids, dtype=np.float64), pts.ravel()])


def series_plan_parse(payload):
    """The inverse of series_plan: (names, points, capacity, kind) of a plan payload, points
    as an integer array [P, 3] (cells) or [P] (wall)."""
    a = np.asarray(payload, dtype=np.float64)
    kind = {v: k for k, v in SERIES_KIND.items()}[int(a[0])]
    npts, nvar, capacity = int(a[1]), int(a[2]), int(a[3])
    table = {v: k for k, v in (OUT if kind == "cells" else WALL_OUT).items()}
    names = [table[int(v)] for v in a[4:4 + nvar]]
    pts = a[4 + nvar:].astype(np.int64)
    pts = pts.reshape(npts, 3) if kind == "cells" else pts.reshape(npts)
    return names, pts, capacity, kind


def series_rows_size(npts, nvar, capacity):
    """Doubles of the buffer a download of AGX_FIELD_SERIES_ROWS fills at most."""
    return 4 + capacity * (1 + nvar * npts)


def series_rows_split(payload):
    """A payload of AGX_FIELD_SERIES_ROWS, {P, V, rows, capacity} and rows x {t, V P values},
    into (t[rows], values[rows, V, P]), oldest row first."""
    a = np.asarray(payload, dtype=np.float64)
    npts, nvar, rows = int(a[0]), int(a[1]), int(a[2])
    body = a[4:4 + rows * (1 + nvar * npts)].reshape(rows, 1 + nvar * npts)
    return body[:, 0].copy(), body[:, 1:].reshape(rows, nvar, npts).copy()


def series_rows_join(t, values, capacity):
    """The inverse of series_rows_split: the payload of t[rows] and values[rows, V, P]."""
    v = np.asarray(values, dtype=np.float64)
    rows, nvar, npts = v.shape
    body = np.concatenate([np.asarray(t, dtype=np.float64).reshape(rows, 1),
                           v.reshape(rows, nvar * npts)], axis=1)
    return np.concatenate([np.array([npts, nvar, rows, capacity], dtype=np.float64),
                           body.ravel()])


def spectra_plan(names, pairs=(), along="i", over=""):
    """The payload of AGX_FIELD_SPECTRA_PLAN: {along, over mask, nvar, npair, nvar ids of OUT,
    npair pairs} as float64.  names out of SPECTRA_NAMES; a pair is two of the names, or two
    indices into them.  No names: the payload that frees the block's spectra."""
    names = list(names)
    flat = []
    for a, b in pairs:
        flat += [float(names.index(x)) if isinstance(x, str) else float(x) for x in (a, b)]
    head = [float("ijk".index(along)), float(cstat_mask(over)) if over else 0.0,
            float(len(names)), float(len(flat) // 2)]
    return np.array(head + [float(OUT[n]) for n in names] + flat, dtype=np.float64)


def spectra_plan_parse(payload):
    """The inverse of spectra_plan: (names, pairs as index pairs, along, over)."""
    a = np.asarray(payload, dtype=np.float64)
    nvar, npair = int(a[2]), int(a[3])
    table = {v: k for k, v in OUT.items()}
    names = [table[int(v)] for v in a[4:4 + nvar]]
    pairs = [(int(x), int(y)) for x, y in a[4 + nvar:4 + nvar + 2 * npair].reshape(npair, 2)]
    over = "".join(d for bit, d in enumerate("ijk") if int(a[1]) >> bit & 1)
    return names, pairs, "ijk"[int(a[0])], over


def spectra_shape(extents, along, over):
    """(remaining extents in (k, j, i) order, nmode) of a plan on a block of extents
    (ni, nj, nk)."""
    a = "ijk".index(along)
    rest = tuple(extents[d] for d in (2, 1, 0) if d != a and "ijk"[d] not in over)
    return rest, extents[a] // 2 + 1


def spectra_accum_size(nvar, npair, nbin, nmode):
    """Doubles of an AGX_FIELD_SPECTRA_ACCUM payload."""
    return 8 + nvar + 2 * npair + (nvar + npair) * nbin * nmode


def spectra_accum_split(payload):
    """An AGX_FIELD_SPECTRA_ACCUM payload into (plan payload, W, samples, S[nspec, nbin,
    nmode]), S raw (nondimensional)."""
    a = np.asarray(payload, dtype=np.float64)
    nvar, npair = int(a[2]), int(a[3])
    np_ = 4 + nvar + 2 * npair
    nbin, nmode = int(a[np_ + 2]), int(a[np_ + 3])
    body = a[np_ + 4:np_ + 4 + (nvar + npair) * nbin * nmode]
    return a[:np_].copy(), float(a[np_]), float(a[np_ + 1]), \
        body.reshape(nvar + npair, nbin, nmode).copy()


# cell planes of the accumulators: 9 means + extras (eddy viscosity; k, omega) + 9 second
# moments; wall values per face
STAT_SECOND = 9
STAT_WALL_VALUES = len(WALL_OUT) + 4

c_dp = C.POINTER(C.c_double)


THERMO = {"caloricallyPerfect": 0, "thermallyPerfect": 1}
MAX_VIB = 4     # AGX_MAX_VIB


class Gas(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "gas_constant", "n", "heat_of_formation", "visc_c1", "visc_s",
        "cond_c1", "cond_s", "t_ref", "rho_ref", "l_ref", "a_ref")] + [
        ("n_vib", C.c_int32), ("pad_", C.c_int32), ("theta_v", C.c_double * MAX_VIB)]


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_eq", "n_ghost", "recon", "limiter", "inviscid_flux", "is_viscous",
        "time_integration", "matrix_solver", "matrix_sweeps",
        "nonlinear_iterations", "equation_set", "inv_flux_jacobian",
        "viscous_recon", "turbulence_model")] + [(n, C.c_double) for n in (
            "kappa", "theta", "zeta", "matrix_relaxation", "dual_time_cfl",
            "dt_nondim", "viscous_cfl_coeff")] + [("gas", Gas)] + [
        ("thermodynamic_model", C.c_int32), ("pad_", C.c_int32)]


class BlockGeom(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "ni", "nj", "nk", "ng", "parent_block", "global_pos")] + [
        (n, c_dp) for n in ("farea_i", "farea_j", "farea_k", "vol", "center",
                            "width_i", "width_j", "width_k", "wall_dist",
                            "nodes")]


class BcState(C.Structure):
    _fields_ = [("pressure", C.c_double), ("density", C.c_double),
                ("velocity", C.c_double * 3),
                ("stagnation_pressure", C.c_double),
                ("stagnation_temperature", C.c_double),
                ("direction", C.c_double * 3),
                ("wall_temperature", C.c_double),
                ("wall_heat_flux", C.c_double),
                ("length_scale", C.c_double),
                ("is_isothermal", C.c_int32), ("is_heat_flux", C.c_int32),
                ("is_nonreflecting", C.c_int32), ("pad_", C.c_int32),
                ("turb_intensity", C.c_double), ("eddy_visc_ratio", C.c_double),
                ("von_karman", C.c_double), ("wall_constant", C.c_double),
                ("is_wall_law", C.c_int32), ("pad2_", C.c_int32)]


class BcSurface(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "bc_type", "imin", "imax", "jmin", "jmax", "kmin", "kmax", "tag")] + [
        ("state", BcState)]


class Connection(C.Structure):
    _fields_ = [("rank", C.c_int32 * 2), ("block", C.c_int32 * 2),
                ("local_block", C.c_int32 * 2), ("boundary", C.c_int32 * 2),
                ("d1_start", C.c_int32 * 2), ("d1_end", C.c_int32 * 2),
                ("d2_start", C.c_int32 * 2), ("d2_end", C.c_int32 * 2),
                ("const_surf", C.c_int32 * 2), ("patch_border", C.c_int32 * 8),
                ("orientation", C.c_int32), ("is_interblock", C.c_int32)]


class Slab(C.Structure):
    _fields_ = [("peer", C.c_int32), ("tag", C.c_int32), ("count", C.c_int64),
                ("send", c_dp), ("recv", c_dp)]


SWAP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(Slab), C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


class Exchange(C.Structure):
    _fields_ = [("user", C.c_void_p), ("swap", SWAP_FN), ("allgather", ALLGATHER_FN),
                ("nranks", C.c_int32), ("host_buffers", C.c_int32)]


class Linf(C.Structure):
    _fields_ = [("linf", C.c_double), ("block", C.c_int32), ("i", C.c_int32),
                ("j", C.c_int32), ("k", C.c_int32), ("eqn", C.c_int32),
                ("pad_", C.c_int32)]


# every symbol include/aither_gfx950.h declares: name -> (restype, argtypes)
_vp = C.c_void_p
_i = C.c_int
SYMBOLS = {
    "last_error": (C.c_char_p, []),
    "version": (C.c_char_p, []),
    "ctx_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "ctx_destroy": (None, [_vp]),
    "ctx_set_stream": (_i, [_vp, _vp]),
    "config_set": (_i, [_vp, C.POINTER(Config)]),
    "block_create": (_i, [_vp, C.POINTER(BlockGeom), C.POINTER(_i)]),
    "block_set_bcs": (_i, [_vp, _i, _i, C.POINTER(BcSurface)]),
    "conn_create": (_i, [_vp, C.POINTER(Connection), C.POINTER(_i)]),
    "setup_finalize": (_i, [_vp]),
    "state_upload": (_i, [_vp, _i, c_dp]),
    "field_download": (_i, [_vp, _i, _i, c_dp]),
    "field_upload": (_i, [_vp, _i, _i, c_dp]),
    "output_pack": (_i, [_vp, _i, _i, C.POINTER(C.c_int32), c_dp]),
    "restart_pack": (_i, [_vp, _i, _i, c_dp]),
    "state_fill": (_i, [_vp, _i, c_dp]),
    "state_from_cloud": (_i, [_vp, _i, C.c_int64, c_dp, c_dp, c_dp]),
    "restart_unpack": (_i, [_vp, _i, _i, c_dp]),
    "plot3d_metrics": (_i, [_vp, _i, _i, _i] + [c_dp] * 9),
    "nearest_wall_distance": (_i, [_vp, C.c_int64, c_dp, C.c_int64, c_dp, c_dp]),
    "mg_restrict": (_i, [_vp, _vp, _i, _i, C.POINTER(C.c_int32), c_dp]),
    "mg_matrix_residual": (_i, [_vp, c_dp]),
    "mg_invert_diagonal": (_i, [_vp]),
    "mg_save_update": (_i, [_vp]),
    "mg_reset_diagonal": (_i, [_vp]),
    "mg_prolong": (_i, [_vp, _vp, _i, C.POINTER(C.c_int32), c_dp]),
    "store_time_n": (_i, [_vp, _i]),
    "iterate": (_i, [_vp, _i, C.c_double, c_dp, C.POINTER(Linf), c_dp]),
    "phase_bc_faces": (_i, [_vp]),
    "phase_bc_edges": (_i, [_vp]),
    "phase_residual": (_i, [_vp, _i, C.c_double]),
    "phase_explicit_update": (_i, [_vp, _i, c_dp, C.POINTER(Linf)]),
    "phase_implicit_begin": (_i, [_vp]),
    "phase_relax_forward": (_i, [_vp, _i]),
    "phase_relax_backward": (_i, [_vp, _i]),
    "phase_matrix_residual": (_i, [_vp, c_dp]),
    "phase_implicit_update": (_i, [_vp, _i, c_dp, C.POINTER(Linf)]),
    "halo_swap_local": (_i, [_vp, _i]),
    "halo_count": (C.c_int64, [_vp, _i, _i]),
    "halo_pack": (_i, [_vp, _i, _i, _vp]),
    "halo_unpack": (_i, [_vp, _i, _i, _vp]),
    "set_exchange": (_i, [_vp, C.POINTER(Exchange)]),
    "rccl_unique_id": (_i, [_vp]),
    "rccl_exchange_create": (_i, [_vp, _vp, _i, _i]),
    "halo_exchange": (_i, [_vp, _i]),
    "timing_enable": (_i, [_vp, _i]),
    "timing_get": (_i, [_vp, _i, c_dp, C.POINTER(C.c_int64)]),
    "timing_reset": (_i, [_vp]),
    "sync": (_i, [_vp]),
}


# Entries that form data on the device and have no host counterpart in the CPU oracle of the
# test suite (the start and resume of a run: the host arrays they replace are the reference
# there).  The product library must export them like every other entry; under any other prefix
# a library may lack them, and the bound name then refuses by name when it is called.
DEVICE_ONLY = ("state_fill", "state_from_cloud", "restart_unpack")


class Api:
    """Namespace of bound functions without the prefix."""

    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix
        for name, (res, args) in SYMBOLS.items():
            if name in DEVICE_ONLY and prefix != "agx_" and not hasattr(lib, prefix + name):
                setattr(self, name, self._not_exported(name))
                continue
            fn = getattr(lib, prefix + name)   # AttributeError if missing
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)

    def _not_exported(self, name):
        def refuse(*_args):
            raise NotImplementedError(f"{self.prefix}{name}: this library does not export it "
                                      "(a device-only entry, abi.DEVICE_ONLY)")
        return refuse

    def check(self, rc, what=""):
        if rc != 0:
            msg = self.last_error()
            raise RuntimeError(f"{self.prefix}{what} failed ({rc}): "
                               f"{msg.decode() if msg else ''}")
