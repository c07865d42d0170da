"""The variables of the reference's nodal function file, restated in numpy.

An independent statement of what WriteNodeFun (output.cpp:452-469) writes for one block:
procBlock::AssignCornerGhostCells (procBlock.cpp:2716-2753), procBlock::CellToNode (:6607-6845)
with ConvertCellToNode (utility.hpp:186-334), the face gradients of CalcGradsI/J/K
(procBlock.cpp:5173-5788, Green-Gauss on the alternate control volume) at every physical face,
and the factors of output.cpp:235-410.  The reference scatters cells and faces to nodes; here a
node gathers, vectorised, in the order the reference's loops reach it (k, j, i ascending; i-faces,
j-faces, k-faces) -- tests/test_node_pack_host.py holds the gather to a transcription of the
scatter loops.

It is fed with downloaded fields only (Solver.download, ghost cells included where the array has
them, [k, j, i, c]): state, residual, dt, wall_dist, volume, farea_i/j/k.

Two statements are the library's, not the reference's: temperature_ and
viscosity_ of the eight corner ghost cells are evaluated from their corner-rule state (the
reference leaves there what the initial condition or a restart put), and viscosityRatio,
turbulentViscosity, f1, f2 are not formed in a turbulent run (0 in a laminar one).
"""
import numpy as np

from aither_amd import abi
from aither_amd.case import fluid

FIELDS = ("state", "residual", "dt", "wall_dist", "volume", "farea_i", "farea_j", "farea_k")
STATE_DERIVED = ("density", "vel_x", "vel_y", "vel_z", "pressure", "mach", "sos", "energy",
                 "enthalpy")
NOT_AT_NODES = ("viscosityRatio", "turbulentViscosity", "f1", "f2")
VEL_NAMES = ("ux", "vx", "wx", "uy", "vy", "wy", "uz", "vz", "wz")


def download_fields(sol, gb):
    return {f: sol.download(f, gb) for f in FIELDS}


def _ijk(a):
    """[k, j, i, c] -> [i, j, k, c]"""
    return np.transpose(a, (2, 1, 0, 3))


def first_layer(a, ng):
    """the physical cells and the first ghost layer of an [i, j, k, c] array with ng layers"""
    c = ng - 1
    return a[c:a.shape[0] - c, c:a.shape[1] - c, c:a.shape[2] - c].copy()


def assign_corner_ghosts(s):
    """AssignCornerGhostCells on an array with one ghost layer: each of the eight corner ghost
    cells is a third of its three edge-ghost neighbours towards the block (i, j, k neighbour)"""
    third = 1.0 / 3.0
    for ig, ii in ((0, 1), (-1, -2)):
        for jg, jj in ((0, 1), (-1, -2)):
            for kg, kk in ((0, 1), (-1, -2)):
                s[ig, jg, kg] = third * (s[ii, jg, kg] + s[ig, jj, kg] + s[ig, jg, kk])
    return s


def boundary_count(ni, nj, nk):
    """per node: in how many directions it lies on the block's boundary (3: AtInteriorCorner,
    2: AtInteriorEdge, 1: AtInterior of the node array, 0: inside)"""
    bi = np.zeros(ni + 1, int); bi[[0, ni]] = 1
    bj = np.zeros(nj + 1, int); bj[[0, nj]] = 1
    bk = np.zeros(nk + 1, int); bk[[0, nk]] = 1
    return bi[:, None, None] + bj[None, :, None] + bk[None, None, :]


def gather8(a):
    """a: [ni + 2, nj + 2, nk + 2, c] -> the sum of the eight cells around each node, in the
    order k, j, i ascending: [ni + 1, nj + 1, nk + 1, c].  (Cells the reference skips are
    entered as zeros: adding zero changes nothing.)"""
    ni, nj, nk = a.shape[0] - 1, a.shape[1] - 1, a.shape[2] - 1
    acc = np.zeros((ni, nj, nk) + a.shape[3:])
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                acc = acc + a[di:di + ni, dj:dj + nj, dk:dk + nk]
    return acc


def cell_to_node(a, ng, ignore_edge=False):
    """ConvertCellToNode of an [i, j, k, c] array with ng ghost layers (0: the no-ghost path)"""
    if ng > 0:
        s = first_layer(a, ng)
        if ignore_edge:      # edge and corner ghost cells are skipped
            gi = np.zeros(s.shape[0], int); gi[[0, -1]] = 1
            gj = np.zeros(s.shape[1], int); gj[[0, -1]] = 1
            gk = np.zeros(s.shape[2], int); gk[[0, -1]] = 1
            skip = gi[:, None, None] + gj[None, :, None] + gk[None, None, :] > 1
            s[skip] = 0.0
    else:
        s = np.pad(a, ((1, 1), (1, 1), (1, 1), (0, 0)))
    node = gather8(s)
    if not ignore_edge:
        return node * 0.125
    nb = boundary_count(a.shape[0] - 2 * ng, a.shape[1] - 2 * ng, a.shape[2] - 2 * ng)
    corner, edge = (0.25, 1.0 / 6.0) if ng > 0 else (1.0, 0.5)
    fac = np.where(nb == 3, corner, np.where(nb == 2, edge, 0.125))
    return node * fac[..., None]


def face_gradients(A, d, ng, n, R):
    """Green-Gauss gradient (CalcGradsI/J/K) at every physical d-face: [faces..., r, f] with
    f: u, v, w, T, rho, p (, k, omega) and r the direction of the derivative.
    A: {name: [i, j, k, c]} with ghost cells; n = (ni, nj, nk)"""
    cnt = list(n)
    cnt[d] += 1
    e = np.eye(3, dtype=int)
    others = [t for t in range(3) if t != d]

    def at(name, off):          # cell or lower-face index (U + off)
        sl = tuple(slice(ng + off[q], ng + off[q] + cnt[q]) for q in range(3))
        return A[name][sl]

    def area(t, off):
        a = at("farea_" + "ijk"[t], off)
        return a[..., :3] * a[..., 3:4]

    def phi(off):
        s = at("state", off)
        with np.errstate(divide="ignore", invalid="ignore"):
            temp = s[..., 4] / (s[..., 0] * R)
        cols = [s[..., 1], s[..., 2], s[..., 3], temp, s[..., 0], s[..., 4]]
        cols += [s[..., q] for q in range(5, s.shape[-1])]
        return np.stack(cols, -1)

    U, L = np.zeros(3, int), -e[d]
    a_up, a_lo = [None] * 3, [None] * 3
    a_up[d] = 0.5 * (area(d, U) + area(d, U + e[d]))
    a_lo[d] = 0.5 * (area(d, U) + area(d, U - e[d]))
    for t in others:
        a_up[t] = 0.5 * (area(t, U + e[t]) + area(t, L + e[t]))
        a_lo[t] = 0.5 * (area(t, U) + area(t, L))
    vol = 0.5 * (at("volume", L) + at("volume", U))
    v_up, v_lo = [None] * 3, [None] * 3
    v_up[d], v_lo[d] = phi(U), phi(L)
    for t in others:
        v_up[t] = 0.25 * (phi(L) + phi(U) + phi(U + e[t]) + phi(L + e[t]))
        v_lo[t] = 0.25 * (phi(L) + phi(U) + phi(U - e[t]) + phi(L - e[t]))
    acc = 0.0
    for t in range(3):
        acc = acc + v_up[t][..., None, :] * a_up[t][..., :, None] \
            - v_lo[t][..., None, :] * a_lo[t][..., :, None]
    return acc / vol[..., None]


def faces_to_nodes(G, n):
    """CellToNode's gradient part: G[d]: [faces of direction d..., ...]; every face to its four
    nodes (i-faces, j-faces, k-faces; within a direction k, j, i ascending), times 1/3, 1/5,
    1/8, 1/12 by the node's place"""
    ni, nj, nk = n
    acc = np.zeros((ni + 1, nj + 1, nk + 1) + G[0].shape[3:])
    for d in range(3):
        pad = [(1, 1)] * 3 + [(0, 0)] * (G[d].ndim - 3)
        pad[d] = (0, 0)
        P = np.pad(G[d], pad)
        t1, t2 = [t for t in range(3) if t != d]          # t1 < t2: t2 is the outer loop
        for o2 in (0, 1):
            for o1 in (0, 1):
                sl = [slice(None)] * 3
                sl[t1] = slice(o1, o1 + n[t1] + 1)
                sl[t2] = slice(o2, o2 + n[t2] + 1)
                acc = acc + P[tuple(sl)]
    nb = boundary_count(ni, nj, nk)
    fac = np.where(nb == 3, 1.0 / 3.0, np.where(nb == 2, 1.0 / 5.0,
                                                np.where(nb == 1, 1.0 / 8.0, 1.0 / 12.0)))
    return acc * fac.reshape(fac.shape + (1,) * (acc.ndim - 3))


def node_vars(fields, gas, ng, rank=0, global_pos=0, turbulent=False):
    """{name: [nk + 1, nj + 1, ni + 1]} for every name of abi.OUT the nodal file can hold,
    dimensional; also "state" [..., c], the nondimensional node state.
    gas: the case's nondimensional gas (aither_amd.case.fluid.Gas)"""
    A = {name: _ijk(np.asarray(a)) for name, a in fields.items()}
    ni, nj, nk = A["dt"].shape[:3]
    n = (ni, nj, nk)
    n_eq = A["state"].shape[-1]
    R = gas.gas_constant
    rR, aR, lR, tR = gas.rho_ref, gas.a_ref, gas.l_ref, gas.t_ref
    muR = gas.visc_c1 * tR ** 1.5 / (tR + gas.visc_s)

    # rule 1: the node state, corner ghost cells by the corner rule
    cells = assign_corner_ghosts(first_layer(A["state"], ng))
    s = gather8(cells) * 0.125
    rho, vel, p = s[..., 0], s[..., 1:4], s[..., 4]
    t_state = p / (rho * R)
    v2 = (vel ** 2).sum(-1)
    cv_s = fluid.cv(gas, t_state)
    cs = np.sqrt((cv_s + R) / cv_s * p / rho)
    en = fluid.spec_energy(gas, t_state) + 0.5 * v2
    # rule 2: the averages of temperature_ and viscosity_
    t_cell = cells[..., 4:5] / (cells[..., 0:1] * R)
    temp = t_cell * tR
    mu_cell = gas.visc_c1 * temp * np.sqrt(temp) / ((temp + gas.visc_s) * muR)
    t_node = (gather8(t_cell) * 0.125)[..., 0]
    mu_node = (gather8(mu_cell) * 0.125)[..., 0]
    cv_n = fluid.cv(gas, t_node)
    # rules 3, 4
    dt = cell_to_node(A["dt"], 0, True)[..., 0]
    res = cell_to_node(A["residual"], 0, True)
    wd = cell_to_node(A["wall_dist"], ng, True)[..., 0]
    # rule 5
    G = faces_to_nodes([face_gradients(A, d, ng, n, R) for d in range(3)], n)   # [..., r, f]

    one = np.ones_like(rho)
    out = {
        "density": rho * rR, "vel_x": vel[..., 0] * aR, "vel_y": vel[..., 1] * aR,
        "vel_z": vel[..., 2] * aR, "pressure": p * rR * aR * aR,
        "mach": np.sqrt(v2) / cs, "sos": cs * aR, "dt": dt / (aR * lR),
        "temperature": t_node * tR, "energy": en * aR * aR,
        "enthalpy": (en + p / rho) * aR * aR,
        "cp": (cv_n + R) * one * aR * aR / tR, "cv": cv_n * one * aR * aR / tR,
        "rank": rank * one, "globalPosition": global_pos * one,
        "viscosity": mu_node * muR, "wallDistance": wd * lR,
        "tke": (s[..., 5] if n_eq > 5 else 0.0 * one) * aR * aR,
        "sdr": (s[..., 6] if n_eq > 5 else 0.0 * one) * aR * aR * rR / muR,
    }
    if not turbulent:
        for name in NOT_AT_NODES:
            out[name] = 0.0 * one
    for q, c in enumerate(VEL_NAMES):
        out["velGrad_" + c] = G[..., q // 3, q % 3] * aR / lR
    scales = (("tempGrad", 3, tR / lR), ("densityGrad", 4, rR / lR),
              ("pressGrad", 5, rR * aR * aR / lR), ("tkeGrad", 6, aR * aR / lR),
              ("omegaGrad", 7, aR * aR * rR / (muR * lR)))
    for name, f, sc in scales:
        for r, c in enumerate("xyz"):
            out[f"{name}_{c}"] = (G[..., r, f] if f < G.shape[-1] else 0.0 * one) * sc
    l2 = lR * lR
    rsc = (rR * aR * l2, rR * aR * aR * l2, rR * aR * aR * l2, rR * aR * aR * l2,
           rR * aR ** 3 * l2, rR * aR ** 3 * l2, rR * rR * aR ** 4 * l2 / muR)
    for q, c in enumerate(("mass", "mom_x", "mom_y", "mom_z", "energy", "tke", "sdr")):
        out["resid_" + c] = (res[..., q] if q < n_eq else 0.0 * one) * rsc[q]
    out["state"] = s
    # [i, j, k, ...] -> [k, j, i, ...]
    return {name: np.swapaxes(v, 0, 2) for name, v in out.items()}


def is_gradient_like(name):
    return "Grad" in name or name.startswith("resid")


def compare(got, ref, names, tol_state, tol_grad, log=print, what="node_pack"):
    """every node: |got - ref| <= tol * largest |ref| of the variable over the block; a
    variable whose reference is identically zero must be exactly zero.  got: [nvar, ...] in
    the order of names.  Prints each figure before it asserts; returns the largest ratio of
    either kind."""
    worst = {}
    for q, name in enumerate(names):
        r = ref[name]
        assert got[q].shape == r.shape, (name, got[q].shape, r.shape)
        scale = np.abs(r).max()
        err = np.abs(got[q] - r).max()
        worst[name] = err / scale if scale > 0.0 else err
        log(f"{what} {name}: max |diff| / scale = {worst[name]:.3e}")
    top = {True: 0.0, False: 0.0}
    for q, name in enumerate(names):
        if np.abs(ref[name]).max() == 0.0:
            assert np.all(got[q] == 0.0), name
            continue
        g = is_gradient_like(name)
        assert worst[name] <= (tol_grad if g else tol_state), (name, worst[name])
        top[g] = max(top[g], worst[name])
    log(f"{what}: largest ratio {top[False]:.3e} (state), {top[True]:.3e} (gradients, residuals)")
    return top[False], top[True]
