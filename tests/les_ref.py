"""The viscous operator of a block with the WALE subgrid model, restated in numpy.

An independent statement of procBlock::CalcViscFluxI/J/K (procBlock.cpp:1233-2135) for
equationSet largeEddySimulation / turbulenceModel wale, every face of a block in all three
directions:

  * the Green-Gauss face gradients of (u, v, w, T) of CalcGradsI/J/K (:5173-5788, VectorGradGG /
    ScalarGradGG utility.cpp:59-188) on the alternate control volume,
  * the face state and viscosity of FaceReconCentral / FaceReconCentral4th
    (reconstruction.hpp:315-379 with LagrangeCoeff utility.cpp:449-483),
  * turbWale::EddyVisc (turbulence.cpp:967-996) with length = half the sum of the two cells'
    widths across the face (procBlock.cpp:1357-1365); the value carries no density and no
    InvNondimScaling, CalcFlux multiplies it by NondimScaling like any viscosity,
  * viscousFlux::CalcFlux (viscousFlux.cpp:58-135): tau with mu + mut, conductivity
    k + mut cp(T_face) / Prt,
  * the accumulation into the residual with the signs of procBlock.cpp:1392-1430 (subtracted
    from the cell below the face, added to the cell above),
  * the viscous part of the spectral radius (ViscCellSpectralRadius spectralRadius.hpp:94-123)
    times viscousCFLCoefficient.  CalcViscFluxI/J/K call it for cell ii at face ii, inside
    `if (ii < PhysEnd - 1)` next to AddToResidual(ii) (:1427-1465): the face is the cell's
    LOWER face of the direction, whatever the comment there says, and so it is here,
  * eddyViscosity_ of a cell, one sixth of the mut of its six faces (:1401-1402, :1436-1437).

It is fed with downloaded fields only (wall_ref.download_fields, ghost cells included,
[k, j, i, c]).  With cw = 0 it is the laminar viscous operator.
"""
import numpy as np

from wall_ref import EPS, GasRef, download_fields, lagrange_coeff   # noqa: F401

CW = 0.544             # turbWale::cw_ turbulence.hpp:664
PRT = 0.9              # turbModel::TurbPrandtlNumber turbulence.hpp:70


def wale_gradient_term(G):
    """a^1.5 / (b^2.5 + a^1.25 + EPS) of turbWale::EddyVisc for velocity gradients
    G[..., 3, 3]: S = (G + G^T) / 2, Sd = (G G + (G G)^T) / 2 - tr(G G) I / 3, a = Sd : Sd,
    b = S : S (DoubleDotTrans: the elementwise product summed, tensor.hpp:180-184, :353-356)"""
    G = np.asarray(G, dtype=np.float64)
    GT = np.swapaxes(G, -1, -2)
    S = 0.5 * (G + GT)
    G2 = G @ G                                            # MatMult
    Sd = 0.5 * (G2 + np.swapaxes(G2, -1, -2)) - \
        (1.0 / 3.0) * np.trace(G2, axis1=-2, axis2=-1)[..., None, None] * np.eye(3)
    a = (Sd * Sd).sum((-1, -2))
    b = (S * S).sum((-1, -2))
    return np.power(a, 1.5) / (np.power(b, 2.5) + np.power(a, 1.25) + EPS)


def wale_mut(G, length, cw=CW):
    return np.power(cw * length, 2.0) * wale_gradient_term(G)


def gamma_prandtl(gas, t):
    """thermodynamic::Gamma and Prandtl = 4 gamma / (9 gamma - 5) (thermodynamic.hpp:55-64)"""
    cp = gas.cp(t)
    gamma = cp / (cp - gas.R)
    return gamma, 4.0 * gamma / (9.0 * gamma - 5.0)


def faces(fields, gas, n, ng, d, fourth=False, cw=CW):
    """All lower d-faces of the cells 0 .. n[d] (the last one is the upper face of the last
    cell) over the physical range of the other two directions.  Arrays [i, j, k, ...] over the
    faces: "mut" (unscaled), "mu" (unscaled laminar), "flux" [..., 5] = CalcFlux times |A|,
    "velGrad" [..., r, c] = d u_c / d x_r, "tempGrad", "state" [..., 5], "t_face"."""
    g = gas
    others = [t for t in range(3) if t != d]
    A = {name: np.transpose(arr, (2, 1, 0, 3)) for name, arr in fields.items()}
    cnt = list(n)
    cnt[d] += 1
    idx = np.meshgrid(*[np.arange(c) for c in cnt], indexing="ij")
    e = np.eye(3, dtype=int)

    def at(name, off):          # cell or lower-face index (U + off)
        return A[name][idx[0] + ng + off[0], idx[1] + ng + off[1], idx[2] + ng + off[2]]

    def area(t, off):           # area vector of the lower t-face of cell U + off
        a = at("farea_" + "ijk"[t], off)
        return a[..., :3] * a[..., 3:4]

    U, L = np.zeros(3, int), -e[d]
    a_up, a_lo = [None] * 3, [None] * 3
    a_up[d] = 0.5 * (area(d, U) + area(d, U + e[d]))
    a_lo[d] = 0.5 * (area(d, U) + area(d, U - e[d]))
    for t in others:
        a_up[t] = 0.5 * (area(t, U + e[t]) + area(t, L + e[t]))
        a_lo[t] = 0.5 * (area(t, U) + area(t, L))
    vol = 0.5 * (at("volume", L) + at("volume", U))          # [..., 1]

    def gg(phi):
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

    G = gg(lambda off: at("state", off)[..., 1:4])                      # [..., r, c]
    gT = gg(lambda off: at("temperature", off))[..., 0]                 # [..., r]

    wname = "width_" + "ijk"[d]
    if fourth:
        offs = [L - e[d], L, U, U + e[d]]
        w = [at(wname, o) for o in offs]
        c = lagrange_coeff(w, 3, 1, 1)
        sf = sum(c[m] * at("state", offs[m]) for m in range(4))
        mu = sum(c[m] * at("viscosity", offs[m]) for m in range(4))[..., 0]
    else:
        c2 = lagrange_coeff([at(wname, L), at(wname, U)], 1, 0, 0)
        sf = c2[0] * at("state", U) + c2[1] * at("state", L)
        mu = (c2[0] * at("viscosity", U) + c2[1] * at("viscosity", L))[..., 0]
    t_f = sf[..., 4] / (sf[..., 0] * g.R)

    length = 0.5 * (at(wname, L) + at(wname, U))[..., 0]
    mut = wale_mut(G, length, cw) if cw else np.zeros_like(mu)

    fa = at("farea_" + "ijk"[d], U)
    nrm, mag = fa[..., :3], fa[..., 3]
    mu_s, mut_s = g.scaling * mu, g.scaling * mut
    lam = -(2.0 / 3.0) * (mu_s + mut_s)
    trace = G[..., 0, 0] + G[..., 1, 1] + G[..., 2, 2]
    sym = G + np.swapaxes(G, -1, -2)
    tau = lam[..., None] * trace[..., None] * nrm + \
        (mu_s + mut_s)[..., None] * np.einsum("...rc,...c->...r", sym, nrm)
    k = g.conductivity(t_f) * g.scaling
    kt = mut_s * g.cp(t_f) / PRT
    qn = (k + kt) * np.einsum("...r,...r->...", gT, nrm)
    flux = np.zeros(mu.shape + (5,))
    flux[..., 1:4] = tau
    flux[..., 4] = (tau * sf[..., 1:4]).sum(-1) + qn
    flux *= mag[..., None]
    return dict(mut=mut, mu=mu, flux=flux, velGrad=G, tempGrad=gT, state=sf, t_face=t_f,
                tau=tau, qn=qn, normal=nrm)


def _lower(a, d, n):      # the faces that are the lower d-face of cells 0 .. n[d]-1
    sl = [slice(None)] * a.ndim
    sl[d] = slice(0, n[d])
    return a[tuple(sl)]


def _upper(a, d, n):
    sl = [slice(None)] * a.ndim
    sl[d] = slice(1, n[d] + 1)
    return a[tuple(sl)]


def operator(fields, gas, n, ng, fourth=False, cw=CW, visc_cfl_coeff=1.0):
    """What one residual adds for the viscous terms, physical cells, [k, j, i, ...]:
      "residual" [..., 5]  the viscous part of residual_ (mass: zero),
      "spec_radius"        the viscous part of specRadius_ (times visc_cfl_coeff),
      "eddy"               eddyViscosity_ (unscaled),
      "mut"                per direction the faces' mut [k, j, i] (n[d] + 1 along d),
      "mu_face"            per direction the faces' laminar viscosity, likewise."""
    g = gas
    A = {name: np.transpose(arr, (2, 1, 0, 3)) for name, arr in fields.items()}
    ni, nj, nk = n
    phys = (slice(ng, ng + ni), slice(ng, ng + nj), slice(ng, ng + nk))
    rho = A["state"][phys][..., 0]
    t_c = A["temperature"][phys][..., 0]
    mu_c = A["viscosity"][phys][..., 0]
    vol = A["volume"][phys][..., 0]
    gamma, prandtl = gamma_prandtl(g, t_c)
    max_term = np.maximum(4.0 / (3.0 * rho), gamma / rho)
    res = np.zeros((ni, nj, nk, 5))
    sr = np.zeros((ni, nj, nk))
    eddy = np.zeros((ni, nj, nk))
    muts, mus = [], []
    for d in range(3):
        f = faces(fields, g, n, ng, d, fourth=fourth, cw=cw)
        # the cell above a face (its lower face): AddToResidual; the cell below:
        # SubtractFromResidual
        res += _lower(f["flux"], d, n)
        res -= _upper(f["flux"], d, n)
        eddy += (1.0 / 6.0) * _lower(f["mut"], d, n)
        eddy += (1.0 / 6.0) * _upper(f["mut"], d, n)
        name = "farea_" + "ijk"[d]
        sl_lo = list(phys)
        sl_up = list(phys)
        sl_up[d] = slice(ng + 1, ng + n[d] + 1)
        fmag = 0.5 * (A[name][tuple(sl_lo)][..., 3] + A[name][tuple(sl_up)][..., 3])
        visc_term = g.scaling * (mu_c / prandtl + _lower(f["mut"], d, n) / PRT)
        sr += visc_cfl_coeff * max_term * visc_term * fmag * fmag / vol
        muts.append(np.transpose(f["mut"], (2, 1, 0)))
        mus.append(np.transpose(f["mu"], (2, 1, 0)))
    tr = lambda a: np.swapaxes(a, 0, 2)
    return dict(residual=tr(res), spec_radius=tr(sr), eddy=tr(eddy), mut=muts, mu_face=mus)


def increment(fields, gas, n, ng, fourth=False, visc_cfl_coeff=1.0):
    """(les, laminar, les - laminar) of operator(): the last is what the WALE model adds"""
    les = operator(fields, gas, n, ng, fourth, CW, visc_cfl_coeff)
    lam = operator(fields, gas, n, ng, fourth, 0.0, visc_cfl_coeff)
    inc = {k: les[k] - lam[k] for k in ("residual", "spec_radius", "eddy")}
    return les, lam, inc


def residual_once(sol, cfl=None, mm=0):
    """One residual of a Solver through the phases (boundary cells, local halo swap, edges,
    agx_phase_residual), nothing updated: the state the residual saw stays on the device"""
    from aither_amd import abi
    api, ctx = sol.api, sol.ctx
    cfl = sol.case.deck.cfl(0) if cfl is None else cfl
    sol.store_time_n(0)
    api.check(api.phase_bc_faces(ctx), "phase_bc_faces")
    api.check(api.halo_swap_local(ctx, abi.HALO_STATE), "halo_swap_local")
    api.check(api.phase_bc_edges(ctx), "phase_bc_edges")
    api.check(api.phase_residual(ctx, mm, cfl), "phase_residual")
    return cfl
