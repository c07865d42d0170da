"""The wall variables of the reference's wall function file, restated in numpy.

An independent statement of what WriteWallFun (output.cpp:472-571) writes for a low-Re
viscousWall surface: the face gradients of CalcGradsI/J/K (procBlock.cpp:5173-5788, Green-Gauss
on the alternate control volume, VectorGradGG / ScalarGradGG utility.cpp:59-188), the face
state of FaceReconCentral / FaceReconCentral4th (reconstruction.hpp:315-350 with LagrangeCoeff,
utility.cpp:449-483), the wallVars of viscousFlux::CalcWallFlux (viscousFlux.cpp:137-211) with
y+ of procBlock.cpp:1372-1375, and the factors of output.cpp:519-553.  Vectorised over a
surface and written once for all six sides: the wall-normal direction d and the two others
are picked by index.

It is fed with downloaded fields only (Solver.download, ghost cells included, [k, j, i, c]):
state, temperature, viscosity, volume, farea_i/j/k, width_i/j/k, wall_dist.
"""
import numpy as np

EPS = 1.0e-30          # macros.hpp.in:20
TURB_MIN = 1.0e-20     # primitive::LimitTurb
FIELDS = ("state", "temperature", "viscosity", "volume", "farea_i", "farea_j", "farea_k",
          "width_i", "width_j", "width_k", "wall_dist")
GRAD_NAMES = ("shearStress", "shearStress_x", "shearStress_y", "shearStress_z", "heatFlux",
              "frictionVelocity", "yplus")
STATE_NAMES = ("density", "pressure", "temperature", "viscosity")


def download_fields(sol, gb, host_geometry=False):
    """host_geometry: the geometry arrays of the case as uploaded (the CPU oracle hands out
    the solution fields only)"""
    if not host_geometry:
        return {f: sol.download(f, gb) for f in FIELDS}
    out = {f: sol.download(f, gb) for f in ("state", "temperature", "viscosity")}
    g = sol.case.blocks[gb].geom
    out["volume"], out["wall_dist"] = g.vol.a, g.wall_dist.a
    for d in "ijk":
        out["farea_" + d], out["width_" + d] = g.farea[d].a, g.width[d].a
    return {f: np.asarray(a).reshape(a.shape if a.ndim == 4 else a.shape + (1,))
            for f, a in out.items()}


class GasRef:
    """transport / thermodynamic constants from the nondimensional gas of a case
    (sutherland transport.cpp:58-68, :114-132; transport.hpp:42-43)."""

    def __init__(self, gas, turb_prandtl=0.9):
        self.R, self.n = gas.gas_constant, gas.n
        self.t_ref, self.rho_ref, self.l_ref, self.a_ref = gas.t_ref, gas.rho_ref, gas.l_ref, gas.a_ref
        self.cond_c1, self.cond_s = gas.cond_c1, gas.cond_s
        self.mu_ref = gas.visc_c1 * gas.t_ref ** 1.5 / (gas.t_ref + gas.visc_s)
        self.k_nondim = gas.a_ref * gas.a_ref * self.mu_ref / gas.t_ref
        self.scaling = self.mu_ref / (gas.rho_ref * gas.a_ref * gas.l_ref)
        self.theta_v = list(getattr(gas, "theta_v", []))
        self.turb_prandtl = turb_prandtl

    def conductivity(self, t):
        temp = t * self.t_ref
        return self.cond_c1 * temp ** 1.5 / (temp + self.cond_s) / self.k_nondim

    def cp(self, t):
        """caloricallyPerfect (thermodynamic.hpp:108-113): (n + 1) R; thermallyPerfect
        (:125-189): plus R sum (theta / T)^2 e^(theta / T) / (e^(theta / T) - 1)^2"""
        cv = self.n * np.ones_like(t)
        for th in self.theta_v:
            x = th / t
            ex = np.exp(x)
            cv = cv + x * x * ex / (ex - 1.0) ** 2
        return self.R * (cv + 1.0)


def lagrange_coeff(w, degree, rr, ii):
    """LagrangeCoeff (utility.cpp:449-483); w: list of width arrays."""
    def sw(start, end):                                  # StencilWidth utility.hpp:104-114
        if end > start:
            return sum(w[start:end])
        if start > end:
            return -1.0 * sum(w[end:start])
        return 0.0
    coeffs = []
    for jj in range(degree + 1):
        c = 0.0
        for mm in range(jj + 1, degree + 2):
            numer, denom = 0.0, 1.0
            for ll in range(degree + 2):
                if ll == mm:
                    continue
                prod = 1.0
                for qq in range(degree + 2):
                    if qq != mm and qq != ll:
                        prod = prod * sw(ii - rr + qq, ii + 1)
                numer = numer + prod
                denom = denom * sw(ii - rr + ll, ii - rr + mm)
            c = c + numer / denom
        coeffs.append(c * w[ii - rr + jj])
    return coeffs


def surface_of(side, rng):
    """dict like Solver.wall_surfaces' entries from a side and (imin, imax, jmin, jmax, kmin, kmax)"""
    d = (side - 1) // 2
    n = [rng[1] - rng[0], rng[3] - rng[2], rng[5] - rng[4]]
    n[d] = 1
    return dict(side=side, range=tuple(rng), shape=(n[2], n[1], n[0]))


def wall_vars(fields, surf, gas, ng, fourth=False, mut_ratio=None, turbulent=False):
    """The wall variables of one low-Re surface: {name: array (nk, nj, ni) of its range},
    dimensional; also "velGrad" [..., r, c] = d u_c / d x_r, "tempGrad" [..., r] and the
    nondimensional "mu", "tau" for the tests of the restatement itself.
    mut_ratio: turbEddyVisc_ / (viscosity_ + EPS) per face (the eddy viscosity is not restated:
    it is taken from the payload), or None for laminar."""
    g = gas
    side, rng = surf["side"], surf["range"]
    d = (side - 1) // 2
    others = [t for t in range(3) if t != d]
    # [k, j, i, c] -> [i, j, k, c]
    A = {name: np.transpose(arr, (2, 1, 0, 3)) for name, arr in fields.items()}
    lo = [rng[0], rng[2], rng[4]]
    n = [rng[1] - rng[0], rng[3] - rng[2], rng[5] - rng[4]]
    n[d] = 1
    idx = np.meshgrid(*[lo[q] + np.arange(n[q]) for q in range(3)], indexing="ij")
    e = np.eye(3, dtype=int)

    def at(name, off):          # cell or lower-face index (U + off)
        return A[name][idx[0] + ng + off[0], idx[1] + ng + off[1], idx[2] + ng + off[2]]

    def area(t, off):           # area vector of the lower t-face of cell U + off
        a = at("farea_" + "ijk"[t], off)
        return a[..., :3] * a[..., 3:4]

    U, L = np.zeros(3, int), -e[d]
    # areas and volume of the alternate control volume
    a_up, a_lo = [None] * 3, [None] * 3
    a_up[d] = 0.5 * (area(d, U) + area(d, U + e[d]))
    a_lo[d] = 0.5 * (area(d, U) + area(d, U - e[d]))
    for t in others:
        a_up[t] = 0.5 * (area(t, U + e[t]) + area(t, L + e[t]))
        a_lo[t] = 0.5 * (area(t, U) + area(t, L))
    vol = 0.5 * (at("volume", L) + at("volume", U))          # [..., 1]

    def gg(phi):
        """Green-Gauss gradient of the cell field phi(off) -> [..., ncomp]: [..., r, c]"""
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

    # face state and viscosity
    wname = "width_" + "ijk"[d]
    if fourth:
        offs = [L - e[d], L, U, U + e[d]]
        w = [at(wname, o) for o in offs]
        c = lagrange_coeff(w, 3, 1, 1)
        sf = sum(c[m] * at("state", offs[m]) for m in range(4))
        mu = sum(c[m] * at("viscosity", offs[m]) for m in range(4))[..., 0]
    c2 = lagrange_coeff([at(wname, L), at(wname, U)], 1, 0, 0)
    central = c2[0] * at("state", U) + c2[1] * at("state", L)
    if not fourth:
        sf = central
        mu = (c2[0] * at("viscosity", U) + c2[1] * at("viscosity", L))[..., 0]
    rho, p = sf[..., 0], sf[..., 4]
    t_f = p / (rho * g.R)
    tke = sdr = np.zeros_like(rho)
    if turbulent:      # (4th order: turbulence variables by the central rule) then LimitTurb
        tke = np.maximum(central[..., 5], TURB_MIN)
        sdr = np.maximum(central[..., 6], TURB_MIN)

    nrm = at("farea_" + "ijk"[d], U)[..., :3]
    mu_s = g.scaling * mu
    mut_s = np.zeros_like(mu_s) if mut_ratio is None else \
        np.transpose(mut_ratio, (2, 1, 0)) * (mu_s + EPS)
    lam = -(2.0 / 3.0) * (mu_s + mut_s)
    trace = G[..., 0, 0] + G[..., 1, 1] + G[..., 2, 2]
    sym = G + np.swapaxes(G, -1, -2)
    tau = lam[..., None] * trace[..., None] * nrm + \
        (mu_s + mut_s)[..., None] * np.einsum("...rc,...c->...r", sym, nrm)
    k = g.conductivity(t_f) * g.scaling
    kt = mut_s * g.cp(t_f) / g.turb_prandtl
    q = (k + kt) * np.einsum("...r,...r->...", gT, nrm)
    tmag = np.sqrt((tau ** 2).sum(-1))
    utau = np.sqrt(tmag / rho)
    y = at("wall_dist", U if side % 2 == 1 else L)[..., 0]
    yplus = y * utau * rho / (mu_s + mut_s)

    rR, aR, lR, tR, muR = g.rho_ref, g.a_ref, g.l_ref, g.t_ref, g.mu_ref
    tau_sc = (1.0 / g.scaling) * muR * aR / lR
    out = {
        "yplus": yplus,
        "shearStress": tmag * tau_sc,
        "viscosityRatio": mut_s / (mu_s + EPS),
        "heatFlux": q * muR * tR / lR,
        "frictionVelocity": utau * aR,
        "density": rho * rR,
        "pressure": rho * g.R * t_f * rR * aR * aR,
        "temperature": t_f * tR,
        "viscosity": mu_s * muR * (1.0 / g.scaling),
        "tke": tke * aR * aR,
        "sdr": sdr * aR * aR * rR / muR,
        "shearStress_x": tau[..., 0] * tau_sc,
        "shearStress_y": tau[..., 1] * tau_sc,
        "shearStress_z": tau[..., 2] * tau_sc,
        "velGrad": G, "tempGrad": gT, "mu": mu_s, "tau": tau, "normal": nrm,
    }
    # [i, j, k, ...] -> [k, j, i, ...]
    return {name: np.swapaxes(v, 0, 2) for name, v in out.items()}


def compare(got, ref, names=None, log=print):
    """Every face of every surface: |got - ref| <= tol * largest |ref| of the variable over
    the block's surfaces; tolerances of tests/test_output_pack.py:100-103 (1e-10 for what is
    formed from the state alone, 1e-8 for what is formed from gradients).  got / ref:
    {name: [array per surface]}.  Prints each figure before it asserts."""
    names = names or (STATE_NAMES + GRAD_NAMES)
    worst = {}
    for name in names:
        tol = 1e-10 if name in STATE_NAMES else 1e-8
        scale = max(np.abs(r).max() for r in ref[name])
        if name.startswith("shearStress_"):        # components: the vector's size
            scale = max(np.abs(r).max() for r in ref["shearStress"])
        err = max(np.abs(a - r).max() for a, r in zip(got[name], ref[name]))
        for a, r in zip(got[name], ref[name]):
            assert a.shape == r.shape, (name, a.shape, r.shape)
        worst[name] = err / scale if scale > 0.0 else err
        log(f"wall_pack {name}: max |diff| / scale = {worst[name]:.3e} (tol {tol:g})")
    for name in names:
        tol = 1e-10 if name in STATE_NAMES else 1e-8
        assert worst[name] <= tol, (name, worst[name])
    return worst
