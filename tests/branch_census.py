"""Which side of each flow-dependent branch does a state select?  A numpy restatement of the
predicates of ausm_flux, roe_flux, muscl / limiter, ghost_state and extrap_hold
(aither_amd/csrc/agx_device.hpp; oracle/oracle.c states the same ones), counted per face.

Test infrastructure: it never calls the HIP library and reads no kernel.  It reads the state
array (ghost cells included) that Solver.download gives for the ORACLE, and the case the
oracle was built from: the unit face normals and cell widths of its host geometry
(blk.geom.farea / width -- the arrays the Solver uploads; the oracle serves no geometry
download), the gas and the nondimensional boundary states (builder.surface_structs).  The
temperature of a thermally perfect gas is p / (rho R) of the state itself.

The flux predicates use FIRST-ORDER left and right states, i.e. the two cells of a face.  A
reconstructed state differs from its cell by a fraction of the cell-to-cell difference, so a
face that is tens of percent away from a threshold is on the same side for either; the
counts asked of a case (>= 8 faces) are far from the handful of faces next to a threshold
that could differ.  Only faces between two physical cells of one block are counted.  The
limiter predicates use the three-cell stencils that lie wholly in physical cells.

Keys (d = i, j, k; a key prefixed "!" counts the other side):
    ausm:d:vel<0  vel>0  vnL>cS  vnR>cS  ml>1  ml<-1  mr>1  mr<-1  mavg<0
        (vnL>cS, vnR>cS: the plain predicates.  ausm:d:vel<0&vnR>cS -- the one combination in
        which fmax(vnR, cS) of the vel < 0 arm returns vnR -- needs vnL < -cS beside
        vnR > cS, two supersonic streams colliding in neighbouring cells; it is counted
        but no smooth field selects it.)
    roe:d:|vn-a|<0.1  |vn+a|<0.1  vn<0
    muscl:vanAlbada:lim=0  den*sq<=0        muscl:minmod:clip0  clip1
    bc:S:characteristic:supIn  subIn  supOut  subOut          (S = surface type 1..6)
    bc:S:inlet:sup  sub
    bc:S:pressureOutlet:fallback  regular
    bc:S:extrap:held  extrapolated     (first call of extrap_hold, factor 2)
    bc:S:extrap:held_deep              (second call, factor = layer >= 2, per face and layer)
margins[key]: smallest relative distance of any face to the threshold of the DISCONTINUOUS
predicates (mach = 1, vn = 0, the outlet's fallback ratio = 1, 2 rho_b - rho_i = 0).
"""
import numpy as np

from aither_amd.case import builder, fluid

EPS = 1.0e-30
AUSM = ("vel<0", "vel>0", "vnL>cS", "vnR>cS", "ml>1", "ml<-1", "mr>1", "mr<-1", "mavg<0")
ROE = ("|vn-a|<0.1", "|vn+a|<0.1", "vn<0")
CHARACTERISTIC = ("supIn", "subIn", "supOut", "subOut")


def _sos(gas, s):
    return np.sqrt(fluid.gamma(gas, s[..., 4] / (s[..., 0] * gas.gas_constant)) *
                   s[..., 4] / s[..., 0])


def _add(out, key, mask):
    out[key] = out.get(key, 0) + int(np.count_nonzero(mask))
    out["!" + key] = out.get("!" + key, 0) + int(np.count_nonzero(~mask))


def _add2(out, key, other, mask):
    out[key] = out.get(key, 0) + int(np.count_nonzero(mask))
    out[other] = out.get(other, 0) + int(np.count_nonzero(~mask))


def _margin(margins, key, dist):
    if dist.size:
        margins[key] = min(margins.get(key, np.inf), float(np.abs(dist).min()))


def _faces(blk, state, d):
    """(left cells, right cells, unit normals) of the faces between physical cells along d"""
    g = blk.geom.ng
    inner = (slice(g, -g),) * 3
    s = np.moveaxis(state[inner], 2 - d, 0)
    a = np.moveaxis(blk.geom.farea["ijk"[d]].a[inner], 2 - d, 0)     # faces 0 .. n
    return s[:-1], s[1:], a[1:-1, ..., :3]


def ausm(gas, l, r, n, out, d):
    vnl, vnr = (l[..., 1:4] * n).sum(-1), (r[..., 1:4] * n).sum(-1)
    cs = np.sqrt(_sos(gas, l) * _sos(gas, r))
    vel = 0.5 * (vnl + vnr)
    c = np.where(vel < 0.0, cs * cs / np.maximum(vnr, cs),
                 np.where(vel > 0.0, cs * cs / np.maximum(vnl, cs), cs))
    ml, mr = vnl / c, vnr / c
    mpl = np.where(np.abs(ml) <= 1.0, 0.25 * (ml + 1.0) ** 2, 0.5 * (ml + np.abs(ml)))
    mmr = np.where(np.abs(mr) <= 1.0, -0.25 * (mr - 1.0) ** 2, 0.5 * (mr - np.abs(mr)))
    pre = f"ausm:{'ijk'[d]}:"
    for name, mask in zip(AUSM, (vel < 0.0, vel > 0.0, vnl > cs, vnr > cs, ml > 1.0, ml < -1.0,
                                 mr > 1.0, mr < -1.0, mpl + mmr < 0.0)):
        _add(out, pre + name, mask)
    _add(out, pre + "vel<0&vnR>cS", (vel < 0.0) & (vnr > cs))


def roe(gas, l, r, n, out, d):
    dr = np.sqrt(r[..., 0] / l[..., 0])
    avg = (l + dr[..., None] * r) / (1.0 + dr[..., None])
    avg[..., 0] = l[..., 0] * dr
    a = _sos(gas, avg)
    vn = (avg[..., 1:4] * n).sum(-1)
    pre = f"roe:{'ijk'[d]}:"
    for name, mask in zip(ROE, (np.abs(vn - a) < 0.1, np.abs(vn + a) < 0.1, vn < 0.0)):
        _add(out, pre + name, mask)


def muscl(blk, state, limiter, out):
    g = blk.geom.ng
    inner = (slice(g, -g),) * 3
    for d in range(3):
        s = np.moveaxis(state[inner][..., :5], 2 - d, 0)
        w = np.moveaxis(blk.geom.width["ijk"[d]].a[inner], 2 - d, 0)
        for uw2, uw1, dw1 in ((slice(0, -2), slice(1, -1), slice(2, None)),     # left states
                              (slice(2, None), slice(1, -1), slice(0, -2))):    # right states
            d_plus = 2.0 * w[uw1] / (w[uw1] + w[dw1])
            d_minus = 2.0 * w[uw1] / (w[uw1] + w[uw2])
            num = EPS + (s[dw1] - s[uw1]) * d_plus
            den = EPS + (s[uw1] - s[uw2]) * d_minus
            if limiter == "vanAlbada":
                sq = (num + den) / (num * num + den * den)
                _add(out, "muscl:vanAlbada:lim=0", num * sq < 0.0)
                _add(out, "muscl:vanAlbada:den*sq<=0", den * sq <= 0.0)
            elif limiter == "minmod":
                r = num / den
                _add(out, "muscl:minmod:clip0", r < 0.0)
                _add(out, "muscl:minmod:clip1", r > 1.0)


def _extrap(out, margins, pre, gh_rho, in_rho, ng):
    """extrap_hold of ghost_state: factor 2 on the boundary state, then factor = layer on the
    result for the deeper layers"""
    first = 2.0 * gh_rho - in_rho
    held = first <= 0.0
    _add2(out, pre + "extrap:held", pre + "extrap:extrapolated", held)
    _margin(margins, pre + "extrap", first / in_rho)
    rho1 = np.where(held, gh_rho, first)
    for layer in range(2, ng + 1):
        deep = layer * rho1 - in_rho
        out[pre + "extrap:held_deep"] = out.get(pre + "extrap:held_deep", 0) + \
            int(np.count_nonzero(deep <= 0.0))
        _margin(margins, pre + "extrap", deep / in_rho)


def boundary(case, gb, state, out, margins):
    blk, gas = case.blocks[gb], case.gas
    g = blk.geom.ng
    structs = builder.surface_structs(case, gb)
    for surf, st in zip(blk.surfaces, structs):
        if surf.bc_type not in ("characteristic", "inlet", "pressureOutlet"):
            continue
        if st.state.is_nonreflecting:
            continue                # (LODI forms: test_parity_gpu's nonreflecting decks)
        side = surf.surface_type()
        d, upper = (side - 1) // 2, side % 2 == 0
        lo = [surf.imin, surf.jmin, surf.kmin]
        hi = [surf.imax, surf.jmax, surf.kmax]
        cell = [slice(lo[q] + g, hi[q] + g) for q in range(3)]
        face = list(cell)
        cell[d] = lo[d] + g - 1 if upper else lo[d] + g        # the adjacent cell
        face[d] = lo[d] + g
        s = state[cell[2], cell[1], cell[0]]
        area = blk.geom.farea["ijk"[d]].a[face[2], face[1], face[0]]
        n = (1.0 if upper else -1.0) * area[..., :3]
        vn = (s[..., 1:4] * n).sum(-1)
        c = _sos(gas, s)
        mach = np.abs(vn) / c
        pre = f"bc:{side}:"
        d_ = st.state
        fs = np.array([d_.density, d_.velocity[0], d_.velocity[1], d_.velocity[2], d_.pressure])
        rc = s[..., 0] * c
        if surf.bc_type == "pressureOutlet":
            dp = s[..., 4] - fs[4]
            gh = s[..., :5].copy()
            gh[..., 0] = s[..., 0] - dp / (c * c)
            gh[..., 1:4] = s[..., 1:4] + n * (dp / rc)[..., None]
            gh[..., 4] = fs[4]
            out["bc:ghost_nonphysical"] = out.get("bc:ghost_nonphysical", 0) + \
                int(np.count_nonzero(~(gh[..., 0] > 0.0)))
            ratio = (gh[..., 1:4] * n).sum(-1) / _sos(gas, gh)
            _add2(out, pre + "pressureOutlet:fallback", pre + "pressureOutlet:regular",
                  ratio >= 1.0)
            _margin(margins, pre + "pressureOutlet", ratio - 1.0)
            continue
        # characteristic / inlet: the incoming-wave ghost (inflow, or any subsonic inlet face)
        vd = fs[1:4] - s[..., 1:4]
        p_in = 0.5 * (fs[4] + s[..., 4] - rc * (n * vd).sum(-1))
        rho_in = fs[0] - (fs[4] - p_in) / (c * c)
        rho_out = s[..., 0] - (s[..., 4] - fs[4]) / (c * c)
        sup, inflow = mach >= 1.0, vn < 0.0
        _margin(margins, pre + "mach", mach - 1.0)
        if surf.bc_type == "inlet":
            _add2(out, pre + "inlet:sup", pre + "inlet:sub", sup)
            bad = ~sup & ~((rho_in > 0.0) & (p_in > 0.0))
            out["bc:ghost_nonphysical"] = out.get("bc:ghost_nonphysical", 0) + \
                int(np.count_nonzero(bad))
            if np.any(~sup):        # (a supersonic inlet face is not extrapolated)
                _extrap(out, margins, pre, rho_in[~sup], s[..., 0][~sup], g)
            continue
        _margin(margins, pre + "vn", vn / c)
        for name, mask in zip(CHARACTERISTIC, (sup & inflow, ~sup & inflow, sup & ~inflow,
                                               ~sup & ~inflow)):
            key = pre + "characteristic:" + name
            out[key] = out.get(key, 0) + int(np.count_nonzero(mask))
        gh_rho = np.where(sup & inflow, fs[0], np.where(sup, s[..., 0],
                                                        np.where(inflow, rho_in, rho_out)))
        gh_p = np.where(sup & inflow, fs[4], np.where(sup, s[..., 4],
                                                      np.where(inflow, p_in, fs[4])))
        out["bc:ghost_nonphysical"] = out.get("bc:ghost_nonphysical", 0) + \
            int(np.count_nonzero(~((gh_rho > 0.0) & (gh_p > 0.0))))
        _extrap(out, margins, pre, gh_rho, s[..., 0], g)


def census(case, states):
    """states: {block: state array with ghosts} as downloaded from the oracle.
    Returns (counts, margins)."""
    out, margins = {}, {}
    deck = case.deck
    for gb, state in states.items():
        blk = case.blocks[gb]
        for d in range(3):
            l, r, n = _faces(blk, state, d)
            (ausm if deck.inviscid_flux == "ausm" else roe)(case.gas, l, r, n, out, d)
        if deck.using_muscl() and deck.limiter in ("vanAlbada", "minmod"):
            muscl(blk, state, deck.limiter, out)
        boundary(case, gb, state, out, margins)
    return out, margins
