"""ReadSolFromRestart (output.cpp:1177-1240) and ReadSolNm1FromRestart (:1242-1305) restated
in numpy from the reference's text: what agx_restart_unpack is held to, bit for bit.

A restart payload holds n_eq + 1 dimensional values per cell -- density, velocity, pressure,
[tke, sdr,] the mass fraction of the single species.  The reference divides each value it has
read (`value /= divisor`), with the divisor formed left to right as its expression stands,
and sets the density to (raw / rho_ref) * mf.  numpy's float64 division is IEEE, so this
module divides by the same divisors in the same order.
"""
import numpy as np


def mu_ref(gas):
    """transport::MuRef (transport.cpp:58-59): Sutherland's law at the reference temperature;
    gas: anything with visc_c1, visc_s, t_ref (agx_gas, case.fluid.Gas)."""
    return gas.visc_c1 * gas.t_ref ** 1.5 / (gas.t_ref + gas.visc_s)


def divisors(gas, which):
    """The seven divisors of which = 0 (primitive, :1197-1222) or 1 (conserved, :1262-1287);
    entry 0 is the density's rho_ref."""
    rR, aR, muR = gas.rho_ref, gas.a_ref, mu_ref(gas)
    if which == 0:
        return [rR, aR, aR, aR, rR * aR * aR, aR * aR, aR * aR * rR / muR]
    return [rR, aR * rR, aR * rR, aR * rR, rR * aR * aR, aR * aR * rR,
            aR * aR * rR * rR / muR]


def unpack(payload, gas, which=0):
    """payload[..., n_eq + 1] -> the nondimensional solution [..., n_eq]: the primitive state
    (which = 0) or the conserved consVarsNm1 (which = 1)."""
    payload = np.asarray(payload, dtype=np.float64)
    n_eq = payload.shape[-1] - 1
    div = divisors(gas, which)
    out = np.empty(payload.shape[:-1] + (n_eq,))
    out[..., 0] = payload[..., 0] / div[0] * payload[..., n_eq]
    for e in range(1, n_eq):
        out[..., e] = payload[..., e] / div[e]
    return out


def padded(phys, ng):
    """The physical cells [nk, nj, ni, n_eq] in the host layout of the state: zero ghost cells."""
    nk, nj, ni, n_eq = phys.shape
    out = np.zeros((nk + 2 * ng, nj + 2 * ng, ni + 2 * ng, n_eq))
    out[ng:ng + nk, ng:ng + nj, ng:ng + ni] = phys
    return out
