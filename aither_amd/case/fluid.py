"""Fluid database and nondimensionalisation (setup-time, host side).

Restates, for a single species (calorically or thermally perfect), what the reference
does in fluid.cpp:83-97 (Nondimensionalize), input.cpp:593-613 (reference speed
of sound) and inputStates.cpp:464-473 (IC / BC state nondimensionalisation).
The arithmetic order of the reference is kept so that the nondimensional
constants agree with it to the last bit.

The numpy functions at the end restate the thermally perfect gas
(thermodynamic.hpp:125-189) for tests and outputs; the solver's own are the
device functions of agx_device.hpp.
"""
from dataclasses import dataclass, field
import math
from typing import List

import numpy as np

UNIVERSAL_GAS_CONST = 8.3144598  # J / mol-K, include/fluid.hpp:44

# Data of the reference's fluidDatabase/*.dat files (NIST values): n, molar
# mass [g/mol], Sutherland viscosity C1/S, Sutherland conductivity C1/S,
# heat of formation [J/mol], vibrational temperatures [K].
FLUID_DATABASE = {
    "air": dict(n=2.5, molar_mass=28.97, visc_c1=1.458e-6, visc_s=110.4,
                cond_c1=2.495e-3, cond_s=194.0, heat_of_formation=0.0,
                vibrational_temperature=[3056.0]),
    "N2": dict(n=2.5, molar_mass=28.0134, visc_c1=1.4742e-06, visc_s=1.2846e+02,
               cond_c1=2.6834e-03, cond_s=2.5615e+02, heat_of_formation=0.0,
               vibrational_temperature=[3392.0]),
}


@dataclass
class Gas:
    """Nondimensional gas model handed to the solver (agx_gas)."""
    gas_constant: float
    n: float
    heat_of_formation: float
    visc_c1: float
    visc_s: float
    cond_c1: float
    cond_s: float
    t_ref: float
    rho_ref: float
    l_ref: float
    a_ref: float
    # thermodynamicModel (input.cpp:795-803) and, thermally perfect, the vibrational
    # temperatures / t_ref (fluid.cpp:92)
    thermodynamic_model: str = "caloricallyPerfect"
    theta_v: List[float] = field(default_factory=list)

    @property
    def gamma(self):
        """The calorically perfect (frozen) ratio of specific heats."""
        r = self.gas_constant
        return (r * (self.n + 1.0)) / (r * self.n)

    @property
    def n_vib(self):
        return len(self.theta_v)


def make_gas(name, t_ref, rho_ref, l_ref=1.0, thermodynamic_model="caloricallyPerfect"):
    db = FLUID_DATABASE[name]
    n = db["n"]
    molar_mass = db["molar_mass"] / 1000.0          # fluid.cpp:133 (kg/mol)
    r_dim = UNIVERSAL_GAS_CONST / molar_mass         # fluid::GasConstant
    # input.cpp:608-613: aRef_ += mixRef * gamma * R * tRef; aRef_ = sqrt(aRef_)
    gamma = (n + 1) / n
    a_ref = 0.0
    a_ref += 1.0 * gamma * r_dim * t_ref
    a_ref = math.sqrt(a_ref)
    # fluid.cpp:83-97
    hf = db["heat_of_formation"]
    hf /= molar_mass * (a_ref * a_ref)
    molar_mass_nd = molar_mass / (rho_ref / math.pow(l_ref, 3.0))
    ugc_nd = UNIVERSAL_GAS_CONST / (a_ref * a_ref * rho_ref /
                                    (t_ref * math.pow(l_ref, 3.0)))
    r_nd = ugc_nd / molar_mass_nd
    # (a_ref stays the calorically perfect one for either model, input.cpp:608-613)
    theta_v = ([v / t_ref for v in db["vibrational_temperature"]]
               if thermodynamic_model == "thermallyPerfect" else [])
    return Gas(gas_constant=r_nd, n=n, heat_of_formation=hf,
               visc_c1=db["visc_c1"], visc_s=db["visc_s"],
               cond_c1=db["cond_c1"], cond_s=db["cond_s"],
               t_ref=t_ref, rho_ref=rho_ref, l_ref=l_ref, a_ref=a_ref,
               thermodynamic_model=thermodynamic_model, theta_v=theta_v)


# ---- thermally perfect gas, numpy (thermodynamic.hpp:125-189) -------------------------
# With x = theta / T and em = exp(-x):
#   e(T)  = hf + n R T + R sum theta em / (1 - em)
#   cv(T) = n R + R sum x^2 em / (1 - em)^2      (= (t / sinh t)^2, t = x / 2)
# A calorically perfect gas (no theta_v) gives the constants n R, (n + 1) R.
def _vib(gas, t):
    t = np.asarray(t, dtype=np.float64)
    ev = np.zeros_like(t)
    cvv = np.zeros_like(t)
    for th in gas.theta_v:
        x = th / t
        em = np.exp(-x)
        om = -np.expm1(-x)
        r = em / om
        ev = ev + th * r
        cvv = cvv + x * x * r / om
    return ev, cvv


def cv(gas, t):
    return gas.gas_constant * (gas.n + _vib(gas, t)[1])


def cp(gas, t):
    return cv(gas, t) + gas.gas_constant


def gamma(gas, t):
    c = cv(gas, t)
    return (c + gas.gas_constant) / c


def spec_energy(gas, t):
    t = np.asarray(t, dtype=np.float64)
    r = gas.gas_constant
    return gas.heat_of_formation + gas.n * r * t + r * _vib(gas, t)[0]


def spec_enthalpy(gas, t):
    return spec_energy(gas, t) + gas.gas_constant * np.asarray(t, dtype=np.float64)


def temperature_from_energy(gas, e, max_iter=50):
    """T with spec_energy(T) = e: Newton's method from the frozen guess (e - hf) / (n R),
    from which the iterates fall monotonically onto the root (e is increasing and convex)."""
    e = np.asarray(e, dtype=np.float64)
    r = gas.gas_constant
    t = (e - gas.heat_of_formation) / (gas.n * r)
    if np.any(~(t > 0.0)):
        raise ValueError("energy below the heat of formation")
    for _ in range(max_iter):
        ev, cvv = _vib(gas, t)
        dt = (gas.heat_of_formation + gas.n * r * t + r * ev - e) / (r * (gas.n + cvv))
        t = t - dt
        if np.all(np.abs(dt) <= 1e-14 * t):
            return t
    raise RuntimeError("temperature_from_energy: no convergence")
