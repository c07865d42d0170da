"""A transonic, sign-changing initial state for the synthetic boxes (closed form, RNG-free).

synthetic.perturbed_state is a smooth +-5 % perturbation of one Mach-0.16 stream with three
positive velocity components: every flow-dependent branch of the flux functions, the limiters
and the ghost states takes one side only.  transonic_state writes a field whose velocity
along one grid axis runs through Mach 1 (0.65 .. 1.35 of the local speed of sound, either
sign) and whose transverse velocities change sign inside the block and on every face; the
case is built with the matching free stream (sign * c_inf along the axis, nothing across it)
so that every characteristic / inlet / supersonicInflow state belongs to the field.

tests/branch_census.py counts which side of each branch a field selects.
"""
import math

import numpy as np

from aither_amd.case import fluid, synthetic

CP, TP = "caloricallyPerfect", "thermallyPerfect"


def free_stream_speed(temperature_factor=1.0, model=CP):
    """Speed of sound [m/s] of the synthetic decks' free stream (make_deck: 1.225 kg/m3,
    temperature_factor x 101325 Pa; 340.3 m/s for the default deck), gamma of its temperature
    for a thermally perfect gas."""
    gas = fluid.make_gas("air", 288.15, 1.225, 1.0, model)
    p = 101325.0 * temperature_factor / (gas.rho_ref * gas.a_ref * gas.a_ref)
    t = p / gas.gas_constant
    return float(np.sqrt(fluid.gamma(gas, t) * p)) * gas.a_ref


def free_stream_velocity(axis, sign, temperature_factor=1.0, model=CP):
    vel = [0.0, 0.0, 0.0]
    vel["ijk".index(axis)] = sign * free_stream_speed(temperature_factor, model)
    return vel


def sound_speed(gas, rho, p):
    return np.sqrt(fluid.gamma(gas, p / (rho * gas.gas_constant)) * p / rho)


def transonic_state(case, axis, sign, swing=0.35, dp=0.08):
    """Physical cells of every block (ghost cells zeroed, as perturbed_state leaves them; the
    ghost layout and the base state rho0, p0, k, omega come from state[g, g, g]):
        rho = rho0 (1 + dp sin 2 pi x cos 2 pi y),  p = p0 (1 + dp cos 2 pi y sin(2 pi z + 0.3)),
        c = sqrt(gamma p / rho),
        velocity along `axis`:  sign c (1 + swing sin pi (x + y + z - 0.4)),
        across it:  0.3 c sin(pi (y + z - 0.9) + 2 pi x),  0.3 c sin(pi (z + x - 1.1) + 2 pi y)."""
    two_pi = 2.0 * math.pi
    d = "ijk".index(axis)
    for blk in case.blocks:
        cen = blk.geom.center.a
        x, y, z = cen[..., 0], cen[..., 1], cen[..., 2]
        g = blk.geom.ng
        base = blk.state[g, g, g, :].copy()
        new = np.empty(cen.shape[:3] + (base.size,))
        new[...] = base
        rho = base[0] * (1.0 + dp * np.sin(two_pi * x) * np.cos(two_pi * y))
        p = base[4] * (1.0 + dp * np.cos(two_pi * y) * np.sin(two_pi * z + 0.3))
        c = sound_speed(case.gas, rho, p)
        new[..., 0], new[..., 4] = rho, p
        new[..., 1 + d] = sign * c * (1.0 + swing * np.sin(math.pi * (x + y + z - 0.4)))
        new[..., 1 + (d + 1) % 3] = 0.3 * c * np.sin(math.pi * (y + z - 0.9) + two_pi * x)
        new[..., 1 + (d + 2) % 3] = 0.3 * c * np.sin(math.pi * (z + x - 1.1) + two_pi * y)
        ni, nj, nk = blk.geom.n
        blk.state[...] = 0.0
        blk.state[g:g + nk, g:g + nj, g:g + ni, :] = new[g:g + nk, g:g + nj, g:g + ni, :]


def density_ramp(case, surface, factor=2.6, cells=3):
    """Multiplies the density of the `cells` layers next to `surface` (1..6) of block 0 by a
    factor rising linearly to `factor` at the boundary: a boundary state of about the free
    stream's density then lies below half the interior one, which is what the hold arm of
    ExtrapolateHoldMixture (2 rho_boundary - rho_interior <= 0) needs."""
    blk = case.blocks[0]
    g = blk.geom.ng
    d, upper = (surface - 1) // 2, surface % 2 == 0
    n = blk.geom.n[d]
    for layer in range(cells):
        f = 1.0 + (factor - 1.0) * (cells - layer) / cells
        idx = [slice(g, -g)] * 3
        pos = g + (n - 1 - layer if upper else layer)
        idx[2 - d] = slice(pos, pos + 1)
        blk.state[tuple(idx) + (0,)] *= f


def transonic_case(axis, sign, kind="single", temperature_factor=1.0, ramp=None, **kw):
    """A synthetic box (kind: "single" | "stacked") with the transonic field and its free
    stream.  ramp: (surface, factor) of density_ramp."""
    model = kw.get("thermodynamic_model", CP)
    kw["velocity"] = free_stream_velocity(axis, sign, temperature_factor, model)
    if temperature_factor != 1.0:
        kw["temperature_factor"] = temperature_factor
    if kind == "stacked":       # stacked along the fast axis: the connection is transonic
        case = synthetic.stacked_blocks_case(axis=axis, amplitude=0.0, **kw)
    else:
        case = synthetic.single_block_case(amplitude=0.0, **kw)
    transonic_state(case, axis, sign)
    if ramp:
        density_ramp(case, *ramp)
    return case
