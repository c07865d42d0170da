"""The decks of the failure-protocol tests (tests/test_failure_protocol_gpu.py and the two-rank
cases of tests/test_distributed_gpu.py) and the numpy judge of the thermally perfect trigger.

| deck   | library  | case                                             | failure                     |
| kp     | 5-eq     | two k-stacked blocks, implicitEuler + LU-SGS     | k_lusgs_kp's spin limit     |
| pipe   | 7-eq     | the reference's wallLaw (two blocks, BLU-SGS)    | k_lusgs_pipe's spin limit   |
| tp     | 5-eq _tp | two k-stacked hot blocks, explicitEuler          | energy below the floor      |

The spin limit is raised by AGX_SPIN_LIMIT=1 at context creation (one poll is not always too
few: a bounded walk of at most WALK calls).  The energy failure is deterministic: at
TP_CFL_TRIGGER one explicit step takes cells below the heat of formation -- energy_margin says
so in numpy, from the CPU oracle's residual and time step, before any kernel is asked."""
import os

import numpy as np

import aither_amd
from aither_amd import abi
from aither_amd.case import fluid, synthetic
from aither_amd.case.builder import build_case
from aither_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK = 20                  # calls at most until the spin limit strikes (a guard)
SPIN_DIMS = (40, 36, 12)   # min(ni, nj) large enough for several diagonals in flight
TP_DIMS = (24, 20, 12)
TP_CFL, TP_CFL_TRIGGER = 0.3, 24.0
SPIN_MATCH = "spin limit"
ENERGY_MATCH = "specific energy"


def deck(name, ranks=None):
    """(library, case) of a deck; ranks=[0, 1] puts its two blocks on two ranks."""
    if name == "kp":
        return aither_amd.load(5), synthetic.stacked_blocks_case(
            SPIN_DIMS, nblocks=2, axis="k", stretch=1.1, ranks=ranks,
            time_integration="implicitEuler", matrix_solver="lusgs", cfl=5.0)
    if name == "pipe":
        inp = os.path.join(ROOT, "tests", "golden", "cases", "wallLaw", "wallLaw.inp")
        return aither_amd.load(7), build_case(inp, ranks=ranks)
    if name == "tp":
        import tp_cases
        return aither_amd.load(5, tp_cases.TP), tp_cases.hot_stacked(
            n=TP_DIMS, nblocks=2, axis="k", stretch=1.1, ranks=ranks,
            time_integration="explicitEuler", cfl=TP_CFL)
    raise KeyError(name)


def local_states(case, rank=0):
    return {gb: blk.state.copy() for gb, blk in enumerate(case.blocks) if blk.rank == rank}


def _cons(gas, s):
    """conserved variables of primitive states [..., rho u v w p] with the numpy gas model"""
    t = s[..., 4] / (s[..., 0] * gas.gas_constant)
    rho_e = s[..., 0] * (fluid.spec_energy(gas, t) + 0.5 * (s[..., 1:4] ** 2).sum(-1))
    return np.stack([s[..., 0]] + [s[..., 0] * s[..., q] for q in (1, 2, 3)] + [rho_e], -1)


def energy_margin(oracle, case, cfl, warm=(), rank=0, exchange=None):
    """{block: min over its cells of e_new - hf} after one explicit Euler update at `cfl`
    (procBlock.cpp:892: U_new = U - dt / V R; e = E - |m|^2 / (2 rho^2)), restated in numpy
    on the CPU oracle's residual and time step -- after the calls `warm` (their CFL numbers)
    have run on the oracle.  Negative: temperature_from_energy has no root there."""
    sol = Solver(oracle, case, rank=rank, exchange=exchange)
    try:
        for nn, c in enumerate(warm):
            sol.store_time_n(nn)
            sol.iterate(0, c)
        oracle.check(oracle.phase_bc_faces(sol.ctx), "phase_bc_faces")
        oracle.check(oracle.halo_exchange(sol.ctx, abi.HALO_STATE), "halo_exchange")
        oracle.check(oracle.phase_bc_edges(sol.ctx), "phase_bc_edges")
        oracle.check(oracle.phase_residual(sol.ctx, 0, cfl), "phase_residual")
        g, gas, out = case.ng, case.gas, {}
        for gb in sol.block_ids:
            s = sol.download("state", gb)[g:-g, g:-g, g:-g]
            res, dt = sol.download("residual", gb), sol.download("dt", gb)[..., 0]
            ni, nj, nk = case.blocks[gb].geom.n
            vol = np.asarray(case.blocks[gb].geom.vol.a).reshape(nk + 2 * g, nj + 2 * g,
                                                                 ni + 2 * g)[g:-g, g:-g, g:-g]
            new = _cons(gas, s) - (dt / vol)[..., None] * res
            e = new[..., 4] / new[..., 0] - 0.5 * (new[..., 1:4] ** 2).sum(-1) / new[..., 0] ** 2
            out[gb] = float((e - gas.heat_of_formation).min())
        return out
    finally:
        sol.close()
