"""Fields whose largest residual is tied bit for bit: the same in every plane along one grid
axis.  Shared by tests/test_parity_measure_host.py (the oracle alone: the maximum really is
tied, off the zero indices, and the first tied cell is reported), tests/test_norm_record_gpu.py
and the multi-rank tests (the L-inf record's location through every device reduction and the
rank merge)."""
import math

import numpy as np

from parity_utils import first_maximum, tied_set
from aither_amd.case import builder, synthetic

TIE_DECKS = {
    # the fused marching stage
    "rk4_muscl_roe": dict(time_integration="rk4", cfl=0.5),
    # k_update + reduce_norms in the 5-equation build: viscous, so the stage is not fused
    # (can_fuse: explicit AND inviscid)
    "visc_explicit": dict(equation_set="navierStokes", time_integration="explicitEuler",
                          cfl=0.3),
    # k_update_d2 + norm_block_fold (scalar LU-SGS on the diagonal-ordered arrays)
    "lusgs_weno_ausm_visc": dict(equation_set="navierStokes", face_reconstruction="weno",
                                 limiter="none", inviscid_flux="ausm",
                                 time_integration="implicitEuler", matrix_solver="lusgs",
                                 cfl=10.0),
    # the rans library's implicit update: k_update in mode 2 + reduce_norms, 7 equations
    # (the diagonal-ordered path is 5-equation only)
    "rans_wilcox_lusgs": dict(equation_set="rans", turbulence_model="kOmegaWilcox2006",
                              time_integration="implicitEuler", matrix_solver="lusgs",
                              cfl=10.0),
}
SPACING = 2.0 ** -3       # dyadic along the extrusion axis: every plane's geometry bit for bit


def extruded_case(n, axis, nblocks=1, ranks=None, **deck_kw):
    """nblocks boxes of n cells stacked along `axis`: slip walls on that axis, a far field on
    the four other sides (so that the largest residual is the field's, not a wall corner's),
    no free-stream velocity along `axis`, the spacing along it dyadic and uniform in the other
    two -- carrying extruded_state."""
    d = "ijk".index(axis)
    vel = [50.0, 20.0, 10.0]
    vel[d] = 0.0
    sides = {s: ("characteristic", 1) for s in range(1, 7) if (s - 1) // 2 != d}
    deck, coords = synthetic._stacked(n, nblocks, axis, 1.0, sides, dict(deck_kw, velocity=vel))
    for b, x in enumerate(coords):
        shape = [1, 1, 1]
        shape[2 - d] = n[d] + 1
        x[..., d] = ((b * n[d] + np.arange(n[d] + 1)) * SPACING).reshape(shape)
    case = builder.build_case(None, deck=deck, coords=coords, ranks=ranks)
    extruded_state(case, axis)
    return case


def extruded_state(case, axis):
    """q (1 + 0.05 sin 2 pi (a + 0.3) sin 2 pi (b + 0.2)) over the two axes a, b other than
    `axis`, the same in every plane along `axis`; no velocity along `axis`.  The phase shifts
    and a window (sin pi a sin pi b)^2, which lets the field meet the far field of the sides
    smoothly, move the maximum of the residual off the cells with a zero index in a or b."""
    d = "ijk".index(axis)
    qa, qb = [q for q in range(3) if q != d]
    for blk in case.blocks:
        c = blk.geom.center.a
        fac = 1.0 + 0.05 * np.sin(2.0 * math.pi * (c[..., qa] + 0.3)) * \
            np.sin(2.0 * math.pi * (c[..., qb] + 0.2)) * \
            (np.sin(math.pi * c[..., qa]) * np.sin(math.pi * c[..., qb])) ** 2
        g = blk.geom.ng
        base = blk.state[g, g, g, :].copy()
        new = base[None, None, None, :] * fac[..., None]
        new[..., 2] = base[2] * (2.0 - fac)          # the velocities out of phase
        new[..., 1 + d] = 0.0
        ni, nj, nk = blk.geom.n
        blk.state[...] = 0.0
        blk.state[g:g + nk, g:g + nj, g:g + ni, :] = new[g:g + nk, g:g + nj, g:g + ni, :]


def tie_box(axis):
    """A small box for the CPU checks: 8 cells along the axis, 8 x 4 across."""
    n = [8, 4, 8]
    d = "ijk".index(axis)
    if n[d] != 8:
        n[d], n[(d + 1) % 3] = 8, 4
    return tuple(n)


def assert_tied_record(case, axis, residual, linf, nblocks):
    """residual: per block; the maximum is tied along `axis` in every block, sits at nonzero
    indices in the free directions, and `linf` names the first tied cell in the reference's
    loop order (block, k, j, i, equation; strict >)."""
    d = "ijk".index(axis)
    tied, gap = tied_set(residual)
    n_axis = case.blocks[0].geom.n[d]
    for b in range(nblocks):
        mine = [t for t in tied if t[0] == b]
        assert len(mine) >= 2, (b, tied)
        assert len(mine) % n_axis == 0, (b, mine)           # whole lines along the axis
    assert gap > 0.0
    for t in tied:
        free = [t[1 + q] for q in range(3) if q != d]
        assert all(v > 0 for v in free), ("a tied maximum at a zero index", t)
    first = first_maximum(residual)
    assert tuple(linf) == first, (linf, first)
    assert first[1] == 0 and first[1 + 1 + d] == 0          # block 0, plane 0 along the axis
    return tied


# ---- the decks by the reduction of update_pass they reach, at the GPU tests' size ---------------
BOX = (70, 36, 6)
PATHS = {"fused": "rk4_muscl_roe", "k_update": "visc_explicit",
         "k_update_d2": "lusgs_weno_ausm_visc", "rans": "rans_wilcox_lusgs"}


def tie_case(path, axis, nblocks, ranks=None):
    return extruded_case(BOX, axis, nblocks, ranks=ranks, **TIE_DECKS[PATHS[path]])
