"""The multigrid transfer operators restated in plain numpy, float64, from the reference alone
(no project code beyond array shapes).  tests/test_mg_transfers_host.py holds the oracle to
these, tests/test_mg_transfers_gpu.py the HIP libraries.

Every function returns (value, magnitude): the magnitude is the same operation applied to
absolute values -- the sum of the absolute terms -- which scales the round-off bound of a
result whose terms may be summed in another order or contracted into fused multiply-adds.

Arrays hold physical cells only, [nk, nj, ni, n_eq]; to_coarse [nk, nj, ni, 3] names the
coarse cell (i, j, k) of every fine cell.
"""
import numpy as np

EPS = 2.0 ** -52
RESTRICT_UNITS = 8.0     # a coarse cell: at most 8 products and 7 additions, maybe contracted
PROLONG_UNITS = 32.0     # about 19 roundings deep: 7 additions, one factor, three levels of
                         # interpolation (two roundings each for the factor 1 - c and the sum)


def _flat(to_coarse, coarse_cells):
    cnk, cnj, cni = coarse_cells
    tc = to_coarse.astype(np.int64)
    return ((tc[..., 2] * cnj + tc[..., 1]) * cni + tc[..., 0]).ravel()


def restrict(fine, to_coarse, coarse_cells, weights=None):
    """BlockRestriction (procBlock.hpp:636-690): the coarse array zeroed, then every fine cell
    in k, j, i order added to its coarse cell -- times its volume weight (state, x), or as it
    is (the forcing term: summed, not volume weighted; weights=None)."""
    fine = np.asarray(fine, dtype=np.float64)
    n_eq = fine.shape[-1]
    term = fine if weights is None else np.asarray(weights)[..., None] * fine
    term = term.reshape(-1, n_eq)
    flat = _flat(to_coarse, coarse_cells)
    out = np.zeros((int(np.prod(coarse_cells)), n_eq))
    mag = np.zeros_like(out)
    np.add.at(out, flat, term)             # (walks the flattened fine array: k, j, i ascending)
    np.add.at(mag, flat, np.abs(term))
    shape = tuple(coarse_cells) + (n_eq,)
    return out.reshape(shape), mag.reshape(shape)


def cell_to_node(cells):
    """ConvertCellToNode(x, ignoreEdge=true, ignoreGhosts=true) (utility.hpp:274-329): every
    cell is added to its eight nodes, then a node is scaled by where it sits in the node array
    (multiArray3d.hpp:1595-1679, no ghost cells): 1 at the block's corners, 1/2 on its edges,
    1/8 everywhere else -- a node inside a face gets half the average of its four cells."""
    cells = np.asarray(cells, dtype=np.float64)
    nk, nj, ni, n_eq = cells.shape
    out = []
    for src in (cells, np.abs(cells)):
        nodes = np.zeros((nk + 1, nj + 1, ni + 1, n_eq))
        for dk in (0, 1):
            for dj in (0, 1):
                for di in (0, 1):
                    nodes[dk:dk + nk, dj:dj + nj, di:di + ni] += src
        ek = np.zeros(nk + 1, dtype=bool); ek[[0, nk]] = True
        ej = np.zeros(nj + 1, dtype=bool); ej[[0, nj]] = True
        ei = np.zeros(ni + 1, dtype=bool); ei[[0, ni]] = True
        on = ek[:, None, None].astype(int) + ej[None, :, None] + ei[None, None, :]
        fac = np.where(on == 3, 1.0, np.where(on == 2, 0.5, 0.125))
        out.append(nodes * fac[..., None])
    return out[0], out[1]


def _lin(d0, d1, c):
    # LinearInterp utility.hpp:341-344
    return (1.0 - c)[..., None] * d0 + c[..., None] * d1


def trilinear(nodes, to_coarse, coeffs):
    """TrilinearInterp (utility.hpp:341-372) of the coarse block's node values to every fine
    cell with its seven coefficients: along k on the four edges, then along i, then along j.
    The magnitude interpolates |nodes| with |1 - c| and |c|."""
    ci, cj, ck = to_coarse[..., 0], to_coarse[..., 1], to_coarse[..., 2]
    res = []
    for src, lin in ((np.asarray(nodes, dtype=np.float64), _lin),
                     (np.abs(nodes), lambda a, b, c: np.abs(1.0 - c)[..., None] * a
                      + np.abs(c)[..., None] * b)):
        n = lambda di, dj, dk: src[ck + dk, cj + dj, ci + di]
        c = coeffs
        d04 = lin(n(0, 0, 0), n(0, 0, 1), c[..., 0])
        d15 = lin(n(1, 0, 0), n(1, 0, 1), c[..., 1])
        d26 = lin(n(0, 1, 0), n(0, 1, 1), c[..., 2])
        d37 = lin(n(1, 1, 0), n(1, 1, 1), c[..., 3])
        d0415 = lin(d04, d15, c[..., 4])
        d2637 = lin(d26, d37, c[..., 5])
        res.append(lin(d0415, d2637, c[..., 6]))
    return res[0], res[1]


def prolong(fine_x, correction, to_coarse, coeffs):
    """SubtractFromUpdate + Prolongation + AddToUpdate (mgSolution.cpp:189-192,
    gridLevel.hpp:159-214): the coarse correction at the coarse nodes, interpolated to the fine
    cells and added to the fine x.  Returns (fine x + interp(nodes(correction)),
    |fine x| + interp(nodes(|correction|)))."""
    nodes, nmag = cell_to_node(correction)
    val, _ = trilinear(nodes, to_coarse, coeffs)
    _, mag = trilinear(nmag, to_coarse, coeffs)
    return fine_x + val, np.abs(fine_x) + mag


def forcing_identity(fine_residuals, to_coarses, coarse_cells):
    """After a restriction the coarse level's matrix residual is forcing - (A x - b) with
    forcing = R(r_fine) + (A x - b) (gridLevel.cpp:568-590): the summed fine matrix residual,
    whatever x the coarse level holds.  With x = 0 on the fine level, implicitEuler and the
    first nonlinear iteration r_fine = b = -residual.  Returns sum over blocks, coarse cells
    and equations of R(-residual)**2."""
    total = 0.0
    for r, tc, cc in zip(fine_residuals, to_coarses, coarse_cells):
        summed, _ = restrict(-np.asarray(r), tc, cc)
        total += float((summed ** 2).sum())
    return total
