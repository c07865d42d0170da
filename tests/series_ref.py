"""numpy references of the time series: the nearest cell with its tie rule, the join over
blocks, the chronology of a ring after drops.  Nothing here calls the library."""
import numpy as np


def nearest(center, points):
    """center[nk, nj, ni, 3]: the centres of the PHYSICAL cells of a block; points[P, 3].
    Returns [P, 4] = (i, j, k, d2): the cell nearest to each point, d2 = dx dx + dy dy + dz dz
    of centre - point, each product and sum rounded (no contraction).  np.argmin returns the
    first minimum of the flattened array, whose order is the linear index (k nj + j) ni + i:
    the tie rule of the library."""
    center = np.asarray(center, dtype=np.float64)
    nk, nj, ni, _ = center.shape
    flat = center.reshape(-1, 3)
    out = np.empty((len(points), 4))
    for p, x in enumerate(np.asarray(points, dtype=np.float64).reshape(-1, 3)):
        d = flat - x
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        q = int(np.argmin(d2))
        out[p] = (q % ni, (q // ni) % nj, q // (ni * nj), d2[q])
    return out


def nearest_loop(center, points):
    """The same by a plain loop over the cells in ascending linear index that replaces the
    minimum on a strictly smaller distance only: the rule spelled out."""
    center = np.asarray(center, dtype=np.float64)
    nk, nj, ni, _ = center.shape
    out = np.empty((len(points), 4))
    for p, x in enumerate(np.asarray(points, dtype=np.float64).reshape(-1, 3)):
        best = None
        for k in range(nk):
            for j in range(nj):
                for i in range(ni):
                    dx, dy, dz = (float(c) for c in center[k, j, i] - x)
                    d2 = dx * dx + dy * dy + dz * dz
                    if best is None or d2 < best[3]:
                        best = (i, j, k, d2)
        out[p] = best
    return out


def join(parts):
    """parts: {gb: [P, 4] of nearest} -> [P, 5] = (gb, i, j, k, d2): per point the block with
    the smallest d2, the lowest gb among equal ones."""
    out = None
    for gb in sorted(parts):
        part = np.column_stack([np.full(len(parts[gb]), float(gb)), parts[gb]])
        if out is None:
            out = part
            continue
        take = part[:, 4] < out[:, 4]      # (ascending gb: equality keeps the lower one)
        out[take] = part[take]
    return out


class Ring:
    """The record as a list: what samples and drops leave, oldest first."""

    def __init__(self, capacity):
        self.capacity, self.rows = capacity, []

    def sample(self, t):
        if len(self.rows) == self.capacity:
            raise OverflowError("full")
        self.rows.append(t)

    def drop(self, n):
        if not 0 <= n <= len(self.rows):
            raise ValueError("drop")
        del self.rows[:n]


def tie_box(n=(4, 3, 2), h=0.5):
    """Centres [nk, nj, ni, 3] of a box of n cells of spacing h (a power of two) with a corner
    at the origin, and points on the face midpoints, edge midpoints and corners of its cells:
    every coordinate and difference is a small multiple of h / 2, so d2 is exact with or
    without contraction and the ties are exact."""
    ni, nj, nk = n
    k, j, i = np.meshgrid(np.arange(nk), np.arange(nj), np.arange(ni), indexing="ij")
    center = np.stack([(i + 0.5) * h, (j + 0.5) * h, (k + 0.5) * h], axis=-1)
    pts = []
    # every point of the lattice of spacing h / 2 inside the box: cell centres (no tie), face
    # midpoints (2 cells tie), edge midpoints (4), corners (8)
    for c in range(2 * nk + 1):
        for b in range(2 * nj + 1):
            for a in range(2 * ni + 1):
                pts.append((a * h / 2, b * h / 2, c * h / 2))
    return center, np.array(pts)
