"""Host references of the time statistics collapsed along index directions
(aither_amd/csrc/agx_stats.hpp at AGX_CSTAT_BASE; include/aither_gfx950.h).

A bin pools N cells with volumes v, time means m_a and time co-moments C_ab (sum of weights W):
    V = sum v,   M_a = sum v m_a / V,   cov_ab = sum v [C_ab / W + (m_a - M_a)(m_b - M_b)] / V
Every function takes the cells of the bins along the LAST axis: vol[..., N], means
{name: [..., N]}, coms {(a, b): [..., N]}, and returns (V, {name: M}, {(a, b): cov}) over the
leading axes.

  west_space   the one-pass recurrence in float64, in the device's order of operations:
                   V += v; r = v / V; cf = v (1 - r); d = m - M
                   M += r d;  T_ab += r (C_ab - T_ab);  D_ab += (cf d_a) d_b
               cov = T / W + D / V
  chunked      the same over chunks of `chunk` cells, the partial (V, M, T, D) of the chunks
               joined in ascending order by the pairwise form (join)
  two_pass     the definition in np.longdouble: the reference
  naive        sums of v m and v (C / W + m_a m_b), E[ab] - E[a] E[b] in float64: what the
               library does NOT do
  count_mean   the unweighted average: what a stretched grid must not be given

THE BOUND.  ulp = 2^-52, N cells per bin, every maximum over the cells of the bin, d = m - M:
    |M - ref|      <=  C1 N ulp max|m|
    |cov_ab - ref| <=  C2 N ulp (max|C_ab| / W + max|m_a| max|d_b| + max|m_b| max|d_a|)
Form, as in stats_ref.py: each of the N steps (or joins) rounds the mean once, relative to
|M| <= max|m|; delta is a difference of two numbers of size max|m|, so its error is absolute in
m and enters delta_a delta_b once per factor; T is a running mean of the C_ab and rounds
relative to max|C_ab|.  It holds for any join order.
Measured worst case of west_space and of chunked (chunks of 4, 64 and 100) against two_pass on
the three families of tests/test_stats_collapse_host.py (random O(1) means and co-moments;
1 + 1e-8 noise; identical cells), 50 bins each of N = 3, 6, 9, 67, 300 and 4096 cells (the
device tests pool bins of 3 cells and up), stretched volumes, as multiples of the right-hand
sides with C = 1:
    means 0.245, co-moments 0.162
both at N = 3 (the worst shrinks with N: 0.03 and 0.006 at N = 67, 0.004 and 0.0008 at 4096); the
co-moments' is the identical family's, where T / W is the float64 quotient and the reference
the extended one.  Recorded as MEASURED_C1 = 0.25, MEASURED_C2 = 0.165.
With the factor of 4 of stats_ref.py on the measured values (the device differs from
west_space by the shape of its joins, which the bound does not depend on, and by where the
dimensional factor is multiplied in): C1 = 4 MEASURED_C1 = 1.0, C2 = 4 MEASURED_C2 = 0.66.  On
the card the device reaches at most 0.54 of the mean bound and 0.29 of the co-moment bound, in
bins of 3 cells, and less than 0.02 of either from 66 cells per bin on
(tests/test_stats_collapse_gpu.py prints the figures).
"""
import numpy as np

ULP = 2.0 ** -52
MEASURED_C1, MEASURED_C2 = 0.25, 0.165
C1, C2 = 4 * MEASURED_C1, 4 * MEASURED_C2
AXIS_BIT = (4, 2, 1)        # the mask bit of the axes of a [nk, nj, ni] array


def to_bins(a, mask):
    """[nk, nj, ni] -> [*remaining extents (k, j, i order), N]: the collapsed directions of
    `mask` (bit 0 = i, 1 = j, 2 = k) moved to the end and flattened, k outer, i inner."""
    a = np.asarray(a)
    keep = [ax for ax in range(3) if not mask & AXIS_BIT[ax]]
    gone = [ax for ax in range(3) if mask & AXIS_BIT[ax]]
    t = np.transpose(a, keep + gone)
    return t.reshape(t.shape[:len(keep)] + (-1,))


def _f64(d):
    return {k: np.asarray(v, dtype=np.float64) for k, v in d.items()}


def serial(vol, means, coms):
    """The recurrence over the last axis: the partial (V, M, T, D)."""
    vol, means, coms = np.asarray(vol, dtype=np.float64), _f64(means), _f64(coms)
    shape = vol.shape[:-1]
    big_v = np.zeros(shape)
    big_m = {n: np.zeros(shape) for n in means}
    big_t = {p: np.zeros(shape) for p in coms}
    big_d = {p: np.zeros(shape) for p in coms}
    for c in range(vol.shape[-1]):
        v = vol[..., c]
        big_v = big_v + v
        r = v / big_v
        cf = v * (1.0 - r)
        d = {n: means[n][..., c] - big_m[n] for n in means}
        for n in means:
            big_m[n] = big_m[n] + r * d[n]
        for p in coms:
            big_t[p] = big_t[p] + r * (coms[p][..., c] - big_t[p])
            big_d[p] = big_d[p] + (cf * d[p[0]]) * d[p[1]]
    return big_v, big_m, big_t, big_d


def join(one, two):
    """Two partials by the pairwise form, r = V2 / (V1 + V2), delta = M2 - M1."""
    v1, m1, t1, d1 = one
    v2, m2, t2, d2 = two
    big_v = v1 + v2
    r = v2 / big_v
    cf = v1 * r
    d = {n: m2[n] - m1[n] for n in m1}
    big_m = {n: m1[n] + r * d[n] for n in m1}
    big_t = {p: t1[p] + r * (t2[p] - t1[p]) for p in t1}
    big_d = {p: d1[p] + d2[p] + (cf * d[p[0]]) * d[p[1]] for p in d1}
    return big_v, big_m, big_t, big_d


def finish(part, big_w):
    big_v, big_m, big_t, big_d = part
    return big_v, big_m, {p: big_t[p] / big_w + big_d[p] / big_v for p in big_t}


def west_space(vol, means, coms, big_w=1.0):
    return finish(serial(vol, means, coms), big_w)


def chunked(vol, means, coms, big_w=1.0, chunk=64):
    vol = np.asarray(vol, dtype=np.float64)
    part = None
    for lo in range(0, vol.shape[-1], chunk):
        sl = slice(lo, lo + chunk)
        nxt = serial(vol[..., sl], {n: np.asarray(m)[..., sl] for n, m in means.items()},
                     {p: np.asarray(c)[..., sl] for p, c in coms.items()})
        part = nxt if part is None else join(part, nxt)
    return finish(part, big_w)


def two_pass(vol, means, coms, big_w=1.0, dtype=np.longdouble):
    """The reference; dtype=np.float64 is the two-pass reduction a caller would write."""
    ld = dtype
    vol = np.asarray(vol, dtype=ld)
    big_v = vol.sum(axis=-1)
    m = {n: np.asarray(x, dtype=ld) for n, x in means.items()}
    big_m = {n: (vol * m[n]).sum(axis=-1) / big_v for n in m}
    cov = {}
    for p, c in coms.items():
        a, b = p
        inner = np.asarray(c, dtype=ld) / ld(big_w) + \
            (m[a] - big_m[a][..., None]) * (m[b] - big_m[b][..., None])
        cov[p] = (vol * inner).sum(axis=-1) / big_v
    return big_v, big_m, cov


def naive(vol, means, coms, big_w=1.0):
    vol, means, coms = np.asarray(vol, dtype=np.float64), _f64(means), _f64(coms)
    big_v = vol.sum(axis=-1)
    big_m = {n: (vol * m).sum(axis=-1) / big_v for n, m in means.items()}
    cov = {}
    for p, c in coms.items():
        a, b = p
        s2 = (vol * (c / big_w + means[a] * means[b])).sum(axis=-1)
        cov[p] = s2 / big_v - big_m[a] * big_m[b]
    return big_v, big_m, cov


def count_mean(vol, means, coms, big_w=1.0):
    """Every cell with the same weight."""
    return west_space(np.ones_like(np.asarray(vol, dtype=np.float64)), means, coms, big_w)


def bounds(vol, means, coms, big_w=1.0, c1=C1, c2=C2):
    """({name: bound of M}, {(a, b): bound of cov}), one value per bin."""
    n = np.asarray(vol).shape[-1]
    _, ref_m, _ = two_pass(vol, means, {})
    big = {k: np.abs(np.asarray(m, dtype=np.float64)).max(axis=-1) for k, m in means.items()}
    dev = {k: np.abs(np.asarray(m, dtype=np.longdouble) - ref_m[k][..., None]).max(axis=-1)
           .astype(np.float64) for k, m in means.items()}
    bm = {k: c1 * n * ULP * big[k] for k in means}
    bc = {}
    for p, c in coms.items():
        a, b = p
        cmax = np.abs(np.asarray(c, dtype=np.float64)).max(axis=-1)
        bc[p] = c2 * n * ULP * (cmax / big_w + big[a] * dev[b] + big[b] * dev[a])
    return bm, bc


def _ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    out = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0),
                   np.where(err == 0, 0.0, np.inf))
    return float(out.max())


def reached(got, vol, means, coms, big_w=1.0, c1=C1, c2=C2):
    """Largest error of got = (V, M, cov) against two_pass as fractions of the bounds:
    (means, co-moments).  A bin whose bound is 0 must be exact."""
    _, gm, gc = got
    _, rm, rc = two_pass(vol, means, coms, big_w)
    bm, bc = bounds(vol, means, coms, big_w, c1, c2)
    wm = max([_ratio(np.abs(gm[n] - rm[n]), bm[n]) for n in means] or [0.0])
    wc = max([_ratio(np.abs(gc[p] - rc[p]), bc[p]) for p in coms] or [0.0])
    return wm, wc
