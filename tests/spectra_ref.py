"""References of the spectra along a homogeneous direction (aither_amd/csrc/agx_spectra.hpp).

reference(): the definition in numpy longdouble -- the line mean, taken and SUBTRACTED in
longdouble (an unshifted longdouble transform is itself wrong by 1e-11 relative on data like
1 + 1e-8 noise), the direct transform with the twiddle index m n mod N formed in integers,
plain means over the lines of a bin and the weighted mean over the samples.

restate(): the device's operations one for one in float64: the serial line mean, the
subtraction, the twiddle table rounded from longdouble, the inner product in ascending n, the
spectrum's arithmetic in the kernel's order, the pooling of the lines into records and of the
records into a bin in the order of agx_spectra_plan.hpp (shape() below is that header's
arithmetic; tests/test_spectra_host.py holds it against the C++), and the recurrence in time.
One difference: the kernel's inner product is a fused multiply-add, numpy's a multiply and an
add, two roundings for the kernel's one; the restatement's error is therefore the larger.

The bound.  ulp = 2^-52, A' = mean |x - mu| along a line (the maximum over the lines and
samples of a bin), L lines of a bin, n samples:
    m >= 1:  |S - ref| <= C1 (N + L + n) ulp A'_a A'_b
    m == 0:  |S - ref| <= C1 (N + L + n) ulp (|mu_a| + A'_a) (|mu_b| + A'_b)
MEASURED_C1 is the largest share (error over (N + L + n) ulp A'A') the float64 restatement
reached against reference() over N = 2, 3, 7, 8, 16, 67, 130, 256, three families (random
O(1), 1 + 1e-8 noise, one harmonic plus a mean), pooled and unpooled, weights 1, 0.5, 2, 0.25,
1 and a single sample of weight 1 (the smallest bound), five lines each
(test_spectra_host.py::test_the_bound_constant_is_what_the_restatement_reaches measures it
again): 0.31 at N = 2, 0.49 at N = 3, 0.26 at 7, 0.18 at 8, 0.11 at 16, 0.07 at 67, 0.04 at
130, 0.03 at 256 -- the errors of a sum grow like sqrt(N), the bound like N.  Recorded as
MEASURED_C1 = 0.5.  With the project's factor of 4 (stats_ref.py: the device contracts and
orders differently, the dimensional factors are multiplied in): C1 = 2.0.
"""
import numpy as np

LD = np.longdouble
ULP = 2.0 ** -52
MEASURED_C1 = 0.5
C1 = 4 * MEASURED_C1
LB, CHUNK, TILE, LDS, MAX_N = 4, 8, 64, 10240, 1024


def n_spec(nvar, pairs):
    return nvar + len(pairs)


def _lines(x, along):
    """x[nvar, nk, nj, ni] as [nvar, n2, n1, N]: (d2, d1, along), d1 the lower index direction
    of the two that are not `along`."""
    axis = {0: 3, 1: 2, 2: 1}
    d1, d2 = (1 if along == 0 else 0), (1 if along == 2 else 2)
    return np.transpose(x, (0, axis[d2], axis[d1], axis[along]))


def _pooled(along, over):
    d1, d2 = (1 if along == 0 else 0), (1 if along == 2 else 2)
    return "ijk"[d1] in over, "ijk"[d2] in over


def reference(samples, weights, pairs, along, over):
    """The spectra of samples (a list of x[nvar, nk, nj, ni]) with weights, in longdouble:
    (S[nspec, *remaining extents (k, j, i), nmode], A1[nvar, *remaining], MU[nvar,
    *remaining]) -- A1 the largest mean |x - mu| and MU the largest |mu| over the lines and
    samples of a bin, in float64."""
    a = "ijk".index(along)
    pool1, pool2 = _pooled(a, over)
    total, big_w = None, LD(0)
    dev = absmu = None
    for x, w in zip(samples, weights):
        xl = _lines(np.asarray(x, dtype=LD), a)
        nvar, n2, n1, n = xl.shape
        mu = xl.sum(axis=3) / LD(n)
        y = xl - mu[..., None]
        m = np.arange(n // 2 + 1)
        q = np.outer(m, np.arange(n)) % n
        ang = LD(2) * np.arccos(LD(-1)) * q.astype(LD) / LD(n)
        co, si = np.cos(ang), np.sin(ang)
        re = np.einsum("vqpn,mn->vqpm", y, co)
        im = np.einsum("vqpn,mn->vqpm", y, si)
        cm = np.full(n // 2 + 1, LD(2))
        if n % 2 == 0:
            cm[n // 2] = LD(1)
        spec = []
        for v in range(nvar):
            p = cm * (re[v] ** 2 + im[v] ** 2) / LD(n) ** 2
            p[..., 0] = mu[v] ** 2
            spec.append(p)
        for va, vb in pairs:
            p = cm * (re[va] * re[vb] + im[va] * im[vb]) / LD(n) ** 2
            p[..., 0] = mu[va] * mu[vb]
            spec.append(p)
        spec = np.array(spec)                      # [nspec, n2, n1, nmode]
        a1 = np.abs(y).mean(axis=3)
        am = np.abs(mu)
        if pool2:
            spec, a1, am = spec.mean(axis=1, keepdims=True), a1.max(axis=1, keepdims=True), \
                am.max(axis=1, keepdims=True)
        if pool1:
            spec, a1, am = spec.mean(axis=2, keepdims=True), a1.max(axis=2, keepdims=True), \
                am.max(axis=2, keepdims=True)
        big_w = big_w + LD(w)
        total = spec * LD(w) if total is None else total + spec * LD(w)
        dev = a1 if dev is None else np.maximum(dev, a1)
        absmu = am if absmu is None else np.maximum(absmu, am)
    total = total / big_w
    keep = tuple(s for s, pooled in zip(total.shape[1:3], (pool2, pool1)) if not pooled)
    return (total.reshape((total.shape[0],) + keep + (total.shape[-1],)),
            dev.astype(np.float64).reshape((dev.shape[0],) + keep),
            absmu.astype(np.float64).reshape((absmu.shape[0],) + keep))


def bound(a1, absmu, pairs, n, lines, nsamples, c1=C1):
    """The bound of every entry: [nspec, *remaining, nmode]."""
    nvar = a1.shape[0]
    ab = [(v, v) for v in range(nvar)] + [tuple(p) for p in pairs]
    out = []
    for va, vb in ab:
        hi = a1[va] * a1[vb]
        lo = (absmu[va] + a1[va]) * (absmu[vb] + a1[vb])
        e = np.repeat(hi[..., None], n // 2 + 1, axis=-1)
        e[..., 0] = lo
        out.append(e)
    return c1 * (n + lines + nsamples) * ULP * np.array(out)


def reached(got, ref, lim):
    """The largest share of the bound: max |got - ref| / bound (0 / 0 counts as 0)."""
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    return float(np.max(np.where(err == 0.0, 0.0, err / np.where(lim > 0, lim, 1e-300))))


# ---- the plan's arithmetic (agx_spectra_plan.hpp) ----------------------------------------------
def shape(ext, along, over_mask, nvar):
    """spectra_shape of the header as a dict; None where N is out of range."""
    n = ext[along]
    if n < 2 or n > MAX_N:
        return None
    d1, d2 = (1 if along == 0 else 0), (1 if along == 2 else 2)
    s = {"n": n, "nmode": n // 2 + 1, "n1": ext[d1], "n2": ext[d2],
         "pool1": over_mask >> d1 & 1, "pool2": over_mask >> d2 & 1}
    # (the tile of a plan of six variables, whatever nvar is: see the header)
    tl = min((LDS - 2 * n) // (6 * (n + 1)), TILE, s["n1"])
    if tl > LB:
        tl -= tl % LB
        best, num, den = tl, 0, 1
        for t in range(LB, tl + 1, LB):
            passes = ((n // 2) * (t // LB) + 255) // 256
            if t * den >= num * passes:
                best, num, den = t, t, passes
        tl = best
    s["tl"] = tl
    s["nt1"] = (s["n1"] + tl - 1) // tl
    s["ng"] = (tl + LB - 1) // LB
    s["steps"] = (s["nt1"] if s["pool1"] else 1) * (s["n2"] if s["pool2"] else 1)
    s["nchunk"] = (s["steps"] + CHUNK - 1) // CHUNK
    s["nfix"] = (1 if s["pool1"] else s["nt1"]) * (1 if s["pool2"] else s["n2"])
    s["nbin"] = (1 if s["pool1"] else s["n1"]) * (1 if s["pool2"] else s["n2"])
    s["nrec"] = s["nchunk"] * (s["ng"] if s["pool1"] else 1)
    s["lines"] = (s["n1"] if s["pool1"] else 1) * (s["n2"] if s["pool2"] else 1)
    return s


def group_lines(s, tile, gr):
    left = min(s["n1"] - tile * s["tl"], s["tl"]) - gr * LB
    return max(0, min(left, LB))


def record_lines(s, rec):
    chunk, gr = (rec // s["ng"], rec % s["ng"]) if s["pool1"] else (rec, 0)
    s0, s1 = chunk * CHUNK, min(chunk * CHUNK + CHUNK, s["steps"])
    if not s["pool1"]:
        return s1 - s0
    return sum(group_lines(s, st % s["nt1"], gr) for st in range(s0, s1))


def record_sequence(s, rec, p1, p2):
    """The lines (p1, p2) record rec of the bin at (p1, p2) pools, in the kernel's order (the
    pooled coordinates of the bin are ignored)."""
    chunk, gr = (rec // s["ng"], rec % s["ng"]) if s["pool1"] else (rec, 0)
    seq = []
    for st in range(chunk * CHUNK, min(chunk * CHUNK + CHUNK, s["steps"])):
        q2 = (st // s["nt1"] if s["pool1"] else st) if s["pool2"] else p2
        if s["pool1"]:
            tile = st % s["nt1"]
            seq += [(tile * s["tl"] + gr * LB + j, q2) for j in range(group_lines(s, tile, gr))]
        else:
            seq.append((p1, q2))
    return seq


def twiddles(n):
    ang = LD(2) * np.arccos(LD(-1)) * np.arange(n).astype(LD) / LD(n)
    return np.cos(ang).astype(np.float64), np.sin(ang).astype(np.float64)


def line_spectra(x, pairs, along, shift=True):
    """The device's per-line arithmetic in float64: p[nspec, n2, n1, nmode] of
    x[nvar, nk, nj, ni].  shift=False: the raw transform, without the mean subtracted (what
    the teeth test shows to be useless)."""
    xl = np.ascontiguousarray(_lines(np.asarray(x, dtype=np.float64), along))
    nvar, n2, n1, n = xl.shape
    total = np.zeros(xl.shape[:3])
    for k in range(n):
        total = total + xl[..., k]
    mu = total / float(n)
    y = xl - mu[..., None] if shift else xl
    co, si = twiddles(n)
    nmode = n // 2 + 1
    m = np.arange(nmode)
    re = np.zeros(xl.shape[:3] + (nmode,))
    im = np.zeros_like(re)
    q = np.zeros(nmode, dtype=np.int64)
    for k in range(n):
        re = y[..., k, None] * co[q] + re
        im = y[..., k, None] * si[q] + im
        q = q + m
        q = np.where(q >= n, q - n, q)
    cm = np.full(nmode, 2.0)
    if n % 2 == 0:
        cm[n // 2] = 1.0
    n2f = float(n) * float(n)
    ab = [(v, v) for v in range(nvar)] + [(min(p), max(p)) for p in pairs]
    out = []
    for va, vb in ab:
        p = cm * (re[va] * re[vb] + im[va] * im[vb]) / n2f
        p[..., 0] = mu[va] * mu[vb]
        out.append(p)
    return np.array(out)


def restate(samples, weights, pairs, along, over):
    """The device's spectra in float64, operation for operation: S[nspec, *remaining extents
    (k, j, i), nmode], nondimensional."""
    a = "ijk".index(along)
    mask = sum(1 << "ijk".index(c) for c in over)
    acc, big_w = None, 0.0
    for x, w in zip(samples, weights):
        nvar = np.asarray(x).shape[0]
        ext = np.asarray(x).shape[:0:-1]
        s = shape(ext, a, mask, nvar)
        p = line_spectra(x, pairs, a)
        rest1 = 1 if s["pool1"] else s["n1"]
        rest2 = 1 if s["pool2"] else s["n2"]
        pooled = np.zeros((p.shape[0], rest2, rest1, s["nmode"]))
        counts = [record_lines(s, r) for r in range(s["nrec"])]
        for b2 in range(rest2):
            for b1 in range(rest1):
                mean, cnt = np.zeros((p.shape[0], s["nmode"])), 0.0
                for rec in range(s["nrec"]):
                    if counts[rec] == 0:
                        continue
                    part = np.zeros_like(mean)
                    for line, (p1, p2) in enumerate(record_sequence(s, rec, b1, b2), 1):
                        part = part + (p[:, p2, p1, :] - part) / float(line)
                    cnt = cnt + float(counts[rec])
                    mean = mean + (float(counts[rec]) / cnt) * (part - mean)
                pooled[:, b2, b1, :] = mean
        big_w = big_w + w
        acc = np.zeros_like(pooled) if acc is None else acc
        acc = acc + (w / big_w) * (pooled - acc)
    keep = tuple(n for n, pl in ((acc.shape[1], s["pool2"]), (acc.shape[2], s["pool1"])) if not pl)
    return acc.reshape((acc.shape[0],) + keep + (acc.shape[-1],))


FACTOR_NAMES = {"density": "rho", "vel_x": "a", "vel_y": "a", "vel_z": "a", "pressure": "p",
                "temperature": "t"}


def factors(names, pairs, rho_ref, a_ref, t_ref):
    """The dimensional factor of every spectrum: the product of its two variables' output
    factors."""
    one = {"rho": rho_ref, "a": a_ref, "p": rho_ref * a_ref * a_ref, "t": t_ref}
    f = [one[FACTOR_NAMES[n]] for n in names]
    return np.array([x * x for x in f] + [f[a] * f[b] for a, b in pairs])
