"""Host references of the time statistics (aither_amd/csrc/agx_stats.hpp).

Three forms of the weighted mean and covariance of a sequence of samples x_n (arrays of one
shape) with weights w_n:

  west       the one-pass recurrence of West (1979) in float64, in the device's order of
             operations (delta from the old mean, mean + (w / W) delta,
             C + (w (1 - w / W) delta_a) delta_b, C / W at the end)
  two_pass   the weighted mean, then the weighted mean of the products of the deviations, in
             np.longdouble: the reference
  naive      sums of w x and w x_a x_b, E[ab] - E[a] E[b] in float64: what the library does
             NOT do; the teeth test shows why

THE BOUND (tests/test_stats_host.py derives and measures it; the GPU tests use the same
constants).  ulp = 2^-52, n samples, every maximum over the samples and the points:
    |mean - ref|  <=  C1 n ulp max|x|
    |cov_ab - ref| <=  C2 n ulp (max|x_a| max|d_b| + max|x_b| max|d_a|),   d = x - mean
Form: each of the n steps of the recurrence rounds the mean once, relative to |mean| <= max|x|;
delta is a difference of two numbers of size max|x|, so its error is ABSOLUTE in x, about
n ulp max|x|, however small delta itself is, and enters the product delta_a delta_b once per
factor.  Measured worst case of `west` against `two_pass` on the three sample families of the
host test (five-step navierStokes oracle run; 1 + 1e-8 pattern; identical samples), weights
(1, 0.5, 2, 0.25, 1), as multiples of the right-hand sides with C = 1:
    means 0.25, co-moments 0.032
With a factor of 4 on the measured values (the device differs from `west` only by
the pack's arithmetic and by where the dimensional factor is multiplied in): C1 = 1.0,
C2 = 0.128.  On the card the device reaches 0.18 - 0.36 of the mean bound and 0.23 - 0.66 of
the second-moment bound (tests/test_stats_gpu.py prints the figures).
"""
import numpy as np

ULP = 2.0 ** -52
MEASURED_C1, MEASURED_C2 = 0.25, 0.032
C1, C2 = 4 * MEASURED_C1, 4 * MEASURED_C2
WEIGHTS = (1.0, 0.5, 2.0, 0.25, 1.0)


def west(samples, weights, pairs):
    """samples: per sample a dict {name: float64 array}; pairs: [(a, b)] names of the
    co-moments.  Returns (means {name: array}, covs {(a, b): array}, W)."""
    names = list(samples[0])
    mean = {n: np.zeros_like(np.asarray(samples[0][n], dtype=np.float64)) for n in names}
    com = {p: np.zeros_like(mean[p[0]]) for p in pairs}
    big_w = 0.0
    for x, w in zip(samples, weights):
        big_w = big_w + w
        r = w / big_w
        cf = w * (1.0 - r)
        d = {n: np.asarray(x[n], dtype=np.float64) - mean[n] for n in names}
        for n in names:
            mean[n] = mean[n] + r * d[n]
        for a, b in pairs:
            com[(a, b)] = com[(a, b)] + (cf * d[a]) * d[b]
    return mean, {p: c / big_w for p, c in com.items()}, big_w


def two_pass(samples, weights, pairs):
    ld = np.longdouble
    names = list(samples[0])
    big_w = sum(ld(w) for w in weights)
    mean = {n: sum(ld(w) * np.asarray(x[n], dtype=ld) for x, w in zip(samples, weights)) / big_w
            for n in names}
    cov = {}
    for a, b in pairs:
        cov[(a, b)] = sum(ld(w) * (np.asarray(x[a], dtype=ld) - mean[a]) *
                          (np.asarray(x[b], dtype=ld) - mean[b])
                          for x, w in zip(samples, weights)) / big_w
    return mean, cov, big_w


def naive(samples, weights, pairs):
    names = list(samples[0])
    big_w = float(sum(weights))
    s1 = {n: sum(w * np.asarray(x[n], dtype=np.float64) for x, w in zip(samples, weights))
          for n in names}
    mean = {n: s1[n] / big_w for n in names}
    cov = {}
    for a, b in pairs:
        s2 = sum(w * np.asarray(x[a], dtype=np.float64) * np.asarray(x[b], dtype=np.float64)
                 for x, w in zip(samples, weights))
        cov[(a, b)] = s2 / big_w - mean[a] * mean[b]
    return mean, cov, big_w


def scales(samples, weights):
    """max|x| and max|x - mean| per name, over samples and points (longdouble mean)."""
    mean, _, _ = two_pass(samples, weights, [])
    big = {n: max(float(np.abs(x[n]).max()) for x in samples) for n in samples[0]}
    dev = {n: max(float(np.abs(np.asarray(x[n], dtype=np.longdouble) - mean[n]).max())
                  for x in samples) for n in samples[0]}
    return big, dev


def mean_bound(samples, weights, name, c1=C1):
    big, _ = scales(samples, weights)
    return c1 * len(samples) * ULP * big[name]


def cov_bound(samples, weights, a, b, c2=C2):
    big, dev = scales(samples, weights)
    return c2 * len(samples) * ULP * (big[a] * dev[b] + big[b] * dev[a])


def worst(samples, weights, pairs, form=west):
    """Largest error of `form` against two_pass, as multiples of the bounds with C = 1:
    (means, co-moments).  A pair whose bound is 0 (identical samples) must be exact."""
    mean, cov, _ = form(samples, weights, pairs)
    rmean, rcov, _ = two_pass(samples, weights, pairs)
    wm = wc = 0.0
    for n in mean:
        bound = mean_bound(samples, weights, n, 1.0)
        err = float(np.abs(mean[n] - rmean[n]).max())
        wm = max(wm, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
    for a, b in pairs:
        bound = cov_bound(samples, weights, a, b, 1.0)
        err = float(np.abs(cov[(a, b)] - rcov[(a, b)]).max())
        wc = max(wc, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
    return wm, wc
