"""The distribution checks of the camera-noise sampler, shared by tests/test_hip_camnoise.py (the kernel) and tests/test_camnoise_host.py
(the same sampler source compiled for the CPU).  The bounds are those of tests/pgnoise_stats.py -- mean and variance within 5 standard
errors of the statistic under the exact law, chi-square at a 1e-6 tail -- with the law's own moments for the standard errors."""
import math

import numpy as np

LAMS = (-0.26, -0.026, 0.0, 0.015, 0.102)          # the shapes of the reference's cameras: both ends, the two nearest 0, and 0 itself


def tl_moment4(lam):
    """E Q^4 of the Tukey-lambda law of scale 1: sum_j C(4, j) (-1)^j B(lam (4 - j) + 1, lam j + 1) / lam^4 (from Q = (u^lam -
    (1 - u)^lam) / lam and the Beta integral), 7 pi^4 / 15 at 0; infinite for lam <= -1/4.  For |lam| < 0.05 the sum cancels to
    O(lam^4): there the quadrature of Q^4 over (0, 1) is used instead.  (It feeds a standard error: 1e-6 relative is plenty.)"""
    from scipy import integrate, special, stats
    if lam <= -0.25:
        return math.inf
    if lam == 0:
        return 7 * math.pi ** 4 / 15
    if abs(lam) < 0.05:
        val, _ = integrate.quad(lambda u: stats.tukeylambda.ppf(u, lam) ** 4, 0.0, 0.5, limit=400, epsabs=0, epsrel=1e-10)
        return 2 * val
    return sum(math.comb(4, j) * (-1) ** j * special.beta(lam * (4 - j) + 1, lam * j + 1) for j in range(5)) / lam ** 4


def check_tukeylambda(t, lam):
    """(row text, failures) for float samples `t` of Tukey-lambda(lam), scale 1: chi-square on 64 equiprobable bins against
    scipy.stats.tukeylambda at the 1e-6 tail; the three quartiles (the fraction of samples below each within 5 standard errors of a
    binomial share); the mean within 5 standard errors; for lam > -1/4 the variance within 5 standard errors from the law's own fourth
    moment (below that the fourth moment is infinite and the sample variance has no standard error)."""
    from scipy import stats
    from yond_public_amd.camnoise import tukeylambda_variance
    t = np.asarray(t, np.float64)
    n = t.size
    fails = []
    if not np.isfinite(t).all():
        fails.append("non-finite variates")
    edges = stats.tukeylambda.ppf(np.arange(1, 64) / 64.0, lam)
    obs = np.bincount(np.searchsorted(edges, t, side="left"), minlength=64).astype(np.float64)
    exp = n / 64.0
    chi2, lim = float(((obs - exp) ** 2 / exp).sum()), float(stats.chi2.isf(1e-6, 63))
    chi = f"chi2 {chi2:7.1f} / df 63 (<= {lim:.1f})"
    if chi2 > lim:
        fails.append(chi)
    for p in (0.25, 0.5, 0.75):
        frac = float((t < stats.tukeylambda.ppf(p, lam)).mean())
        if abs(frac - p) > 5 * math.sqrt(p * (1 - p) / n):
            fails.append(f"share below the {p} quantile {frac:.5f}")
    var = tukeylambda_variance(lam)
    m, v = float(t.mean()), float(t.var())
    se_m = math.sqrt(var / n)
    if abs(m) > 5 * se_m:
        fails.append(f"mean {m:.3e} (+- {5 * se_m:.3e})")
    row = f"lam {lam:7.3f}: mean {m:10.3e} ({abs(m) / se_m:4.2f} se)  var {v:10.5f} vs {var:10.5f}"
    if lam > -0.25:
        se_v = math.sqrt((tl_moment4(lam) - var * var) / n)
        row += f" ({abs(v - var) / se_v:4.2f} se)"
        if abs(v - var) > 5 * se_v:
            fails.append(f"var {v} vs {var} (+- {5 * se_v:.3g})")
    return row + "  " + chi, fails


def check_moments(x, mean, var, m4c, what):
    """Failures of samples `x` whose law has the given mean, variance and fourth CENTRAL moment: both within 5 standard errors."""
    x = np.asarray(x, np.float64)
    n = x.size
    m, v = float(x.mean()), float(x.var())
    se_m, se_v = math.sqrt(var / n), math.sqrt((m4c - var * var) / n)
    print(f"{what}: n {n}, mean {m:.4e} vs {mean:.4e} ({abs(m - mean) / se_m:4.2f} se), var {v:.6e} vs {var:.6e} ({abs(v - var) / se_v:4.2f} se)")
    fails = []
    if abs(m - mean) > 5 * se_m:
        fails.append(f"{what}: mean {m} vs {mean} (+- {5 * se_m:.3g})")
    if abs(v - var) > 5 * se_v:
        fails.append(f"{what}: var {v} vs {var} (+- {5 * se_v:.3g})")
    return fails
