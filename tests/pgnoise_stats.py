"""The distribution checks of the Poisson-Gaussian sampler, shared by tests/test_hip_pgnoise.py (the kernel) and
tests/test_pgnoise_host.py (the same sampler source compiled for the CPU).  Every bound comes from the Poisson law itself:
mean and variance within 5 standard errors, chi-square against scipy.stats.poisson at a 1e-6 tail."""
import numpy as np

BASE_LADDER = [0, 1e-3, 0.05, 0.5, 1, 3, 9.5, 10, 10.5, 12, 20, 29.5, 30, 30.5, 50, 100, 1e3, 1.17e4, 1.6e5, 2e6, 8e6]


def ladder(switch_lambdas):
    """The lambdas of the ladder tests as float32 values: the base ladder plus every regime threshold times (1 - 2^-10), 1, (1 + 2^-10)."""
    lams = list(BASE_LADDER)
    for s in switch_lambdas:
        lams += [s * (1 - 2.0 ** -10), s, s * (1 + 2.0 ** -10)]
    return [float(np.float32(v)) for v in lams]


def chi2_poisson(k, lam):
    """(chi2, df, threshold) of integer samples `k` against Poisson(lam), or None when fewer than two bins remain.  Right-closed
    integer edges unique(ppf(j / 64)), j = 1..63; expected counts from CDF differences; a bin expecting < 20 joins its neighbour."""
    from scipy import stats
    n = k.size
    if lam <= 0:
        return None
    edges = np.unique(stats.poisson.ppf(np.arange(1, 64) / 64.0, lam))
    cdf = np.concatenate([[0.0], stats.poisson.cdf(edges, lam), [1.0]])
    exp = list(np.diff(cdf) * n)
    obs = list(np.bincount(np.searchsorted(edges, k, side="left"), minlength=edges.size + 1).astype(np.float64))
    i = 0
    while len(exp) > 1 and i < len(exp):
        if exp[i] < 20:
            j = i + 1 if i + 1 < len(exp) else i - 1
            exp[j] += exp[i]
            obs[j] += obs[i]
            del exp[i], obs[i]
            i = 0
        else:
            i += 1
    if len(exp) < 2:
        return None
    exp, obs = np.array(exp), np.array(obs)
    return float(((obs - exp) ** 2 / exp).sum()), len(exp) - 1, float(stats.chi2.isf(1e-6, len(exp) - 1))


def check_counts(k, lam):
    """One ladder row for integer samples `k` (float64 array) of Poisson(lam): (row text, list of failures)."""
    n = k.size
    fails = []
    if not np.array_equal(k, np.rint(k)) or k.min() < 0:
        fails.append("counts are not non-negative integers")
    m, v = k.mean(), k.var()
    tm, tv = 5 * np.sqrt(lam / n), 5 * np.sqrt((lam + 2 * lam * lam) / n)
    if abs(m - lam) > tm:
        fails.append(f"mean {m} vs {lam} (+- {tm:.3g})")
    if abs(v - lam) > tv:
        fails.append(f"var {v} vs {lam} (+- {tv:.3g})")
    c = chi2_poisson(k, lam)
    if c is None:
        chi = "chi2 -"
        if lam == 0 and k.max() != 0:
            fails.append("lambda 0 gave a non-zero count")
    else:
        chi = f"chi2 {c[0]:8.1f} / df {c[1]:2d} (<= {c[2]:.1f})"
        if c[0] > c[2]:
            fails.append(chi)
    se_m, se_v = (abs(m - lam) / (tm / 5) if lam else 0.0), (abs(v - lam) / (tv / 5) if lam else 0.0)
    row = f"lambda {lam:14.6f}: mean {m:14.5f} ({se_m:4.2f} se)  var {v:16.4f} ({se_v:4.2f} se)  {chi}"
    return row, fails
